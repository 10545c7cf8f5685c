// tests/test_reference_ca.py: the reference's own cost-aggregation filters (ca_filter/GuidedFilter.cpp, BilateralFilter.cpp,
// BoxCA.cpp, GFCA.cpp, BFCA.cpp, compiled UNMODIFIED against the test-only stand-in in tests/helpers/refcheck/) run on a guide and
// a stack of cost slabs; the filtered stack is written out for comparison with tests/ca_ref.py and the HIP kernels.  Test
// infrastructure; nothing of the reference is copied into the repository.
//
//   cacheck <in.bin> <out.bin>
//   in:  int32 w, h, n, method; guide (h, w, 3) f64; stack (n, h, w) f64        out: stack (n, h, w) f64
//   method 0 / 1 / 2: BoxCA / GFCA / BFCA::aggreCV(guide, guide, n, stack) through CAMethod* (slices 1 .. n-1 filtered)
//   method 11 / 12:   CumSum(slab, 1 / 2) of every slab                 method 100 + r: BoxFilter(slab, r) of every slab
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>
#include <opencv2/opencv.hpp>
#include "ca_method.h"
#include "ca_filter/BoxCA.h"
#include "ca_filter/GFCA.h"
#include "ca_filter/BFCA.h"
#include "ca_filter/GuidedFilter.h"

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: cacheck <in.bin> <out.bin>\n"); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  int hdr[4];
  in.read(reinterpret_cast<char *>(hdr), sizeof hdr);
  const int w = hdr[0], h = hdr[1], n = hdr[2], method = hdr[3];
  if (!in || w < 1 || h < 1 || n < 1) { std::fprintf(stderr, "cacheck: bad header\n"); return 2; }
  Mat guide(h, w, CV_64FC3);
  in.read(reinterpret_cast<char *>(guide.data), (std::streamsize)sizeof(double) * 3 * w * h);
  std::vector<Mat> vol(n);
  for (int d = 0; d < n; ++d) {
    vol[d] = Mat(h, w, CV_64FC1);
    in.read(reinterpret_cast<char *>(vol[d].data), (std::streamsize)sizeof(double) * w * h);
  }
  if (!in) { std::fprintf(stderr, "cacheck: short input\n"); return 2; }
  try {
    if (method >= 0 && method <= 2) {
      std::unique_ptr<CAMethod> ca;
      if (method == 0) ca.reset(new BoxCA());
      else if (method == 1) ca.reset(new GFCA());
      else ca.reset(new BFCA());
      ca->aggreCV(guide, guide, n, vol.data());
    } else if (method == 11 || method == 12) {
      for (int d = 0; d < n; ++d) vol[d] = CumSum(vol[d], method - 10);
    } else if (method > 100) {
      for (int d = 0; d < n; ++d) vol[d] = BoxFilter(vol[d], method - 100);
    } else {
      std::fprintf(stderr, "cacheck: unknown method %d\n", method);
      return 2;
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "cacheck: %s\n", e.what());
    return 1;
  }
  std::ofstream out(argv[2], std::ios::binary);
  for (int d = 0; d < n; ++d) {
    if (vol[d].rows != h || vol[d].cols != w || vol[d].type() != CV_64FC1) { std::fprintf(stderr, "cacheck: slab %d changed shape\n", d); return 1; }
    out.write(reinterpret_cast<const char *>(vol[d].data), (std::streamsize)sizeof(double) * w * h);
  }
  return out ? 0 : 1;
}
