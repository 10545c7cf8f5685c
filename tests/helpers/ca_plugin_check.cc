// Test helper (GPU): the CAMethod classes of the host layer (ca_filter/device_ca.h) driven as a plugin author would drive the
// reference's GFCA / BoxCA / BFCA: aggreCV(lImg, rImg, maxDis, costVol) on CV_64FC3 / CV_64FC1 Mats.
//   ca_plugin_check <in.bin> <out.bin>
// in.bin: int32 w, h, n, method (0 BOX, 1 GF, 2 BF), then the guide h*w*3 doubles, then n slabs of h*w doubles;
// out.bin: the n slabs after aggreCV.  Also checks that a 1-channel guide is rejected.
#include <cstdio>
#include <memory>
#include <vector>

#include "ca_filter/device_ca.h"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int hdr[4];
  if (std::fread(hdr, sizeof(int), 4, f) != 4) return 3;
  const int w = hdr[0], h = hdr[1], n = hdr[2], method = hdr[3];
  std::vector<double> g((size_t)w * h * 3), v((size_t)n * w * h);
  if (std::fread(g.data(), sizeof(double), g.size(), f) != g.size() || std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) return 3;
  std::fclose(f);
  std::unique_ptr<CAMethod> ca(method == 0 ? static_cast<CAMethod *>(new BoxCA) : method == 1 ? static_cast<CAMethod *>(new GFCA)
                                                                                                : static_cast<CAMethod *>(new BFCA));
  Mat guide, other;
  guide.create(h, w, CV_64FC3);
  other.create(h, w, CV_64FC3);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w * 3; ++x) guide.ptr<double>(y)[x] = g[(size_t)y * w * 3 + x];
  std::vector<Mat> vol(n);
  for (int d = 0; d < n; ++d) {
    vol[d].create(h, w, CV_64FC1);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) vol[d].ptr<double>(y)[x] = v[((size_t)d * h + y) * w + x];
  }
  try {
    ca->aggreCV(guide, other, n, vol.data());
  } catch (const std::exception &e) {
    std::printf("aggreCV failed: %s\n", e.what());
    return 4;
  }
  Mat gray;
  gray.create(h, w, CV_64FC1);
  bool rejected = false;
  try {
    ca->aggreCV(gray, gray, n, vol.data());
  } catch (const std::exception &) {
    rejected = true;
  }
  if (!rejected) return 5;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  for (int d = 0; d < n; ++d)
    for (int y = 0; y < h; ++y) std::fwrite(vol[d].ptr<double>(y), sizeof(double), w, o);
  std::fclose(o);
  std::printf("ok\n");
  return 0;
}
