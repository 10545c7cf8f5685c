// Test helper (GPU): the CENGRD cost through the C++ host layer.
//   cengrd_check <in.bin> <out.bin>
// in.bin: int32 w, h, max_dis, scale_num, iters, then the left and the right image (BGR, h*w*3 bytes each).
// The cost is PreCSPC(l, r, D, 35, scale_num, new CenGrdCC, 0.3) (scale_num > 0) or PreSSPC over a CenGrdCC; seed 12345 (the C ABI's
// default).  out.bin: per view h*w*6 doubles (norm, param) then h*w doubles (min_cost) after PatchMatch(iters), then CenGrdCC::buildCV
// and buildRightCV of the pair (max_dis + 1 slabs of h*w doubles each).
// Also checks the factory: getCCType("CENGRD") is a CenGrdCC, "CG" and "BSM" stay NULL (exit 5 otherwise).
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/cspm.h"
#include "cc/cengrd_cc.h"
#include "cs_patchmatch.h"
#include "get_method.h"
#include "plane_cost/pre_cs_pc.h"
#include "plane_cost/pre_ss_pc.h"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::unique_ptr<CCMethod> named(getCCType("CENGRD")), named2(GetCCType("CENGRD"));
  if (!named || !dynamic_cast<CenGrdCC *>(named.get()) || !named2 || !dynamic_cast<CenGrdCC *>(named2.get()) || getCCType("CG") != NULL ||
      getCCType("BSM") != NULL)
    return 5;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int hdr[5];
  if (std::fread(hdr, sizeof(int), 5, f) != 5) return 3;
  const int w = hdr[0], h = hdr[1], D = hdr[2], scale_num = hdr[3], iters = hdr[4];
  Mat l(h, w, CV_8UC3), r(h, w, CV_8UC3);
  for (Mat *m : {&l, &r})
    for (int y = 0; y < h; ++y)
      if (std::fread(m->ptr<unsigned char>(y), 1, (size_t)w * 3, f) != (size_t)w * 3) return 3;
  std::fclose(f);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  try {
    std::unique_ptr<CCMethod> cc(new CenGrdCC);  // the plane cost does not own its CCMethod
    std::unique_ptr<IPlaneCost> cost(scale_num > 0 ? static_cast<IPlaneCost *>(new PreCSPC(l, r, D, 35, scale_num, cc.get(), 0.3))
                                                   : static_cast<IPlaneCost *>(new PreSSPC(l, r, D, 35, cc.get())));
    CSPatchMatch m(l, r, D, 4);
    m.PatchMatch(iters, cost.get(), false);
    for (int v = 0; v < kViewNum; ++v) {
      std::vector<Plane> pl;
      std::vector<double> c;
      m.planes(v == 0 ? kLeft : kRight, &pl, &c);
      for (size_t i = 0; i < pl.size(); ++i) {
        const Vec3d n = pl[i].norm(), p = pl[i].param();
        const double q[6] = {n[0], n[1], n[2], p[0], p[1], p[2]};
        std::fwrite(q, sizeof(double), 6, o);
      }
      std::fwrite(c.data(), sizeof(double), c.size(), o);
    }
    // the CCMethod boundary: CV_64FC3 RGB images, as PreCSPC hands them to a plugin (pre_cs_pc.cc:60-64)
    Mat rgb[2];
    const Mat *src[2] = {&l, &r};
    for (int v = 0; v < 2; ++v) {
      rgb[v].create(h, w, CV_64FC3);
      for (int y = 0; y < h; ++y) {
        const unsigned char *s = src[v]->ptr<unsigned char>(y);
        double *d = rgb[v].ptr<double>(y);
        for (int x = 0; x < w; ++x)
          for (int c = 0; c < 3; ++c) d[3 * x + c] = s[3 * x + (2 - c)];
      }
    }
    for (int right = 0; right < 2; ++right) {
      std::vector<Mat> vol(D + 1);
      if (right) named->buildRightCV(rgb[0], rgb[1], D + 1, vol.data());
      else named->buildCV(rgb[0], rgb[1], D + 1, vol.data());
      for (int d = 0; d <= D; ++d)
        for (int y = 0; y < h; ++y) std::fwrite(vol[d].ptr<double>(y), sizeof(double), w, o);
    }
  } catch (const std::exception &e) {
    std::printf("failed: %s\n", e.what());
    return 4;
  }
  std::fclose(o);
  std::printf("ok\n");
  return 0;
}
