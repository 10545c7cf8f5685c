// Test helper (GPU): segment planes through the C++ host layer (cs_patchmatch.h SegmentPlanes, commfunc.h SegmentImage / SegmentPlanes).
//   seg_check <in.bin> <out.bin>
// in.bin: int32 w, h, max_dis, scale_num, iters, step, warm iterations, then the left and the right image (BGR, h*w*3 bytes each).
// The cost is PreCSPC (scale_num > 0) or PreSSPC over GRD, lambda 0.3; seed 12345 (the C ABI's default); the other segment parameters
// are the defaults.
// out.bin: per view h*w*6 doubles (norm, param) then h*w doubles (min_cost) of PatchMatchBegin(iters), SegmentPlanes(merge = true),
// PatchMatchFromBegin(warm), PatchMatchEnd; then, for the left view, SegmentImage's labels as h*w doubles, and SegmentPlanes of the
// matcher's left disparity map under them: h*w*6 doubles, `fitted` as h*w doubles, and three doubles per segment.
// Also checks that CSPatchMatch::SegmentPlanes refuses a foreign IPlaneCost (exit 5 otherwise).
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/cspm.h"
#include "cs_patchmatch.h"
#include "get_method.h"
#include "plane_cost/pre_cs_pc.h"
#include "plane_cost/pre_ss_pc.h"

class ConstantCost : public IPlaneCost {  // a plugin cost: not one of the library's device costs
 public:
  virtual double GetPlaneCost(const int &, const int &, const Plane &, const RefView &) const { return 0.0; }
};

static void dump_planes(FILE *o, const std::vector<Plane> &pl) {
  for (size_t i = 0; i < pl.size(); ++i) {
    const Vec3d n = pl[i].norm(), p = pl[i].param();
    const double q[6] = {n[0], n[1], n[2], p[0], p[1], p[2]};
    std::fwrite(q, sizeof(double), 6, o);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int hdr[7];
  if (std::fread(hdr, sizeof(int), 7, f) != 7) return 3;
  const int w = hdr[0], h = hdr[1], D = hdr[2], scale_num = hdr[3], iters = hdr[4], warm = hdr[6];
  cspm_seg_params seg;
  cspm_seg_default_params(&seg);
  seg.step = hdr[5];
  Mat l(h, w, CV_8UC3), r(h, w, CV_8UC3);
  for (Mat *m : {&l, &r})
    for (int y = 0; y < h; ++y)
      if (std::fread(m->ptr<unsigned char>(y), 1, (size_t)w * 3, f) != (size_t)w * 3) return 3;
  std::fclose(f);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  try {
    std::unique_ptr<CCMethod> cc(GetCCType("GRD"));
    std::unique_ptr<IPlaneCost> cost(scale_num > 0 ? static_cast<IPlaneCost *>(new PreCSPC(l, r, D, 35, scale_num, cc.get(), 0.3))
                                                   : static_cast<IPlaneCost *>(new PreSSPC(l, r, D, 35, cc.get())));
    CSPatchMatch a(l, r, D, 4);
    a.PatchMatchBegin(iters, cost.get(), false);
    a.SegmentPlanes(cost.get(), seg, true);
    a.PatchMatchFromBegin(warm, cost.get(), false);
    a.PatchMatchEnd();
    for (int v = 0; v < kViewNum; ++v) {
      std::vector<Plane> pl;
      std::vector<double> c;
      a.planes(v == 0 ? kLeft : kRight, &pl, &c);
      dump_planes(o, pl);
      std::fwrite(c.data(), sizeof(double), c.size(), o);
    }
    std::vector<double> d;
    a.disparity(kLeft, &d);
    Mat disp(h, w, CV_64FC1), labels, fitted;
    for (int y = 0; y < h; ++y) std::copy(d.begin() + (size_t)y * w, d.begin() + (size_t)(y + 1) * w, disp.ptr<double>(y));
    SegmentImage(l, labels, &seg);
    std::vector<Plane> pl;
    std::vector<double> abc, tmp((size_t)w * h);
    SegmentPlanes(disp, NULL, labels, &seg, D, &pl, &fitted, &abc);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) tmp[(size_t)y * w + x] = labels.at<int32_t>(y, x);
    std::fwrite(tmp.data(), sizeof(double), tmp.size(), o);
    dump_planes(o, pl);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) tmp[(size_t)y * w + x] = fitted.at<unsigned char>(y, x);
    std::fwrite(tmp.data(), sizeof(double), tmp.size(), o);
    std::fwrite(abc.data(), sizeof(double), abc.size(), o);
  } catch (const std::exception &e) {
    std::printf("failed: %s\n", e.what());
    return 4;
  }
  std::fclose(o);
  ConstantCost foreign;
  CSPatchMatch c(l, r, D, 4);
  try {
    c.SegmentPlanes(&foreign, seg, true);
    return 5;
  } catch (const std::exception &e) {
    std::printf("foreign refused: %s\n", e.what());
  }
  std::printf("ok\n");
  return 0;
}
