// Test helper (GPU): a carried start through the C++ host layer (cs_patchmatch.h PatchMatchCarried).
//   carry_check <in.bin> <out.bin>
// in.bin: int32 w, h, max_dis, scale_num, iters0, iters, then 5 doubles (the calibration f, cx, cy, baseline, doffs of both frames), 9 + 3
// doubles (the motion X_1 = R X_0 + t between the two left cameras), then the left and right image of frame 0 and of frame 1 (BGR,
// h*w*3 bytes each).
// The cost is PreCSPC (scale_num > 0) or PreSSPC over GRD, lambda 0.3; seed 12345 (the C ABI's default).
// Frame 0 runs PatchMatch(iters0); frame 1, on a second matcher and cost object, PatchMatchCarried(iters) from it.
// out.bin, per view of frame 1: h*w*6 doubles (norm, param) then h*w doubles (min_cost).
// Also checks that a foreign IPlaneCost and a previous matcher without a run are refused (exit 5 otherwise).
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

static IPlaneCost *make_cost(const Mat &l, const Mat &r, int D, int scale_num, CCMethod *cc) {
  if (scale_num > 0) return new PreCSPC(l, r, D, 35, scale_num, cc, 0.3);
  return new PreSSPC(l, r, D, 35, cc);
}

static void dump(FILE *o, const CSPatchMatch &m) {
  for (int v = 0; v < kViewNum; ++v) {
    std::vector<Plane> pl;
    std::vector<double> cost;
    m.planes(v == 0 ? kLeft : kRight, &pl, &cost);
    for (size_t i = 0; i < pl.size(); ++i) {
      const Vec3d n = pl[i].norm(), p = pl[i].param();
      const double q[6] = {n[0], n[1], n[2], p[0], p[1], p[2]};
      std::fwrite(q, sizeof(double), 6, o);
    }
    std::fwrite(cost.data(), sizeof(double), cost.size(), o);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int hdr[6];
  double num[17];
  if (std::fread(hdr, sizeof(int), 6, f) != 6 || std::fread(num, sizeof(double), 17, f) != 17) return 3;
  const int w = hdr[0], h = hdr[1], D = hdr[2], scale_num = hdr[3], iters0 = hdr[4], iters = hdr[5];
  const cspm_calib cal = {num[0], num[1], num[2], num[3], num[4]};
  const double *R = num + 5, *t = num + 14;
  Mat img[4];
  for (Mat &m : img) {
    m = Mat(h, w, CV_8UC3);
    for (int y = 0; y < h; ++y)
      if (std::fread(m.ptr<unsigned char>(y), 1, (size_t)w * 3, f) != (size_t)w * 3) return 3;
  }
  std::fclose(f);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  std::unique_ptr<CCMethod> cc(GetCCType("GRD"));
  try {
    std::unique_ptr<IPlaneCost> cost_a(make_cost(img[0], img[1], D, scale_num, cc.get()));
    CSPatchMatch a(img[0], img[1], D, 4);
    a.PatchMatch(iters0, cost_a.get(), false);
    std::unique_ptr<IPlaneCost> cost_b(make_cost(img[2], img[3], D, scale_num, cc.get()));
    CSPatchMatch b(img[2], img[3], D, 4);
    b.PatchMatchCarried(iters, cost_b.get(), false, a, cal, cal, R, t);
    dump(o, b);
    std::fclose(o);
    ConstantCost foreign;
    CSPatchMatch c(img[2], img[3], D, 4);
    try {
      c.PatchMatchCarried(1, &foreign, false, a, cal, cal, R, t);
      return 5;
    } catch (const std::exception &e) {
      std::printf("foreign refused: %s\n", e.what());
    }
    CSPatchMatch fresh(img[0], img[1], D, 4);
    try {
      c.PatchMatchCarried(1, cost_b.get(), false, fresh, cal, cal, R, t);
      return 5;
    } catch (const std::exception &e) {
      std::printf("no run refused: %s\n", e.what());
    }
  } catch (const std::exception &e) {
    std::printf("failed: %s\n", e.what());
    return 4;
  }
  std::printf("ok\n");
  return 0;
}
