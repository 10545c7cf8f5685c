// Test helper (GPU): plane fitting through the C++ host layer (cs_patchmatch.h FitPlanes and the AddCandidateDisparity overload that
// fits).
//   fit_check <in.bin> <out.bin>
// in.bin: int32 w, h, max_dis, scale_num, ca_method (CSPM_CA_*), iters, fit radius, then the left and the right image (BGR, h*w*3 bytes
// each), then a left-view disparity map of h*w doubles (non-finite or negative: no node).
// The cost is PreCSPC (scale_num > 0) or PreSSPC over GRD, lambda 0.3; seed 12345 (the C ABI's default); the other fit parameters are
// the defaults.
// out.bin, per run and view: h*w*6 doubles (norm, param) then h*w doubles (min_cost).  Run A: AddCandidateDisparity(kLeft, disp, fit)
// then PatchMatchSeeded(iters).  Run B: a second matcher and cost object, LocalStereo(ca_method), FitPlanes(merge = false), then
// PatchMatchFrom(iters).  Also checks that FitPlanes refuses a foreign IPlaneCost (exit 5 otherwise).
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
  int hdr[7];
  if (std::fread(hdr, sizeof(int), 7, f) != 7) return 3;
  const int w = hdr[0], h = hdr[1], D = hdr[2], scale_num = hdr[3], ca = hdr[4], iters = hdr[5];
  cspm_fit_params fit;
  cspm_fit_default_params(&fit);
  fit.radius = hdr[6];
  Mat l(h, w, CV_8UC3), r(h, w, CV_8UC3), disp(h, w, CV_64FC1);
  for (Mat *m : {&l, &r})
    for (int y = 0; y < h; ++y)
      if (std::fread(m->ptr<unsigned char>(y), 1, (size_t)w * 3, f) != (size_t)w * 3) return 3;
  for (int y = 0; y < h; ++y)
    if (std::fread(disp.ptr<double>(y), sizeof(double), (size_t)w, f) != (size_t)w) return 3;
  std::fclose(f);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  try {
    std::unique_ptr<CCMethod> cc(GetCCType("GRD"));
    std::unique_ptr<IPlaneCost> cost_a(make_cost(l, r, D, scale_num, cc.get()));
    CSPatchMatch a(l, r, D, 4);
    a.AddCandidateDisparity(kLeft, disp, fit);
    a.PatchMatchSeeded(iters, cost_a.get(), false);
    dump(o, a);
    std::unique_ptr<IPlaneCost> cost_b(make_cost(l, r, D, scale_num, cc.get()));
    CSPatchMatch b(l, r, D, 4);
    b.LocalStereo(ca, cost_b.get(), false);
    b.FitPlanes(cost_b.get(), fit, false);
    b.PatchMatchFrom(iters, cost_b.get(), false);
    dump(o, b);
  } catch (const std::exception &e) {
    std::printf("failed: %s\n", e.what());
    return 4;
  }
  std::fclose(o);
  ConstantCost foreign;
  CSPatchMatch c(l, r, D, 4);
  try {
    c.FitPlanes(&foreign, fit, false);
    return 5;
  } catch (const std::exception &e) {
    std::printf("foreign refused: %s\n", e.what());
  }
  std::printf("ok\n");
  return 0;
}
