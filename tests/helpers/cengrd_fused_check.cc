// Test helper (GPU): fused CENGRD cells through the C++ host layer.
//   cengrd_fused_check <in.bin> <out.bin>
// in.bin: int32 w, h, max_dis, scale_num, iters, then the left and the right image (BGR, h*w*3 bytes each).
// Runs PreCSPC / PreSSPC over `new CenGrdCC(-1, true)` (fused cells) and over `new CenGrdCC` (volumes) on one device slot that keeps
// its context, so the second object reuses the first one's context: CSPM_OPT_CENGRD_FUSED_ACTIVE must read 1, then 0 (exit 5
// otherwise), and the two fields must agree bit for bit (exit 7).  out.bin: the fused run's field, per view h*w*6 doubles (norm,
// param) then h*w doubles (min_cost).
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/cspm.h"
#include "cc/cengrd_cc.h"
#include "cs_patchmatch.h"
#include "plane_cost/device_plane_cost.h"
#include "plane_cost/pre_cs_pc.h"
#include "plane_cost/pre_ss_pc.h"

static std::vector<double> run(const Mat &l, const Mat &r, int D, int scale_num, int iters, bool fused, long long want_active, bool *active_ok) {
  std::unique_ptr<CCMethod> cc(new CenGrdCC(-1, fused));
  std::unique_ptr<IPlaneCost> cost(scale_num > 0 ? static_cast<IPlaneCost *>(new PreCSPC(l, r, D, 35, scale_num, cc.get(), 0.3))
                                                 : static_cast<IPlaneCost *>(new PreSSPC(l, r, D, 35, cc.get())));
  long long active = -1;
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(cost.get());
  *active_ok = dev && cspm_get_option(dev->device_ctx(), CSPM_OPT_CENGRD_FUSED_ACTIVE, &active) == CSPM_OK && active == want_active;
  CSPatchMatch m(l, r, D, 4);
  m.PatchMatch(iters, cost.get(), false);
  std::vector<double> out;
  for (int v = 0; v < kViewNum; ++v) {
    std::vector<Plane> pl;
    std::vector<double> c;
    m.planes(v == 0 ? kLeft : kRight, &pl, &c);
    for (size_t i = 0; i < pl.size(); ++i) {
      const Vec3d n = pl[i].norm(), p = pl[i].param();
      const double q[6] = {n[0], n[1], n[2], p[0], p[1], p[2]};
      out.insert(out.end(), q, q + 6);
    }
    out.insert(out.end(), c.begin(), c.end());
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
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
  try {
    DeviceSlot slot(0, true);  // keeps its context: the volume-sourced object inherits the fused one's options and buffers
    DeviceSlot::Use use(slot);
    bool ok_fused = false, ok_vol = false;
    const std::vector<double> fused = run(l, r, D, scale_num, iters, true, 1, &ok_fused);
    const std::vector<double> vol = run(l, r, D, scale_num, iters, false, 0, &ok_vol);
    if (!ok_fused || !ok_vol) return 5;
    if (fused.size() != vol.size() || std::memcmp(fused.data(), vol.data(), fused.size() * sizeof(double)) != 0) return 7;
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    std::fwrite(fused.data(), sizeof(double), fused.size(), o);
    std::fclose(o);
  } catch (const std::exception &e) {
    std::printf("failed: %s\n", e.what());
    return 4;
  }
  std::printf("ok\n");
  return 0;
}
