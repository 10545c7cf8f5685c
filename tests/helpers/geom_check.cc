// geom_check.cc -- CSPatchMatch::Reproject of the host layer against the C ABI on the same device context: after a PatchMatch run on a
// synthetic pair, every output of Reproject (RAW, PP with a median setting, RAW with a fit) equals what cspm_reproject returns for the
// same arguments, the cloud is as long as the count, and a call before any run throws.
// usage: geom_check        prints "geom_check ok" and exits 0, or says what failed and exits 1
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cs_patchmatch.h"
#include "cc/grd_cc.h"
#include "plane_cost/pre_cs_pc.h"

static int g_bad = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_bad;                                              \
    }                                                       \
  } while (0)

template <class T>
static bool SameBytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main() {
  const int w = 77, h = 41, max_dis = 16;
  Mat l(h, w, CV_8UC3), r(h, w, CV_8UC3);
  unsigned s = 12345u;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int k = 0; k < 3; ++k) {
        s = s * 1664525u + 1013904223u;
        const unsigned char tex = (unsigned char)(((x * 7 + y * 13) & 63) * 3 + ((s >> 24) & 15));
        l.ptr<unsigned char>(y)[3 * x + k] = tex;
        r.ptr<unsigned char>(y)[3 * x + k] = tex;
      }
  for (int y = 0; y < h; ++y)  // the right image: the left one shifted by 5 (a fronto-parallel scene)
    for (int x = 0; x + 5 < w; ++x)
      for (int k = 0; k < 3; ++k) r.ptr<unsigned char>(y)[3 * x + k] = l.ptr<unsigned char>(y)[3 * (x + 5) + k];
  const cspm_calib calib = {300.0, 38.5, 20.25, 0.25, 3.5};
  cspm_geom_params g;
  cspm_geom_default_params(&g);
  g.min_cos = 0.5;
  g.left_frame = 1;
  try {
    CSPatchMatch fresh(l, r, max_dis, 4);
    bool threw = false;
    try {
      fresh.Reproject(kLeft, calib, g, CSPM_GEOM_RAW, NULL, NULL, NULL, NULL, NULL, NULL);
    } catch (const std::exception &) {
      threw = true;
    }
    EXPECT(threw);

    GrdCC cc;
    PreCSPC cost(l, r, max_dis, 9, 3, &cc, 0.3);
    CSPatchMatch pm(l, r, max_dis, 4);
    pm.set_seed(7);
    pm.SetMedianFilter(1);
    pm.PatchMatch(1, &cost, false);
    cspm_ctx *ctx = cost.device_ctx();
    cspm_fit_params fit;
    cspm_fit_default_params(&fit);
    fit.radius = 2;
    const size_t n = (size_t)w * h;
    for (int view = 0; view < 2; ++view)
      for (int mode = 0; mode < 3; ++mode) {
        const int source = mode == 1 ? CSPM_GEOM_PP : CSPM_GEOM_RAW;
        const cspm_fit_params *f = mode == 2 ? &fit : NULL;
        std::vector<double> depth, xyz, normal;
        std::vector<uint8_t> keep;
        std::vector<cspm_point> cloud;
        const size_t count = pm.Reproject(view == 0 ? kLeft : kRight, calib, g, source, f, &depth, &xyz, &normal, &keep, &cloud);
        std::vector<double> depth2(n), xyz2(3 * n), normal2(3 * n);
        std::vector<uint8_t> keep2(n);
        std::vector<cspm_point> cloud2(n);
        unsigned int count2 = 0;
        EXPECT(cspm_set_pp_median(ctx, 1) == CSPM_OK);
        EXPECT(cspm_reproject(ctx, view, source, &calib, &g, f, depth2.data(), xyz2.data(), normal2.data(), keep2.data(), cloud2.data(), n, &count2) == CSPM_OK);
        cloud2.resize(count2);
        EXPECT(count == count2 && cloud.size() == count && count > 0 && count <= n);
        EXPECT(SameBytes(depth, depth2) && SameBytes(xyz, xyz2) && SameBytes(normal, normal2) && SameBytes(keep, keep2) && SameBytes(cloud, cloud2));
        EXPECT(pm.Reproject(view == 0 ? kLeft : kRight, calib, g, source, f, NULL, NULL, NULL, NULL, NULL) == count);  // the count alone
      }
    cspm_geom_params bad = g;
    bad.min_cos = 2.0;
    bool threw2 = false;
    try {
      pm.Reproject(kLeft, calib, bad, CSPM_GEOM_RAW, NULL, NULL, NULL, NULL, NULL, NULL);
    } catch (const std::exception &) {
      threw2 = true;
    }
    EXPECT(threw2);
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  if (g_bad) return 1;
  std::printf("geom_check ok\n");
  return 0;
}
