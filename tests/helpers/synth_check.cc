// synth_check.cc -- CSPatchMatch::Synthesize of the host layer against the C ABI on the same device context: after a PatchMatch run on a
// synthetic pair, every output of Synthesize (RAW, PP with a median setting; both views, one view without the fill) equals what
// cspm_synthesize returns for the same arguments, t = 0 from the left view alone gives the left image back wherever the pixel's own plane
// is usable, and a call before any run
// or with a bad t throws.
// usage: synth_check        prints "synth_check ok" and exits 0, or says what failed and exits 1
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
  cspm_synth_params sp;
  cspm_synth_default_params(&sp);
  try {
    CSPatchMatch fresh(l, r, max_dis, 4);
    bool threw = false;
    try {
      fresh.Synthesize(0.5, sp, CSPM_GEOM_RAW, NULL, NULL, NULL);
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
    const size_t n = (size_t)w * h;
    for (int mode = 0; mode < 4; ++mode) {
      const int source = mode & 1 ? CSPM_GEOM_PP : CSPM_GEOM_RAW;
      cspm_synth_params p = sp;
      if (mode & 2) {
        p.views = 1;
        p.fill = 0;
      }
      const double t = mode & 2 ? 1.0 : 0.5;
      Mat bgr;
      std::vector<double> disp;
      std::vector<uint8_t> mask;
      pm.Synthesize(t, p, source, &bgr, &disp, &mask);
      EXPECT(bgr.rows == h && bgr.cols == w && bgr.channels() == 3);
      std::vector<uint8_t> img((size_t)3 * n), img2((size_t)3 * n), mask2(n);
      for (int y = 0; y < h; ++y) std::memcpy(&img[(size_t)3 * w * y], bgr.ptr<unsigned char>(y), (size_t)3 * w);
      std::vector<double> disp2(n);
      EXPECT(cspm_set_pp_median(ctx, 1) == CSPM_OK);
      EXPECT(cspm_synthesize(ctx, source, &p, t, img2.data(), (size_t)3 * w, disp2.data(), mask2.data()) == CSPM_OK);
      EXPECT(SameBytes(img, img2) && SameBytes(disp, disp2) && SameBytes(mask, mask2));
      size_t holes = 0;
      for (size_t i = 0; i < n; ++i) holes += mask[i] == 0;
      EXPECT(mode & 2 ? holes > 0 && holes < n : holes == 0);
      pm.Synthesize(t, p, source, NULL, NULL, &mask);  // one output alone
      EXPECT(SameBytes(mask, mask2));
    }
    cspm_synth_params one = sp;
    one.views = 1;
    Mat back;
    std::vector<uint8_t> seen;
    pm.Synthesize(0.0, one, CSPM_GEOM_RAW, &back, NULL, &seen);
    size_t own = 0;
    bool same = true;  // where the pixel's own plane is usable (a disparity >= 0) it lands on itself: the left image comes back
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        if (seen[(size_t)y * w + x] != 1) continue;
        ++own;
        same = same && std::memcmp(back.ptr<unsigned char>(y) + 3 * x, l.ptr<unsigned char>(y) + 3 * x, 3) == 0;
      }
    EXPECT(same && own > n / 2);
    bool threw2 = false;
    try {
      pm.Synthesize(1.5, sp, CSPM_GEOM_RAW, &back, NULL, NULL);
    } catch (const std::exception &) {
      threw2 = true;
    }
    EXPECT(threw2);
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  if (g_bad) return 1;
  std::printf("synth_check ok\n");
  return 0;
}
