// smooth_check.cc -- CSPatchMatch::SetSmoothing and SmoothDisparity of the host layer against the C ABI: after a PatchMatch run on a
// synthetic pair, PostProcessedDisparity with smoothing equals cspm_postprocess_f64 on the same context with the same settings, differs
// from the unsmoothed maps and returns to them when smoothing is switched off; SmoothDisparity on Mats equals
// cspm_smooth_disparity_host, in place too; what the C ABI refuses throws.
// usage: smooth_check        prints "smooth_check ok" and exits 0, or says what failed and exits 1
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

static bool SameBytes(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

template <class F>
static bool Throws(F f) {
  try {
    f();
  } catch (const std::exception &) {
    return true;
  }
  return false;
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
  const size_t n = (size_t)w * h;
  try {
    cspm_smooth_params p;
    EXPECT(cspm_smooth_default_params(&p) == CSPM_OK && p.lambda == 100.0 && p.sigma_color == 20.0 && p.iterations == 3 && p.fill_conf == 0.25);
    p.sigma_color = 12.0;
    p.iterations = 2;
    p.fill_conf = 0.5;

    GrdCC cc;
    PreCSPC cost(l, r, max_dis, 9, 3, &cc, 0.3);
    CSPatchMatch pm(l, r, max_dis, 4);
    pm.set_seed(7);
    pm.SetMedianFilter(1);
    pm.PatchMatch(1, &cost, false);
    cspm_ctx *ctx = cost.device_ctx();
    std::vector<double> l0, r0, l1, r1, l2(n), r2(n), l3, r3;
    pm.PostProcessedDisparity(&l0, &r0);
    pm.SetSmoothing(&p);
    pm.PostProcessedDisparity(&l1, &r1);
    EXPECT(cspm_set_pp_median(ctx, 1) == CSPM_OK && cspm_set_pp_smooth(ctx, &p) == CSPM_OK);
    EXPECT(cspm_postprocess_f64(ctx, l2.data(), r2.data(), NULL, NULL) == CSPM_OK);
    EXPECT(SameBytes(l1, l2) && SameBytes(r1, r2));
    EXPECT(!SameBytes(l0, l1) && !SameBytes(r0, r1));
    pm.SetSmoothing(NULL);
    pm.PostProcessedDisparity(&l3, &r3);
    EXPECT(SameBytes(l0, l3) && SameBytes(r0, r3));
    int on = 1;
    EXPECT(cspm_get_pp_smooth(ctx, NULL, &on) == CSPM_OK && on == 0);  // written into the context by the post-processing
    cspm_smooth_params bad = p;
    bad.iterations = 9;
    EXPECT(Throws([&] { pm.SetSmoothing(&bad); }));
    bad = p;
    bad.fill_conf = 1.5;
    EXPECT(Throws([&] { pm.SetSmoothing(&bad); }));
    bad = p;
    bad.lambda = -1.0;
    EXPECT(Throws([&] { pm.SetSmoothing(&bad); }));

    // SmoothDisparity: the left map with a hole, half confidences, the left image as guide
    Mat disp(h, w, CV_64FC1), conf(h, w, CV_64FC1), out, out_plain;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        disp.at<double>(y, x) = (x + y) % 11 == 0 ? std::numeric_limits<double>::quiet_NaN() : l0[(size_t)y * w + x];
        conf.at<double>(y, x) = (x * 3 + y) % 4 == 0 ? 0.5 : 1.0;
      }
    SmoothDisparity(disp, &conf, &l, &p, max_dis, out);
    std::vector<double> want(n), got(out.ptr<double>(0), out.ptr<double>(0) + n);
    EXPECT(cspm_smooth_disparity_host(0, disp.ptr<double>(0), conf.ptr<double>(0), l.ptr<unsigned char>(0), w, h, &p, max_dis, want.data()) == CSPM_OK);
    EXPECT(out.rows == h && out.cols == w && out.type() == CV_64FC1 && SameBytes(got, want));
    bool finite = true;
    for (size_t i = 0; i < n; ++i) finite = finite && got[i] >= 0.0 && got[i] <= max_dis;
    EXPECT(finite);  // the holes are filled and the clamp holds
    SmoothDisparity(disp, NULL, NULL, NULL, 0, out_plain);
    EXPECT(cspm_smooth_disparity_host(0, disp.ptr<double>(0), NULL, NULL, w, h, NULL, 0, want.data()) == CSPM_OK);
    EXPECT(std::memcmp(out_plain.ptr<double>(0), want.data(), n * sizeof(double)) == 0);
    Mat inplace = disp.clone();
    SmoothDisparity(inplace, &conf, &l, &p, max_dis, inplace);
    EXPECT(std::memcmp(inplace.ptr<double>(0), got.data(), n * sizeof(double)) == 0);
    Mat wrong(h, w, CV_8UC3), small(h - 1, w, CV_64FC1);
    EXPECT(Throws([&] { SmoothDisparity(wrong, NULL, NULL, NULL, 0, out); }));
    EXPECT(Throws([&] { SmoothDisparity(disp, &small, NULL, NULL, 0, out); }));
    EXPECT(Throws([&] { SmoothDisparity(disp, NULL, &disp, NULL, 0, out); }));
    EXPECT(Throws([&] { SmoothDisparity(disp, NULL, NULL, &bad, 0, out); }));
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  if (g_bad) return 1;
  std::printf("smooth_check ok\n");
  return 0;
}
