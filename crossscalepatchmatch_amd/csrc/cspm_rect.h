// cspm_rect.h -- rectification of a calibrated raw stereo pair (include/cspm.h "rectification"): the specification R,
// one pixel at a time.
//
// rect_map_pixel() evaluates the map M_v for one rectified pixel and rect_remap_pixel() the bilinear remap of one; every kernel that needs
// either calls it, so the one-shot entry and the context path cannot differ by a bit.  Two element-wise passes, no atomics, no LDS, no
// workgroup waits for another:
//   k_rect_map    one LANE per rectified pixel in flat raster order (as k_geom_dense): the two 8-byte planes sx, sy and the byte plane
//                 valid, all coalesced.  Built once per rig and kept.
//   k_rect_remap  one WAVE per 64 consecutive x of one output row, kRectWaves waves per workgroup: neighbouring lanes read neighbouring
//                 map entries and -- the map being smooth -- gather from near-contiguous raw addresses.  The raw image is read through
//                 the packed B | G<<8 | R<<16 words of k_pack_bgr (one 4-byte load per tap instead of three byte loads); the result is
//                 the packed 8UC3 row cspm_set_images_device consumes.
// Rectified -> raw is the FORWARD distortion model: no iteration anywhere.  Every product, sum and quotient is one IEEE f64 operation in
// the association the specification states (-ffp-contract=off, and the pragma below); `/` is correctly rounded on the device.
#pragma once
#include "cspm_device.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kRectBlock = 256;  // lanes per workgroup of both passes: 4 waves
constexpr int kRectWaves = kRectBlock / kWave;

struct RectView {  // one view of a rectification as the kernels need it
  double f, cx, cy;  // the common projection
  double r[9];       // R_v, row-major: X_rect = R_v * X_cam; the kernels apply its transpose
  double fx, fy, cxraw, cyraw, skew, k1, k2, p1, p2, k3;
  int raw_w, raw_h;
};
struct RectPix {
  double sx, sy;
  bool valid;
};

__device__ __forceinline__ RectPix rect_map_pixel(const RectView &k, int x, int y) {
  const double u = ((double)x - k.cx) / k.f, wv = ((double)y - k.cy) / k.f;
  const double X = (k.r[0] * u + k.r[3] * wv) + k.r[6];
  const double Y = (k.r[1] * u + k.r[4] * wv) + k.r[7];
  const double Z = (k.r[2] * u + k.r[5] * wv) + k.r[8];
  const bool front = Z > 0.0;
  const double a = X / Z, b = Y / Z, r2 = a * a + b * b;
  const double rad = 1.0 + r2 * (k.k1 + r2 * (k.k2 + r2 * k.k3));
  const double ad = a * rad + ((2.0 * k.p1) * a * b + k.p2 * (r2 + 2.0 * a * a));
  const double bd = b * rad + (k.p1 * (r2 + 2.0 * b * b) + (2.0 * k.p2) * a * b);
  RectPix p;
  p.sx = (k.fx * ad + k.skew * bd) + k.cxraw;
  p.sy = k.fy * bd + k.cyraw;
  p.valid = front && p.sx >= 0.0 && p.sx <= (double)(k.raw_w - 1) && p.sy >= 0.0 && p.sy <= (double)(k.raw_h - 1);  // false for NaN
  return p;
}

// the remapped pixel as B | G<<8 | R<<16; (sx, sy) is a VALID map entry: 0 <= sx <= raw_w-1 and 0 <= sy <= raw_h-1, so every tap is inside
__device__ __forceinline__ uint32_t rect_remap_pixel(const uint32_t *__restrict__ raw, int raw_w, int raw_h, double sx, double sy) {
  const int x0 = (int)floor(sx), y0 = (int)floor(sy);
  const int x1 = min(x0 + 1, raw_w - 1), y1 = min(y0 + 1, raw_h - 1);
  const double tx = sx - (double)x0, ty = sy - (double)y0;
  const uint32_t p00 = raw[(size_t)y0 * raw_w + x0], p01 = raw[(size_t)y0 * raw_w + x1];
  const uint32_t p10 = raw[(size_t)y1 * raw_w + x0], p11 = raw[(size_t)y1 * raw_w + x1];
  uint32_t packed = 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double i00 = (double)((p00 >> (8 * ch)) & 255u), i01 = (double)((p01 >> (8 * ch)) & 255u);
    const double i10 = (double)((p10 >> (8 * ch)) & 255u), i11 = (double)((p11 >> (8 * ch)) & 255u);
    const double top = i00 + tx * (i01 - i00);
    const double bot = i10 + tx * (i11 - i10);
    const double val = top + ty * (bot - top);
    packed |= (uint32_t)min(max(round2int(val), 0), 255) << (8 * ch);
  }
  return packed;
}

// the map of one view: sx = map[0 .. n), sy = map[n .. 2n), valid n bytes
__global__ __launch_bounds__(kRectBlock) void k_rect_map(RectView k, int W, long long n, double *__restrict__ map, uint8_t *__restrict__ valid) {
  const long long i = (long long)blockIdx.x * kRectBlock + (int)threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const RectPix p = rect_map_pixel(k, x, y);
  map[i] = p.sx;
  map[n + i] = p.sy;
  valid[i] = p.valid ? 1 : 0;
}

// one wave per 64 consecutive x of one output row; dst: packed 8UC3 rows of dst_stride bytes (bytes beyond 3*W of a row are untouched)
__global__ __launch_bounds__(kRectBlock) void k_rect_remap(const double *__restrict__ map, const uint8_t *__restrict__ valid, const uint32_t *__restrict__ raw,
                                                           int raw_w, int raw_h, int W, int H, uint8_t *__restrict__ dst, size_t dst_stride) {
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int segs = (int)(((long long)W + kWave - 1) / kWave);
  const long long item = (long long)blockIdx.x * kRectWaves + tid / kWave;
  if (item >= (long long)segs * H) return;
  const int y = (int)(item / segs);
  const long long xl = (item - (long long)y * segs) * kWave + lane;
  if (xl >= W) return;
  const int x = (int)xl;
  const long long n = (long long)W * H, i = (long long)y * W + x;
  uint32_t packed = 0u;  // an invalid pixel is (0, 0, 0)
  if (valid[i]) packed = rect_remap_pixel(raw, raw_w, raw_h, map[i], map[n + i]);
  uint8_t *o = dst + (size_t)y * dst_stride + 3 * (size_t)x;
  o[0] = (uint8_t)(packed & 255u);
  o[1] = (uint8_t)((packed >> 8) & 255u);
  o[2] = (uint8_t)((packed >> 16) & 255u);
}

}  // namespace cspm
