// cspm_synth.h -- view synthesis (include/cspm.h "view synthesis"): the specification N, one target row per
// workgroup.
//
// A rectified stereo warp never leaves its image row, so the depth test of the forward warp needs no global atomics and no waiting
// between workgroups: k_synth_row owns row y of the target and of both source views and resolves visibility in LDS.
//   pass 1  one lane per source pixel and view: the footprint's candidates d' -> atomicMax of the order-preserving 64-bit key
//           (f64_key) into the view's depth buffer in LDS
//   pass 2  the same candidates recomputed (the same function, the same bits): where the key equals the buffer's, atomicMin of
//           the source x into the view's winner buffer.  Max then min: the result is the rule "greatest d', then smallest x"
//           whatever the lane order.
//   pass 3  one lane per target pixel: the winners' xs, d' and colours recomputed from the winning source pixel, the merge, and
//           the merged pixel parked in LDS (its disparity over view 0's key, its rounded colour and mask over view 0's winner)
//   pass 4  the fill as a row scan: a wave takes 64 consecutive target pixels, a ballot of the non-holes gives the nearest
//           non-hole inside the chunk (clz / ctz), per-chunk first / last non-hole indices in LDS carry across chunks; then the
//           outputs, one pixel per lane, consecutive lanes on consecutive pixels.
// A row is not segmented: its LDS is kSynthLdsPerPixel bytes per pixel plus two ints per 64 pixels, which admits rows of up to
// kSynthMaxWidth pixels in the CU's 160 KiB; a 3000-pixel row takes 72 KiB (two workgroups per CU).  Wider images are refused by
// the entries (CSPM_ERR_ARG).
// Every product, sum and quotient is one IEEE f64 operation in the association the specification states (-ffp-contract=off, and
// the pragma below); `/` is correctly rounded on the device.
#pragma once
#include "cspm_device.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kSynthBlock = 256;  // lanes per workgroup: 4 waves
constexpr int kSynthWaves = kSynthBlock / kWave;
constexpr int kSynthLdsPerPixel = 24;  // per view a u64 depth key and an i32 winner
constexpr int kSynthMaxWidth = 6784;   // 106 chunks of 64: 24 * 6784 + 8 * 106 = 163664 <= 163840
inline size_t synth_lds_bytes(int W) { return (size_t)kSynthLdsPerPixel * W + 2 * sizeof(int) * ((W + kWave - 1) / kWave); }

struct SynthView {
  const double *disp;     // W*H
  const uint8_t *valid;   // W*H bytes or null: every pixel
  const double *a;        // W*H x-slopes or null: all 0
  const uint8_t *a_mask;  // W*H bytes or null: where 0 the slope is 0 (a filled pixel has no plane of its own)
  const uint32_t *pix;    // W*H packed B | G<<8 | R<<16 (k_pack_bgr)
};
struct SynthParams {
  double sigma[2];  // -t and 1 - t
  double w0, w1;    // 1 - t and t: the merge weights
  double max_stretch, merge_diff;
  int views, fill;
};
struct SynthOut {
  uint8_t *bgr;  // rows of `stride` bytes or null
  size_t stride;
  double *disp;   // W*H or null
  uint8_t *mask;  // W*H or null
};

// step 1 for one source pixel: whether it is used, and what its candidates are computed from
struct SynthSrc {
  double D, a, g, u, hi;
  int first;  // the first covered column (>= 0); W when the pixel is not used
};
__device__ __forceinline__ SynthSrc synth_src(const SynthView &v, double sigma, double max_stretch, int W, size_t row, int x) {
  const size_t i = row + (size_t)x;
  SynthSrc s;
  s.D = v.disp[i];
  const bool V = v.valid == nullptr || v.valid[i] != 0;
  double A = v.a ? v.a[i] : 0.0;
  if (v.a_mask != nullptr && v.a_mask[i] == 0) A = 0.0;
  s.a = fabs(A) <= kDoubleMax ? A : 0.0;  // finite: false for NaN and for +-inf
  s.g = 1.0 + sigma * s.a;
  s.u = (double)x + sigma * s.D;
  const double half = 0.5 * s.g;
  const double lo = s.u - half;
  s.hi = s.u + half;
  const bool used = V && fabs(s.D) <= kDoubleMax && s.D >= 0.0 && s.g > 0.0 && s.g <= max_stretch && lo <= (double)(W - 1);
  s.first = used ? (lo <= 0.0 ? 0 : (int)ceil(lo)) : W;
  return s;
}
// the source position and the disparity of source pixel x's plane at target column xp
__device__ __forceinline__ void synth_at(const SynthSrc &s, int x, int xp, double &xs, double &dp) {
  xs = (double)x + ((double)xp - s.u) / s.g;
  dp = s.D + s.a * (xs - (double)x);
}

__global__ __launch_bounds__(kSynthBlock) void k_synth_row(SynthView v0, SynthView v1, SynthParams p, SynthOut out, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char synth_smem[];
  unsigned long long *key0 = reinterpret_cast<unsigned long long *>(synth_smem);
  unsigned long long *key1 = key0 + W;
  int *win0 = reinterpret_cast<int *>(key1 + W);
  int *win1 = win0 + W;
  int *s_last = win1 + W;
  const int nchunk = (W + kWave - 1) / kWave;
  int *s_first = s_last + nchunk;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int y = (int)blockIdx.x;
  const size_t row = (size_t)y * W;
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);

  for (int x = tid; x < W; x += kSynthBlock) {
    key0[x] = 0ull;  // below the key of every candidate: a candidate is never NaN
    key1[x] = 0ull;
    win0[x] = 0x7FFFFFFF;
    win1[x] = 0x7FFFFFFF;
  }
  __syncthreads();
  // pass 1 (max of d') and pass 2 (min of x among the winners)
  for (int pass = 0; pass < 2; ++pass) {
    for (int v = 0; v < 2; ++v) {
      if (!(p.views >> v & 1)) continue;
      const SynthView &sv = v ? v1 : v0;
      unsigned long long *key = v ? key1 : key0;
      int *win = v ? win1 : win0;
      for (int x = tid; x < W; x += kSynthBlock) {
        const SynthSrc s = synth_src(sv, p.sigma[v], p.max_stretch, W, row, x);
        for (int xp = s.first; xp < W && (double)xp < s.hi; ++xp) {
          double xs, dp;
          synth_at(s, x, xp, xs, dp);
          const unsigned long long k = f64_key(dp);
          if (pass == 0) atomicMax(&key[xp], k);
          else if (key[xp] == k) atomicMin(&win[xp], x);
        }
      }
    }
    __syncthreads();
  }
  // pass 3: colours and the merge, one lane per target pixel
  for (int xp = tid; xp < W; xp += kSynthBlock) {
    double Z[2] = {0.0, 0.0}, C[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    bool have[2] = {false, false};
    for (int v = 0; v < 2; ++v) {
      const int x = v ? win1[xp] : win0[xp];
      if (x == 0x7FFFFFFF) continue;
      const SynthView &sv = v ? v1 : v0;
      const SynthSrc s = synth_src(sv, p.sigma[v], p.max_stretch, W, row, x);
      double xs;
      synth_at(s, x, xp, xs, Z[v]);
      const double fl = floor(xs);
      const double f = xs - fl;
      const double wm = (double)(W - 1);  // clamped as doubles: xs stays within a few thousand pixels of x, but nothing relies on it
      const int ia = (int)fmin(fmax(fl, 0.0), wm), ib = (int)fmin(fmax(fl + 1.0, 0.0), wm);
      const uint32_t pa = sv.pix[row + (size_t)ia], pb = sv.pix[row + (size_t)ib];
      const double fa = 1.0 - f;
      for (int ch = 0; ch < 3; ++ch) C[v][ch] = fa * (double)((pa >> (8 * ch)) & 255u) + f * (double)((pb >> (8 * ch)) & 255u);
      have[v] = true;
    }
    int m = 0, pick = 0;
    if (have[0] && have[1]) {
      if (fabs(Z[0] - Z[1]) <= p.merge_diff) m = 3;
      else if (Z[0] >= Z[1]) m = 1;
      else { m = 2; pick = 1; }
    } else if (have[0]) m = 1;
    else if (have[1]) { m = 2; pick = 1; }
    double Zm = kNaN;
    uint32_t packed = 0u;
    if (m != 0) {
      Zm = m == 3 ? p.w0 * Z[0] + p.w1 * Z[1] : Z[pick];
      for (int ch = 0; ch < 3; ++ch) {
        const double c = m == 3 ? p.w0 * C[0][ch] + p.w1 * C[1][ch] : C[pick][ch];
        packed |= (uint32_t)min(max(round2int(c), 0), 255) << (8 * ch);
      }
      packed |= (uint32_t)m << 24;
    }
    key0[xp] = (unsigned long long)__double_as_longlong(Zm);
    win0[xp] = (int)packed;
  }
  __syncthreads();
  // pass 4: the fill's chunk summaries (first and last non-hole of every 64 target pixels), then the outputs
  if (p.fill) {
    for (int ch = wave; ch < nchunk; ch += kSynthWaves) {
      const int xp = ch * kWave + lane;
      const unsigned long long b = __ballot(xp < W && ((uint32_t)win0[min(xp, W - 1)] >> 24) != 0u);
      if (lane == 0) {
        s_last[ch] = b ? ch * kWave + 63 - __clzll((long long)b) : -1;
        s_first[ch] = b ? ch * kWave + __ffsll((unsigned long long)b) - 1 : -1;
      }
    }
    __syncthreads();
  }
  for (int ch = wave; ch < nchunk; ch += kSynthWaves) {
    const int xp = ch * kWave + lane;
    const uint32_t own = (uint32_t)win0[min(xp, W - 1)];
    const unsigned long long b = __ballot(xp < W && (own >> 24) != 0u);
    if (xp >= W) continue;  // the chunk loop is uniform over the wave and nothing below votes
    uint32_t px = own;
    double Zo = __longlong_as_double((long long)key0[xp]);
    if ((own >> 24) == 0u && p.fill) {
      const unsigned long long below = b & ((1ull << lane) - 1ull);
      const unsigned long long above = lane == kWave - 1 ? 0ull : b & ~((2ull << lane) - 1ull);
      int L = -1, R = -1;
      if (below) L = ch * kWave + 63 - __clzll((long long)below);
      else for (int c = ch - 1; c >= 0 && L < 0; --c) L = s_last[c];
      if (above) R = ch * kWave + __ffsll(above) - 1;
      else for (int c = ch + 1; c < nchunk && R < 0; ++c) R = s_first[c];
      int src = L;
      if (L < 0) src = R;
      else if (R >= 0 && __longlong_as_double((long long)key0[R]) < __longlong_as_double((long long)key0[L])) src = R;
      if (src >= 0) {
        px = ((uint32_t)win0[src] & 0x00FFFFFFu) | (4u << 24);
        Zo = __longlong_as_double((long long)key0[src]);
      }
    }
    if (out.bgr) {
      uint8_t *o = out.bgr + (size_t)y * out.stride + (size_t)xp * 3;
      o[0] = (uint8_t)(px & 255u);
      o[1] = (uint8_t)((px >> 8) & 255u);
      o[2] = (uint8_t)((px >> 16) & 255u);
    }
    if (out.disp) out.disp[row + (size_t)xp] = Zo;
    if (out.mask) out.mask[row + (size_t)xp] = (uint8_t)(px >> 24);
  }
}

}  // namespace cspm
