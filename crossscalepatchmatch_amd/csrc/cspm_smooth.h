// cspm_smooth.h -- edge-aware global smoothing of an f64 disparity map (an addition; include/cspm.h "smoothing"):
// the fast global smoother, S(D, C, I, lambda, sigma, T, max_dis) -> O.  Numerators N = c * D and denominators M = c are diffused by T
// rounds of a horizontal and a vertical pass; a pass solves, per image line, one tridiagonal system with the two right-hand sides by the
// Thomas recurrence in the order the specification writes down, and O = N / M.
//
//   k_smooth_init    N, M from D and the confidences (a map, a consistency mask with fill_conf, or all 1)
//   k_smooth_cols    the vertical pass: one LANE per column, consecutive lanes = consecutive columns, so every load and store of the sweep
//                    is coalesced as it stands.  Rows are taken kSmBatch at a time: the batch's loads are issued together, then the
//                    dependent chain runs on registers.
//   k_smooth_rows    the horizontal pass: one LANE per row, a single-wave workgroup owns kSmRows rows and walks x in chunks of kSmChunk
//                    columns.  A chunk of N, M and the weights (forward) or ct (backward) is loaded coalesced -- half a wave per row
//                    segment -- into LDS tiles, the lanes run their recurrences on the tiles, and the tiles are stored the same way.  A
//                    tile row is kSmStride = kSmChunk + 1 doubles: odd, so the per-lane ds_read_b64 (banks (a/4) mod 64, 32-lane groups)
//                    and ds_write_b64 ((a/4) mod 32, 16-lane groups) of lane l at l * kSmStride + i touch every bank pair once, and
//                    the coalesced side is consecutive doubles whatever the stride.
//   k_smooth_finish  O = N / M where M > 0, clamped; elsewhere D's own bits
//
// Both views and both right-hand sides share a launch; ct and the reciprocal are shared between the right-hand sides.  The forward sweep
// leaves ft in N and M and ct in a scratch plane, the backward sweep reads them back.  The guide weights come from the 766-entry
// exp(-k / sigma) table (host libm, staged in LDS) inside the sweep; nothing is materialised per pass.  One true division per element;
// every product, sum and difference rounded on its own (-ffp-contract=off, and the pragma below).  No atomics, nothing waits for another
// workgroup.  Bandwidth does not bound these kernels; the dependent chain and, in the row pass, the tile transfers that the same wave
// issues without overlapping them with the chain do (8.4 ms per 1242x375 pair at T = 3).
#pragma once
#include "cspm_kernels.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kSmLut = 766;                  // |dB| + |dG| + |dR| = 0 .. 765
constexpr int kSmRows = 64;                  // rows of a workgroup of the horizontal pass: one lane each
constexpr int kSmChunk = 32;                 // columns of a chunk
constexpr int kSmStride = kSmChunk + 1;      // doubles per tile row: odd (see above)
constexpr int kSmTile = kSmRows * kSmStride; // doubles per tile
constexpr int kSmBatch = 8;                  // rows of the vertical pass whose loads are in flight together
constexpr int kSmMaxIters = 8;

struct SmoothView {
  double *N, *M, *ct;   // W*H each; N and M hold ft between the two sweeps of a pass
  const uint32_t *pix;  // packed B | G<<8 | R<<16 (k_pack_bgr), rows Wp apart, first pixel at pad; not read without a guide
};
struct SmoothPair {
  SmoothView v[2];
  int Wp, pad;
};

// c[p] per view: a confidence map (conf), or 1.0 / fill_conf by a consistency mask (ok), or all 1 (both null)
struct SmoothConf {
  const double *conf[2];
  const uint8_t *ok[2];
  double fill_conf;
};

__global__ void k_smooth_init(const double *__restrict__ d0, const double *__restrict__ d1, SmoothConf cf, SmoothPair s, long long n, int views) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * views) return;
  const int v = i >= n ? 1 : 0;
  const long long p = i - v * n;
  const double d = (v ? d1 : d0)[p];
  double c = 1.0;
  if (cf.conf[v]) c = cf.conf[v][p];
  else if (cf.ok[v]) c = cf.ok[v][p] != 0 ? 1.0 : cf.fill_conf;
  const bool node = fabs(d) <= kDoubleMax;  // finite: false for NaN and for +-inf
  s.v[v].N[p] = node ? c * d : 0.0;
  s.v[v].M[p] = node ? c : 0.0;
}

__global__ void k_smooth_finish(double *__restrict__ d0, double *__restrict__ d1, SmoothPair s, long long n, int views, double max_dis) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * views) return;
  const int v = i >= n ? 1 : 0;
  const long long p = i - v * n;
  const double m = s.v[v].M[p];
  if (!(m > 0.0)) return;  // also a NaN: D keeps its bits
  double z = s.v[v].N[p] / m;
  if (max_dis > 0.0) {
    z = z > 0.0 ? z : 0.0;
    z = z < max_dis ? z : max_dis;
  }
  (v ? d1 : d0)[p] = z;
}

// what a lane carries from element i-1 to element i of the forward sweep (all 0.0 in front of the line: with a = 0.0 the general step
// then is the specification's first step bit for bit) and from i+1 to i of the backward sweep
struct SmCarry {
  double ct, fn, fm;
};
// forward step: fn / fm come in as F[i] of the two right-hand sides and leave as ft[i]; returns ct[i]
__device__ __forceinline__ double sm_forward(double lam, double wl, double wr, bool first, bool last, double &fn, double &fm, SmCarry &k) {
  const double a = first ? 0.0 : -(lam * wl);
  const double cc = last ? 0.0 : -(lam * wr);
  const double b = (1.0 - a) - cc;
  const double r = 1.0 / (b - k.ct * a);
  k.ct = cc * r;
  k.fn = (fn - k.fn * a) * r;
  k.fm = (fm - k.fm * a) * r;
  fn = k.fn;
  fm = k.fm;
  return k.ct;
}
// backward step: U[i] = ft[i] - ct[i] * U[i+1]; behind the line U = 0.0 and ct[n-1] = 0.0 * r = 0.0, so U[n-1] = ft[n-1] - 0.0
__device__ __forceinline__ void sm_backward(double ct, double &fn, double &fm, SmCarry &k) {
  k.fn = fn - ct * k.fn;
  k.fm = fm - ct * k.fm;
  fn = k.fn;
  fm = k.fm;
}

__device__ __forceinline__ int sm_sad(uint32_t p, uint32_t q) { return (int)__builtin_amdgcn_sad_u8(p & 0xFFFFFFu, q & 0xFFFFFFu, 0u); }

// The vertical pass.  grid (ceil(W / 64), views), 64 lanes.
template <bool GUIDE>
__global__ __launch_bounds__(kWave) void k_smooth_cols(SmoothPair s, int W, int H, double lam, const double *__restrict__ lut) {
  __shared__ double s_lut[GUIDE ? kSmLut : 1];
  const int lane = (int)threadIdx.x;
  if (GUIDE) {
    for (int t = lane; t < kSmLut; t += kWave) s_lut[t] = lut[t];
    __syncthreads();
  }
  const int x = (int)blockIdx.x * kWave + lane;
  if (x >= W) return;
  const SmoothView V = s.v[blockIdx.y];
  const uint32_t *pix = GUIDE ? V.pix + s.pad + x : nullptr;
  double *N = V.N + x, *M = V.M + x, *ct = V.ct + x;

  SmCarry k{0.0, 0.0, 0.0};
  double wl = 1.0;
  for (int y0 = 0; y0 < H; y0 += kSmBatch) {
    double fn[kSmBatch], fm[kSmBatch], wr[kSmBatch];
#pragma unroll
    for (int j = 0; j < kSmBatch; ++j) {
      const int y = y0 + j;
      fn[j] = fm[j] = 0.0;
      wr[j] = 1.0;
      if (y < H) {
        fn[j] = N[(size_t)y * W];
        fm[j] = M[(size_t)y * W];
        if (GUIDE && y + 1 < H) wr[j] = s_lut[sm_sad(pix[(size_t)y * s.Wp], pix[(size_t)(y + 1) * s.Wp])];
      }
    }
#pragma unroll
    for (int j = 0; j < kSmBatch; ++j) {
      const int y = y0 + j;
      if (y < H) {
        const double c = sm_forward(lam, wl, wr[j], y == 0, y == H - 1, fn[j], fm[j], k);
        wl = wr[j];
        N[(size_t)y * W] = fn[j];
        M[(size_t)y * W] = fm[j];
        ct[(size_t)y * W] = c;
      }
    }
  }

  k = SmCarry{0.0, 0.0, 0.0};
  for (int y1 = H - 1; y1 >= 0; y1 -= kSmBatch) {
    double fn[kSmBatch], fm[kSmBatch], c[kSmBatch];
#pragma unroll
    for (int j = 0; j < kSmBatch; ++j) {
      const int y = y1 - j;
      fn[j] = fm[j] = c[j] = 0.0;
      if (y >= 0) {
        fn[j] = N[(size_t)y * W];
        fm[j] = M[(size_t)y * W];
        c[j] = ct[(size_t)y * W];
      }
    }
#pragma unroll
    for (int j = 0; j < kSmBatch; ++j) {
      const int y = y1 - j;
      if (y >= 0) {
        sm_backward(c[j], fn[j], fm[j], k);
        N[(size_t)y * W] = fn[j];
        M[(size_t)y * W] = fm[j];
      }
    }
  }
}

// a chunk between global memory and an LDS tile, coalesced: element t of the chunk is (row t / kSmChunk, column t % kSmChunk)
__device__ __forceinline__ void sm_tile_load(double *tile, const double *__restrict__ g, int W, int H, int y0, int x0, int lane) {
#pragma unroll 8
  for (int t = lane; t < kSmRows * kSmChunk; t += kWave) {
    const int r = t / kSmChunk, i = t - r * kSmChunk;
    const int y = y0 + r, x = x0 + i;
    if (y < H && x < W) tile[r * kSmStride + i] = g[(size_t)y * W + x];
  }
}
__device__ __forceinline__ void sm_tile_store(const double *tile, double *__restrict__ g, int W, int H, int y0, int x0, int lane) {
#pragma unroll 8
  for (int t = lane; t < kSmRows * kSmChunk; t += kWave) {
    const int r = t / kSmChunk, i = t - r * kSmChunk;
    const int y = y0 + r, x = x0 + i;
    if (y < H && x < W) g[(size_t)y * W + x] = tile[r * kSmStride + i];
  }
}

// The horizontal pass.  grid (ceil(H / kSmRows), views), 64 lanes; lane l owns row blockIdx.x * kSmRows + l.
template <bool GUIDE>
__global__ __launch_bounds__(kWave) void k_smooth_rows(SmoothPair s, int W, int H, double lam, const double *__restrict__ lut) {
  __shared__ double s_n[kSmTile], s_m[kSmTile], s_c[kSmTile];  // s_c: the weights to the right neighbour, then ct
  __shared__ double s_lut[GUIDE ? kSmLut : 1];
  const int lane = (int)threadIdx.x;
  const int y0 = (int)blockIdx.x * kSmRows;
  const bool live = y0 + lane < H;
  const SmoothView V = s.v[blockIdx.y];
  if (GUIDE)
    for (int t = lane; t < kSmLut; t += kWave) s_lut[t] = lut[t];
  const int base = lane * kSmStride;

  SmCarry k{0.0, 0.0, 0.0};
  double wl = 1.0;
  for (int x0 = 0; x0 < W; x0 += kSmChunk) {
    const int cw = min(kSmChunk, W - x0);
    __syncthreads();  // the previous chunk's tiles are stored (and the table is staged)
    sm_tile_load(s_n, V.N, W, H, y0, x0, lane);
    sm_tile_load(s_m, V.M, W, H, y0, x0, lane);
    if (GUIDE) {
#pragma unroll 8
      for (int t = lane; t < kSmRows * kSmChunk; t += kWave) {
        const int r = t / kSmChunk, i = t - r * kSmChunk;
        const int y = y0 + r, x = x0 + i;
        if (y < H && x + 1 < W) {
          const uint32_t *p = V.pix + (size_t)y * s.Wp + s.pad + x;
          s_c[r * kSmStride + i] = s_lut[sm_sad(p[0], p[1])];
        }
      }
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < cw; ++i) {
        const int x = x0 + i;
        const bool last = x == W - 1;
        const double wr = GUIDE && !last ? s_c[base + i] : 1.0;
        double fn = s_n[base + i], fm = s_m[base + i];
        s_c[base + i] = sm_forward(lam, wl, wr, x == 0, last, fn, fm, k);
        wl = wr;
        s_n[base + i] = fn;
        s_m[base + i] = fm;
      }
    }
    __syncthreads();
    sm_tile_store(s_n, V.N, W, H, y0, x0, lane);
    sm_tile_store(s_m, V.M, W, H, y0, x0, lane);
    sm_tile_store(s_c, V.ct, W, H, y0, x0, lane);
  }

  k = SmCarry{0.0, 0.0, 0.0};
  for (int x0 = (W - 1) / kSmChunk * kSmChunk; x0 >= 0; x0 -= kSmChunk) {
    const int cw = min(kSmChunk, W - x0);
    __syncthreads();
    sm_tile_load(s_n, V.N, W, H, y0, x0, lane);
    sm_tile_load(s_m, V.M, W, H, y0, x0, lane);
    sm_tile_load(s_c, V.ct, W, H, y0, x0, lane);
    __syncthreads();
    if (live) {
      for (int i = cw - 1; i >= 0; --i) {
        double fn = s_n[base + i], fm = s_m[base + i];
        sm_backward(s_c[base + i], fn, fm, k);
        s_n[base + i] = fn;
        s_m[base + i] = fm;
      }
    }
    __syncthreads();
    sm_tile_store(s_n, V.N, W, H, y0, x0, lane);
    sm_tile_store(s_m, V.M, W, H, y0, x0, lane);
  }
}

}  // namespace cspm
