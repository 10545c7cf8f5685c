// cspm_seg.h -- superpixel segment planes (include/cspm.h "segment planes"): the grid SLIC
// S(I, s, m, T) -> labels and the robust per-segment plane fit P(D, V, labels, s, max_dis, tau, R, min_support).  Everything whose result
// depends on the order of a reduction is an int64 sum, so lanes and waves may add in any order and the result is the specification's.
//
// k_seg_init: one lane per segment; the centre is the home cell's middle pixel (clamped to the image), 16 * its position and colour.
//
// k_seg_assign: one LANE per pixel, a workgroup per tile of kSegTileW x kSegTileH pixels, lanes along x.  The centres of the cells
// that touch the tile, plus one cell all round, are staged into LDS once: at most (63/s + 2 + 2) x (3/s + 2 + 2) <= 19 x 4 = 76 centres
// of five ints at the smallest step 4 (1520 bytes: the wave limit binds, not LDS).  A lane then takes its up-to-nine integer distances
// from LDS -- lanes of one cell read the same words (a broadcast) -- and writes its label.  No atomics, nothing waits for anything.
//
// k_seg_update and k_seg_fit: a segment's members lie in the 3s x 3s pixels around its home cell (the 3 x 3 property), so a GROUP of
// lanes OWNS a segment, scans that window (clipped to the image) with its lanes along x and reduces its private int64 sums: first
// across the 64 lanes of a wave by shuffles, then, through kSegWaves x 9 int64 words of LDS (288 bytes), across the waves of the group.
// The group is one wave (four segments per workgroup) up to kSegWaveStep and the whole workgroup of four waves above it, where a
// window holds up to 192 x 192 pixels.  The group's first lane finishes: the rounded centre update, or the 3 x 3 solve by cofactors
// under fp contract(off).  No global atomics, no zeroing pass, nothing waits for another workgroup; a segment's record is written by its
// owner alone.  k_seg_fit runs its R + 1 rounds in one launch: the owner publishes the round's plane and a go flag through LDS (24 + 4
// bytes per group), two workgroup barriers per round, the same count for every lane (a finished or absent segment scans nothing but
// still meets the barriers).
//
// k_seg_scatter: one lane per pixel reads its label's plane and writes the six plane doubles and `fitted`, into a candidate buffer
// (unfitted: six NaNs) or into a stored field (unfitted: left as it is) -- FitOut's keep_unfitted, as in cspm_fit.h.
#pragma once
#include "cspm_device.h"
#include "cspm_fit.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kSegTileW = 64, kSegTileH = 4, kSegBlock = kSegTileW * kSegTileH;
constexpr int kSegMinStep = 4, kSegMaxStep = 64;
constexpr int kSegStage = ((kSegTileW - 1) / kSegMinStep + 4) * ((kSegTileH - 1) / kSegMinStep + 4);  // 19 x 4 centres
constexpr int kSegWaves = kSegBlock / kWave;
constexpr int kSegWaveStep = 16;       // up to this step a wave owns a segment, above it a workgroup
constexpr double kSegMaxAbsD = 32768.0;  // a node's |D| bound: q = llrint(D * 65536) stays within 2^31

struct SegGrid {
  int W, H, s, nx, ny;
};
inline int seg_per_block(int s) { return s <= kSegWaveStep ? kSegWaves : 1; }

__global__ void k_seg_init(SegGrid g, const uint32_t *__restrict__ pix, int *__restrict__ cen) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= g.nx * g.ny) return;
  const int gy = k / g.nx, gx = k - gy * g.nx;
  const int x = min(g.W - 1, gx * g.s + g.s / 2), y = min(g.H - 1, gy * g.s + g.s / 2);
  const uint32_t p = pix[(long long)y * g.W + x];
  int *c = cen + 5LL * k;
  c[0] = 16 * x;
  c[1] = 16 * y;
  c[2] = 16 * (int)(p & 0xFFu);
  c[3] = 16 * (int)((p >> 8) & 0xFFu);
  c[4] = 16 * (int)((p >> 16) & 0xFFu);
}

__global__ __launch_bounds__(kSegBlock) void k_seg_assign(SegGrid g, const uint32_t *__restrict__ pix, const int *__restrict__ cen, int m,
                                                          int *__restrict__ labels) {
  __shared__ int sC[kSegStage * 5];
  const int tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kSegTileW, y0 = (int)blockIdx.y * kSegTileH;
  const int x1 = min(x0 + kSegTileW, g.W) - 1, y1 = min(y0 + kSegTileH, g.H) - 1;
  const int cx0 = max(0, x0 / g.s - 1), cx1 = min(g.nx - 1, x1 / g.s + 1);
  const int cy0 = max(0, y0 / g.s - 1), cy1 = min(g.ny - 1, y1 / g.s + 1);
  const int ncx = cx1 - cx0 + 1, ncy = cy1 - cy0 + 1;
  const int words = min(ncx * ncy, kSegStage) * 5;  // ncx * ncy <= kSegStage for every step >= kSegMinStep
  for (int t = tid; t < words; t += kSegBlock) {
    const int cell = t / 5, comp = t - cell * 5;
    const int cy = cell / ncx, cx = cell - cy * ncx;
    sC[t] = cen[5LL * ((long long)(cy0 + cy) * g.nx + cx0 + cx) + comp];
  }
  __syncthreads();
  const int x = x0 + tid % kSegTileW, y = y0 + tid / kSegTileW;
  if (x >= g.W || y >= g.H) return;
  const long long i = (long long)y * g.W + x;
  const uint32_t p = pix[i];
  const long long B = 16 * (long long)(p & 0xFFu), G = 16 * (long long)((p >> 8) & 0xFFu), R = 16 * (long long)((p >> 16) & 0xFFu);
  const long long X = 16LL * x, Y = 16LL * y;
  const long long ss = (long long)g.s * g.s, mm = (long long)m * m;
  const int hx = min(g.nx - 1, x / g.s), hy = min(g.ny - 1, y / g.s);
  long long best = 0x7FFFFFFFFFFFFFFFLL;
  int lab = hy * g.nx + hx;
  for (int gy = hy - 1; gy <= hy + 1; ++gy) {
    if (gy < 0 || gy >= g.ny) continue;
    for (int gx = hx - 1; gx <= hx + 1; ++gx) {
      if (gx < 0 || gx >= g.nx) continue;
      const int *c = sC + ((gy - cy0) * ncx + (gx - cx0)) * 5;
      const long long dx = X - c[0], dy = Y - c[1], db = B - c[2], dg = G - c[3], dr = R - c[4];
      const long long dist = (db * db + dg * dg + dr * dr) * ss + (dx * dx + dy * dy) * mm;
      if (dist < best) {  // the first candidate with the strictly smallest Dist
        best = dist;
        lab = gy * g.nx + gx;
      }
    }
  }
  labels[i] = lab;
}

// a group's sums: v[] summed over the wave by shuffles; lane 0 of every wave leaves its totals in part[wave][NV]; one barrier
template <int NV>
__device__ __forceinline__ void seg_reduce(long long (&v)[NV], long long *part, int tid) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += __shfl_down(v[i], off, kWave);
  if ((tid & (kWave - 1)) == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) part[(tid / kWave) * NV + i] = v[i];
  __syncthreads();
}
// ... and what the group's first lane reads back: its own wave's totals, or all waves' when the workgroup is the group
template <int NV>
__device__ __forceinline__ void seg_totals(long long (&v)[NV], const long long *part, int slot, int per_block) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (per_block == 1) {
      long long t = 0;
      for (int w = 0; w < kSegWaves; ++w) t += part[w * NV + i];
      v[i] = t;
    } else {
      v[i] = part[slot * NV + i];
    }
  }
}

// the window of segment k clipped to the image: [wx0, wx0 + ww) x [wy0, wy0 + wh); empty for k >= K
struct SegWin {
  int wx0, wy0, ww, wh;
};
__device__ __forceinline__ SegWin seg_window(const SegGrid &g, int k) {
  SegWin w{0, 0, 0, 0};
  if (k >= g.nx * g.ny) return w;
  const int gy = k / g.nx, gx = k - gy * g.nx;
  const int ox = gx * g.s, oy = gy * g.s;
  w.wx0 = max(0, ox - g.s);
  w.wy0 = max(0, oy - g.s);
  w.ww = min(g.W, ox + 2 * g.s) - w.wx0;
  w.wh = min(g.H, oy + 2 * g.s) - w.wy0;
  return w;
}

__global__ __launch_bounds__(kSegBlock) void k_seg_update(SegGrid g, const uint32_t *__restrict__ pix, const int *__restrict__ labels, int *__restrict__ cen,
                                                          int *__restrict__ counts, int per_block) {
  __shared__ long long part[kSegWaves * 6];
  const int tid = (int)threadIdx.x;
  const int gl = kSegBlock / per_block, slot = tid / gl, li = tid - slot * gl;
  const int k = (int)blockIdx.x * per_block + slot;
  const SegWin w = seg_window(g, k);
  long long v[6] = {0, 0, 0, 0, 0, 0};  // n, sums of x, y, B, G, R
  for (int t = li; t < w.ww * w.wh; t += gl) {
    const int ry = t / w.ww, x = w.wx0 + (t - ry * w.ww), y = w.wy0 + ry;
    const long long i = (long long)y * g.W + x;
    if (labels[i] == k) {
      const uint32_t p = pix[i];
      v[0] += 1;
      v[1] += x;
      v[2] += y;
      v[3] += (long long)(p & 0xFFu);
      v[4] += (long long)((p >> 8) & 0xFFu);
      v[5] += (long long)((p >> 16) & 0xFFu);
    }
  }
  seg_reduce<6>(v, part, tid);
  if (li != 0 || k >= g.nx * g.ny) return;
  seg_totals<6>(v, part, slot, per_block);
  const long long n = v[0];
  counts[k] = (int)n;
  if (n > 0)  // (2 * Sum + n) / (2 * n) with Sum = 16 * the members' sum; an empty segment keeps its centre
    for (int j = 0; j < 5; ++j) cen[5LL * k + j] = (int)((2 * 16 * v[1 + j] + n) / (2 * n));
}

struct SegFitIn {
  const double *disp;    // W*H
  const uint8_t *valid;  // W*H bytes, or null: every pixel
  const int *labels;     // W*H, obeying the 3 x 3 property
};

// segplane: K records of four doubles (a, b, c0, c), NaN for an unfitted segment; inliers: K ints, 0 for an unfitted segment
__global__ __launch_bounds__(kSegBlock) void k_seg_fit(SegGrid g, SegFitIn in, double tau, int R, int min_support, double *__restrict__ segplane,
                                                       int *__restrict__ inliers, int per_block) {
  __shared__ long long part[kSegWaves * 9];
  __shared__ double s_pl[kSegWaves * 3];
  __shared__ int s_go[kSegWaves];
  const int tid = (int)threadIdx.x;
  const int gl = kSegBlock / per_block, slot = tid / gl, li = tid - slot * gl;
  const int k = (int)blockIdx.x * per_block + slot;
  const bool exists = k < g.nx * g.ny;
  const SegWin w = seg_window(g, k);
  const int ox = exists ? (k % g.nx) * g.s : 0, oy = exists ? (k / g.nx) * g.s : 0;
  double a = 0.0, b = 0.0, c0 = 0.0;  // the owner's: the plane so far
  int n_in = 0;
  bool fitted = false;
  for (int r = 0; r <= R; ++r) {
    const bool go = r == 0 ? exists : s_go[slot] != 0;
    double pa = 0.0, pb = 0.0, pc = 0.0, thr = 0.0;
    if (r > 0 && go) {
      pa = s_pl[slot * 3];
      pb = s_pl[slot * 3 + 1];
      pc = s_pl[slot * 3 + 2];
      thr = tau * (double)(1 << (R - r));
    }
    long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // Sw, Su, Sv, Suu, Suv, Svv, Se, Sue, Sve
    if (go)
      for (int t = li; t < w.ww * w.wh; t += gl) {
        const int ry = t / w.ww, x = w.wx0 + (t - ry * w.ww), y = w.wy0 + ry;
        const long long i = (long long)y * g.W + x;
        if (in.labels[i] != k) continue;
        const double D = in.disp[i];
        if (!((in.valid == nullptr || in.valid[i] != 0) && fabs(D) <= kSegMaxAbsD)) continue;  // not a node (false for NaN and inf)
        const long long u = x - ox, vv = y - oy;
        if (r > 0) {
          const double t0 = (pa * (double)u + pb * (double)vv) + pc;
          if (!(fabs(D - t0) <= thr)) continue;
        }
        const long long q = llrint(D * 65536.0);
        v[0] += 1;
        v[1] += u;
        v[2] += vv;
        v[3] += u * u;
        v[4] += u * vv;
        v[5] += vv * vv;
        v[6] += q;
        v[7] += u * q;
        v[8] += vv * q;
      }
    seg_reduce<9>(v, part, tid);
    if (li == 0) {
      int next = 0;
      if (go) {
        seg_totals<9>(v, part, slot, per_block);
        const double Sw = (double)v[0], Su = (double)v[1], Sv = (double)v[2], Suu = (double)v[3], Suv = (double)v[4], Svv = (double)v[5];
        const double Se = (double)v[6], Sue = (double)v[7], Sve = (double)v[8];
        const double C00 = Svv * Sw - Sv * Sv;
        const double C01 = Suv * Sw - Sv * Su;
        const double C02 = Suv * Sv - Svv * Su;
        const double C11 = Suu * Sw - Su * Su;
        const double C12 = Suu * Sv - Suv * Su;
        const double C22 = Suu * Svv - Suv * Suv;
        const double det = (Suu * C00 - Suv * C01) + Su * C02;
        if (v[0] >= (long long)min_support && det > 1e-6 * ((Suu * Svv) * Sw)) {
          const double scale = 1.0 / 65536.0;  // exact
          a = (((C00 * Sue - C01 * Sve) + C02 * Se) / det) * scale;
          b = (((C11 * Sve - C01 * Sue) - C12 * Se) / det) * scale;
          c0 = (((C02 * Sue - C12 * Sve) + C22 * Se) / det) * scale;
          n_in = (int)v[0];
          fitted = true;
          next = 1;
          s_pl[slot * 3] = a;
          s_pl[slot * 3 + 1] = b;
          s_pl[slot * 3 + 2] = c0;
        }
      }
      s_go[slot] = next;  // a degenerate round ends the segment's rounds; the plane so far stays
    }
    __syncthreads();
  }
  if (li != 0 || !exists) return;
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  double *o = segplane + 4LL * k;
  o[0] = fitted ? a : kNaN;
  o[1] = fitted ? b : kNaN;
  o[2] = fitted ? c0 : kNaN;
  o[3] = fitted ? (c0 - a * (double)ox) - b * (double)oy : kNaN;
  inliers[k] = fitted ? n_in : 0;
}

__global__ void k_seg_scatter(SegGrid g, const int *__restrict__ labels, const double *__restrict__ segplane, const int *__restrict__ inliers,
                              double max_dis, FitOut out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)g.W * g.H) return;
  const int y = (int)(i / g.W), x = (int)(i - (long long)y * g.W);
  const int k = labels[i];
  if (inliers[k] <= 0) {  // an unfitted segment: no candidate
    if (!out.keep_unfitted) {
      const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
      out.nx[i] = kNaN; out.ny[i] = kNaN; out.nz[i] = kNaN;
      out.a[i] = kNaN; out.b[i] = kNaN; out.c[i] = kNaN;
    }
    if (out.fitted) out.fitted[i] = 0;
    return;
  }
  const int gy = k / g.nx, gx = k - gy * g.nx;
  const double u = (double)(x - gx * g.s), v = (double)(y - gy * g.s);
  const double a = segplane[4LL * k], b = segplane[4LL * k + 1], c0 = segplane[4LL * k + 2];
  const double t = (a * u + b * v) + c0;
  double z = t > 0.0 ? t : 0.0;
  z = z < max_dis ? z : max_dis;
  const double m0 = -a, m1 = -b, m2 = 1.0;
  double s = m0 * m0;  // the norm as the per-pixel fit takes it (k_fit_planes)
  s += m1 * m1;
  s += m2 * m2;
  const double inv = 1. / fmax(__dsqrt_rn(s), kDoubleEps);
  const double nx = m0 * inv, ny = m1 * inv, nz = m2 * inv;
  double pa, pb, pc;
  plane_param(nx, ny, nz, (double)x, (double)y, z, pa, pb, pc);
  out.nx[i] = nx; out.ny[i] = ny; out.nz[i] = nz;
  out.a[i] = pa; out.b[i] = pb; out.c[i] = pc;
  if (out.fitted) out.fitted[i] = 1;
}

}  // namespace cspm
