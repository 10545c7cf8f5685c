// cspm_carry.h -- a plane field carried across a rigid motion into another camera's disparity space and pixel grid, visibility resolved
// (include/cspm.h "plane-field carry"): the specification C, one pixel at a time.
//
// carry_plane() is steps 4 and 5 of C (the plane in the target's disparity space: it depends on the source plane alone, not on the
// pixel), carry_pixel() steps 1 to 6 for one source pixel.  Every kernel that needs either calls these two, so the key a pixel wrote,
// the key it compares with and the record the resolve writes cannot differ by a bit.  The two-pass scheme cspm_synth.h runs in LDS, in
// global memory, because a target pixel's contenders come from anywhere in the source:
//   k_carry_splat<0>  one LANE per source pixel in flat raster order.  A contender does a 64-bit atomicMin of the bit pattern of its
//                     depth Q[2] on key[g]: a positive finite double orders as its bits.
//   k_carry_splat<1>  the same function gives the same bits; where key[g] equals them, a 32-bit atomicMin of m on win[g].  The launch
//                     boundary is what orders it behind every key of pass 0: nothing waits for another workgroup.
//   k_carry_resolve   one LANE per target pixel: the plane of its own winner or, for the fill, of the winners of its four neighbours,
//                     recomputed from the source plane (three 8-byte gathers each), then the record, S and `source`.
// key and win start as all ones (one memset of the 12 bytes per target pixel): no depth has that pattern and no pixel that index.
// Every index derived from a double is bounds-tested on the double before it is converted.  Every product, sum, quotient, floor and
// square root is one IEEE f64 operation in the association the specification states (-ffp-contract=off, and the pragma below).
#pragma once
#include "cspm_device.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kCarryBlock = 256;
constexpr unsigned int kCarryNone = 0xFFFFFFFFu;  // win[g] of a pixel without a winner

struct CarryCam {  // one view of a rectified pair; cxv = cx + view * doffs and fB = f * B are computed once on the host
  double f, cxv, cy, B, doffs, fB;
};
struct CarryPar {  // kernel arguments: the two cameras, the motion X_t = R X_s + t, the target's max_dis
  CarryCam s, t;
  double R[9], tr[3];
  double max_dis;
  int ws, hs, wt, ht;
  int fill;
};
struct CarrySrc {
  const double *a, *b, *c;  // ws*hs each
  const uint8_t *mask;      // ws*hs bytes, or null: every pixel
};
struct CarryOut {
  double *nx, *ny, *nz, *a, *b, *c;  // wt*ht each
  uint8_t *state;                    // wt*ht bytes or null
  int *source;                       // wt*ht or null
  int keep_empty;                    // 1: a pixel of state 0 keeps its six values (a stored field); 0: they become NaN (a candidate field)
};

__device__ __forceinline__ bool carry_finite(double v) { return fabs(v) <= kDoubleMax; }

// steps 4 and 5: false unless hq > 0 (the target camera is on the plane's visible side)
__device__ __forceinline__ bool carry_plane(const CarryPar &k, double a, double b, double c, double &pa, double &pb, double &pc) {
  const double n0 = a * k.s.f, n1 = b * k.s.f;
  const double n2 = ((a * k.s.cxv + b * k.s.cy) + c) + k.s.doffs;
  const double r0 = (k.R[0] * n0 + k.R[1] * n1) + k.R[2] * n2;
  const double r1 = (k.R[3] * n0 + k.R[4] * n1) + k.R[5] * n2;
  const double r2 = (k.R[6] * n0 + k.R[7] * n1) + k.R[8] * n2;
  const double hq = k.s.fB + ((r0 * k.tr[0] + r1 * k.tr[1]) + r2 * k.tr[2]);
  pa = (k.t.B * r0) / hq;
  pb = (k.t.B * r1) / hq;
  pc = (((k.t.fB * r2) / hq - pa * k.t.cxv) - pb * k.t.cy) - k.t.doffs;
  return hq > 0.0;  // a NaN fails
}

// steps 1 to 6 for source pixel m: false unless it is a contender; then *g is its target pixel and *depth its Q[2]
__device__ __forceinline__ bool carry_pixel(const CarryPar &k, const CarrySrc &src, long long m, long long *g, double *depth) {
  if (src.mask != nullptr && src.mask[m] == 0) return false;
  const double a = src.a[m], b = src.b[m], c = src.c[m];
  if (!(carry_finite(a) && carry_finite(b) && carry_finite(c))) return false;
  const int yi = (int)(m / k.ws), xi = (int)(m - (long long)yi * k.ws);
  const double x = (double)xi, y = (double)yi;
  const double D = (a * x + b * y) + c;
  const double tt = D + k.s.doffs;
  if (!(tt > 0.0)) return false;
  const double Z = k.s.fB / tt;
  const double u = x - k.s.cxv, wv = y - k.s.cy;
  const double X = (u * Z) / k.s.f;
  const double Y = (wv * Z) / k.s.f;
  const double Q0 = ((k.R[0] * X + k.R[1] * Y) + k.R[2] * Z) + k.tr[0];
  const double Q1 = ((k.R[3] * X + k.R[4] * Y) + k.R[5] * Z) + k.tr[1];
  const double Q2 = ((k.R[6] * X + k.R[7] * Y) + k.R[8] * Z) + k.tr[2];
  if (!(Q2 > 0.0)) return false;
  const double pu = (k.t.f * Q0) / Q2 + k.t.cxv;
  const double pv = (k.t.f * Q1) / Q2 + k.t.cy;
  const double fx = floor(pu + 0.5), fy = floor(pv + 0.5);
  if (!(fx >= 0.0 && fx <= (double)(k.wt - 1) && fy >= 0.0 && fy <= (double)(k.ht - 1))) return false;  // on the doubles: a NaN fails
  double pa, pb, pc;
  if (!carry_plane(k, a, b, c, pa, pb, pc)) return false;
  if (!(carry_finite(pa) && carry_finite(pb) && carry_finite(pc))) return false;
  const double z = (pa * fx + pb * fy) + pc;
  if (!(z >= 0.0 && z <= k.max_dis)) return false;
  *g = (long long)(int)fy * k.wt + (int)fx;
  *depth = Q2;  // > 0 and, with a finite in-range pixel behind it, finite
  return true;
}

template <int PASS>
__global__ __launch_bounds__(kCarryBlock) void k_carry_splat(CarryPar k, CarrySrc src, unsigned long long *key, unsigned int *win) {
  const long long m = (long long)blockIdx.x * kCarryBlock + threadIdx.x;
  if (m >= (long long)k.ws * k.hs) return;
  long long g;
  double depth;
  if (!carry_pixel(k, src, m, &g, &depth)) return;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(depth);
  if (PASS == 0) atomicMin(key + g, bits);
  else if (key[g] == bits) atomicMin(win + g, (unsigned int)m);
}

__global__ __launch_bounds__(kCarryBlock) void k_carry_resolve(CarryPar k, CarrySrc src, const unsigned int *__restrict__ win, CarryOut out) {
  const long long g = (long long)blockIdx.x * kCarryBlock + threadIdx.x;
  if (g >= (long long)k.wt * k.ht) return;
  const int yi = (int)(g / k.wt), xi = (int)(g - (long long)yi * k.wt);
  const double x = (double)xi, y = (double)yi;
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  int state = 0;
  unsigned int from = win[g];
  double pa = 0.0, pb = 0.0, z = 0.0;
  if (from != kCarryNone) {
    double pc;
    carry_plane(k, src.a[from], src.b[from], src.c[from], pa, pb, pc);
    z = (pa * x + pb * y) + pc;  // the z of step 6: the pixel is the winner's (fx, fy)
    state = 1;
  } else if (k.fill) {
    const int ox[4] = {-1, 1, 0, 0}, oy[4] = {0, 0, -1, 1};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qx = xi + ox[j], qy = yi + oy[j];
      if (qx < 0 || qx >= k.wt || qy < 0 || qy >= k.ht) continue;
      const unsigned int wq = win[(long long)qy * k.wt + qx];
      if (wq == kCarryNone) continue;
      double qa, qb, qc;
      carry_plane(k, src.a[wq], src.b[wq], src.c[wq], qa, qb, qc);
      const double zq = (qa * x + qb * y) + qc;
      if (!(zq >= 0.0 && zq <= k.max_dis)) continue;
      if (state == 0 || zq < z) {  // the smallest z (the background side), the first in the order on a tie
        pa = qa; pb = qb; z = zq; from = wq;
        state = 2;
      }
    }
  }
  if (out.state) out.state[g] = (uint8_t)state;
  if (out.source) out.source[g] = state ? (int)from : -1;
  if (state == 0) {
    if (!out.keep_empty) {
      out.nx[g] = kNaN; out.ny[g] = kNaN; out.nz[g] = kNaN;
      out.a[g] = kNaN; out.b[g] = kNaN; out.c[g] = kNaN;
    }
    return;
  }
  const double m0 = -pa, m1 = -pb, m2 = 1.0;
  const double len = __dsqrt_rn((pa * pa + pb * pb) + 1.0);
  const double inv = 1. / fmax(len, kDoubleEps);
  const double nx = m0 * inv, ny = m1 * inv, nz = m2 * inv;
  double fa, fb, fc;
  plane_param(nx, ny, nz, x, y, z, fa, fb, fc);  // Plane(normal, (x, y, z)), as the plane fit finishes
  out.nx[g] = nx; out.ny[g] = ny; out.nz[g] = nz;
  out.a[g] = fa; out.b[g] = fb; out.c[g] = fc;
}

inline unsigned carry_blocks(long long n) { return (unsigned)((n + kCarryBlock - 1) / kCarryBlock); }

// the memset and the three launches of one carry; key = wt*ht 64-bit words, win = wt*ht 32-bit words right behind them
inline hipError_t carry_launch(hipStream_t stream, const CarryPar &k, const CarrySrc &src, unsigned long long *key, const CarryOut &out) {
  const long long ns = (long long)k.ws * k.hs, nt = (long long)k.wt * k.ht;
  unsigned int *win = reinterpret_cast<unsigned int *>(key + nt);
  const hipError_t e = hipMemsetAsync(key, 0xFF, (size_t)nt * 12, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_carry_splat<0>, dim3(carry_blocks(ns)), dim3(kCarryBlock), 0, stream, k, src, key, win);
  hipLaunchKernelGGL(k_carry_splat<1>, dim3(carry_blocks(ns)), dim3(kCarryBlock), 0, stream, k, src, key, win);
  hipLaunchKernelGGL(k_carry_resolve, dim3(carry_blocks(nt)), dim3(kCarryBlock), 0, stream, k, src, (const unsigned int *)win, out);
  return hipGetLastError();
}

}  // namespace cspm
