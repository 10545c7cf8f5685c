// cspm_fuse.h -- depth-map fusion (include/cspm.h "depth-map fusion"): the specification F, one pixel at a time.
//
// fuse_pixel() evaluates steps 3 and 4 of F for one reference pixel; the pass that decides and the pass that writes the records both
// call it, so a record cannot differ from its decision by a bit.  No LDS beyond the ballot sums, no atomics, no workgroup waits for
// another (the stance of cspm_geom.h):
//   k_fuse_store  the elementwise part of cspm_fuse_push: the slot's depth becomes NaN where G's keep is 0, the level-0 pixel is copied.
//   k_fuse_view   one LANE per reference pixel in flat raster order, kGeomBlock pixels per workgroup, ONE LAUNCH PER PASS r.  Reads only
//                 used_r, writes S_r, the marks used_k (k != r, always the value 1: racing lanes store the same byte) and the
//                 workgroup's kept count.  The launch boundary is what orders pass r behind the marks of the passes before it.
//   k_geom_scan   (cspm_geom.h) turns the counts of ALL passes, K * blocks of them, into exclusive offsets and the total.
//   k_fuse_counts the kept pixels per view, from the offsets.
//   k_fuse_cloud  one launch over (blocks, K): a pixel whose S byte says kept RECOMPUTES its sums (as k_geom_cloud recomputes G) and
//                 writes its record at rank = workgroup offset + kept pixels of the earlier waves + mbcnt of the ballot.  It reads S, not
//                 `used`: later passes have marked used_r since pass r looked at it.
// The camera table is indexed by the loop counter, which is wave-uniform: its reads are scalar loads.  The per-view gathers are
// data-dependent 8-byte loads.  Every product, sum, quotient, floor and square root is one IEEE f64 operation in the association the
// specification states (-ffp-contract=off, and the pragma below).
#pragma once
#include "cspm_geom.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kFuseMaxViews = 64;

struct FuseCam {  // one row of the camera table: the pinhole camera and its camera -> world pose, R row-major
  double f, cx, cy;
  double R[9];
  double t[3];
};
struct FuseMaps {           // the slots of all views, view k at k * n (normal: k * 3n, three planes of n)
  const double *depth;
  const double *normal;     // null: no view has normals
  const uint32_t *pix;      // B | G<<8 | R<<16; 0 in a view without an image.  null: no view has an image
  uint8_t *used;
  uint8_t *state;           // S
};
struct FusePar {
  double mr2, max_rel_depth, min_cos;
  int min_views, suppress;
};
struct FuseSum {
  double SP[3], SN[3];
  int SC[3];
  int c;
  unsigned long long seen;  // bit k: view k is consistent
};

__device__ __forceinline__ bool fuse_finite(double v) { return fabs(v) <= kDoubleMax; }

// back(k, x, y, Z) then world(k, .)
__device__ __forceinline__ void fuse_world(const FuseCam &k, double x, double y, double Z, double W[3]) {
  const double u = x - k.cx, wv = y - k.cy;
  const double X = (u * Z) / k.f;
  const double Y = (wv * Z) / k.f;
  for (int i = 0; i < 3; ++i) W[i] = ((k.R[3 * i] * X + k.R[3 * i + 1] * Y) + k.R[3 * i + 2] * Z) + k.t[i];
}
__device__ __forceinline__ void fuse_cam(const FuseCam &k, const double W[3], double Q[3]) {
  const double d0 = W[0] - k.t[0], d1 = W[1] - k.t[1], d2 = W[2] - k.t[2];
  for (int j = 0; j < 3; ++j) Q[j] = (k.R[j] * d0 + k.R[3 + j] * d1) + k.R[6 + j] * d2;
}
__device__ __forceinline__ void fuse_rot(const FuseCam &k, const double n[3], double N[3]) {
  for (int i = 0; i < 3; ++i) N[i] = (k.R[3 * i] * n[0] + k.R[3 * i + 1] * n[1]) + k.R[3 * i + 2] * n[2];
}
// proj(k, Q) and the rounding of step 4: false unless the pixel lies inside the image; *m = fy * w + fx
__device__ __forceinline__ bool fuse_project(const FuseCam &k, const double Q[3], int w, int h, double *fx, double *fy, long long *m) {
  if (!(Q[2] > 0.0)) return false;
  const double pu = (k.f * Q[0]) / Q[2] + k.cx;
  const double pv = (k.f * Q[1]) / Q[2] + k.cy;
  *fx = floor(pu + 0.5);
  *fy = floor(pv + 0.5);
  if (!(*fx >= 0.0 && *fx <= (double)(w - 1) && *fy >= 0.0 && *fy <= (double)(h - 1))) return false;  // on the doubles: a NaN fails
  *m = (long long)(int)*fy * w + (int)*fx;
  return true;
}

// steps 3 and 4 for pixel i = y*w + x of view r whose depth Z is valid
template <bool NORMALS>
__device__ __forceinline__ FuseSum fuse_pixel(const FuseCam *__restrict__ cams, const FuseMaps &v, const FusePar &p, int K, int r, int w, int h, long long n,
                                              long long i, double Z) {
  const int y = (int)(i / w), x = (int)(i - (long long)y * w);
  const FuseCam &cr = cams[r];
  FuseSum s;
  double P[3], Nr[3] = {0.0, 0.0, 0.0};
  fuse_world(cr, (double)x, (double)y, Z, P);
  for (int a = 0; a < 3; ++a) s.SP[a] = P[a];
  s.SN[0] = s.SN[1] = s.SN[2] = 0.0;
  if (NORMALS) {
    const double *nm = v.normal + (size_t)r * 3 * n;
    const double nr[3] = {nm[i], nm[n + i], nm[2 * n + i]};
    fuse_rot(cr, nr, Nr);
    if (fuse_finite(Nr[0]) && fuse_finite(Nr[1]) && fuse_finite(Nr[2]))
      for (int a = 0; a < 3; ++a) s.SN[a] = Nr[a];
  }
  s.SC[0] = s.SC[1] = s.SC[2] = 0;
  if (v.pix) {
    const uint32_t px = v.pix[(size_t)r * n + i];
    s.SC[0] = (int)(px & 255u); s.SC[1] = (int)((px >> 8) & 255u); s.SC[2] = (int)((px >> 16) & 255u);
  }
  s.c = 0;
  s.seen = 0ull;
  for (int k = 0; k < K; ++k) {
    if (k == r) continue;
    const FuseCam &ck = cams[k];
    double Q[3], fx, fy;
    long long mk;
    fuse_cam(ck, P, Q);
    if (!fuse_project(ck, Q, w, h, &fx, &fy, &mk)) continue;
    const double Zk = v.depth[(size_t)k * n + mk];
    if (!(fuse_finite(Zk) && Zk > 0.0)) continue;
    double Pk[3], Q2[3];
    fuse_world(ck, fx, fy, Zk, Pk);
    fuse_cam(cr, Pk, Q2);
    if (!(Q2[2] > 0.0)) continue;
    const double pu2 = (cr.f * Q2[0]) / Q2[2] + cr.cx;
    const double pv2 = (cr.f * Q2[1]) / Q2[2] + cr.cy;
    const double ex = pu2 - (double)x, ey = pv2 - (double)y;
    if (!(ex * ex + ey * ey <= p.mr2)) continue;
    if (!(fabs(Q2[2] - Z) <= p.max_rel_depth * Z)) continue;
    double Nk[3] = {0.0, 0.0, 0.0};
    if (NORMALS) {
      const double *nm = v.normal + (size_t)k * 3 * n;
      const double nk[3] = {nm[mk], nm[n + mk], nm[2 * n + mk]};
      fuse_rot(ck, nk, Nk);
      if (p.min_cos > 0.0 && !((Nr[0] * Nk[0] + Nr[1] * Nk[1]) + Nr[2] * Nk[2] >= p.min_cos)) continue;  // a NaN fails
    }
    s.c += 1;
    s.seen |= 1ull << k;
    for (int a = 0; a < 3; ++a) s.SP[a] = s.SP[a] + Pk[a];
    if (NORMALS && fuse_finite(Nk[0]) && fuse_finite(Nk[1]) && fuse_finite(Nk[2]))
      for (int a = 0; a < 3; ++a) s.SN[a] = s.SN[a] + Nk[a];
    if (v.pix) {
      const uint32_t px = v.pix[(size_t)k * n + mk];
      s.SC[0] += (int)(px & 255u); s.SC[1] += (int)((px >> 8) & 255u); s.SC[2] += (int)((px >> 16) & 255u);
    }
  }
  return s;
}

// the workgroup's number of lanes with `flag`, to counts[blockIdx.x]
__device__ __forceinline__ void fuse_block_count(bool flag, unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x;
  const unsigned long long ballot = __ballot(flag);
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = (unsigned int)__popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
    for (int w = 0; w < kGeomWaves; ++w) s += s_wave[w];
    counts[blockIdx.x] = s;
  }
}

// the elementwise part of a push of the stored field: depth holds G's depth, keep G's keep, src the view's level-0 pixels
__global__ __launch_bounds__(256) void k_fuse_store(double *__restrict__ depth, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ src,
                                                    uint32_t *__restrict__ pix, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (keep[i] == 0) depth[i] = __longlong_as_double(0x7FF8000000000000LL);
  pix[i] = src[i] & 0x00FFFFFFu;
}

// pass r: S, the marks, the workgroup's kept count (counts = this pass's part of the count array)
template <bool NORMALS>
__global__ __launch_bounds__(kGeomBlock) void k_fuse_view(const FuseCam *__restrict__ cams, FuseMaps v, FusePar p, int K, int r, int w, int h, long long n,
                                                          unsigned int *__restrict__ counts) {
  const long long i = (long long)blockIdx.x * kGeomBlock + (int)threadIdx.x;
  bool kept = false;
  if (i < n) {
    const double Z = v.depth[(size_t)r * n + i];
    uint8_t S = 0;
    if (fuse_finite(Z) && Z > 0.0) {
      if (p.suppress && v.used[(size_t)r * n + i] != 0) {
        S = 0x80;
      } else {
        const FuseSum s = fuse_pixel<NORMALS>(cams, v, p, K, r, w, h, n, i, Z);
        kept = s.c >= p.min_views;
        S = (uint8_t)(s.c | (kept ? 0x40 : 0));
        if (kept && p.suppress && s.seen != 0ull) {
          // the pixels m_k of the consistent views, recomputed from the same P by the same operations
          const int y = (int)(i / w), x = (int)(i - (long long)y * w);
          double P[3];
          fuse_world(cams[r], (double)x, (double)y, Z, P);
          for (int k = 0; k < K; ++k) {
            if (!((s.seen >> k) & 1ull)) continue;
            double Q[3], fx, fy;
            long long mk;
            fuse_cam(cams[k], P, Q);
            if (fuse_project(cams[k], Q, w, h, &fx, &fy, &mk)) v.used[(size_t)k * n + mk] = 1;
          }
        }
      }
    }
    v.state[(size_t)r * n + i] = S;
  }
  fuse_block_count(kept, counts);
}

// offsets[0 .. K*nb) and *total -> the kept pixels of every view
__global__ void k_fuse_counts(const unsigned int *__restrict__ offsets, const unsigned int *__restrict__ total, int K, unsigned int nb,
                              unsigned int *__restrict__ view_counts) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= K) return;
  const unsigned int end = k + 1 < K ? offsets[(size_t)(k + 1) * nb] : *total;
  view_counts[k] = end - offsets[(size_t)k * nb];
}

// the records of the kept pixels in (view, raster) order, the first `cap` of them; grid (blocks, K)
template <bool NORMALS>
__global__ __launch_bounds__(kGeomBlock) void k_fuse_cloud(const FuseCam *__restrict__ cams, FuseMaps v, FusePar p, int K, int w, int h, long long n,
                                                           const unsigned int *__restrict__ offsets, uint4 *__restrict__ cloud, unsigned int cap) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int r = (int)blockIdx.y;
  const long long i = (long long)blockIdx.x * kGeomBlock + tid;
  const bool kept = i < n && (v.state[(size_t)r * n + i] & 0x40) != 0;
  const unsigned long long ballot = __ballot(kept);
  if ((tid & (kWave - 1)) == 0) s_wave[wave] = (unsigned int)__popcll(ballot);
  __syncthreads();
  if (!kept) return;
  unsigned int rank = offsets[(size_t)r * gridDim.x + blockIdx.x];
  for (int q = 0; q < wave; ++q) rank += s_wave[q];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
  if (rank >= cap) return;
  const FuseSum s = fuse_pixel<NORMALS>(cams, v, p, K, r, w, h, n, i, v.depth[(size_t)r * n + i]);
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  const double den = (double)(s.c + 1);
  double N[3] = {kNaN, kNaN, kNaN};
  if (NORMALS) {
    const double len = __dsqrt_rn((s.SN[0] * s.SN[0] + s.SN[1] * s.SN[1]) + s.SN[2] * s.SN[2]);
    for (int a = 0; a < 3; ++a) N[a] = s.SN[a] / len;
  }
  uint32_t bgra = 0u;
  if (v.pix) {
    const int d1 = s.c + 1, d2 = 2 * d1;
    bgra = (uint32_t)((2 * s.SC[0] + d1) / d2) | ((uint32_t)((2 * s.SC[1] + d1) / d2) << 8) | ((uint32_t)((2 * s.SC[2] + d1) / d2) << 16) | 0xFF000000u;
  }
  uint4 r0, r1;
  r0.x = __float_as_uint(__double2float_rn(s.SP[0] / den));
  r0.y = __float_as_uint(__double2float_rn(s.SP[1] / den));
  r0.z = __float_as_uint(__double2float_rn(s.SP[2] / den));
  r0.w = __float_as_uint(__double2float_rn(N[0]));
  r1.x = __float_as_uint(__double2float_rn(N[1]));
  r1.y = __float_as_uint(__double2float_rn(N[2]));
  r1.z = bgra;
  r1.w = (uint32_t)i;
  cloud[2 * (size_t)rank] = r0;
  cloud[2 * (size_t)rank + 1] = r1;
}

}  // namespace cspm
