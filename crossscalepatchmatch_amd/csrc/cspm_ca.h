// cspm_ca.h -- cost aggregation (CAMethod::aggreCV, ca_method.h:8-25) and the cross-scale winner-take-all over the aggregated
// volumes: the BOX, GF and BF filters of the reference's ca_filter/ directory as HIP kernels for gfx950.
//
// Every filter works on a STACK of f64 slabs (h x w each, row-major).  BoxFilter (GuidedFilter.cpp:71-122) is two serial
// cumulative sums with band differences: CumSum over y, then over x.  Both passes are run by the same scheme, a "walk": a lane
// owns one column of the pass and walks along it, carrying two running sums -- `lead`, the cumulative sum up to the row it is about
// to add, and `trail`, the cumulative sum up to the row the window has left.  Each is the reference's serial sum over the same
// elements in the same order, so lead - trail is bit for bit the reference's cum[y+r] - cum[y-r-1].  The Y walk (lanes along x,
// coalesced) writes its result TRANSPOSED ([x][y]); the X walk then reads that layout with lanes along y, again coalesced, and
// hands each box value to an epilogue that applies the elementwise steps of the filter before anything is written back.
//
// Compiled with -ffp-contract=off (cspm_device.h): every product and sum below is rounded on its own, as in the reference.
#pragma once
#include "cspm_device.h"

namespace cspm {

constexpr int kCaBlock = 64;  // one wave per workgroup: a walk is one lane per column

// the window of BoxFilter at index i of a dimension of n (the three bands, GuidedFilter.cpp:81-119; n >= 2r+1): cum[min(i+r, n-1)]
// minus cum[i-r-1] from i = r+1 on
__device__ __forceinline__ int ca_lead_idx(int i, int r, int n) { return i + r < n - 1 ? i + r : n - 1; }

// N = BoxFilter(ones): sums of ones are exact integers, so N is the clipped window area exactly
__device__ __forceinline__ double ca_count(int y, int x, int r, int W, int H) {
  const int ny = ca_lead_idx(y, r, H) - (y - r - 1 >= 0 ? y - r - 1 : -1);
  const int nx = ca_lead_idx(x, r, W) - (x - r - 1 >= 0 ? x - r - 1 : -1);
  return (double)ny * (double)nx;
}

// ---- inputs of the Y walk: element k of item j at natural pixel index pix ----
struct CaInPlain {  // the stack itself: item j, slab k at base + (j*K + k)*px
  const double *base;
  int K;
  size_t px;
  __device__ double operator()(int j, int k, size_t pix) const { return base[((size_t)j * K + k) * px + pix]; }
};
struct CaInGuide {  // GF, guide-only terms (GuidedFilter.cpp:177-208): I_0..I_2, then I_c*I_c' for c <= c' in the reference's order
  const double *g;  // 3 natural slabs (channel-major)
  size_t px;
  __device__ double operator()(int, int k, size_t pix) const {
    if (k < 3) return g[k * px + pix];
    const int c = k < 6 ? 0 : (k < 8 ? 1 : 2);
    const int cp = k < 6 ? k - 3 : (k < 8 ? k - 5 : 2);
    return g[c * px + pix] * g[cp * px + pix];  // multiply(rgb[c], rgb[c_p], tmp)
  }
};
struct CaInGfP {  // GF, per slice (GuidedFilter.cpp:180-186): p, then I_c * p
  const double *p;  // slice j at p + j*px
  const double *g;
  size_t px;
  __device__ double operator()(int j, int k, size_t pix) const {
    const double v = p[(size_t)j * px + pix];
    return k == 0 ? v : g[(k - 1) * px + pix] * v;  // multiply(rgb[c], p, tmp)
  }
};

// Y walk: lane = column x of item j (grid: ceil(W/64) x items); K running pairs; box-over-y of element k written to
// out[(j*K + k)][x][y] (transposed).  The cumulative sum over y starts from the 0.0 of Mat::zeros (CumSum d == 1: cur = pre + src).
template <int K, class In>
__global__ __launch_bounds__(kCaBlock) void k_ca_ywalk(In in, int W, int H, int r, double *__restrict__ out) {
  const int x = blockIdx.x * kCaBlock + threadIdx.x;
  const int j = blockIdx.y;
  if (x >= W) return;
  const size_t px = (size_t)W * H;
  double lead[K], trail[K];
#pragma unroll
  for (int k = 0; k < K; ++k) lead[k] = trail[k] = 0.0;
  int li = -1, ti = -1;
  double *o = out + (size_t)j * K * px + (size_t)x * H;
  for (int y = 0; y < H; ++y) {
    const int lt = ca_lead_idx(y, r, H);
    for (; li < lt; ++li) {
      const size_t pix = (size_t)(li + 1) * W + x;
#pragma unroll
      for (int k = 0; k < K; ++k) lead[k] += in(j, k, pix);
    }
    if (y <= r) {
#pragma unroll
      for (int k = 0; k < K; ++k) o[k * px + y] = lead[k];
    } else {
      for (; ti < y - r - 1; ++ti) {
        const size_t pix = (size_t)(ti + 1) * W + x;
#pragma unroll
        for (int k = 0; k < K; ++k) trail[k] += in(j, k, pix);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) o[k * px + y] = lead[k] - trail[k];
    }
  }
}

// X walk: lane = row y of item j over the transposed Y-walk output t[(j*K + k)][x][y]; the cumulative sum over x starts with
// the first element itself (CumSum d == 2: cur[0] = src[0]) -- -0.0 is the additive identity that reproduces it, sign of zero
// included.  ep(j, y, x, box[K]) consumes BoxFilter's value at (y, x) of every element of item j.
template <int K, class Ep>
__global__ __launch_bounds__(kCaBlock) void k_ca_xwalk(const double *__restrict__ t, int W, int H, int r, Ep ep) {
  const int y = blockIdx.x * kCaBlock + threadIdx.x;
  const int j = blockIdx.y;
  if (y >= H) return;
  const size_t px = (size_t)W * H;
  const double *src = t + (size_t)j * K * px + y;
  double lead[K], trail[K], box[K];
#pragma unroll
  for (int k = 0; k < K; ++k) lead[k] = trail[k] = -0.0;
  int li = -1, ti = -1;
  for (int x = 0; x < W; ++x) {
    const int lt = ca_lead_idx(x, r, W);
    for (; li < lt; ++li) {
#pragma unroll
      for (int k = 0; k < K; ++k) lead[k] += src[k * px + (size_t)(li + 1) * H];
    }
    if (x <= r) {
#pragma unroll
      for (int k = 0; k < K; ++k) box[k] = lead[k];
    } else {
      for (; ti < x - r - 1; ++ti) {
#pragma unroll
        for (int k = 0; k < K; ++k) trail[k] += src[k * px + (size_t)(ti + 1) * H];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) box[k] = lead[k] - trail[k];
    }
    ep(j, y, x, box);
  }
}

// ---- epilogues ----
struct CaEpStore {  // BOX: BoxFilter(p, 3) unnormalised (BoxCA.cpp:10), natural layout
  double *out;
  int W;
  size_t px;
  __device__ void operator()(int j, int y, int x, const double *box) const { out[(size_t)j * px + (size_t)y * W + x] = box[0]; }
};

// GF guide terms, TRANSPOSED layout [x][y] (read by the X walks' lanes along y): g[0..2] = I_c, m[0..2] = mean_I, cof[0..8] = the
// three cofactor rows of FAST_INV, idet = 1/DET (GuidedFilter.cpp:248-263)
struct CaGuideT {
  double *g, *m, *cof, *idet;
};
struct CaEpGuide {
  CaGuideT gt;
  const double *gn;  // the guide, natural layout
  int W, H, r;
  double eps;
  __device__ void operator()(int, int y, int x, const double *box) const {
    const size_t px = (size_t)W * H, ti = (size_t)x * H + y, ni = (size_t)y * W + x;
    const double N = ca_count(y, x, r, W, H);
    double m[3], v[6];
    for (int c = 0; c < 3; ++c) m[c] = box[c] / N;  // mean_I[c] = BoxFilter(rgb[c], r) / N
    int k = 0;
    for (int c = 0; c < 3; ++c)
      for (int cp = c; cp < 3; ++cp, ++k) {
        v[k] = box[3 + k] / N;  // var_I[k] = BoxFilter(rgb[c]*rgb[c_p], r) / N
        v[k] -= m[c] * m[cp];   // var_I[k] -= mean_I[c]*mean_I[c_p]
      }
    const double a11 = v[0] + eps, a12 = v[1], a13 = v[2];
    const double a21 = v[1], a22 = v[3] + eps, a23 = v[4];
    const double a31 = v[2], a32 = v[4], a33 = v[5] + eps;
    double DET = a11 * (a33 * a22 - a32 * a23) - a21 * (a33 * a12 - a32 * a13) + a31 * (a23 * a12 - a22 * a13);
    DET = 1 / DET;
    const double cof[9] = {a33 * a22 - a32 * a23, a31 * a23 - a33 * a21, a32 * a21 - a31 * a22,
                           a32 * a13 - a33 * a12, a33 * a11 - a31 * a13, a31 * a12 - a32 * a11,
                           a23 * a12 - a22 * a13, a21 * a13 - a23 * a11, a22 * a11 - a21 * a12};
    for (int c = 0; c < 3; ++c) {
      gt.g[c * px + ti] = gn[c * px + ni];
      gt.m[c * px + ti] = m[c];
    }
    for (int q = 0; q < 9; ++q) gt.cof[q * px + ti] = cof[q];
    gt.idet[ti] = DET;
  }
};
// GF step 1 (GuidedFilter.cpp:180-191, 248-291): box[0] = BoxFilter(p), box[1+c] = BoxFilter(I_c*p) -> b, a_0, a_1, a_2 of the
// slice, natural layout, item j's four slabs at out + (4j + k)*px
struct CaEpGfA {
  CaGuideT gt;
  double *out;
  int W, H, r;
  __device__ void operator()(int j, int y, int x, const double *box) const {
    const size_t px = (size_t)W * H, ti = (size_t)x * H + y, ni = (size_t)y * W + x;
    const double N = ca_count(y, x, r, W, H);
    const double mean_p = box[0] / N;
    double cov[3], m[3];
    for (int c = 0; c < 3; ++c) {
      m[c] = gt.m[c * px + ti];
      const double mean_Ip = box[1 + c] / N;
      cov[c] = mean_Ip - m[c] * mean_p;  // cov_Ip[c] = mean_Ip[c] - mean_I[c]*mean_p
    }
    const double DET = gt.idet[ti];
    double a[3];
    for (int c = 0; c < 3; ++c) {
      const double *cf = gt.cof + (size_t)3 * c * px + ti;
      a[c] = DET * (cov[0] * cf[0] + cov[1] * cf[px] + cov[2] * cf[2 * px]);
    }
    double b = mean_p;  // b = mean_p.clone(); b -= a[c]*mean_I[c]
    for (int c = 0; c < 3; ++c) b -= a[c] * m[c];
    double *o = out + (size_t)4 * j * px + ni;
    o[0] = b;
    o[px] = a[0];
    o[2 * px] = a[1];
    o[3 * px] = a[2];
  }
};
// GF step 2 (GuidedFilter.cpp:292-297): q = BoxFilter(b); q += BoxFilter(a_c)*I_c; q /= N -> slice j of out, natural layout
struct CaEpGfQ {
  CaGuideT gt;
  double *out;
  int W, H, r;
  __device__ void operator()(int j, int y, int x, const double *box) const {
    const size_t px = (size_t)W * H, ti = (size_t)x * H + y;
    double q = box[0];
    for (int c = 0; c < 3; ++c) q += box[1 + c] * gt.g[c * px + ti];
    q /= ca_count(y, x, r, W, H);
    out[(size_t)j * px + (size_t)y * W + x] = q;
  }
};

// BF (BilateralFilter.cpp:51-95, colour branch): one lane per pixel, each tap's weight computed once and applied to a register
// block of kBfSlices slices; wrap-around borders; the device's f64 exp
constexpr int kBfSlices = 8;
__global__ __launch_bounds__(256) void k_ca_bf(const double *__restrict__ g, const double *__restrict__ p, int W, int H, int n,
                                               double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t px = (size_t)W * H;
  if (i >= (long long)px) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const int hw = 35 / 2;
  double sig_sp = 35 / 2.0f;  // BilateralFilter.cpp:14
  const double sig_clr = 0.03;  // BilateralFilter.h:5
  const double ss = sig_sp * sig_sp, sc = sig_clr * sig_clr;
  const double p0 = g[i], p1 = g[px + i], p2 = g[2 * px + i];
  for (int j0 = 0; j0 < n; j0 += kBfSlices) {
    const int nj = n - j0 < kBfSlices ? n - j0 : kBfSlices;
    double sum[kBfSlices], sumWgt = 0.0;
#pragma unroll
    for (int k = 0; k < kBfSlices; ++k) sum[k] = 0.0;
    for (int wy = -hw; wy <= hw; ++wy) {
      int qy = y + wy;
      if (qy < 0) qy += H;
      if (qy >= H) qy -= H;
      for (int wx = -hw; wx <= hw; ++wx) {
        int qx = x + wx;
        if (qx < 0) qx += W;
        if (qx >= W) qx -= W;
        const size_t q = (size_t)qy * W + qx;
        const double spDis = wx * wx + wy * wy;
        double clrDis = 0.0;
        clrDis += fabs(p0 - g[q]);
        clrDis += fabs(p1 - g[px + q]);
        clrDis += fabs(p2 - g[2 * px + q]);
        clrDis *= 0.333333333;
        const double wgt = exp(-spDis / ss - clrDis * clrDis / sc);
        const double *pq = p + (size_t)j0 * px + q;
#pragma unroll
        for (int k = 0; k < kBfSlices; ++k)
          if (k < nj) sum[k] += wgt * pq[(size_t)k * px];
        sumWgt += wgt;
      }
    }
#pragma unroll
    for (int k = 0; k < kBfSlices; ++k)
      if (k < nj) out[(size_t)(j0 + k) * px + i] = sum[k] / sumWgt;
  }
}

// the guide of local stereo: the level image, BGR -> RGB, each 8-bit value times (double)(1.0f/255.0f); natural layout, 3 slabs
__global__ void k_ca_guide_u32(const uint32_t *__restrict__ pix, int W, int H, int Wp, int pad, double *__restrict__ g) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t px = (size_t)W * H;
  if (i >= (long long)px) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const uint32_t v = pix[(size_t)y * Wp + pad + x];
  const double s = (double)(1.0f / 255.0f);
  g[i] = (double)((v >> 16) & 255u) * s;     // R
  g[px + i] = (double)((v >> 8) & 255u) * s; // G
  g[2 * px + i] = (double)(v & 255u) * s;    // B
}

// max over an aggregated level volume (pre_cs_pc.cc:74-83), as an order-preserving key
__global__ __launch_bounds__(256) void k_ca_max(const double *__restrict__ vol, long long cells, unsigned long long *max_key) {
  unsigned long long key = f64_key(-1.7976931348623157e308);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (long long)gridDim.x * blockDim.x) {
    const unsigned long long k = f64_key(vol[i]);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long other = __shfl_xor(key, off, kWave);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(max_key, key);
}

// the coarse levels of the cross-scale WTA: aggregated volumes of levels 1.., their max, their weights
struct CaLevels {
  int levels, cs;
  int W[CSPM_MAX_LEVELS], H[CSPM_MAX_LEVELS], D[CSPM_MAX_LEVELS];
  const double *vol[CSPM_MAX_LEVELS];  // level s >= 1: D_s + 1 aggregated slabs
  double wgt[CSPM_MAX_LEVELS];
  const unsigned long long *max_key;   // [levels]: M[v][s] = max(-1.0, max of the aggregated volume)
};

// One batch of level-0 slices a0[0 .. n) = aggregated slices d0 .. d0+n-1 folded into the running (best cost, best d) per pixel:
// d = d0 .. d0+n-2, ascending, strict < (pre_cs_pc.cc:157-183 / pre_ss_pc.cc:99-111 with the window reduced to its centre, whose
// weight lookup_exp_[0] is 1.0)
__global__ __launch_bounds__(256) void k_ca_wta(CaLevels lv, const double *__restrict__ a0, int d0, int n, double *__restrict__ best,
                                                int *__restrict__ best_d) {
  const int W = lv.W[0], H = lv.H[0];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t px = (size_t)W * H;
  if (i >= (long long)px) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  double bc = best[i];
  int bd = best_d[i];
  for (int j = 0; j + 1 < n; ++j) {
    const int d = d0 + j;
    double cost = 0.0;
    for (int s = 0; s < lv.levels; ++s) {
      double q = (double)d;
      for (int k = 0; k < s; ++k) q /= 2.0;
      const int f = (int)q;
      double c;
      if (f <= 0 || f >= lv.D[s]) {
        c = key_f64(lv.max_key[s]);
        c = c > -1.0 ? c : -1.0;
      } else {
        const double fw = (f + 1) - q;
        double lo, hi;
        if (s == 0) {
          lo = a0[(size_t)(f - d0) * px + i];
          hi = a0[(size_t)(f + 1 - d0) * px + i];
        } else {
          const size_t ps = (size_t)lv.W[s] * lv.H[s], o = (size_t)(y >> s) * lv.W[s] + (x >> s);
          lo = lv.vol[s][(size_t)f * ps + o];
          hi = lv.vol[s][(size_t)(f + 1) * ps + o];
        }
        c = fw * lo + (1 - fw) * hi;
      }
      if (lv.cs) {
        double sc = 0.0;
        sc += 1.0 * c;  // scale_cost += wgt * tmp, wgt = lookup_exp_[0]
        cost += sc * lv.wgt[s];
      } else {
        cost += 1.0 * c;
      }
    }
    if (bd == 0 || cost < bc) {
      bc = cost;
      bd = d;
    }
  }
  best[i] = bc;
  best_d[i] = bd;
}

// the WTA plane: Plane(Vec3d(0, 0, 1), Point3d(x, y, d*)) (plane.h:15-34) and its cost
__global__ void k_ca_planes(Field f, long long n, const double *__restrict__ best, const int *__restrict__ best_d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = (double)best_d[i];
  f.nx[i] = 0.0;
  f.ny[i] = 0.0;
  f.nz[i] = 1.0;
  f.a[i] = -0.0 / 1.0;
  f.b[i] = -0.0 / 1.0;
  double s = 0.0 * 0.0;  // norm . point, cv::Matx::dot order, over denom = 1
  s += 0.0 * 0.0;
  s += 1.0 * d;
  f.c[i] = s / 1.0;
  f.cost[i] = best[i];
}

}  // namespace cspm
