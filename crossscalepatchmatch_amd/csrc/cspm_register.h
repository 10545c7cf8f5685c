// cspm_register.h -- registration of a fusion view against other fusion views (include/cspm.h "depth-view registration", DESIGN.md
// section 26): the specification R, projective point-to-plane Gauss-Newton over the fusion slots.
//
// One iteration is two launches on the context stream; nothing returns to the host between iterations:
//   k_reg_pairs   one LANE per source sample in flat order q = j*ws + i, kRegBlock samples per workgroup.  The current source camera (the
//                 scratch row `pose`) and the target rows of the camera table are read by wave-uniform index: scalar loads, as in
//                 k_fuse_view.  Each lane keeps the 29 sums of its sample in registers (the loops over them are unrolled: no indexing by
//                 a runtime value), the workgroup reduces them in the tree R states and writes ONE 29-double partial.  No atomics, no
//                 workgroup waits for another.
//   k_reg_solve   one workgroup: lane j sums the partials j, j + 256, .. ascending, the same tree reduces the 256 sums, lane 0 solves the
//                 6 x 6 system by LDL^T, updates the scratch row with the Cayley map and appends the iteration's record.  Plain stores.
// The tree: step s = 128 and 64 go through LDS (lane i adds the value of lane i + s: the upper waves store, the lower ones add), the steps
// 32 .. 1 are an xor-butterfly inside wave 0: lane i < s adds lane i + s = i ^ s, so lane 0 ends with exactly the tree's sum; the other
// lanes compute sums nobody reads.  Every product, sum and quotient is one IEEE f64 operation in the association R writes
// (-ffp-contract=off, and the pragma below).
#pragma once
#include "cspm_fuse.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kRegBlock = 256;  // samples (lanes) per workgroup: 4 waves
constexpr int kRegSums = 29;    // A (21, a <= b row-major), b (6), cost, pairs
constexpr int kRegMaxIters = 64;

struct RegPar {
  double max_dist2, huber, min_cos, pivot_rel, min_pairs;
  int stride, ws;
  long long samples;
};
struct RegRec {  // the layout of cspm_reg_iter
  double pairs, cost, rot2, trans2;
  int status, pad;
};

// the tree over the 256 lanes' sums; the result is in lane 0.  s_red: kRegSums * 128 doubles
__device__ __forceinline__ void reg_block_reduce(double (&acc)[kRegSums], double *__restrict__ s_red) {
  const int tid = (int)threadIdx.x;
  if (tid >= 128) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) s_red[q * 128 + (tid - 128)] = acc[q];
  }
  __syncthreads();
  if (tid < 128) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) acc[q] = acc[q] + s_red[q * 128 + tid];
  }
  __syncthreads();
  if (tid >= 64 && tid < 128) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) s_red[q * 128 + (tid - 64)] = acc[q];
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) acc[q] = acc[q] + s_red[q * 128 + tid];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int q = 0; q < kRegSums; ++q) acc[q] = acc[q] + __shfl_xor(acc[q], s, kWave);
    }
  }
}

// one iteration's sums: part[blockIdx.x * kRegSums ..]
__global__ __launch_bounds__(kRegBlock) void k_reg_pairs(const FuseCam *__restrict__ cams, const FuseCam *__restrict__ pose, const double *__restrict__ depth,
                                                         const double *__restrict__ normal, int K, int src, unsigned long long targets, int w, int h,
                                                         long long n, RegPar p, double *__restrict__ part) {
  __shared__ double s_red[kRegSums * 128];
  double acc[kRegSums];
#pragma unroll
  for (int q = 0; q < kRegSums; ++q) acc[q] = 0.0;
  const long long smp = (long long)blockIdx.x * kRegBlock + (int)threadIdx.x;
  if (smp < p.samples) {
    const int j = (int)(smp / p.ws), i = (int)(smp - (long long)j * p.ws);
    const int x = i * p.stride, y = j * p.stride;  // < w, < h: ws = ceil(w / stride), hs = ceil(h / stride)
    const long long m = (long long)y * w + x;
    const double Z = depth[(size_t)src * n + m];
    if (fuse_finite(Z) && Z > 0.0) {
      const FuseCam &cs = *pose;
      double P[3], L[3];
      fuse_world(cs, (double)x, (double)y, Z, P);
      for (int a = 0; a < 3; ++a) L[a] = P[a] - cs.t[a];
      double Ns[3] = {0.0, 0.0, 0.0};
      if (p.min_cos > 0.0) {
        const double *nm = normal + (size_t)src * 3 * n;
        const double ns[3] = {nm[m], nm[n + m], nm[2 * n + m]};
        fuse_rot(cs, ns, Ns);
      }
      for (int k = 0; k < K; ++k) {
        if (!((targets >> k) & 1ull)) continue;
        const FuseCam &ck = cams[k];
        double Q[3], fx, fy;
        long long mk;
        fuse_cam(ck, P, Q);
        if (!fuse_project(ck, Q, w, h, &fx, &fy, &mk)) continue;
        const double Zk = depth[(size_t)k * n + mk];
        if (!(fuse_finite(Zk) && Zk > 0.0)) continue;
        double Pk[3], N[3];
        fuse_world(ck, fx, fy, Zk, Pk);
        const double *nm = normal + (size_t)k * 3 * n;
        const double nk[3] = {nm[mk], nm[n + mk], nm[2 * n + mk]};
        fuse_rot(ck, nk, N);
        if (!(fuse_finite(N[0]) && fuse_finite(N[1]) && fuse_finite(N[2]))) continue;
        const double d0 = Pk[0] - P[0], d1 = Pk[1] - P[1], d2 = Pk[2] - P[2];
        if (!((d0 * d0 + d1 * d1) + d2 * d2 <= p.max_dist2)) continue;  // a NaN fails
        if (p.min_cos > 0.0 && !((Ns[0] * N[0] + Ns[1] * N[1]) + Ns[2] * N[2] >= p.min_cos)) continue;
        const double r = (N[0] * d0 + N[1] * d1) + N[2] * d2;
        const double J[6] = {L[1] * N[2] - L[2] * N[1], L[2] * N[0] - L[0] * N[2], L[0] * N[1] - L[1] * N[0], N[0], N[1], N[2]};
        const double ar = fabs(r);
        const double wt = (p.huber == 0.0 || ar <= p.huber) ? 1.0 : p.huber / ar;
        double g[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] = wt * J[a];
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
          for (int b = a; b < 6; ++b, ++q) acc[q] = acc[q] + g[a] * J[b];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + g[a] * r;
        acc[27] = acc[27] + (wt * r) * r;
        acc[28] = acc[28] + 1.0;
      }
    }
  }
  reg_block_reduce(acc, s_red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) part[(size_t)blockIdx.x * kRegSums + q] = acc[q];
  }
}

// the iteration's step: reduces the nb partials, solves, updates *pose, writes *rec
__global__ __launch_bounds__(kRegBlock) void k_reg_solve(const double *__restrict__ part, int nb, RegPar p, FuseCam *__restrict__ pose, RegRec *__restrict__ rec) {
  __shared__ double s_red[kRegSums * 128];
  double acc[kRegSums];
#pragma unroll
  for (int q = 0; q < kRegSums; ++q) acc[q] = 0.0;
  for (int B = (int)threadIdx.x; B < nb; B += kRegBlock) {
#pragma unroll
    for (int q = 0; q < kRegSums; ++q) acc[q] = acc[q] + part[(size_t)B * kRegSums + q];
  }
  reg_block_reduce(acc, s_red);
  if (threadIdx.x != 0) return;
  RegRec out;
  out.pairs = acc[28];
  out.cost = acc[27];
  out.rot2 = out.trans2 = 0.0;
  out.status = 0;
  out.pad = 0;
  double A[6][6], Lm[6][6], D[6], xi[6];
  {
    int q = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b, ++q) A[a][b] = A[b][a] = acc[q];
    }
  }
  if (acc[28] < p.min_pairs) out.status = 1;
  if (out.status == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dj = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj = dj - (Lm[j][k] * Lm[j][k]) * D[k];
      D[j] = dj;
      if (out.status == 0 && !(dj > p.pivot_rel * A[j][j])) out.status = 2;  // a NaN fails
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double l = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) l = l - (Lm[i][k] * Lm[j][k]) * D[k];
        Lm[i][j] = l / dj;
      }
    }
  }
  if (out.status == 0) {
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double v = acc[21 + i];
#pragma unroll
      for (int k = 0; k < i; ++k) v = v - Lm[i][k] * yv[k];
      yv[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = yv[i] / D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double v = xi[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) v = v - Lm[k][i] * xi[k];
      xi[i] = v;
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) fin = fin && fuse_finite(xi[i]);
    if (!fin) out.status = 3;
  }
  if (out.status == 0) {
    out.rot2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2];
    out.trans2 = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5];
    const double a0 = 0.5 * xi[0], a1 = 0.5 * xi[1], a2 = 0.5 * xi[2];
    const double s = (a0 * a0 + a1 * a1) + a2 * a2;
    const double pm = 1.0 - s, qp = 1.0 + s;
    double E[9];
    E[0] = (pm + 2.0 * (a0 * a0)) / qp;
    E[1] = (2.0 * (a0 * a1) - 2.0 * a2) / qp;
    E[2] = (2.0 * (a0 * a2) + 2.0 * a1) / qp;
    E[3] = (2.0 * (a0 * a1) + 2.0 * a2) / qp;
    E[4] = (pm + 2.0 * (a1 * a1)) / qp;
    E[5] = (2.0 * (a1 * a2) - 2.0 * a0) / qp;
    E[6] = (2.0 * (a0 * a2) - 2.0 * a1) / qp;
    E[7] = (2.0 * (a1 * a2) + 2.0 * a0) / qp;
    E[8] = (pm + 2.0 * (a2 * a2)) / qp;
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = pose->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) pose->R[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) pose->t[i] = pose->t[i] + xi[3 + i];
  }
  *rec = out;
}

}  // namespace cspm
