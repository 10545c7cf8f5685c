// cspm_tsdf.h -- TSDF fusion of depth views (include/cspm.h "TSDF fusion"): the specification T.
//
// The volume is three planes of nx*ny*nz elements in flat order v = (k*ny + j)*nx + i: D (f32), W (f32) and the colour word
// b | g<<8 | r<<16 | has<<24 -- 12 bytes per voxel, each plane read and written coalesced by lanes that run along i.
//   k_tsdf_clear      D = 1, W = 0, colour 0.
//   k_tsdf_integrate  one LANE per voxel in flat order, one launch per view.  A voxel is read and written by its own lane only: no atomics,
//                     nothing depends on scheduling.  The camera row is cams[slot] with `slot` a kernel argument: wave-uniform, scalar
//                     loads (as in k_fuse_view).  The view's maps are read by data-dependent 8-byte gathers at the projected pixel.
//   k_tsdf_raycast    one LANE per pixel, one WAVE per 8 x 8 pixel tile (lane = 8*(y & 7) + (x & 7)), a workgroup = four tiles side by
//                     side (32 x 8 pixels).  The rays of a tile stay within a narrow pyramid, so at every step the 64 lanes gather their
//                     eight corners from a compact block of voxels (about the same few rows of a few slices); a row of 64 pixels would
//                     spread the same lanes over eight times the width in one direction and touch that many more cache lines per step.
//   k_tsdf_count      the crossings of a workgroup's voxels: three ballots per wave, summed through LDS.
//   k_geom_scan       (cspm_geom.h) turns the counts into exclusive offsets and the total.
//   k_tsdf_points     recomputes the crossings; rank = workgroup offset + crossings of the earlier waves + crossings of the wave's earlier
//                     lanes (mbcnt of the three ballots) + the lane's own earlier axes.  A record is two 16-byte stores (k_geom_cloud's).
// No LDS beyond the ballot sums, no atomics, no workgroup waits for another, no scratch.  Every product, sum, quotient, floor and square
// root is one IEEE f64 operation in the association the specification states (-ffp-contract=off, and the pragma below).
#pragma once
#include "cspm_fuse.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kTsdfBlock = 256;              // voxels (lanes) per workgroup of the clear, integrate, count and record passes
constexpr int kTsdfWaves = kTsdfBlock / kWave;
constexpr int kTsdfTileW = 32, kTsdfTileH = 8;  // pixels of a raycast workgroup: four 8 x 8 waves side by side
constexpr int kTsdfMaxSteps = 1 << 20;       // a ray takes at most this many samples (status 2 beyond)

struct TsdfVol {
  float *D, *W;
  uint32_t *C;
  double origin[3];
  double voxel, trunc, max_weight, min_cos, step;  // step = step_rel * trunc, computed once on the host
  int nx, ny, nz;
};
struct TsdfRayOut {     // device outputs of a raycast, each may be null
  double *depth;        // w*h
  double *normal;       // three planes of w*h
  uint32_t *pix;        // w*h packed b | g<<8 | r<<16
  uint8_t *bgr;         // 8UC3 rows of bgr_stride bytes
  size_t bgr_stride;
  uint8_t *status;      // w*h
};

__device__ __forceinline__ double tsdf_lerp(double a, double b, double t) { return a + t * (b - a); }
__device__ __forceinline__ double tsdf_centre(const TsdfVol &V, int a, int idx) { return V.origin[a] + ((double)idx + 0.5) * V.voxel; }
__device__ __forceinline__ double tsdf_round_colour(double v) { return floor(v + 0.5); }

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_clear(TsdfVol V, long long nvox) {
  const long long v = (long long)blockIdx.x * kTsdfBlock + (int)threadIdx.x;
  if (v >= nvox) return;
  V.D[v] = 1.0f;
  V.W[v] = 0.0f;
  V.C[v] = 0u;
}

// one view into the volume.  depth, normal, pix: the slot's maps (normal and pix are not read unless NORMALS / COLOUR)
template <bool NORMALS, bool COLOUR>
__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_integrate(const FuseCam *__restrict__ cams, int slot, const double *__restrict__ depth,
                                                               const double *__restrict__ normal, const uint32_t *__restrict__ pix, int w, int h,
                                                               long long n, TsdfVol V, long long nvox) {
  const long long v = (long long)blockIdx.x * kTsdfBlock + (int)threadIdx.x;
  if (v >= nvox) return;
  const int i = (int)(v % V.nx);
  const long long q = v / V.nx;
  const int j = (int)(q % V.ny), k = (int)(q / V.ny);
  const FuseCam &ck = cams[slot];
  const double C[3] = {tsdf_centre(V, 0, i), tsdf_centre(V, 1, j), tsdf_centre(V, 2, k)};
  double Q[3], fx, fy;
  long long m;
  fuse_cam(ck, C, Q);
  if (!fuse_project(ck, Q, w, h, &fx, &fy, &m)) return;  // behind, outside
  const double Z = depth[m];
  if (!(fuse_finite(Z) && Z > 0.0)) return;              // hole
  const double sdf = Z - Q[2];
  if (!(sdf >= -V.trunc)) return;                        // occluded
  if (NORMALS && V.min_cos > 0.0) {
    const double n0 = normal[m], n1 = normal[n + m], n2 = normal[2 * n + m];
    const double u = fx - ck.cx, wv = fy - ck.cy;
    const double X = (u * Z) / ck.f;
    const double Y = (wv * Z) / ck.f;
    const double num = (n0 * X + n1 * Y) + n2 * Z;
    const double ln = __dsqrt_rn((n0 * n0 + n1 * n1) + n2 * n2);
    const double ls = __dsqrt_rn((X * X + Y * Y) + Z * Z);
    const double c = (-num) / (ln * ls);
    if (!(c >= V.min_cos)) return;                       // grazing; a NaN fails
  }
  double d = sdf / V.trunc;
  if (d > 1.0) d = 1.0;
  const double Wo = (double)V.W[v];
  const double Wn = Wo + 1.0;
  V.D[v] = __double2float_rn(((double)V.D[v] * Wo + d) / Wn);
  V.W[v] = __double2float_rn(Wn > V.max_weight ? V.max_weight : Wn);
  if (COLOUR && sdf <= V.trunc) {
    const uint32_t old = V.C[v], px = pix[m];
    const double Wc = (old >> 24) != 0u ? Wo : 0.0;
    const double den = Wc + 1.0;
    uint32_t out = 1u << 24;
    for (int a = 0; a < 3; ++a) {
      const double co = (double)((old >> (8 * a)) & 255u), cn = (double)((px >> (8 * a)) & 255u);
      out |= (uint32_t)tsdf_round_colour((co * Wc + cn) / den) << (8 * a);
    }
    V.C[v] = out;
  }
}

// the cell of the world point P: false unless 0 <= floor(g) <= n - 2 on every axis (tested on the doubles, a NaN fails)
__device__ __forceinline__ bool tsdf_locate(const TsdfVol &V, const double P[3], long long *base, double fr[3]) {
  const int dim[3] = {V.nx, V.ny, V.nz};
  int c[3];
  for (int a = 0; a < 3; ++a) {
    const double g = (P[a] - V.origin[a]) / V.voxel - 0.5;
    const double fl = floor(g);
    if (!(fl >= 0.0 && fl <= (double)(dim[a] - 2))) return false;
    c[a] = (int)fl;
    fr[a] = g - fl;
  }
  *base = ((long long)c[2] * V.ny + c[1]) * V.nx + c[0];
  return true;
}
// corner q = dz*4 + dy*2 + dx of the cell at `base`
__device__ __forceinline__ long long tsdf_corner(const TsdfVol &V, long long base, int q) {
  return base + (q & 1) + (long long)((q >> 1) & 1) * V.nx + (long long)(q >> 2) * V.nx * V.ny;
}
// the eight corners' D as doubles; false when a corner has W = 0 (d is then not filled)
__device__ __forceinline__ bool tsdf_corners(const TsdfVol &V, long long base, double d[8]) {
  bool known = true;
  for (int q = 0; q < 8; ++q) known = known && V.W[tsdf_corner(V, base, q)] > 0.0f;
  if (!known) return false;
  for (int q = 0; q < 8; ++q) d[q] = (double)V.D[tsdf_corner(V, base, q)];
  return true;
}
__device__ __forceinline__ double tsdf_trilinear(const double d[8], const double fr[3]) {
  const double c00 = tsdf_lerp(d[0], d[1], fr[0]), c10 = tsdf_lerp(d[2], d[3], fr[0]);
  const double c01 = tsdf_lerp(d[4], d[5], fr[0]), c11 = tsdf_lerp(d[6], d[7], fr[0]);
  return tsdf_lerp(tsdf_lerp(c00, c10, fr[1]), tsdf_lerp(c01, c11, fr[1]), fr[2]);
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_raycast(FuseCam cam, TsdfVol V, int w, int h, double z_near, TsdfRayOut out) {
  const int tid = (int)threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int x = (int)blockIdx.x * kTsdfTileW + wave * 8 + (lane & 7);
  const int y = (int)blockIdx.y * kTsdfTileH + (lane >> 3);
  if (x >= w || y >= h) return;
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  const double dc[3] = {((double)x - cam.cx) / cam.f, ((double)y - cam.cy) / cam.f, 1.0};
  double dir[3];
  fuse_rot(cam, dc, dir);
  const int dim[3] = {V.nx, V.ny, V.nz};
  int status = 0;
  double l0 = z_near, l1 = __longlong_as_double(0x7FF0000000000000LL);
  bool in = V.nx >= 2 && V.ny >= 2 && V.nz >= 2;
  for (int a = 0; a < 3 && in; ++a) {
    const double lo = V.origin[a] + 0.5 * V.voxel;
    const double hi = V.origin[a] + ((double)dim[a] - 0.5) * V.voxel;
    if (dir[a] == 0.0) {
      in = cam.t[a] >= lo && cam.t[a] <= hi;
    } else {
      double ta = (lo - cam.t[a]) / dir[a];
      double tb = (hi - cam.t[a]) / dir[a];
      if (ta > tb) { const double s = ta; ta = tb; tb = s; }
      if (ta > l0) l0 = ta;
      if (tb < l1) l1 = tb;
    }
  }
  in = in && l0 <= l1;
  double depth = kNaN, lam_hit = kNaN;
  if (in) {
    status = 2;
    bool has_prev = false;
    double prev = 0.0, lam_prev = 0.0;
    for (int m = 0; m < kTsdfMaxSteps; ++m) {
      const double lam = l0 + (double)m * V.step;
      if (!(lam <= l1)) break;
      const double P[3] = {cam.t[0] + lam * dir[0], cam.t[1] + lam * dir[1], cam.t[2] + lam * dir[2]};
      long long base;
      double fr[3], d[8];
      if (!(tsdf_locate(V, P, &base, fr) && tsdf_corners(V, base, d))) {
        has_prev = false;
        continue;
      }
      const double cur = tsdf_trilinear(d, fr);
      if (cur > 0.0) {
        has_prev = true;
        prev = cur;
        lam_prev = lam;
        continue;
      }
      if (has_prev) {
        status = 1;
        lam_hit = lam_prev + (V.step * prev) / (prev - cur);
      } else {
        status = 3;
      }
      break;
    }
  }
  double N[3] = {kNaN, kNaN, kNaN};
  uint32_t px = 0u;
  if (status == 1) {
    depth = lam_hit;
    const double P[3] = {cam.t[0] + lam_hit * dir[0], cam.t[1] + lam_hit * dir[1], cam.t[2] + lam_hit * dir[2]};
    long long base;
    double fr[3], d[8];
    if (tsdf_locate(V, P, &base, fr) && tsdf_corners(V, base, d)) {
      double g[3];
      g[0] = tsdf_lerp(tsdf_lerp(d[1] - d[0], d[3] - d[2], fr[1]), tsdf_lerp(d[5] - d[4], d[7] - d[6], fr[1]), fr[2]);
      g[1] = tsdf_lerp(tsdf_lerp(d[2] - d[0], d[3] - d[1], fr[0]), tsdf_lerp(d[6] - d[4], d[7] - d[5], fr[0]), fr[2]);
      g[2] = tsdf_lerp(tsdf_lerp(d[4] - d[0], d[5] - d[1], fr[0]), tsdf_lerp(d[6] - d[2], d[7] - d[3], fr[0]), fr[1]);
      const double len = __dsqrt_rn((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
      const double nw[3] = {g[0] / len, g[1] / len, g[2] / len};
      for (int jx = 0; jx < 3; ++jx) N[jx] = (cam.R[jx] * nw[0] + cam.R[3 + jx] * nw[1]) + cam.R[6 + jx] * nw[2];
      uint32_t cw[8];
      bool coloured = true;
      for (int q = 0; q < 8; ++q) {
        cw[q] = V.C[tsdf_corner(V, base, q)];
        coloured = coloured && (cw[q] >> 24) != 0u;
      }
      if (coloured)
        for (int a = 0; a < 3; ++a) {
          double c[8];
          for (int q = 0; q < 8; ++q) c[q] = (double)((cw[q] >> (8 * a)) & 255u);
          px |= (uint32_t)tsdf_round_colour(tsdf_trilinear(c, fr)) << (8 * a);
        }
    }
  }
  const size_t n = (size_t)w * h, p = (size_t)y * w + x;
  if (out.depth) out.depth[p] = depth;
  if (out.normal) {
    out.normal[p] = N[0];
    out.normal[n + p] = N[1];
    out.normal[2 * n + p] = N[2];
  }
  if (out.pix) out.pix[p] = px;
  if (out.bgr) {
    uint8_t *row = out.bgr + (size_t)y * out.bgr_stride + 3 * (size_t)x;
    row[0] = (uint8_t)(px & 255u);
    row[1] = (uint8_t)((px >> 8) & 255u);
    row[2] = (uint8_t)((px >> 16) & 255u);
  }
  if (out.status) out.status[p] = (uint8_t)status;
}

// the crossings of voxel v towards +x, +y, +z: f[a] and the neighbour's flat index nb[a]
__device__ __forceinline__ void tsdf_crossings(const TsdfVol &V, long long v, long long nvox, int idx[3], bool f[3], long long nb[3]) {
  f[0] = f[1] = f[2] = false;
  if (v >= nvox) return;
  idx[0] = (int)(v % V.nx);
  const long long q = v / V.nx;
  idx[1] = (int)(q % V.ny);
  idx[2] = (int)(q / V.ny);
  if (!(V.W[v] > 0.0f)) return;
  const bool pos = V.D[v] > 0.0f;
  const int dim[3] = {V.nx, V.ny, V.nz};
  const long long stride[3] = {1, V.nx, (long long)V.nx * V.ny};
  for (int a = 0; a < 3; ++a) {
    if (idx[a] + 1 >= dim[a]) continue;
    nb[a] = v + stride[a];
    f[a] = V.W[nb[a]] > 0.0f && (V.D[nb[a]] > 0.0f) != pos;
  }
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_count(TsdfVol V, long long nvox, unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kTsdfWaves];
  const int tid = (int)threadIdx.x;
  const long long v = (long long)blockIdx.x * kTsdfBlock + tid;
  int idx[3];
  bool f[3];
  long long nb[3];
  tsdf_crossings(V, v, nvox, idx, f, nb);
  const unsigned int c = (unsigned int)(__popcll(__ballot(f[0])) + __popcll(__ballot(f[1])) + __popcll(__ballot(f[2])));
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = c;
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
    for (int q = 0; q < kTsdfWaves; ++q) s += s_wave[q];
    counts[blockIdx.x] = s;
  }
}

// the central-difference gradient of D at voxel (idx): a component is NaN when a neighbour is outside the volume or has W = 0
__device__ __forceinline__ void tsdf_gradient(const TsdfVol &V, long long v, const int idx[3], double G[3]) {
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  const int dim[3] = {V.nx, V.ny, V.nz};
  const long long stride[3] = {1, V.nx, (long long)V.nx * V.ny};
  for (int a = 0; a < 3; ++a) {
    G[a] = kNaN;
    if (idx[a] < 1 || idx[a] + 1 >= dim[a]) continue;
    const long long hi = v + stride[a], lo = v - stride[a];
    if (V.W[hi] > 0.0f && V.W[lo] > 0.0f) G[a] = (double)V.D[hi] - (double)V.D[lo];
  }
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_points(TsdfVol V, long long nvox, const unsigned int *__restrict__ offsets, uint4 *__restrict__ cloud,
                                                            unsigned int cap) {
  __shared__ unsigned int s_wave[kTsdfWaves];
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const long long v = (long long)blockIdx.x * kTsdfBlock + tid;
  int idx[3];
  bool f[3];
  long long nb[3];
  tsdf_crossings(V, v, nvox, idx, f, nb);
  unsigned int before = 0, all = 0;
  for (int a = 0; a < 3; ++a) {
    const unsigned long long ballot = __ballot(f[a]);
    before += __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
    all += (unsigned int)__popcll(ballot);
  }
  if ((tid & (kWave - 1)) == 0) s_wave[wave] = all;
  __syncthreads();
  if (!(f[0] || f[1] || f[2])) return;
  unsigned int rank = offsets[blockIdx.x] + before;
  for (int q = 0; q < wave; ++q) rank += s_wave[q];
  const double Da = (double)V.D[v];
  const uint32_t ca = V.C[v];
  double Ga[3];
  tsdf_gradient(V, v, idx, Ga);
  const double Ca[3] = {tsdf_centre(V, 0, idx[0]), tsdf_centre(V, 1, idx[1]), tsdf_centre(V, 2, idx[2])};
  for (int a = 0; a < 3; ++a) {
    if (!f[a]) continue;
    if (rank >= cap) return;
    int jdx[3] = {idx[0], idx[1], idx[2]};
    jdx[a] += 1;
    const double Db = (double)V.D[nb[a]];
    const double t = Da / (Da - Db);
    double Gb[3], G[3], P[3];
    tsdf_gradient(V, nb[a], jdx, Gb);
    for (int e = 0; e < 3; ++e) {
      P[e] = tsdf_lerp(Ca[e], tsdf_centre(V, e, jdx[e]), t);
      G[e] = tsdf_lerp(Ga[e], Gb[e], t);
    }
    const double len = __dsqrt_rn((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
    const uint32_t cb = V.C[nb[a]];
    uint32_t bgra = 0u;
    if ((ca >> 24) != 0u && (cb >> 24) != 0u) {
      bgra = 0xFF000000u;
      for (int e = 0; e < 3; ++e)
        bgra |= (uint32_t)tsdf_round_colour(tsdf_lerp((double)((ca >> (8 * e)) & 255u), (double)((cb >> (8 * e)) & 255u), t)) << (8 * e);
    }
    uint4 r0, r1;
    r0.x = __float_as_uint(__double2float_rn(P[0]));
    r0.y = __float_as_uint(__double2float_rn(P[1]));
    r0.z = __float_as_uint(__double2float_rn(P[2]));
    r0.w = __float_as_uint(__double2float_rn(G[0] / len));
    r1.x = __float_as_uint(__double2float_rn(G[1] / len));
    r1.y = __float_as_uint(__double2float_rn(G[2] / len));
    r1.z = bgra;
    r1.w = (uint32_t)v;
    cloud[2 * (size_t)rank] = r0;
    cloud[2 * (size_t)rank + 1] = r1;
    rank += 1;
  }
}

}  // namespace cspm
