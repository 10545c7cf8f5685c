// cspm_mesh.h -- a triangle mesh from a disparity map and its plane slopes (include/cspm.h "triangle meshes"): the
// specification M.  Two neighbouring pixels are connected when each one's plane predicts the other's disparity; a vertex is the pixel's
// point of G (cspm_geom.h), evaluated by geom_pixel itself, so a vertex and a cloud point of one pixel cannot differ by a bit.
//
// One LANE per pixel in flat raster order, kGeomBlock consecutive pixels per workgroup, so that wave and workgroup order is raster order;
// no atomics, no workgroup waits for another (the stance of sections 16 and 19).  After k_geom_dense has written `keep`:
//   k_mesh_quad    the quad whose origin is the pixel: reads the four corners (the row below at the same x: coalesced), writes the quad
//                  byte Q and the workgroup's number of faces (ballot popcounts of bit 0 and bit 1, summed through LDS).
//   k_mesh_use     is the pixel a vertex?  keep and the four quad bytes around it; writes the workgroup's number of vertices.
//   k_geom_scan    (cspm_geom.h) on both count arrays.
//   k_mesh_vertex  recomputes the pixel like k_geom_cloud; rank = workgroup offset + earlier waves + mbcnt.  Writes the pixel -> vertex
//                  map for every vertex and the record of the first `cap` of them.
//   k_mesh_face    rank = workgroup offset + faces of earlier waves + mbcnt of the bit-0 ballot + mbcnt of the bit-1 ballot; T0 goes to
//                  `rank`, T1 one record behind it when T0 exists.  Three 4-byte stores per face (a 12-byte record is 4-byte aligned).
// Every sum, product and difference of the edge test is one IEEE f64 operation in the association the specification states.
#pragma once
#include "cspm_geom.h"

#pragma clang fp contract(off)

namespace cspm {

struct MeshMaps {          // the per-pixel scratch of one mesh
  uint8_t *keep;           // W*H bytes: G's keep
  uint8_t *quad;           // W*H bytes: Q
  uint32_t *vmap;          // W*H: the vertex number of a pixel that is a vertex (not written elsewhere)
};

// the slopes of the edge test: the pixel's (A, Bs) when both are finite, else (0, 0)
template <bool SLOPES>
__device__ __forceinline__ void mesh_slopes(const GeomIn &in, long long i, double &a, double &b) {
  a = 0.0; b = 0.0;
  if (SLOPES) {
    const double A = in.a[i], Bs = in.b[i];
    const bool masked = in.slope_mask != nullptr && in.slope_mask[i] == 0;
    if (!masked && fabs(A) <= kDoubleMax && fabs(Bs) <= kDoubleMax) { a = A; b = Bs; }
  }
}

struct MeshCorner {
  double D, a, b;
  bool keep;
};

// pred(s,t) = (D_s + a_s * dx) + b_s * dy with (dx, dy) = t - s;  E = both predictions within tau
__device__ __forceinline__ bool mesh_edge(const MeshCorner &s, const MeshCorner &t, double dx, double dy, double tau) {
  const double pst = (s.D + s.a * dx) + s.b * dy;
  const double pts = (t.D + t.a * (-dx)) + t.b * (-dy);
  return fabs(pst - t.D) <= tau && fabs(pts - s.D) <= tau;
}

// is pixel (x, y) a corner of an emitted triangle?  the four quads it belongs to
__device__ __forceinline__ bool mesh_used(const uint8_t *__restrict__ Q, int W, int x, int y, long long i) {
  bool used = false;
  {  // p00 of its own quad: main T0 and T1, anti T0
    const unsigned q = Q[i];
    used = (q & 4u) ? (q & 1u) != 0 : (q & 3u) != 0;
  }
  if (x > 0) {  // p10 of the quad on the left: main T1, anti T0 and T1
    const unsigned q = Q[i - 1];
    used = used || ((q & 4u) ? (q & 3u) != 0 : (q & 2u) != 0);
  }
  if (y > 0) {  // p01 of the quad above: main T0, anti T0 and T1
    const unsigned q = Q[i - W];
    used = used || ((q & 4u) ? (q & 3u) != 0 : (q & 1u) != 0);
  }
  if (x > 0 && y > 0) {  // p11 of the quad above left: main T0 and T1, anti T1
    const unsigned q = Q[i - W - 1];
    used = used || ((q & 4u) ? (q & 2u) != 0 : (q & 3u) != 0);
  }
  return used;
}

// the workgroup's sum of a per-wave count -> counts[blockIdx.x]
__device__ __forceinline__ void mesh_block_count(unsigned int wave_count, unsigned int *s_wave, unsigned int *__restrict__ counts) {
  const int tid = (int)threadIdx.x;
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = wave_count;
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
    for (int w = 0; w < kGeomWaves; ++w) s += s_wave[w];
    counts[blockIdx.x] = s;
  }
}

// the quad pass: Q and the workgroup's face count
template <bool SLOPES>
__global__ __launch_bounds__(kGeomBlock) void k_mesh_quad(GeomIn in, const uint8_t *__restrict__ keep, int W, int H, long long n, double tau,
                                                          uint8_t *__restrict__ Q, unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const long long i = (long long)blockIdx.x * kGeomBlock + (int)threadIdx.x;
  unsigned q = 0;
  if (i < n) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    if (x < W - 1 && y < H - 1) {
      const long long idx[4] = {i, i + 1, i + W, i + W + 1};  // p00, p10, p01, p11: all below n
      MeshCorner c[4];
      for (int k = 0; k < 4; ++k) {
        c[k].keep = keep[idx[k]] != 0;
        c[k].D = in.disp[idx[k]];
        mesh_slopes<SLOPES>(in, idx[k], c[k].a, c[k].b);
      }
      const bool main_ok = c[0].keep && c[3].keep, anti_ok = c[1].keep && c[2].keep;
      if (main_ok || anti_ok) {
        const bool anti = main_ok && anti_ok ? !(fabs(c[0].D - c[3].D) <= fabs(c[1].D - c[2].D)) : anti_ok;
        bool t0, t1;
        if (!anti) {  // T0 = (p00, p01, p11), T1 = (p00, p11, p10)
          const bool diag = mesh_edge(c[0], c[3], 1.0, 1.0, tau);
          t0 = c[2].keep && diag && mesh_edge(c[0], c[2], 0.0, 1.0, tau) && mesh_edge(c[2], c[3], 1.0, 0.0, tau);
          t1 = c[1].keep && diag && mesh_edge(c[3], c[1], 0.0, -1.0, tau) && mesh_edge(c[1], c[0], -1.0, 0.0, tau);
        } else {      // T0 = (p00, p01, p10), T1 = (p10, p01, p11)
          const bool diag = mesh_edge(c[2], c[1], 1.0, -1.0, tau);
          t0 = c[0].keep && diag && mesh_edge(c[0], c[2], 0.0, 1.0, tau) && mesh_edge(c[1], c[0], -1.0, 0.0, tau);
          t1 = c[3].keep && diag && mesh_edge(c[2], c[3], 1.0, 0.0, tau) && mesh_edge(c[3], c[1], 0.0, -1.0, tau);
        }
        q = (t0 ? 1u : 0u) | (t1 ? 2u : 0u) | (anti ? 4u : 0u);
      }
    }
    Q[i] = (uint8_t)q;
  }
  const unsigned long long b0 = __ballot((q & 1u) != 0), b1 = __ballot((q & 2u) != 0);
  mesh_block_count((unsigned int)(__popcll(b0) + __popcll(b1)), s_wave, counts);
}

// the vertex-use pass: the workgroup's vertex count
__global__ __launch_bounds__(kGeomBlock) void k_mesh_use(const uint8_t *__restrict__ keep, const uint8_t *__restrict__ Q, int W, long long n, int all_vertices,
                                                         unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const long long i = (long long)blockIdx.x * kGeomBlock + (int)threadIdx.x;
  bool vert = false;
  if (i < n && keep[i] != 0) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    vert = all_vertices != 0 || mesh_used(Q, W, x, y, i);
  }
  mesh_block_count((unsigned int)__popcll(__ballot(vert)), s_wave, counts);
}

// the vertex pass: the pixel -> vertex map, and the first `cap` records (cloud == null or cap == 0: the map alone)
template <bool SLOPES>
__global__ __launch_bounds__(kGeomBlock) void k_mesh_vertex(GeomCam k, GeomIn in, const uint8_t *__restrict__ keep, const uint8_t *__restrict__ Q, int W,
                                                            long long n, int all_vertices, const unsigned int *__restrict__ offsets,
                                                            uint32_t *__restrict__ vmap, uint4 *__restrict__ cloud, unsigned int cap) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const long long i = (long long)blockIdx.x * kGeomBlock + tid;
  bool vert = false;
  if (i < n && keep[i] != 0) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    vert = all_vertices != 0 || mesh_used(Q, W, x, y, i);
  }
  const unsigned long long ballot = __ballot(vert);
  if ((tid & (kWave - 1)) == 0) s_wave[wave] = (unsigned int)__popcll(ballot);
  __syncthreads();
  if (!vert) return;
  unsigned int rank = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
  vmap[i] = rank;
  if (cloud == nullptr || rank >= cap) return;
  const GeomPix p = geom_pixel<SLOPES>(k, in, W, i);  // keep[i] is this function's own answer: the record is the cloud's
  uint32_t bgra = 0u;
  if (in.pix) bgra = (in.pix[i] & 0x00FFFFFFu) | 0xFF000000u;
  uint4 r0, r1;
  r0.x = __float_as_uint(__double2float_rn(p.X));
  r0.y = __float_as_uint(__double2float_rn(p.Y));
  r0.z = __float_as_uint(__double2float_rn(p.Z));
  r0.w = __float_as_uint(__double2float_rn(p.nx));
  r1.x = __float_as_uint(__double2float_rn(p.ny));
  r1.y = __float_as_uint(__double2float_rn(p.nz));
  r1.z = bgra;
  r1.w = (uint32_t)i;
  cloud[2 * (size_t)rank] = r0;
  cloud[2 * (size_t)rank + 1] = r1;
}

// the face pass: the first `cap` faces in raster order of the quad origin, T0 before T1
__global__ __launch_bounds__(kGeomBlock) void k_mesh_face(const uint8_t *__restrict__ Q, const uint32_t *__restrict__ vmap, int W, long long n,
                                                          const unsigned int *__restrict__ offsets, uint32_t *__restrict__ faces, unsigned int cap) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const long long i = (long long)blockIdx.x * kGeomBlock + tid;
  const unsigned q = i < n ? Q[i] : 0u;
  const bool t0 = (q & 1u) != 0, t1 = (q & 2u) != 0;
  const unsigned long long b0 = __ballot(t0), b1 = __ballot(t1);
  if ((tid & (kWave - 1)) == 0) s_wave[wave] = (unsigned int)(__popcll(b0) + __popcll(b1));
  __syncthreads();
  if (!t0 && !t1) return;
  unsigned int rank = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b0, 0u));
  rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b1, 0u));
  // a quad with a face is not in the last column or row: the three other corners exist, and every corner of a face is a vertex
  const uint32_t v00 = vmap[i], v11 = vmap[i + W + 1];
  const bool anti = (q & 4u) != 0;
  if (t0) {
    if (rank < cap) {
      uint32_t *f = faces + 3 * (size_t)rank;
      f[0] = v00;
      f[1] = vmap[i + W];
      f[2] = anti ? vmap[i + 1] : v11;
    }
    ++rank;
  }
  if (t1 && rank < cap) {
    uint32_t *f = faces + 3 * (size_t)rank;
    f[0] = anti ? vmap[i + 1] : v00;
    f[1] = anti ? vmap[i + W] : v11;
    f[2] = anti ? v11 : vmap[i + 1];
  }
}

}  // namespace cspm
