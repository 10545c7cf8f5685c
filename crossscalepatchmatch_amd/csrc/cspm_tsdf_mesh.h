// cspm_tsdf_mesh.h -- triangles of the TSDF volume's zero level set (include/cspm.h "TSDF meshes"): the
// specification MC.  The vertices ARE the surface points of cspm_tsdf.h, record for record; this file adds the connectivity.
//
// A cell is owned by the lane of its corner-0 voxel: one LANE per voxel in flat order, lanes along i, kTsdfBlock voxels per workgroup (the
// grid of k_tsdf_count).  The eight corners are the rows (j, k), (j+1, k), (j, k+1), (j+1, k+1) at columns i and i+1: eight coalesced loads
// of W, then eight of D; the i+1 column is a second load of the same rows one element on (the same cache lines but for one per row and wave),
// so the wave's last lane and the end of a row need no case of their own.
//   k_tsdf_first        first[v] = the rank of voxel v's first surface point: k_tsdf_points' rank arithmetic, written out for every voxel.
//   k_tsdf_mesh_count   the triangles of a workgroup's cells: the table's count per lane, summed over the wave by a butterfly of lane
//                       exchanges and over the waves through LDS.
//   k_geom_scan         (cspm_geom.h) turns the counts into exclusive offsets and the total.
//   k_tsdf_mesh_faces   recomputes the case; rank = workgroup offset + triangles of the earlier waves + triangles of the wave's earlier lanes
//                       (an inclusive scan by lane exchange: a SUM of counts 0 .. 5, not a ballot).  A triangle's three vertex numbers are
//                       first[] of the voxel that owns the edge plus that voxel's crossings on the axes before the edge's; a face is three
//                       4-byte stores, a lane's faces are contiguous.
// The case table (cspm_mc_table.h, generated) is 4 KiB of __constant__ memory read by per-lane index.  The triangle loop is unrolled so that
// every table byte is picked at a constant position: no per-lane array, no scratch.  No atomics, no workgroup waits for another.
#pragma once
#include "cspm_mc_table.h"
#include "cspm_tsdf.h"

namespace cspm {

constexpr int kMcMaxTris = 5;  // triangles of one cell at most (the table's largest count)
static_assert(1 + 3 * kMcMaxTris <= kMcRow, "a table row holds the count and three edge numbers per triangle");

// the case of the cell whose corner 0 is voxel v = (idx): -1 when there is no such cell or a corner has W = 0
__device__ __forceinline__ int tsdf_mesh_case(const TsdfVol &V, long long v, long long nvox, int idx[3]) {
  if (v >= nvox) return -1;
  idx[0] = (int)(v % V.nx);
  const long long q = v / V.nx;
  idx[1] = (int)(q % V.ny);
  idx[2] = (int)(q / V.ny);
  if (idx[0] + 2 > V.nx || idx[1] + 2 > V.ny || idx[2] + 2 > V.nz) return -1;
  bool known = true;
  for (int c = 0; c < 8; ++c) known = known && V.W[tsdf_corner(V, v, c)] > 0.0f;
  if (!known) return -1;
  int cs = 0;
  for (int c = 0; c < 8; ++c) cs |= (V.D[tsdf_corner(V, v, c)] > 0.0f ? 1 : 0) << c;
  return cs;
}
__device__ __forceinline__ unsigned int tsdf_mesh_tris(int cs) { return cs < 0 ? 0u : (unsigned int)kMcTable[cs][0]; }

// the number of the vertex on edge e = 4*a + u + 2*w of the cell at v = (idx) with case cs: first[] of the edge's voxel (its lower corner)
// plus that voxel's counted neighbours on the axes before a.  The voxel is a corner of a known cell: W > 0, and D > 0 iff its case bit.
__device__ __forceinline__ unsigned int tsdf_mesh_vertex(const TsdfVol &V, const unsigned int *__restrict__ first, long long v, const int idx[3], int cs,
                                                         int e) {
  const int a = e >> 2, u = e & 1, w = (e >> 1) & 1;
  const int o[3] = {a == 0 ? 0 : u, a == 0 ? u : (a == 1 ? 0 : w), a == 2 ? 0 : w};
  const long long vu = tsdf_corner(V, v, o[0] | o[1] << 1 | o[2] << 2);
  const bool pos = ((cs >> (o[0] | o[1] << 1 | o[2] << 2)) & 1) != 0;
  const int dim[3] = {V.nx, V.ny, V.nz};
  const long long stride[3] = {1, V.nx, (long long)V.nx * V.ny};
  unsigned int num = first[vu];
  for (int b = 0; b < 2; ++b) {
    if (b >= a || idx[b] + o[b] + 1 >= dim[b]) continue;
    const long long nb = vu + stride[b];
    if (V.W[nb] > 0.0f && (V.D[nb] > 0.0f) != pos) num += 1u;
  }
  return num;
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_first(TsdfVol V, long long nvox, const unsigned int *__restrict__ offsets, unsigned int *__restrict__ first) {
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
  if (v >= nvox) return;
  unsigned int rank = offsets[blockIdx.x] + before;
  for (int q = 0; q < wave; ++q) rank += s_wave[q];
  first[v] = rank;
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_mesh_count(TsdfVol V, long long nvox, unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kTsdfWaves];
  const int tid = (int)threadIdx.x;
  const long long v = (long long)blockIdx.x * kTsdfBlock + tid;
  int idx[3];
  unsigned int s = tsdf_mesh_tris(tsdf_mesh_case(V, v, nvox, idx));
  for (int d = kWave / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned int t = 0;
    for (int q = 0; q < kTsdfWaves; ++q) t += s_wave[q];
    counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_mesh_faces(TsdfVol V, long long nvox, const unsigned int *__restrict__ offsets,
                                                                const unsigned int *__restrict__ first, uint32_t *__restrict__ faces, unsigned int cap) {
  __shared__ unsigned int s_wave[kTsdfWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long v = (long long)blockIdx.x * kTsdfBlock + tid;
  int idx[3];
  const int cs = tsdf_mesh_case(V, v, nvox, idx);
  const unsigned int cnt = tsdf_mesh_tris(cs);
  unsigned int s = cnt;  // inclusive scan over the wave
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned int t = __shfl_up(s, d);
    if (lane >= d) s += t;
  }
  if (lane == kWave - 1) s_wave[wave] = s;
  __syncthreads();
  if (cnt == 0) return;
  unsigned int rank = offsets[blockIdx.x] + (s - cnt);
  for (int q = 0; q < wave; ++q) rank += s_wave[q];
  const uint4 row = *reinterpret_cast<const uint4 *>(kMcTable[cs]);
  const unsigned int word[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
  for (int t = 0; t < kMcMaxTris; ++t) {
    if ((unsigned int)t >= cnt || rank >= cap) return;
    uint32_t *out = faces + 3 * (size_t)rank;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int at = 1 + 3 * t + m;  // a constant: the unrolled loops pick the byte without indexing
      out[m] = tsdf_mesh_vertex(V, first, v, idx, cs, (int)((word[at / 4] >> (8 * (at % 4))) & 255u));
    }
    rank += 1;
  }
}

}  // namespace cspm
