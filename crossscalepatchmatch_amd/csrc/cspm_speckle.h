// cspm_speckle.h -- the speckle filter of PostProcessing (an addition): connected-component labelling on the
// device.  S(D, V, max_size, max_diff) -> V':  nodes are the pixels with V = 1; two 4-neighbours are joined when |D[p] - D[q]| <= thr in
// f64 (false for a NaN); n(p) = size of p's component (0 for a non-node); V'[p] = V[p] && n(p) > max_size.
//
// Label equivalence in two levels.  A label is a 32-bit pixel index; parent[p] <= p always, a root has parent[p] == p.
//   k_speckle_tiles   one workgroup per 64 x 16 tile and view: union-find over the tile's links in LDS; writes parent[p] = the tile-local
//                     root (as a global pixel index) and cnt[p] = the tile-local component size at that root, 0 elsewhere
//   k_speckle_borders one lane per pixel: the links that cross a tile border, united on the global parents with atomicMin
//   k_speckle_sizes   every tile-local root that is not its component's root adds its size to the root's (atomicAdd)
//   k_speckle_apply   n(p) = cnt[root(p)]; the mask update, the removed-pixel count, optionally n(p) itself
// No workgroup waits for another: no spin-wait, no grid-wide sync; the launches are the only ordering.  Integer min and add commute, so
// the partition, the sizes and the masks do not depend on scheduling (which node ends up as a component's root is not part of the result).
#pragma once
#include "cspm_kernels.h"

namespace cspm {

constexpr int kSpkTileW = 64;   // a wavefront owns one tile row at a time: its 64 labels are 64 consecutive dwords of LDS, one per bank
constexpr int kSpkTileH = 16;
constexpr int kSpkBlock = 256;  // four wavefronts, four tile rows each
constexpr int kSpkTilePx = kSpkTileW * kSpkTileH;
constexpr int kSpkOwn = kSpkTilePx / kSpkBlock;

// one view's map, mask and scratch (parent and cnt: n int32 each)
template <class T>
struct SpkView {
  const T *d;
  uint8_t *valid;
  int *parent, *cnt;
};
template <class T>
struct SpkViews { SpkView<T> v[2]; };

__device__ __forceinline__ bool spk_joined(double a, double b, double thr) { return fabs(a - b) <= thr; }

// Unite the sets of a and b in the forest L (LDS or global; every access is an atomicMin, so a value read is never stale).
// What the forest and the pairs still being united connect never shrinks: with a > b and old = L[a] before the atomicMin,
//   old == a            a was a root and now hangs under b: done;
//   old <  a, old <= b  L[a] is unchanged, a ~ old holds through it, and old and b remain to be united;
//   old <  a, old >  b  L[a] = b replaces the edge a - old, and old and b remain to be united.
// TERMINATION: L[x] <= x for every x, and an atomicMin with b < a keeps that: parent labels only ever decrease.  So old <= a, and every
// round either ends or replaces the pair (a, b) by (old, b) with old < a and b < a: max(a, b) strictly decreases and is bounded by 0 --
// at most max(a, b) rounds whatever other lanes and workgroups do, and nothing is waited for.
__device__ __forceinline__ void spk_unite(int *L, int a, int b) {
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) break;
    a = old;
  }
}

// the root of p.  TERMINATION: every step goes to L[p] < p (parent labels only ever decrease along a path), at most p steps.  Called
// only where no launch-mate writes L: after the barrier in k_speckle_tiles, and in the launches after k_speckle_borders.
__device__ __forceinline__ int spk_root(const int *L, int p) {
  for (int q = L[p]; q != p; q = L[p]) p = q;
  return p;
}

// Tile-local labelling in LDS.  grid (tiles_x * tiles_y, views), kSpkBlock lanes.  Pixels of the tile outside the image are non-nodes.
template <class T>
__global__ __launch_bounds__(kSpkBlock) void k_speckle_tiles(SpkViews<T> views, int W, int H, double thr) {
  __shared__ double val[kSpkTilePx];
  __shared__ int lab[kSpkTilePx];  // the tile's forest over local indices r * 64 + c; -1 = not a node
  __shared__ int cnt[kSpkTilePx];
  const SpkView<T> V = blockIdx.y ? views.v[1] : views.v[0];  // a select, not an index: the argument stays in registers
  const unsigned tiles_x = (unsigned)(W + kSpkTileW - 1) / kSpkTileW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kSpkTileW, y0 = (int)(blockIdx.x / tiles_x) * kSpkTileH;
  const int c = (int)threadIdx.x & (kSpkTileW - 1), r0 = (int)threadIdx.x / kSpkTileW;
  const int x = x0 + c;
#pragma unroll
  for (int k = 0; k < kSpkOwn; ++k) {
    const int r = r0 + k * (kSpkBlock / kSpkTileW), p = r * kSpkTileW + c, y = y0 + r;
    const bool in = x < W && y < H;
    const size_t g = in ? (size_t)y * W + x : 0;
    val[p] = in ? (double)V.d[g] : 0.0;
    lab[p] = in && V.valid[g] != 0 ? p : -1;
    cnt[p] = 0;
  }
  __syncthreads();
  // the links to the right and downwards inside the tile (lab[q] >= 0 is all that is read of a neighbour: a node's label stays >= 0)
#pragma unroll
  for (int k = 0; k < kSpkOwn; ++k) {
    const int r = r0 + k * (kSpkBlock / kSpkTileW), p = r * kSpkTileW + c;
    if (lab[p] < 0) continue;
    if (c + 1 < kSpkTileW && lab[p + 1] >= 0 && spk_joined(val[p], val[p + 1], thr)) spk_unite(lab, p + 1, p);
    if (r + 1 < kSpkTileH && lab[p + kSpkTileW] >= 0 && spk_joined(val[p], val[p + kSpkTileW], thr)) spk_unite(lab, p + kSpkTileW, p);
  }
  __syncthreads();
  int root[kSpkOwn];
#pragma unroll
  for (int k = 0; k < kSpkOwn; ++k) {
    const int p = (r0 + k * (kSpkBlock / kSpkTileW)) * kSpkTileW + c;
    root[k] = lab[p] < 0 ? -1 : spk_root(lab, p);
    if (root[k] >= 0) atomicAdd(&cnt[root[k]], 1);
  }
  __syncthreads();
  // local raster order is global raster order inside a tile: the local root's pixel index is <= the pixel's own
#pragma unroll
  for (int k = 0; k < kSpkOwn; ++k) {
    const int r = r0 + k * (kSpkBlock / kSpkTileW), p = r * kSpkTileW + c, y = y0 + r;
    if (x >= W || y >= H) continue;
    const size_t g = (size_t)y * W + x;
    const int q = root[k];
    V.parent[g] = q < 0 ? (int)g : (y0 + q / kSpkTileW) * W + x0 + (q & (kSpkTileW - 1));
    V.cnt[g] = q == p ? cnt[p] : 0;
  }
}

// The links across tile borders: pixel (x, y) with its left neighbour where x is a multiple of 64, with its upper one where y is a
// multiple of 16.  grid (ceil(n / 256), views).  A non-node has parent[p] == p and cnt[p] == 0 and is never united.
template <class T>
__global__ void k_speckle_borders(SpkViews<T> views, int W, int H, double thr) {
  const SpkView<T> V = blockIdx.y ? views.v[1] : views.v[0];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const bool left = x > 0 && (x & (kSpkTileW - 1)) == 0, up = y > 0 && (y & (kSpkTileH - 1)) == 0;
  if ((!left && !up) || V.valid[i] == 0) return;
  const double d = (double)V.d[i];
  if (left && V.valid[i - 1] != 0 && spk_joined(d, (double)V.d[i - 1], thr)) spk_unite(V.parent, (int)i, (int)i - 1);
  if (up && V.valid[i - W] != 0 && spk_joined(d, (double)V.d[i - W], thr)) spk_unite(V.parent, (int)i, (int)i - W);
}

// Component sizes at the roots.  Only tile-local roots carry a count; a component's root is one of them (a pixel that is not a
// tile-local root has parent[p] < p from the start and never becomes a root) and only receives.  What a lane reads of cnt[p] and then
// uses belongs to a non-root, which no lane adds to.
__global__ void k_speckle_sizes(const int *__restrict__ parent0, const int *__restrict__ parent1, int *cnt0, int *cnt1, long long n) {
  const int *parent = blockIdx.y ? parent1 : parent0;
  int *cnt = blockIdx.y ? cnt1 : cnt0;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = cnt[i];
  if (s == 0) return;
  const int r = spk_root(parent, (int)i);
  if (r != (int)i) atomicAdd(&cnt[r], s);
}

// V'[p] = V[p] && n(p) > max_size, in place; removed += pixels taken out of the mask; size_out (may be null) = n(p).
__global__ void k_speckle_apply(const int *__restrict__ parent0, const int *__restrict__ parent1, const int *__restrict__ cnt0,
                                const int *__restrict__ cnt1, uint8_t *__restrict__ valid0, uint8_t *__restrict__ valid1, long long n, int max_size,
                                unsigned int *removed, int *__restrict__ size_out) {
  const int *parent = blockIdx.y ? parent1 : parent0, *cnt = blockIdx.y ? cnt1 : cnt0;
  uint8_t *valid = blockIdx.y ? valid1 : valid0;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool gone = false;
  if (i < n) {
    const bool ok = valid[i] != 0;
    const int size = ok ? cnt[spk_root(parent, (int)i)] : 0;
    gone = ok && size <= max_size;
    if (gone) valid[i] = 0;
    if (size_out) size_out[i] = size;
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(gone);
  if (b != 0 && (int)threadIdx.x % kWave == __builtin_ctzll(b)) atomicAdd(removed, (unsigned int)__builtin_popcountll(b));
}

}  // namespace cspm
