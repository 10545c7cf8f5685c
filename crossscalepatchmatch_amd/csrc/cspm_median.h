// cspm_median.h -- the plain median filter (an addition), the last and optional step of PostProcessing and two
// stand-alone entries.  Window: the (2r+1)^2 taps D[clamp(y+j, 0, h-1)][clamp(x+i, 0, w-1)], i, j in -r .. r.
//   M8   u8, 1 .. 4 interleaved channels: the tap of 0-based rank 2r^2 + 2r per channel
//   M64  f64: a NaN tap does not vote, a NaN centre stays (its own bits); otherwise the tap of rank (n - 1) / 2 among the n voting taps
//        in the order of the order-preserving 64-bit key of the bit pattern; the output is that tap's bits
//
// One workgroup per 64 x 16 tile, view and channel; a wavefront owns one tile row at a time (four rows each, as in k_speckle_tiles).
// The tile and its clamped halo of r are staged in LDS once: bytes for u8, keys for f64 with a NaN tap staged as the all-ones key (the
// key of a NaN pattern, above +inf: no vote ever reaches it because the rank stays below n).  Selection descends from the most
// significant bit: every round counts the staged taps that agree with the prefix found so far and have the round's bit clear; the rank
// tells on which side the answer lies.  8 rounds for bytes, 64 for keys, the same instruction stream in every lane, nothing kept per tap
// in registers.  The 64 lanes of a wavefront read 64 consecutive bytes (16 dwords, each broadcast to four lanes) or 64 consecutive
// 8-byte keys (every bank once per half-wave) of one staged row: no bank conflict for any row stride.  No atomics; no workgroup waits for
// another; source and destination never alias (the callers see to it), so no lane reads what the launch wrote.
#pragma once
#include "cspm_kernels.h"

namespace cspm {

constexpr int kMedTileW = 64;
constexpr int kMedTileH = 16;
constexpr int kMedBlock = 256;  // four wavefronts, four tile rows each
constexpr int kMedOwn = kMedTileH * kMedTileW / kMedBlock;
constexpr int kMedMaxR = 7;  // CSPM_MEDIAN_MAX_RADIUS

// RT = 1, 2, 3: the radius at compile time (window loops unrolled, LDS sized for it); RT = 0: the radius is an argument, 1 .. kMedMaxR
template <int RT>
struct MedGeom {
  static constexpr int kR = RT ? RT : kMedMaxR;
  static constexpr int kSW = kMedTileW + 2 * kR;  // staged row stride, elements
  static constexpr int kSH = kMedTileH + 2 * kR;
  static constexpr int kUnroll = RT ? 2 * RT + 1 : 1;  // the window loops: unrolled where the radius is known
  static constexpr int kUnrollBits = RT ? 8 : 1;       // the eight rounds of M8 likewise
};

__device__ __forceinline__ int med_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// order-preserving key of an f64 bit pattern: -inf < finite < +inf, -0.0 < +0.0
__device__ __forceinline__ unsigned long long med_key(unsigned long long u) { return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
__device__ __forceinline__ unsigned long long med_unkey(unsigned long long k) { return (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k; }
__device__ __forceinline__ bool med_is_nan(unsigned long long u) { return (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }

// M8.  grid (tiles_x * tiles_y, channels, views); src / dst rows are sstride / dstride bytes apart, pixels cn bytes.
template <int RT>
__global__ __launch_bounds__(kMedBlock) void k_median_u8(const uint8_t *__restrict__ src0, const uint8_t *__restrict__ src1, uint8_t *__restrict__ dst0,
                                                        uint8_t *__restrict__ dst1, size_t sstride, size_t dstride, int W, int H, int cn, int r_arg) {
  using G = MedGeom<RT>;
  __shared__ uint8_t s[G::kSW * G::kSH];
  const int r = RT ? RT : r_arg;
  const uint8_t *src = blockIdx.z ? src1 : src0;
  uint8_t *dst = blockIdx.z ? dst1 : dst0;
  const int ch = (int)blockIdx.y;
  const unsigned tiles_x = (unsigned)(W + kMedTileW - 1) / kMedTileW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kMedTileW, y0 = (int)(blockIdx.x / tiles_x) * kMedTileH;
  const int sw = kMedTileW + 2 * r, sh = kMedTileH + 2 * r;
  for (int i = (int)threadIdx.x; i < sw * sh; i += kMedBlock) {
    const int sy = i / sw, sx = i - sy * sw;
    const int gy = med_clamp(y0 + sy - r, H - 1), gx = med_clamp(x0 + sx - r, W - 1);
    s[sy * G::kSW + sx] = src[(size_t)gy * sstride + (size_t)gx * cn + ch];
  }
  __syncthreads();
  const int c = (int)threadIdx.x & (kMedTileW - 1), r0 = (int)threadIdx.x / kMedTileW;
  const int x = x0 + c, side = 2 * r + 1;
  for (int k = 0; k < kMedOwn; ++k) {
    const int row = r0 + k * (kMedBlock / kMedTileW), y = y0 + row;
    const uint8_t *win = s + row * G::kSW + c;  // the window's upper left tap
    int rank = 2 * r * r + 2 * r;
    unsigned prefix = 0;
#pragma unroll G::kUnrollBits
    for (int b = 7; b >= 0; --b) {
      int below = 0;  // taps that share the prefix above bit b and have bit b clear
#pragma unroll G::kUnroll
      for (int j = 0; j < (RT ? 2 * RT + 1 : side); ++j)
#pragma unroll G::kUnroll
        for (int i = 0; i < (RT ? 2 * RT + 1 : side); ++i) below += (((unsigned)win[j * G::kSW + i] ^ prefix) >> b) == 0;
      const bool up = rank >= below;
      rank -= up ? below : 0;
      prefix |= up ? 1u << b : 0u;
    }
    if (x < W && y < H) dst[(size_t)y * dstride + (size_t)x * cn + ch] = (uint8_t)prefix;
  }
}

// M64 on packed W x H maps of f64 bit patterns.  grid (tiles_x * tiles_y, views).
template <int RT>
__global__ __launch_bounds__(kMedBlock) void k_median_f64(const unsigned long long *__restrict__ src0, const unsigned long long *__restrict__ src1,
                                                         unsigned long long *__restrict__ dst0, unsigned long long *__restrict__ dst1, int W, int H,
                                                         int r_arg) {
  using G = MedGeom<RT>;
  __shared__ unsigned long long s[G::kSW * G::kSH];
  const int r = RT ? RT : r_arg;
  const unsigned long long *src = blockIdx.y ? src1 : src0;
  unsigned long long *dst = blockIdx.y ? dst1 : dst0;
  const unsigned tiles_x = (unsigned)(W + kMedTileW - 1) / kMedTileW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kMedTileW, y0 = (int)(blockIdx.x / tiles_x) * kMedTileH;
  const int sw = kMedTileW + 2 * r, sh = kMedTileH + 2 * r;
  for (int i = (int)threadIdx.x; i < sw * sh; i += kMedBlock) {
    const int sy = i / sw, sx = i - sy * sw;
    const int gy = med_clamp(y0 + sy - r, H - 1), gx = med_clamp(x0 + sx - r, W - 1);
    const unsigned long long u = src[(size_t)gy * W + gx];
    s[sy * G::kSW + sx] = med_is_nan(u) ? ~0ull : med_key(u);
  }
  __syncthreads();
  const int c = (int)threadIdx.x & (kMedTileW - 1), r0 = (int)threadIdx.x / kMedTileW;
  const int x = x0 + c, side = 2 * r + 1;
  for (int k = 0; k < kMedOwn; ++k) {
    const int row = r0 + k * (kMedBlock / kMedTileW), y = y0 + row;
    const unsigned long long *win = s + row * G::kSW + c;
    int votes = 0;
#pragma unroll G::kUnroll
    for (int j = 0; j < (RT ? 2 * RT + 1 : side); ++j)
#pragma unroll G::kUnroll
      for (int i = 0; i < (RT ? 2 * RT + 1 : side); ++i) votes += win[j * G::kSW + i] != ~0ull;
    // votes == 0 only under a NaN centre (the centre votes otherwise), whose output is not the selection's
    int rank = votes > 0 ? (votes - 1) / 2 : 0;
    unsigned long long prefix = 0;
    for (int b = 63; b >= 0; --b) {
      int below = 0;
#pragma unroll G::kUnroll
      for (int j = 0; j < (RT ? 2 * RT + 1 : side); ++j)
#pragma unroll G::kUnroll
        for (int i = 0; i < (RT ? 2 * RT + 1 : side); ++i) below += ((win[j * G::kSW + i] ^ prefix) >> b) == 0;
      const bool up = rank >= below;
      rank -= up ? below : 0;
      prefix |= up ? 1ull << b : 0ull;
    }
    if (x < W && y < H) {
      const size_t g = (size_t)y * W + x;
      const unsigned long long centre = src[g];
      dst[g] = med_is_nan(centre) ? centre : med_unkey(prefix);
    }
  }
}

}  // namespace cspm
