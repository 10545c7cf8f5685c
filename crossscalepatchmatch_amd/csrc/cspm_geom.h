// cspm_geom.h -- metric depth, camera-space points, unit normals and a compacted point cloud from a disparity map and its plane
// slopes (include/cspm.h "reprojection"): the specification G, one pixel at a time.
//
// geom_pixel() evaluates G for one pixel; every kernel that needs a pixel's values calls it, so the dense planes and the cloud
// cannot differ by a bit.  Three passes, no atomics, no workgroup waits for another (the stance of the speckle filter, section 16):
//   k_geom_dense  one LANE per pixel in flat raster order, kGeomBlock consecutive pixels per workgroup: wave and workgroup order is
//                 raster order.  Writes the requested dense planes and `keep` (coalesced 8-byte / 1-byte stores) and, when a cloud
//                 or a count is wanted, the workgroup's number of kept pixels: ballot popcount per wave, summed through LDS.
//   k_geom_scan   ONE workgroup turns the counts into exclusive offsets in place, kGeomScanBlock counts per pass with a carry,
//                 and writes the total.
//   k_geom_cloud  recomputes the pixel; rank = workgroup offset + kept pixels of the workgroup's earlier waves + mbcnt of the
//                 ballot.  A kept lane with rank < cap writes its 32-byte record as two 16-byte stores; a wave's records are contiguous.
// Every product, sum, quotient and square root is one IEEE f64 operation in the association the specification states
// (-ffp-contract=off, and the pragma below); `/` and __dsqrt_rn are correctly rounded on the device (section 17's precedent).
#pragma once
#include "cspm_device.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kGeomBlock = 256;       // pixels (lanes) per workgroup of the dense and cloud passes: 4 waves
constexpr int kGeomWaves = kGeomBlock / kWave;
constexpr int kGeomScanBlock = 1024;  // counts per pass of the scan's one workgroup: 16 waves

struct GeomCam {  // the calibration and parameters as the kernels need them; cxv and fB are computed once on the host
  double f, cxv, cy, baseline, doffs, fB;
  double z_near, z_far, min_cos;
  int add_baseline;  // left_frame && view == 1
};
struct GeomIn {
  const double *disp;         // W*H
  const uint8_t *valid;       // W*H bytes, or null: every pixel
  const double *a, *b;        // W*H slopes; not read by the kernels without slopes
  const uint8_t *slope_mask;  // W*H bytes or null: where 0 the pixel's slopes are NaN (a filled pixel has no plane of its own)
  const uint32_t *pix;        // W*H packed B | G<<8 | R<<16 (k_pack_bgr), or null: no colour
};
struct GeomOut {
  double *depth;   // W*H or null
  double *xyz;     // 3 planes of W*H or null
  double *normal;  // 3 planes of W*H or null
  uint8_t *keep;   // W*H bytes or null
};
struct GeomPix {
  double X, Y, Z, nx, ny, nz;
  bool ok, keep;
};

template <bool SLOPES>
__device__ __forceinline__ GeomPix geom_pixel(const GeomCam &k, const GeomIn &in, int W, long long i) {
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
  const double D = in.disp[i];
  const bool V = in.valid == nullptr || in.valid[i] != 0;
  GeomPix p;
  const double t = D + k.doffs;
  bool ok = V && fabs(D) <= kDoubleMax && t > 0.0;  // finite: false for NaN and for +-inf
  const double Z = k.fB / t;
  const double u = (double)x - k.cxv, wv = (double)y - k.cy;
  double X = (u * Z) / k.f;
  const double Y = (wv * Z) / k.f;
  if (k.add_baseline) X = X + k.baseline;
  ok = ok && Z >= k.z_near && Z <= k.z_far;
  p.X = X; p.Y = Y; p.Z = Z;
  p.ok = ok;
  p.nx = kNaN; p.ny = kNaN; p.nz = kNaN;
  p.keep = ok;
  if (SLOPES) {
    double A = in.a[i], Bs = in.b[i];
    if (in.slope_mask != nullptr && in.slope_mask[i] == 0) { A = kNaN; Bs = kNaN; }
    const double n0 = A * k.f, n1 = Bs * k.f, n2 = (t - A * u) - Bs * wv;
    const double len = __dsqrt_rn((n0 * n0 + n1 * n1) + n2 * n2);
    p.nx = -n0 / len; p.ny = -n1 / len; p.nz = -n2 / len;
    const double c = (k.f * t) / (len * __dsqrt_rn((u * u + wv * wv) + k.f * k.f));
    p.keep = ok && (k.min_cos == 0.0 || c >= k.min_cos);  // a NaN cosine fails the test
  }
  return p;
}

// pass 1: dense planes, keep, and the workgroup's kept count (counts == null: no cloud and no count were asked for)
template <bool SLOPES>
__global__ __launch_bounds__(kGeomBlock) void k_geom_dense(GeomCam k, GeomIn in, GeomOut out, int W, long long n, unsigned int *__restrict__ counts) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x;
  const long long i = (long long)blockIdx.x * kGeomBlock + tid;
  bool keep = false;
  if (i < n) {
    const GeomPix p = geom_pixel<SLOPES>(k, in, W, i);
    const double kNaN = __longlong_as_double(0x7FF8000000000000LL);
    keep = p.keep;
    if (out.depth) out.depth[i] = p.ok ? p.Z : kNaN;
    if (out.xyz) {
      out.xyz[i] = p.ok ? p.X : kNaN;
      out.xyz[n + i] = p.ok ? p.Y : kNaN;
      out.xyz[2 * n + i] = p.ok ? p.Z : kNaN;
    }
    if (SLOPES && out.normal) {
      out.normal[i] = p.ok ? p.nx : kNaN;
      out.normal[n + i] = p.ok ? p.ny : kNaN;
      out.normal[2 * n + i] = p.ok ? p.nz : kNaN;
    }
    if (out.keep) out.keep[i] = keep ? 1 : 0;
  }
  if (counts == nullptr) return;  // uniform over the grid
  const unsigned long long ballot = __ballot(keep);
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = (unsigned int)__popcll(ballot);
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
    for (int w = 0; w < kGeomWaves; ++w) s += s_wave[w];
    counts[blockIdx.x] = s;
  }
}

// pass 2: counts[0 .. nblocks) -> exclusive offsets, in place; *total = the sum.  One workgroup.
__global__ __launch_bounds__(kGeomScanBlock) void k_geom_scan(unsigned int *__restrict__ counts, int nblocks, unsigned int *__restrict__ total) {
  constexpr int kWaves = kGeomScanBlock / kWave;
  __shared__ unsigned int s_wave[kWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  unsigned int carry = 0;
  for (int base = 0; base < nblocks; base += kGeomScanBlock) {
    const int i = base + tid;
    const unsigned int v = i < nblocks ? counts[i] : 0u;
    unsigned int s = v;  // inclusive scan over the wave
    for (int d = 1; d < kWave; d <<= 1) {
      const unsigned int t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (lane == kWave - 1) s_wave[wave] = s;
    __syncthreads();
    unsigned int before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      const unsigned int t = s_wave[w];
      if (w < wave) before += t;
      all += t;
    }
    if (i < nblocks) counts[i] = carry + before + (s - v);
    carry += all;
    __syncthreads();  // s_wave is rewritten by the next pass
  }
  if (tid == 0) *total = carry;
}

// pass 3: the kept pixels' records in raster order, the first `cap` of them
template <bool SLOPES>
__global__ __launch_bounds__(kGeomBlock) void k_geom_cloud(GeomCam k, GeomIn in, int W, long long n, const unsigned int *__restrict__ offsets,
                                                           uint4 *__restrict__ cloud, unsigned int cap) {
  __shared__ unsigned int s_wave[kGeomWaves];
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const long long i = (long long)blockIdx.x * kGeomBlock + tid;
  GeomPix p{};
  p.keep = false;
  if (i < n) p = geom_pixel<SLOPES>(k, in, W, i);
  const unsigned long long ballot = __ballot(p.keep);
  if ((tid & (kWave - 1)) == 0) s_wave[wave] = (unsigned int)__popcll(ballot);
  __syncthreads();
  if (!p.keep) return;
  unsigned int rank = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  rank += __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
  if (rank >= cap) return;
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

}  // namespace cspm
