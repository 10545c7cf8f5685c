// cspm_pp.h -- sub-pixel PostProcessing on the unquantised plane disparities (an addition).
//
// The reference post-processes its 8-bit maps only (cs_patchmatch.cc:347-588; k_lr_check / k_fill_rows / k_weighted_median of
// cspm_kernels.h).  These kernels run the same three steps on d = a*x + b*y + c in f64:
//   k_lr_check_f64          one lane per pixel and view: the consistency flag of the f64 maps
//   k_fill_rows<FillF64>    the row scan of k_fill_rows; an inconsistent pixel takes the nearer side's plane evaluated AT the pixel,
//                           not rounded, clamped to [0, max_dis]
//   k_weighted_median_f64   one WAVEFRONT per listed pixel.  "Bin" of the reference's histogram = distinct value: the window's
//                           contributions are compacted into wave-private LDS in window order, sorted by (value bits, window
//                           rank) with a bitonic network, and every run of equal values is summed serially in window order -- the
//                           sums a 2^63-bin histogram would hold, bit for bit.
#pragma once
#include "cspm_kernels.h"

#pragma clang fp contract(off)

namespace cspm {

// LeftRightCheck (:347-369) on the f64 maps.  The maps hold the raw plane disparities of both views.
__global__ void k_lr_check_f64(const double *__restrict__ d0, const double *__restrict__ d1, int W, int H, uint8_t *__restrict__ ok0,
                               uint8_t *__restrict__ ok1) {
  const long long n = (long long)W * H;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  const int v = i >= n ? 1 : 0;
  i -= v * n;
  const double *mine = v ? d1 : d0, *theirs = v ? d0 : d1;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const double d = mine[i];
  const long long ox = (long long)x + (long long)(2 * v - 1) * (long long)round2int(d);
  bool ok = false;
  if (ox >= 0 && ox < W) ok = fabs(d - theirs[(long long)y * W + ox]) <= 0.5 && d > 0.0;
  (v ? ok1 : ok0)[i] = ok ? 1 : 0;
}

// what k_fill_rows stores for an inconsistent pixel of the f64 maps: the value itself, clamped like saturate_cast clamps the 8-bit one
struct FillF64 {
  double max_dis;
  double *d0, *d1;
  __device__ __forceinline__ void store(int v, long long i, double d) const { (v ? d1 : d0)[i] = d < 0.0 ? 0.0 : (d > max_dis ? max_dis : d); }
};

constexpr int kPpWnd = 35;                      // WeightedMedian's window (cs_patchmatch.cc:571)
constexpr int kPpMaxEntries = kPpWnd * kPpWnd;  // 1225 contributions at most
constexpr int kPpSlots = 2048;                  // the bitonic network's largest size
constexpr int kPpOwn = (kPpMaxEntries + kWave - 1) / kWave;  // sorted entries a lane owns (entry k belongs to lane k % 64)
constexpr int kPpGrid = 10;                     // workgroups per CU of a launch (5 are resident: 30 KB of LDS each)

// Wave-private LDS, structure of arrays: consecutive lanes touch consecutive 8-byte keys at every compare-exchange distance >= 32,
// and at the short distances a 32-lane group spreads over 64 banks two deep at worst -- an array of 16- or 24-byte structs would
// put every lane of a group on the same bank pair.  30336 bytes: five single-wave workgroups per CU.
struct PpWave {
  unsigned long long val[kPpSlots];  // bits of the contributed disparities (> 0.0 and finite: the bits order like the values)
  double wgt[kPpMaxEntries + 7];     // window order first, sorted order after the sort; 4 slots of slack for the run sums' block reads
  unsigned short idx[kPpSlots];      // window rank (position in the compacted window order): ties of the sort keep window order
};

// WeightedMedian(valid, 35, WMF_GAMMA) (:430-506) of the f64 maps: inconsistent pixels only, consistent neighbours only.  Every sum
// is a dependent f64 chain in the order DESIGN.md section 12 states: sum_wgt over the window (rows outer, columns inner), each
// distinct value's weights in window order, the walk over the distinct values in ascending order.
__global__ __launch_bounds__(kWave) void k_weighted_median_f64(const uint32_t *__restrict__ pix0, const uint32_t *__restrict__ pix1, int Wp, int pad, int W,
                                                               int H, const uint8_t *__restrict__ ok0, const uint8_t *__restrict__ ok1,
                                                               const double *__restrict__ lut, double *__restrict__ d0, double *__restrict__ d1,
                                                               const unsigned int *__restrict__ todo, const unsigned int *__restrict__ todo_cnt) {
  __shared__ PpWave S;
  constexpr int half_wnd = kPpWnd / 2;
  const int lane = (int)threadIdx.x;
  const long long n = (long long)W * H;
  for (int v = 0; v < 2; ++v) {
    const uint32_t *pix = v ? pix1 : pix0;
    const uint8_t *ok = v ? ok1 : ok0;
    double *dmap = v ? d1 : d0;
    const unsigned int total_px = todo_cnt[v];
    for (unsigned int item = blockIdx.x; item < total_px; item += gridDim.x) {
      const unsigned int i = todo[(size_t)v * n + item];
      const int y = (int)(i / (unsigned int)W), x = (int)(i - (unsigned int)y * (unsigned int)W);
      const uint32_t centre = pix[(size_t)y * Wp + pad + x];
      const int qx = x - half_wnd + lane;
      const bool col_in = lane < kPpWnd && qx >= 0 && qx < W;
      const int y_lo = max(0, y - half_wnd), y_hi = min(H - 1, y + half_wnd);
      // 1. gather: the consistent neighbours' (value bits, weight), compacted in window order
      int cnt = 0;  // wave-uniform
      for (int qy0 = y_lo; qy0 <= y_hi; qy0 += kMedianRows) {
        unsigned long long bits[kMedianRows];
        double wgt[kMedianRows];
        bool use[kMedianRows];
#pragma unroll
        for (int r = 0; r < kMedianRows; ++r) {  // independent gathers of up to kMedianRows window rows
          const int qy = min(qy0 + r, y_hi);
          const size_t q = (size_t)qy * W + (col_in ? qx : x);
          use[r] = col_in && qy0 + r <= y_hi && ok[q] != 0;
          bits[r] = (unsigned long long)__double_as_longlong(dmap[q]);  // a consistent pixel's value is never written by this kernel
          wgt[r] = lut[__builtin_amdgcn_sad_u8(centre, pix[(size_t)qy * Wp + pad + (col_in ? qx : x)], 0u)];
        }
#pragma unroll
        for (int r = 0; r < kMedianRows; ++r) {
          const unsigned long long b = __builtin_amdgcn_ballot_w64(use[r]);
          const int slot = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u));
          if (use[r]) {  // slot < 1225: at most 35 lanes of at most 35 rows
            S.val[slot] = bits[r];
            S.wgt[slot] = wgt[r];
            S.idx[slot] = (unsigned short)slot;
          }
          cnt += __builtin_popcountll(b);
        }
      }
      wave_lds_fence();
      // sum_wgt: one chain over the window order (every lane runs it on the same broadcast reads)
      double total = 0.0;
#pragma unroll 8
      for (int m = 0; m < cnt; ++m) total += S.wgt[m];
      const double half_total = total / 2.0;
      if (half_total > 0.0) {  // else no consistent neighbour: the filled value stays
        // 2. sort by (value, window rank): a bitonic network over the next power of two, the tail padded with keys above every value
        int np2 = 2 * kWave;
        while (np2 < cnt) np2 <<= 1;
        for (int k = cnt + lane; k < np2; k += kWave) {
          S.val[k] = ~0ULL;
          S.idx[k] = (unsigned short)k;
        }
        wave_lds_fence();
        for (int k = 2; k <= np2; k <<= 1) {
          for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (np2 >> 1); p += kWave) {
              const int a = 2 * p - (p & (j - 1)), b = a + j;  // a < b < np2 <= kPpSlots
              const bool up = (a & k) == 0;
              const unsigned long long va = S.val[a], vb = S.val[b];
              const unsigned short ia = S.idx[a], ib = S.idx[b];
              const bool gt = va > vb || (va == vb && ia > ib);
              if (gt == up) {
                S.val[a] = vb; S.val[b] = va;
                S.idx[a] = ib; S.idx[b] = ia;
              }
            }
            wave_lds_fence();
          }
        }
        // 3. the weights into sorted order (through registers: the permutation is in place)
        double reg[kPpOwn];
#pragma unroll
        for (int j = 0; j < kPpOwn; ++j) {
          const int k = lane + kWave * j;
          reg[j] = k < cnt ? S.wgt[S.idx[k]] : 0.0;
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kPpOwn; ++j) {
          const int k = lane + kWave * j;
          if (k < cnt) S.wgt[k] = reg[j];
        }
        wave_lds_fence();
        // 4. bin(u): a lane takes the whole run of every run head it owns and adds its weights serially (window order within the
        //    run); four entries are fetched together so a long run pays one LDS round trip per four additions
        unsigned int heads = 0;
#pragma unroll
        for (int j = 0; j < kPpOwn; ++j) {
          const int k = lane + kWave * j;
          reg[j] = 0.0;
          if (k < cnt && (k == 0 || S.val[k - 1] != S.val[k])) {
            heads |= 1u << j;
            const unsigned long long u = S.val[k];
            double s = 0.0;
            int m = k;
            bool more = true;
            while (more) {  // m + 4 <= cnt + 3 < kPpSlots and the slack of wgt
              double w[4];
              unsigned long long nv[4];
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                w[t] = S.wgt[m + t];
                nv[t] = S.val[m + t + 1];
              }
#pragma unroll
              for (int t = 0; t < 4; ++t)
                if (more) {
                  s += w[t];
                  more = m + t + 1 < cnt && nv[t] == u;
                }
              m += 4;
            }
            reg[j] = s;
          }
        }
        // 5. the walk over the distinct values in ascending order: entry k sits in lane k % 64, register k / 64
        double run = 0.0;
        int median = -1;
#pragma unroll
        for (int j = 0; j < kPpOwn; ++j) {
          if (median < 0 && kWave * j < cnt) {
            for (unsigned long long pending = __builtin_amdgcn_ballot_w64((heads >> j) & 1u); pending; pending &= pending - 1) {
              const int src = __builtin_ctzll(pending);
              run += lane_value(reg[j], src);
              if (run >= half_total) { median = kWave * j + src; break; }
            }
          }
        }
        if (lane == 0 && median >= 0) dmap[i] = __longlong_as_double((long long)S.val[median]);
      }
      wave_lds_fence();  // the next pixel's gather overwrites what this one still read
    }
  }
}

}  // namespace cspm
