// cspm_fit.h -- slanted planes fitted to a disparity map (include/cspm.h "plane fitting"): a local weighted
// least-squares plane per pixel, F(D, V, I, radius, max_diff, min_support, use_guide, max_dis) -> (planes, fitted).
//
// k_fit_planes: one LANE per pixel, a workgroup per tile of kFitTileW x kFitTileH pixels, lanes along x.  The workgroup stages its tile
// plus a halo of `radius` pixels once into LDS -- D with every non-node (V = 0, D not finite, outside the image) folded to NaN, the
// packed BGR guide, and the 766-entry exp(-k/10) table -- and the (2r+1)^2 taps of a lane then read LDS only.  A wave's 64 lanes read 64
// consecutive doubles (ds_read_b64: each 32-lane half covers the 64 banks once) and 64 consecutive colours: conflict-free whatever the
// row stride; only the table lookup is a data-dependent gather.  Nine f64 running sums per lane, serial in the window's raster order,
// every product and sum rounded on its own (-ffp-contract=off, and the pragma below), then the 3x3 solve by cofactors with three true
// divisions.  No cross-lane reduction, no atomics, nothing waits for another workgroup.
//
// LDS: (64 + 2r) * (4 + 2r) * 12 bytes + 6128 for the table: 18.6 KB at the default radius 5 (eight workgroups fit a CU's 160 KB; the
// wave limit, 8 workgroups of 4 waves, binds first), 50.8 KB at the largest radius 17 (three).
#pragma once
#include "cspm_device.h"

#pragma clang fp contract(off)

namespace cspm {

constexpr int kFitTileW = 64, kFitTileH = 4, kFitBlock = kFitTileW * kFitTileH;
constexpr int kFitMaxRadius = 17;
constexpr int kFitLut = 766;  // |dB| + |dG| + |dR| = 0 .. 765

struct FitIn {
  const double *disp;    // W*H
  const uint8_t *valid;  // W*H bytes, or null: every pixel
  const uint32_t *pix;   // W*H packed B | G<<8 | R<<16 (k_pack_bgr); not read without a guide
  const double *lut;     // kFitLut entries exp(-k/10), host-computed; not read without a guide
};
struct FitOut {
  double *nx, *ny, *nz, *a, *b, *c;  // W*H each
  uint8_t *fitted;                   // W*H bytes or null
  int keep_unfitted;                 // 1: a non-node's six values are left as they are (a stored field); 0: they become NaN (a candidate field)
};

inline size_t fit_lds_bytes(int r) {
  return (size_t)(kFitTileW + 2 * r) * (kFitTileH + 2 * r) * (sizeof(double) + sizeof(uint32_t)) + kFitLut * sizeof(double);
}

template <bool GUIDE>
__global__ __launch_bounds__(kFitBlock) void k_fit_planes(FitIn in, FitOut out, int W, int H, int r, double tau, int min_support, double max_dis) {
  extern __shared__ double fit_lds[];
  const int TW = kFitTileW + 2 * r, TH = kFitTileH + 2 * r, cells = TW * TH;
  double *sD = fit_lds;
  double *sLut = sD + cells;
  uint32_t *sPix = reinterpret_cast<uint32_t *>(sLut + kFitLut);
  const int tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kFitTileW, y0 = (int)blockIdx.y * kFitTileH;
  const double kNaN = __longlong_as_double(0x7FF8000000000000LL);

  for (int t = tid; t < cells; t += kFitBlock) {
    const int ly = t / TW, lx = t - ly * TW;
    const int gx = x0 - r + lx, gy = y0 - r + ly;
    double d = kNaN;
    uint32_t px = 0u;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const long long g = (long long)gy * W + gx;
      const double dv = in.disp[g];
      const bool node = (in.valid == nullptr || in.valid[g] != 0) && fabs(dv) <= kDoubleMax;  // finite: false for NaN and for +-inf
      if (node) d = dv;
      if (GUIDE) px = in.pix[g];
    }
    sD[t] = d;
    if (GUIDE) sPix[t] = px;
  }
  if (GUIDE)
    for (int t = tid; t < kFitLut; t += kFitBlock) sLut[t] = in.lut[t];
  __syncthreads();

  const int tx = tid % kFitTileW, ty = tid / kFitTileW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const long long g = (long long)y * W + x;
  const int centre = (ty + r) * TW + tx + r;
  const double Dp = sD[centre];
  if (!(Dp == Dp)) {  // not a node: no candidate
    if (!out.keep_unfitted) {
      out.nx[g] = kNaN; out.ny[g] = kNaN; out.nz[g] = kNaN;
      out.a[g] = kNaN; out.b[g] = kNaN; out.c[g] = kNaN;
    }
    if (out.fitted) out.fitted[g] = 0;
    return;
  }
  const uint32_t pp = GUIDE ? sPix[centre] : 0u;
  const int pb = (int)(pp & 0xFFu), pg = (int)((pp >> 8) & 0xFFu), pr = (int)((pp >> 16) & 0xFFu);

  double Sw = 0.0, Su = 0.0, Sv = 0.0, Suu = 0.0, Suv = 0.0, Svv = 0.0, Se = 0.0, Sue = 0.0, Sve = 0.0;
  int n = 0;
  for (int j = -r; j <= r; ++j) {
    const double v = (double)j;
    const int row = (ty + r + j) * TW + tx + r;
    for (int i = -r; i <= r; ++i) {
      const double e = sD[row + i] - Dp;
      if (fabs(e) <= tau) {  // false for a NaN: a tap outside the image or on a non-node
        double wq = 1.0;
        if (GUIDE) {
          const uint32_t q = sPix[row + i];
          const int k = abs((int)(q & 0xFFu) - pb) + abs((int)((q >> 8) & 0xFFu) - pg) + abs((int)((q >> 16) & 0xFFu) - pr);
          wq = sLut[k];
        }
        const double u = (double)i;
        Sw = Sw + wq * 1.0;
        Su = Su + wq * u;
        Sv = Sv + wq * v;
        Suu = Suu + wq * (u * u);
        Suv = Suv + wq * (u * v);
        Svv = Svv + wq * (v * v);
        Se = Se + wq * e;
        Sue = Sue + wq * (u * e);
        Sve = Sve + wq * (v * e);
        ++n;
      }
    }
  }

  const double C00 = Svv * Sw - Sv * Sv;
  const double C01 = Suv * Sw - Sv * Su;
  const double C02 = Suv * Sv - Svv * Su;
  const double C11 = Suu * Sw - Su * Su;
  const double C12 = Suu * Sv - Suv * Su;
  const double C22 = Suu * Svv - Suv * Suv;
  const double det = (Suu * C00 - Suv * C01) + Su * C02;
  double a = 0.0, b = 0.0, c0 = 0.0;
  if (n >= min_support && det > 1e-6 * ((Suu * Svv) * Sw)) {
    a = ((C00 * Sue - C01 * Sve) + C02 * Se) / det;
    b = ((C11 * Sve - C01 * Sue) - C12 * Se) / det;
    c0 = ((C02 * Sue - C12 * Sve) + C22 * Se) / det;
  }
  double z = Dp + c0;
  z = z > 0.0 ? z : 0.0;
  z = z < max_dis ? z : max_dis;
  const double m0 = -a, m1 = -b, m2 = 1.0;
  double s = m0 * m0;  // the norm as InitRandomPlane takes it (init_plane, cspm_rows.h)
  s += m1 * m1;
  s += m2 * m2;
  const double inv = 1. / fmax(__dsqrt_rn(s), kDoubleEps);
  const double nx = m0 * inv, ny = m1 * inv, nz = m2 * inv;
  double pa, pb_, pc;
  plane_param(nx, ny, nz, (double)x, (double)y, z, pa, pb_, pc);
  out.nx[g] = nx; out.ny[g] = ny; out.nz[g] = nz;
  out.a[g] = pa; out.b[g] = pb_; out.c[g] = pc;
  if (out.fitted) out.fitted[g] = 1;
}

}  // namespace cspm
