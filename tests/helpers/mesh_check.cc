// mesh_check.cc -- CSPatchMatch::Mesh of the host layer against the C ABI on the same device context: after a PatchMatch run on a
// synthetic pair, every output of Mesh (RAW, PP with a median setting, RAW with a fit) equals what cspm_mesh returns for the same
// arguments, the vectors are as long as the counts, and a call before any run or with a bad parameter throws.
// usage: mesh_check        prints "mesh_check ok" and exits 0, or says what failed and exits 1
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cs_patchmatch.h"
#include "cc/grd_cc.h"
#include "plane_cost/pre_cs_pc.h"

static int g_bad = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_bad;                                              \
    }                                                       \
  } while (0)

template <class T>
static bool SameBytes(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main() {
  const int w = 77, h = 41, max_dis = 16;
  Mat l(h, w, CV_8UC3), r(h, w, CV_8UC3);
  unsigned s = 12345u;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int k = 0; k < 3; ++k) {
        s = s * 1664525u + 1013904223u;
        const unsigned char tex = (unsigned char)(((x * 7 + y * 13) & 63) * 3 + ((s >> 24) & 15));
        l.ptr<unsigned char>(y)[3 * x + k] = tex;
        r.ptr<unsigned char>(y)[3 * x + k] = tex;
      }
  for (int y = 0; y < h; ++y)  // the right image: the left one shifted by 5 (a fronto-parallel scene)
    for (int x = 0; x + 5 < w; ++x)
      for (int k = 0; k < 3; ++k) r.ptr<unsigned char>(y)[3 * x + k] = l.ptr<unsigned char>(y)[3 * (x + 5) + k];
  const cspm_calib calib = {300.0, 38.5, 20.25, 0.25, 3.5};
  cspm_geom_params g;
  cspm_geom_default_params(&g);
  g.min_cos = 0.5;
  g.left_frame = 1;
  cspm_mesh_params mp;
  EXPECT(cspm_mesh_default_params(&mp) == CSPM_OK && mp.max_diff == 1.0 && mp.all_vertices == 0);
  try {
    CSPatchMatch fresh(l, r, max_dis, 4);
    bool threw = false;
    try {
      fresh.Mesh(kLeft, calib, g, mp, CSPM_GEOM_RAW, NULL, NULL, NULL, NULL);
    } catch (const std::exception &) {
      threw = true;
    }
    EXPECT(threw);

    GrdCC cc;
    PreCSPC cost(l, r, max_dis, 9, 3, &cc, 0.3);
    CSPatchMatch pm(l, r, max_dis, 4);
    pm.set_seed(7);
    pm.SetMedianFilter(1);
    pm.PatchMatch(1, &cost, false);
    cspm_ctx *ctx = cost.device_ctx();
    cspm_fit_params fit;
    cspm_fit_default_params(&fit);
    fit.radius = 2;
    const size_t n = (size_t)w * h, max_faces = 2 * (size_t)(w - 1) * (h - 1);
    for (int view = 0; view < 2; ++view)
      for (int mode = 0; mode < 3; ++mode) {
        const int source = mode == 1 ? CSPM_GEOM_PP : CSPM_GEOM_RAW;
        const cspm_fit_params *f = mode == 2 ? &fit : NULL;
        mp.all_vertices = mode == 2 ? 1 : 0;
        std::vector<cspm_point> verts;
        std::vector<cspm_face> faces;
        std::vector<uint8_t> quad;
        const size_t nf = pm.Mesh(view == 0 ? kLeft : kRight, calib, g, mp, source, f, &verts, &faces, &quad);
        std::vector<cspm_point> verts2(n);
        std::vector<cspm_face> faces2(max_faces);
        std::vector<uint8_t> quad2(n);
        unsigned int nv2 = 0, nf2 = 0;
        EXPECT(cspm_set_pp_median(ctx, 1) == CSPM_OK);
        EXPECT(cspm_mesh(ctx, view, source, &calib, &g, f, &mp, verts2.data(), n, faces2.data(), max_faces, quad2.data(), &nv2, &nf2) == CSPM_OK);
        verts2.resize(nv2);
        faces2.resize(nf2);
        EXPECT(nf == nf2 && faces.size() == nf && verts.size() == nv2 && nv2 > 0 && nv2 <= n && nf > 0 && nf <= max_faces);
        EXPECT(SameBytes(verts, verts2) && SameBytes(faces, faces2) && SameBytes(quad, quad2));
        for (size_t k = 0; k < faces.size(); ++k) EXPECT(faces[k].v[0] < nv2 && faces[k].v[1] < nv2 && faces[k].v[2] < nv2);
        EXPECT(pm.Mesh(view == 0 ? kLeft : kRight, calib, g, mp, source, f, NULL, NULL, NULL) == nf);  // the counts alone
      }
    cspm_mesh_params bad = mp;
    bad.max_diff = -1.0;
    bool threw2 = false;
    try {
      pm.Mesh(kLeft, calib, g, bad, CSPM_GEOM_RAW, NULL, NULL, NULL, NULL);
    } catch (const std::exception &) {
      threw2 = true;
    }
    EXPECT(threw2);
  } catch (const std::exception &e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  if (g_bad) return 1;
  std::printf("mesh_check ok\n");
  return 0;
}
