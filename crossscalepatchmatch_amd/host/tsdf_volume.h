// tsdf_volume.h -- class TsdfVolume: the views a DepthFusion collected, integrated in list order into one TSDF volume whose surface
// points come back as a cloud (include/cspm.h "TSDF fusion") or as the vertices of a triangle mesh ("TSDF meshes",
// section 29), and the frame-to-model registration of those views against raycasts of the growing volume.  An addition; the reference has nothing like it.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cspm.h"
#include "depth_fusion.h"

// "a,b,c" -> three doubles: exactly three numbers separated by commas, blanks allowed around them, nothing else
inline bool ParseTsdfTriple(const char *s, double out[3]) {
  if (!s) return false;
  for (int i = 0; i < 3; ++i) {
    char *end = NULL;
    const double v = std::strtod(s, &end);
    if (end == s) return false;
    out[i] = v;
    s = end;
    while (*s == ' ' || *s == '\t') ++s;
    if (i < 2) {
      if (*s != ',') return false;
      ++s;
    }
  }
  return *s == '\0';
}
// the same for three ints that fit: "nx,ny,nz"
inline bool ParseTsdfDims(const char *s, int out[3]) {
  double v[3];
  if (!ParseTsdfTriple(s, v)) return false;
  for (int i = 0; i < 3; ++i) {
    if (!(v[i] >= -2147483648.0 && v[i] <= 2147483647.0) || v[i] != (double)(int)v[i]) return false;
    out[i] = (int)v[i];
  }
  return true;
}

class TsdfVolume {
 public:
  explicit TsdfVolume(const cspm_tsdf_params &params) : p_(params) {}
  const cspm_tsdf_params &params() const { return p_; }

  // T over the fusion's views in slot order.  Returns the number of surface points; cloud: the records in (voxel, axis) order.  Throws for
  // what DepthFusion::Views and the C ABI refuse.
  size_t Fuse(int device, const DepthFusion &fusion, std::vector<cspm_point> *cloud) const {
    int w = 0, h = 0;
    const std::vector<cspm_fuse_view> arr = fusion.Views(&w, &h);
    unsigned int count = 0;
    // the count first, then a buffer of exactly that size
    int rc = cspm_tsdf_depth_maps(device, &p_, arr.data(), (int)arr.size(), w, h, NULL, 0, &count, NULL, NULL, NULL);
    if (rc == CSPM_OK && cloud) {
      cloud->resize(count);
      rc = cspm_tsdf_depth_maps(device, &p_, arr.data(), (int)arr.size(), w, h, cloud->data(), cloud->size(), &count, NULL, NULL, NULL);
    }
    if (rc != CSPM_OK) throw std::runtime_error(std::string("cspm_tsdf_depth_maps: ") + cspm_last_error(NULL));
    return count;
  }

  // MC over the same views: the surface points as vertices and the faces over them.  Returns the number of faces.  Throws like Fuse.
  size_t Mesh(int device, const DepthFusion &fusion, std::vector<cspm_point> *vertices, std::vector<cspm_face> *faces) const {
    int w = 0, h = 0;
    const std::vector<cspm_fuse_view> arr = fusion.Views(&w, &h);
    unsigned int nv = 0, nf = 0;
    // the counts first, then buffers of exactly those sizes
    int rc = cspm_tsdf_mesh_depth_maps(device, &p_, arr.data(), (int)arr.size(), w, h, NULL, 0, NULL, 0, &nv, &nf);
    if (rc == CSPM_OK && (vertices || faces)) {
      if (vertices) vertices->resize(nv);
      if (faces) faces->resize(nf);
      rc = cspm_tsdf_mesh_depth_maps(device, &p_, arr.data(), (int)arr.size(), w, h, vertices ? vertices->data() : NULL, vertices ? vertices->size() : 0,
                                     faces ? faces->data() : NULL, faces ? faces->size() : 0, &nv, &nf);
    }
    if (rc != CSPM_OK) throw std::runtime_error(std::string("cspm_tsdf_mesh_depth_maps: ") + cspm_last_error(NULL));
    return nf;
  }

  // The poses of the pairs refined in list order FRAME TO MODEL: pair 0 keeps its pose and is integrated; pair i's left view starts from
  // its own pose, or with `chain` from pair i - 1's refined pose, and is registered (cspm_fuse_register) against a raycast of the
  // volume built from pairs 0 .. i - 1 at pair i - 1's left camera (cspm_tsdf_raycast_push); then its views are integrated with the
  // refined pose.  per_pair and records as in DepthFusion::Register.  The volume lives in a context of its own for the call.
  void Register(int device, DepthFusion *fusion, const cspm_reg_params &params, int per_pair, bool chain,
                std::vector<std::vector<cspm_reg_iter> > *records) const {
    int w = 0, h = 0;
    std::vector<cspm_fuse_view> arr = fusion->Views(&w, &h);
    const size_t pairs = arr.size() / (size_t)per_pair;
    if (records) records->assign(pairs, std::vector<cspm_reg_iter>());
    Ctx c(device);
    c.check(cspm_tsdf_begin(c.ctx, &p_), "cspm_tsdf_begin");
    for (size_t i = 0; i < pairs; ++i) {
      if (i > 0) {
        if (chain) {
          fusion->SetPose(i, per_pair, arr[(i - 1) * per_pair].R, arr[(i - 1) * per_pair].t);
          arr = fusion->Views(&w, &h);
        }
        const cspm_fuse_view &src = arr[i * per_pair], &prev = arr[(i - 1) * per_pair];
        cspm_tsdf_camera cam;
        cam.f = prev.f; cam.cx = prev.cx; cam.cy = prev.cy;
        for (int k = 0; k < 9; ++k) cam.R[k] = prev.R[k];
        for (int k = 0; k < 3; ++k) cam.t[k] = prev.t[k];
        double R[9], t[3];
        std::vector<cspm_reg_iter> it((size_t)params.iters);
        c.check(cspm_fuse_begin(c.ctx, w, h, 2), "cspm_fuse_begin");
        c.check(cspm_fuse_push_maps(c.ctx, src.depth, src.normal, NULL, 0, src.f, src.cx, src.cy, src.R, src.t), "cspm_fuse_push_maps");
        c.check(cspm_tsdf_raycast_push(c.ctx, &cam, 0.0), "cspm_tsdf_raycast_push");
        c.check(cspm_fuse_register(c.ctx, 0, 2ull, &params, NULL, NULL, 0, R, t, it.data()), "cspm_fuse_register");
        c.check(cspm_fuse_end(c.ctx), "cspm_fuse_end");
        fusion->SetPose(i, per_pair, R, t);
        arr = fusion->Views(&w, &h);
        if (records) (*records)[i] = it;
      }
      c.check(cspm_fuse_begin(c.ctx, w, h, per_pair), "cspm_fuse_begin");
      for (int v = 0; v < per_pair; ++v) {
        const cspm_fuse_view &a = arr[i * per_pair + v];
        c.check(cspm_fuse_push_maps(c.ctx, a.depth, a.normal, a.bgr, a.bgr_stride, a.f, a.cx, a.cy, a.R, a.t), "cspm_fuse_push_maps");
        c.check(cspm_tsdf_integrate(c.ctx, v), "cspm_tsdf_integrate");
      }
      c.check(cspm_fuse_end(c.ctx), "cspm_fuse_end");
    }
  }

 private:
  struct Ctx {
    cspm_ctx *ctx = NULL;
    explicit Ctx(int device) {
      if (cspm_create(&ctx, device) != CSPM_OK) throw std::runtime_error(std::string("cspm_create: ") + cspm_last_error(NULL));
    }
    ~Ctx() { cspm_destroy(ctx); }
    void check(int rc, const char *what) const {
      if (rc != CSPM_OK) throw std::runtime_error(std::string(what) + ": " + cspm_last_error(ctx));
    }
  };
  cspm_tsdf_params p_;
};
