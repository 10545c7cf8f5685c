// depth_fusion.h -- class DepthFusion: the views of several pairs collected on the host and fused into one cloud by
// cspm_fuse_depth_maps (include/cspm.h "depth-map fusion").  An addition; the reference has nothing like it.
// A view is what CSPatchMatch::Reproject returns for one view of a pair (depth, keep, normal) with the pair's calibration and the pose of
// its rectified left camera.  The slots are numbered by the caller, so workers may fill them in any order and the cloud does not depend
// on that order: SetPairView on different slots is safe from different threads.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cspm.h"
#include "pose_io.h"

class DepthFusion {
 public:
  explicit DepthFusion(size_t slots) : views_(slots) {}
  size_t size() const { return views_.size(); }

  // slot <- view `view` (0 left, 1 right) of a pair: depth and keep wid x hei, normal three planes of wid x hei (Reproject's outputs with
  // left_frame == 0), bgr a wid x hei 8UC3 image with rows of bgr_stride bytes or NULL, pose the camera -> world pose of the pair's
  // rectified LEFT camera.  The depth is kept where keep != 0 and NaN elsewhere; the right view gets cx + doffs and t + R (baseline, 0, 0).
  void SetPairView(size_t slot, int view, const cspm_calib &calib, const CameraPose &pose, int wid, int hei, const std::vector<double> &depth,
                   const std::vector<uint8_t> &keep, const std::vector<double> &normal, const uint8_t *bgr, size_t bgr_stride) {
    const size_t n = (size_t)wid * hei;
    if (slot >= views_.size() || depth.size() != n || keep.size() != n || normal.size() != 3 * n) throw std::runtime_error("DepthFusion::SetPairView: bad sizes");
    View &v = views_[slot];
    v.wid = wid; v.hei = hei;
    v.depth.resize(n);
    for (size_t i = 0; i < n; ++i) v.depth[i] = keep[i] ? depth[i] : std::numeric_limits<double>::quiet_NaN();
    v.normal = normal;
    v.bgr.clear();
    if (bgr) {
      v.bgr.resize(3 * n);
      for (int y = 0; y < hei; ++y) std::copy(bgr + (size_t)y * bgr_stride, bgr + (size_t)y * bgr_stride + 3 * (size_t)wid, v.bgr.begin() + 3 * (size_t)wid * y);
    }
    v.f = calib.f; v.cx = calib.cx + (double)view * calib.doffs; v.cy = calib.cy;
    v.view = view; v.baseline = calib.baseline;
    for (int i = 0; i < 9; ++i) v.R[i] = pose.R[i];
    for (int i = 0; i < 3; ++i) v.t[i] = view == 1 ? pose.t[i] + pose.R[3 * i] * calib.baseline : pose.t[i];
    v.set = true;
  }

  // The poses of the pairs refined in list order by cspm_register_depth_maps (include/cspm.h "depth-view registration", DESIGN.md section
  // 26); per_pair = 1 (left views only) or 2 (slot 2 i + 1 is pair i's right view).  Pair 0 keeps its pose.  Pair i's left view starts from
  // its own pose, or with `chain` from pair i - 1's refined pose, and is registered against the left views of the `window` pairs before
  // it, which go into the call in list order with the source behind them; its right view follows by the baseline.  records: per pair the
  // iterations of its registration (none for pair 0).  Throws like Fuse.
  void Register(int device, const cspm_reg_params &params, int window, int per_pair, bool chain, std::vector<std::vector<cspm_reg_iter> > *records) {
    const size_t pairs = views_.size() / (size_t)per_pair;
    for (size_t k = 0; k < views_.size(); ++k) {
      if (!views_[k].set) throw std::runtime_error("DepthFusion::Register: a view is missing");
      if (views_[k].wid != views_[0].wid || views_[k].hei != views_[0].hei) throw std::runtime_error("DepthFusion::Register: the views are not of one size");
    }
    if (records) records->assign(pairs, std::vector<cspm_reg_iter>());
    for (size_t i = 1; i < pairs; ++i) {
      View &src = views_[i * per_pair];
      if (chain) SetLeftPose(i, per_pair, views_[(i - 1) * per_pair].R, views_[(i - 1) * per_pair].t);
      const size_t first = i > (size_t)window ? i - (size_t)window : 0;
      std::vector<cspm_fuse_view> arr;
      for (size_t j = first; j <= i; ++j) arr.push_back(AbiView(views_[j * per_pair]));
      const int s = (int)arr.size() - 1;
      double R[9], t[3];
      std::vector<cspm_reg_iter> it((size_t)params.iters);
      if (cspm_register_depth_maps(device, &params, arr.data(), (int)arr.size(), src.wid, src.hei, s, (1ull << s) - 1ull, R, t, it.data()) != CSPM_OK)
        throw std::runtime_error(std::string("cspm_register_depth_maps: ") + cspm_last_error(NULL));
      SetLeftPose(i, per_pair, R, t);
      if (records) (*records)[i] = it;
    }
  }
  // the camera -> world pose of pair i's left view
  CameraPose LeftPose(size_t i, int per_pair) const {
    const View &v = views_[i * per_pair];
    CameraPose p;
    for (int k = 0; k < 9; ++k) p.R[k] = v.R[k];
    for (int k = 0; k < 3; ++k) p.t[k] = v.t[k];
    return p;
  }

  // the slots as the C ABI takes them (pointers into this object: valid until a view is set again), and their common size.  Throws for an
  // unset slot and for views of different sizes.
  std::vector<cspm_fuse_view> Views(int *w, int *h) const {
    if (views_.empty()) throw std::runtime_error("DepthFusion::Views: no views");
    std::vector<cspm_fuse_view> arr(views_.size());
    for (size_t k = 0; k < views_.size(); ++k) {
      const View &v = views_[k];
      if (!v.set) throw std::runtime_error("DepthFusion::Views: a view is missing");
      if (v.wid != views_[0].wid || v.hei != views_[0].hei) throw std::runtime_error("DepthFusion::Views: the views are not of one size");
      arr[k] = AbiView(v);
    }
    *w = views_[0].wid;
    *h = views_[0].hei;
    return arr;
  }
  // pair i's left view takes (R, t) and its right view follows by the baseline (what Register does with a refined pose)
  void SetPose(size_t i, int per_pair, const double *R, const double *t) { SetLeftPose(i, per_pair, R, t); }

  // F over the slots in their order.  Returns the number of kept pixels; cloud: the records in (slot, raster) order; view_counts: the
  // kept pixels per slot.  Throws for an unset slot, views of different sizes and for what the C ABI refuses.
  size_t Fuse(int device, const cspm_fuse_params &params, std::vector<cspm_point> *cloud, std::vector<unsigned int> *view_counts) const {
    if (views_.empty()) throw std::runtime_error("DepthFusion::Fuse: no views");
    std::vector<cspm_fuse_view> arr(views_.size());
    for (size_t k = 0; k < views_.size(); ++k) {
      const View &v = views_[k];
      if (!v.set) throw std::runtime_error("DepthFusion::Fuse: a view is missing");
      if (v.wid != views_[0].wid || v.hei != views_[0].hei) throw std::runtime_error("DepthFusion::Fuse: the views are not of one size");
      arr[k] = AbiView(v);
    }
    const int w = views_[0].wid, h = views_[0].hei;
    unsigned int count = 0;
    std::vector<unsigned int> counts(views_.size());
    // the count first, then a buffer of exactly that size
    int rc = cspm_fuse_depth_maps(device, &params, arr.data(), (int)arr.size(), w, h, NULL, 0, &count, counts.data(), NULL);
    if (rc == CSPM_OK && cloud) {
      cloud->resize(count);
      rc = cspm_fuse_depth_maps(device, &params, arr.data(), (int)arr.size(), w, h, cloud->data(), cloud->size(), &count, counts.data(), NULL);
    }
    if (rc != CSPM_OK) throw std::runtime_error(std::string("cspm_fuse_depth_maps: ") + cspm_last_error(NULL));
    if (view_counts) *view_counts = counts;
    return count;
  }

 private:
  struct View;
  static cspm_fuse_view AbiView(const View &v) {
    cspm_fuse_view a;
    a.depth = v.depth.data();
    a.normal = v.normal.data();
    a.bgr = v.bgr.empty() ? NULL : v.bgr.data();
    a.bgr_stride = 3 * (size_t)v.wid;
    a.f = v.f; a.cx = v.cx; a.cy = v.cy;
    for (int i = 0; i < 9; ++i) a.R[i] = v.R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = v.t[i];
    return a;
  }
  // pair i's left view takes (R, t); its right view, if there is one, R and t + R (baseline, 0, 0) as in SetPairView
  void SetLeftPose(size_t i, int per_pair, const double *R, const double *t) {
    for (int v = 0; v < per_pair; ++v) {
      View &d = views_[i * per_pair + v];
      double Rn[9], tn[3];
      for (int k = 0; k < 9; ++k) Rn[k] = R[k];
      for (int k = 0; k < 3; ++k) tn[k] = d.view == 1 ? t[k] + R[3 * k] * d.baseline : t[k];
      for (int k = 0; k < 9; ++k) d.R[k] = Rn[k];
      for (int k = 0; k < 3; ++k) d.t[k] = tn[k];
    }
  }
  struct View {
    bool set = false;
    int wid = 0, hei = 0, view = 0;
    double baseline = 0;
    std::vector<double> depth, normal;
    std::vector<uint8_t> bgr;
    double f = 0, cx = 0, cy = 0, R[9] = {0}, t[3] = {0};
  };
  std::vector<View> views_;
};
