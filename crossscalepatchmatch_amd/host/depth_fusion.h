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
    for (int i = 0; i < 9; ++i) v.R[i] = pose.R[i];
    for (int i = 0; i < 3; ++i) v.t[i] = view == 1 ? pose.t[i] + pose.R[3 * i] * calib.baseline : pose.t[i];
    v.set = true;
  }

  // F over the slots in their order.  Returns the number of kept pixels; cloud: the records in (slot, raster) order; view_counts: the
  // kept pixels per slot.  Throws for an unset slot, views of different sizes and for what the C ABI refuses.
  size_t Fuse(int device, const cspm_fuse_params &params, std::vector<cspm_point> *cloud, std::vector<unsigned int> *view_counts) const {
    if (views_.empty()) throw std::runtime_error("DepthFusion::Fuse: no views");
    std::vector<cspm_fuse_view> arr(views_.size());
    for (size_t k = 0; k < views_.size(); ++k) {
      const View &v = views_[k];
      if (!v.set) throw std::runtime_error("DepthFusion::Fuse: a view is missing");
      if (v.wid != views_[0].wid || v.hei != views_[0].hei) throw std::runtime_error("DepthFusion::Fuse: the views are not of one size");
      cspm_fuse_view &a = arr[k];
      a.depth = v.depth.data();
      a.normal = v.normal.data();
      a.bgr = v.bgr.empty() ? NULL : v.bgr.data();
      a.bgr_stride = 3 * (size_t)v.wid;
      a.f = v.f; a.cx = v.cx; a.cy = v.cy;
      for (int i = 0; i < 9; ++i) a.R[i] = v.R[i];
      for (int i = 0; i < 3; ++i) a.t[i] = v.t[i];
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
  struct View {
    bool set = false;
    int wid = 0, hei = 0;
    std::vector<double> depth, normal;
    std::vector<uint8_t> bgr;
    double f = 0, cx = 0, cy = 0, R[9] = {0}, t[3] = {0};
  };
  std::vector<View> views_;
};
