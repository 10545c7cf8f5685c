// commfunc.h -- shared constants and scalar helpers of the host layer; same names and meaning as the
// reference's CSPM/commfunc.h:24-29,117-145 so plugin code written against it compiles unchanged.
#pragma once
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>

#include "cv_compat.h"
#include "gflags_compat.h"

using namespace std;
using namespace cv;

const int kViewNum = 2;                                   // commfunc.h:24
const double kDoubleEps = 0.00000001;                     // commfunc.h:26
const double kDoubleMax = numeric_limits<double>::max();  // commfunc.h:27
enum RefView { kLeft = 0, kRight = 1 };                   // commfunc.h:29

// commfunc.h:117-121: round-half-to-even through the 2^52+2^51 magic constant
inline int Round2Int(double d) {
  d += 6755399441055744.0;
  int32_t lo;
  std::memcpy(&lo, &d, sizeof lo);
  return lo;
}
// commfunc.cc:11-25, `MedianFilter(in, out, r)` on a Mat of depth 8U with 1 .. 4 channels, in place or not: the median of the
// (2r+1) x (2r+1) window with the border replicated (include/cspm.h M8), computed on the calling thread's device; r in 1 .. 7.
// Throws std::runtime_error for another depth, an empty image or a radius outside the range.  Defined in host_impl.cc.
void MedianFilter(const Mat &src, Mat &dst, int r);
// an addition (include/cspm.h "smoothing", cspm_smooth_disparity_host): the edge-aware global smoother on a CV_64FC1 disparity map,
// computed on the calling thread's device.  conf: a CV_64FC1 map of confidences in [0, 1] or NULL (all 1); guide: a CV_8UC3 image or
// NULL (every weight 1); params NULL = the defaults (fill_conf is not used); max_dis > 0 clamps the smoothed values.  dst may be src.
// Throws std::runtime_error for another type, differing sizes and for what the C ABI refuses.  Defined in host_impl.cc.
struct cspm_smooth_params;
void SmoothDisparity(const Mat &src, const Mat *conf, const Mat *guide, const cspm_smooth_params *params, int max_dis, Mat &dst);
// additions (include/cspm.h "segment planes", cspm_segment_host / cspm_segment_planes_host), computed on the calling thread's device;
// params NULL = the defaults.  SegmentImage: the superpixel labels (CV_32SC1) of a CV_8UC3 image.  SegmentPlanes: one robustly fitted
// plane per segment of a CV_64FC1 disparity map under a CV_32SC1 label map of the same size for the grid of params->step; valid: a
// CV_8UC1 mask or NULL (every pixel).  planes: rows x cols Planes, row-major, those of unfitted segments with NaN entries; fitted:
// CV_8UC1 or NULL; seg_abc: three doubles (a, b, c) per segment or NULL.  Both throw std::runtime_error for another type, differing
// sizes and for what the C ABI refuses (labels outside the 3 x 3 cells of their pixel among it).  Defined in host_impl.cc.
// an addition (include/cspm.h "rectification", cspm_rectify_host): two RAW CV_8UC3 photographs of the rig's size undistorted and
// row-aligned on the calling thread's device; rect comes from cspm_rectify_compute.  l_out / r_out: CV_8UC3 of rect.w x rect.h, pixels
// without a source black; l_valid / r_valid: CV_8UC1 masks of the pixels that have one, or NULL.  Throws std::runtime_error for another
// type or size and for what the C ABI refuses.  Defined in host_impl.cc.
struct cspm_rig;
struct cspm_rectification;
void RectifyPair(const cspm_rig &rig, const cspm_rectification &rect, const Mat &l_raw, const Mat &r_raw, Mat &l_out, Mat &r_out, Mat *l_valid,
                 Mat *r_valid);
struct cspm_seg_params;
class Plane;
void SegmentImage(const Mat &img, Mat &labels, const cspm_seg_params *params);
void SegmentPlanes(const Mat &disp, const Mat *valid, const Mat &labels, const cspm_seg_params *params, int max_dis, std::vector<Plane> *planes, Mat *fitted,
                   std::vector<double> *seg_abc);

// commfunc.h:129-145: a single wrap-around
inline int HandleBorder(const int &loc, const int &size) { return loc < 0 ? loc + size : (loc >= size ? loc - size : loc); }
