// host_impl.cc -- GrdCC, DevicePlaneCost (PreSSPC / PreCSPC) and CSPatchMatch above the C ABI of
// libcspm_hip.so.  No arithmetic of the hot path happens here.
#include <mutex>
#include <vector>

#include "../../include/cspm.h"
#include "ca_filter/device_ca.h"
#include "cc/cen_cc.h"
#include "cc/cengrd_cc.h"
#include "cc/grd_cc.h"
#include "cs_patchmatch.h"
#include "plane_cost/device_plane_cost.h"

namespace {
void check(int rc, cspm_ctx *ctx, const char *what) {
  if (rc != CSPM_OK) throw std::runtime_error(std::string(what) + ": " + cspm_last_error(ctx));
}
// CV_64F copy of a Mat with packed rows
std::vector<double> packed64(const Mat &m) {
  CV_Assert(m.depth() == CV_64F);
  const size_t row = (size_t)m.cols * m.channels();
  std::vector<double> v(row * m.rows);
  for (int y = 0; y < m.rows; ++y) std::memcpy(&v[y * row], m.ptr<double>(y), row * sizeof(double));
  return v;
}
}  // namespace

// ---------------------------------------------------------------- GrdCC (cc/grd_cc.cpp:60-154)
void GrdCC::build(const Mat &lImg, const Mat &rImg, int maxDis, Mat *vol, int right) {
  CV_Assert(lImg.type() == CV_64FC3 && rImg.type() == CV_64FC3);  // grd_cc.cpp:63
  CV_Assert(lImg.rows == rImg.rows && lImg.cols == rImg.cols && maxDis >= 1 && vol);
  const int h = lImg.rows, w = lImg.cols;
  std::vector<double> l = packed64(lImg), r = packed64(rImg), out((size_t)maxDis * h * w);
  check(cspm_grd_build_cv_host(device_ >= 0 ? device_ : DeviceSlot::current().device(), l.data(), r.data(), w, h, maxDis, right, out.data()), NULL, "GrdCC");
  for (int d = 0; d < maxDis; ++d) {
    if (vol[d].rows != h || vol[d].cols != w || vol[d].type() != CV_64FC1) vol[d].create(h, w, CV_64FC1);
    for (int y = 0; y < h; ++y) std::memcpy(vol[d].ptr<double>(y), &out[((size_t)d * h + y) * w], sizeof(double) * w);
  }
}
void GrdCC::buildCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol) { build(lImg, rImg, maxDis, costVol, 0); }
void GrdCC::buildRightCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *rCostVol) { build(lImg, rImg, maxDis, rCostVol, 1); }

// ---------------------------------------------------------------- CenCC (cc/cen_cc.cc:4-137)
void CenCC::build(const Mat &lImg, const Mat &rImg, int maxDis, Mat *vol, int right) {
  CV_Assert(lImg.type() == CV_64FC3 && rImg.type() == CV_64FC3);  // cen_cc.cc:7
  CV_Assert(lImg.rows == rImg.rows && lImg.cols == rImg.cols && maxDis >= 1 && vol);
  const int h = lImg.rows, w = lImg.cols;
  std::vector<double> l = packed64(lImg), r = packed64(rImg), out((size_t)maxDis * h * w);
  check(cspm_cen_build_cv_host(device_ >= 0 ? device_ : DeviceSlot::current().device(), l.data(), r.data(), w, h, maxDis, right, out.data()), NULL, "CenCC");
  for (int d = 0; d < maxDis; ++d) {
    if (vol[d].rows != h || vol[d].cols != w || vol[d].type() != CV_64FC1) vol[d].create(h, w, CV_64FC1);
    for (int y = 0; y < h; ++y) std::memcpy(vol[d].ptr<double>(y), &out[((size_t)d * h + y) * w], sizeof(double) * w);
  }
}
void CenCC::buildCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol) { build(lImg, rImg, maxDis, costVol, 0); }
void CenCC::buildRightCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *rCostVol) { build(lImg, rImg, maxDis, rCostVol, 1); }

// ---------------------------------------------------------------- CenGrdCC (CENGRD: include/cspm.h)
void CenGrdCC::build(const Mat &lImg, const Mat &rImg, int maxDis, Mat *vol, int right) {
  CV_Assert(lImg.type() == CV_64FC3 && rImg.type() == CV_64FC3);
  CV_Assert(lImg.rows == rImg.rows && lImg.cols == rImg.cols && maxDis >= 1 && vol);
  const int h = lImg.rows, w = lImg.cols;
  std::vector<double> l = packed64(lImg), r = packed64(rImg), out((size_t)maxDis * h * w);
  check(cspm_cengrd_build_cv_host(device_ >= 0 ? device_ : DeviceSlot::current().device(), l.data(), r.data(), w, h, maxDis, right, out.data()), NULL, "CenGrdCC");
  for (int d = 0; d < maxDis; ++d) {
    if (vol[d].rows != h || vol[d].cols != w || vol[d].type() != CV_64FC1) vol[d].create(h, w, CV_64FC1);
    for (int y = 0; y < h; ++y) std::memcpy(vol[d].ptr<double>(y), &out[((size_t)d * h + y) * w], sizeof(double) * w);
  }
}
void CenGrdCC::buildCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol) { build(lImg, rImg, maxDis, costVol, 0); }
void CenGrdCC::buildRightCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *rCostVol) { build(lImg, rImg, maxDis, rCostVol, 1); }

// ---------------------------------------------------------------- BoxCA / GFCA / BFCA (ca_filter/*.cpp)
void DeviceCA::aggreCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol) {
  (void)rImg;  // unused, as in the reference
  CV_Assert(lImg.type() == CV_64FC3);  // the colour branch (GuidedFilter.cpp:171, BilateralFilter.cpp:56)
  CV_Assert(maxDis >= 1 && costVol);
  const int h = lImg.rows, w = lImg.cols;
  for (int d = 0; d < maxDis; ++d) CV_Assert(costVol[d].type() == CV_64FC1 && costVol[d].rows == h && costVol[d].cols == w);
  std::vector<double> g = packed64(lImg), vol((size_t)maxDis * h * w);
  for (int d = 0; d < maxDis; ++d)
    for (int y = 0; y < h; ++y) std::memcpy(&vol[((size_t)d * h + y) * w], costVol[d].ptr<double>(y), sizeof(double) * w);
  check(cspm_aggregate_cv_host(DeviceSlot::current().device(), method_, g.data(), w, h, maxDis, vol.data()), NULL, "CAMethod::aggreCV");
  for (int d = 1; d < maxDis; ++d)
    for (int y = 0; y < h; ++y) std::memcpy(costVol[d].ptr<double>(y), &vol[((size_t)d * h + y) * w], sizeof(double) * w);
}

// ---------------------------------------------------------------- DeviceSlot, PreSSPC / PreCSPC / GrdPC / CSPC
int DevicePlaneCost::device = 0;
bool DevicePlaneCost::keep_context = false;

namespace {
// the only process-wide state of the host layer: the registry of live contexts and the default slot, both behind one mutex
std::mutex g_host_mutex;
std::vector<cspm_ctx *> g_live;
thread_local DeviceSlot *t_slot = NULL;
DeviceSlot &default_slot() {
  static DeviceSlot slot;
  return slot;
}
void forget(std::vector<cspm_ctx *> &v, const cspm_ctx *c) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == c) { v.erase(v.begin() + i); return; }
}
long long option(cspm_ctx *ctx, int key) {
  long long v = 0;
  return cspm_get_option(ctx, key, &v) == CSPM_OK ? v : 0;
}
}  // namespace

DeviceSlot::Use::Use(DeviceSlot &slot) : prev_(t_slot) { t_slot = &slot; }
DeviceSlot::Use::~Use() { t_slot = prev_; }

int DeviceSlot::device_count() { return cspm_device_count(); }

DeviceSlot &DeviceSlot::current() {
  if (t_slot) return *t_slot;
  DeviceSlot &d = default_slot();
  cspm_ctx *stale = NULL;
  {
    std::lock_guard<std::mutex> lock(g_host_mutex);  // the default slot follows the statics (the reference-shaped, single-threaded flow)
    if (d.device_ != DevicePlaneCost::device && d.parked_) { stale = d.parked_; d.parked_ = NULL; forget(g_live, stale); }
    d.device_ = DevicePlaneCost::device;
    d.keep_ = DevicePlaneCost::keep_context;
  }
  if (stale) cspm_destroy(stale);
  return d;
}

cspm_ctx *DeviceSlot::take() {
  std::lock_guard<std::mutex> lock(g_host_mutex);
  cspm_ctx *c = parked_;
  parked_ = NULL;
  return c;
}
bool DeviceSlot::park(cspm_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_host_mutex);
  if (!keep_ || parked_) return false;
  parked_ = ctx;
  return true;
}
void DeviceSlot::release() {
  cspm_ctx *c = take();
  if (!c) return;
  DevicePlaneCost::disown(c);
  cspm_destroy(c);
}

void DevicePlaneCost::adopt(cspm_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_host_mutex);
  g_live.push_back(ctx);
}
void DevicePlaneCost::disown(cspm_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_host_mutex);
  forget(g_live, ctx);
}
bool DevicePlaneCost::is_live(const cspm_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_host_mutex);
  for (size_t i = 0; i < g_live.size(); ++i)
    if (g_live[i] == ctx) return true;
  return false;
}
void DevicePlaneCost::release_kept_context() { default_slot().release(); }

void DevicePlaneCost::open_context(const Mat &l_img, const Mat &r_img) {
  CV_Assert(l_img.type() == CV_8UC3 && r_img.type() == CV_8UC3);  // pre_cs_pc.cc:25, pre_ss_pc.cc:24, grd_pc.cc:22, cspc.cc:24
  CV_Assert(l_img.rows == r_img.rows && l_img.cols == r_img.cols);
  if (!slot_) slot_ = &DeviceSlot::current();
  ctx_ = slot_->take();
  const bool parked = ctx_ != NULL;
  if (!ctx_) {
    check(cspm_create(&ctx_, slot_->device()), NULL, "cspm_create");
    adopt(ctx_);
    if (slot_->shared_gpu() && !std::getenv("CSPM_SWEEP_FOLD"))  // the environment variable, if set, has decided at cspm_create
      check(cspm_set_option(ctx_, CSPM_OPT_SWEEP_FOLD, 1), ctx_, "cspm_set_option");
  }
  base_sweep_fallbacks_ = option(ctx_, CSPM_OPT_SWEEP_FALLBACKS);
  base_volume_fallbacks_ = option(ctx_, CSPM_OPT_VOLUME_FALLBACKS);
  const Mat l = l_img.clone(), r = r_img.clone();  // packed rows
  if (slot_->rect_on_) {  // raw photographs: the maps are built by the context's first pair and kept, every pair is remapped on the device
    if (l.cols != slot_->rig_.raw_w || l.rows != slot_->rig_.raw_h) throw std::runtime_error("the raw images are not of the rig's size");
    check(cspm_set_rectification(ctx_, &slot_->rig_, &slot_->rect_), ctx_, "cspm_set_rectification");
    check(cspm_set_images_raw(ctx_, l.data, r.data, l.step), ctx_, "cspm_set_images_raw");
    return;
  }
  if (parked) check(cspm_set_rectification(ctx_, NULL, NULL), ctx_, "cspm_set_rectification");  // no launch, nothing to free unless the slot rectified before
  check(cspm_set_images(ctx_, l.data, r.data, l.cols, l.rows, l.step), ctx_, "cspm_set_images");
}

void DevicePlaneCost::LevelImages(Mat *l_img, Mat *r_img) const {
  int w = 0, h = 0, d = 0;
  check(cspm_get_level_dims(ctx_, 0, &w, &h, &d), ctx_, "cspm_get_level_dims");
  Mat *out[kViewNum] = {l_img, r_img};
  for (int v = 0; v < kViewNum; ++v) {
    if (!out[v]) continue;
    Mat m(h, w, CV_8UC3);  // packed rows
    check(cspm_get_level_image(ctx_, v, 0, m.data), ctx_, "cspm_get_level_image");
    *out[v] = m;
  }
}

// include/cspm.h R on two raw Mats (cspm_rectify_host per view on the calling thread's device)
void RectifyPair(const cspm_rig &rig, const cspm_rectification &rect, const Mat &l_raw, const Mat &r_raw, Mat &l_out, Mat &r_out, Mat *l_valid,
                 Mat *r_valid) {
  const Mat *raw[kViewNum] = {&l_raw, &r_raw};
  Mat *valid[kViewNum] = {l_valid, r_valid};
  Mat res[kViewNum];
  for (int v = 0; v < kViewNum; ++v) {
    if (raw[v]->empty() || raw[v]->type() != CV_8UC3 || raw[v]->cols != rig.raw_w || raw[v]->rows != rig.raw_h)
      throw std::runtime_error("RectifyPair: two CV_8UC3 images of the rig's size expected");
    if (rect.w < 1 || rect.h < 1) throw std::runtime_error("RectifyPair: an empty rectification");
    res[v].create(rect.h, rect.w, CV_8UC3);
    Mat m;
    if (valid[v]) m.create(rect.h, rect.w, CV_8UC1);
    check(cspm_rectify_host(DeviceSlot::current().device(), &rig, &rect, v, raw[v]->data, raw[v]->step, res[v].data, res[v].step, NULL,
                            valid[v] ? m.data : NULL),
          NULL, "RectifyPair");
    if (valid[v]) *valid[v] = m;
  }
  l_out = res[kLeft];
  r_out = res[kRight];
}

// a constructor that throws never runs the destructor: hand the context back (or destroy it) before the exception leaves
#define CSPM_CTOR_GUARD(body)        \
  try {                              \
    body                             \
  } catch (...) {                    \
    close_context();                 \
    throw;                           \
  }

void DevicePlaneCost::close_context() {
  if (!ctx_) return;
  if (slot_) {
    const long long ds = option(ctx_, CSPM_OPT_SWEEP_FALLBACKS) - base_sweep_fallbacks_, dv = option(ctx_, CSPM_OPT_VOLUME_FALLBACKS) - base_volume_fallbacks_;
    std::lock_guard<std::mutex> lock(g_host_mutex);  // the default slot is shared by every thread that names none
    slot_->sweep_fallbacks_ += ds;
    slot_->volume_fallbacks_ += dv;
  }
  if (!(slot_ && slot_->park(ctx_))) {
    disown(ctx_);
    cspm_destroy(ctx_);
  }
  ctx_ = NULL;
}

// GrdPC / CSPC
DevicePlaneCost::DevicePlaneCost(const Mat &l_img, const Mat &r_img, int max_disp, int wnd_size, int scale_num, double reg_lambda, DeviceSlot *slot)
    : ctx_(NULL), slot_(slot), base_sweep_fallbacks_(0), base_volume_fallbacks_(0) {
  CSPM_CTOR_GUARD(
    open_context(l_img, r_img);
    check(cspm_build_cost_img(ctx_, max_disp, wnd_size, scale_num, reg_lambda), ctx_, "cspm_build_cost_img");
  )
}

DevicePlaneCost::DevicePlaneCost(const Mat &l_img, const Mat &r_img, int max_disp, int wnd_size, int scale_num,
                                 CCMethod *cc_method, double reg_lambda, DeviceSlot *slot)
    : ctx_(NULL), slot_(slot), base_sweep_fallbacks_(0), base_volume_fallbacks_(0) {
  if (!cc_method) throw std::runtime_error("PreSSPC/PreCSPC: NULL CCMethod (unknown --cc_name)");  // the reference dereferences it
  CSPM_CTOR_GUARD(
    open_context(l_img, r_img);
    if (dynamic_cast<GrdCC *>(cc_method)) {
      // the known cost function: pyramid, gradients, max_cost, scale weights all on the device
      check(cspm_build_cost_grd(ctx_, max_disp, wnd_size, scale_num, reg_lambda), ctx_, "cspm_build_cost_grd");
    } else if (dynamic_cast<CenCC *>(cc_method)) {
      check(cspm_build_cost_cen(ctx_, max_disp, wnd_size, scale_num, reg_lambda), ctx_, "cspm_build_cost_cen");
    } else if (const CenGrdCC *cg = dynamic_cast<CenGrdCC *>(cc_method)) {
      // set either way: a parked context keeps the option of the cost object before this one
      check(cspm_set_option(ctx_, CSPM_OPT_CENGRD_FUSED, cg->fused() ? 1 : 0), ctx_, "cspm_set_option");
      check(cspm_build_cost_cengrd(ctx_, max_disp, wnd_size, scale_num, reg_lambda), ctx_, "cspm_build_cost_cengrd");
    } else {
      // a foreign CCMethod: let it fill host volumes level by level exactly as pre_cs_pc.cc:57-74 does
      check(cspm_begin_cost(ctx_, max_disp, wnd_size, scale_num, reg_lambda), ctx_, "cspm_begin_cost");
      const int levels = cspm_get_levels(ctx_);
      for (int s = 0; s < levels; ++s)
        for (int v = 0; v < kViewNum; ++v) upload_foreign(cc_method, v, s);
      check(cspm_finish_cost(ctx_), ctx_, "cspm_finish_cost");
    }
  )
}

void DevicePlaneCost::upload_foreign(CCMethod *cc, int view, int level) {
  int w, h, D;
  check(cspm_get_level_dims(ctx_, level, &w, &h, &D), ctx_, "cspm_get_level_dims");
  Mat rgb[2];
  for (int v = 0; v < 2; ++v) {  // cvtColor(BGR2RGB) + convertTo(CV_64F), pre_cs_pc.cc:60-64
    std::vector<unsigned char> bgr((size_t)w * h * 3);
    check(cspm_get_level_image(ctx_, v, level, bgr.data()), ctx_, "cspm_get_level_image");
    rgb[v].create(h, w, CV_64FC3);
    for (int y = 0; y < h; ++y) {
      double *o = rgb[v].ptr<double>(y);
      for (int x = 0; x < w; ++x)
        for (int c = 0; c < 3; ++c) o[3 * x + c] = bgr[((size_t)y * w + x) * 3 + (2 - c)];
    }
  }
  std::vector<Mat> vol(D + 1);
  for (int d = 0; d <= D; ++d) vol[d] = Mat::zeros(h, w, CV_64FC1);  // pre_cs_pc.cc:50-53
  if (view == kLeft) cc->buildCV(rgb[0], rgb[1], D + 1, vol.data());
  else cc->buildRightCV(rgb[0], rgb[1], D + 1, vol.data());
  for (int d = 0; d <= D; ++d)
    check(cspm_upload_cost_slab(ctx_, view, level, d, vol[d].ptr<double>(0), vol[d].step / sizeof(double)), ctx_, "cspm_upload_cost_slab");
}

DevicePlaneCost::~DevicePlaneCost() { close_context(); }

double DevicePlaneCost::GetPlaneCost(const int &ref_x, const int &ref_y, const Plane &plane, const RefView &view) const {
  const int xy[2] = {ref_x, ref_y};
  const Vec3d n = plane.norm(), p = plane.param();
  const double np[6] = {n[0], n[1], n[2], p[0], p[1], p[2]};
  double cost = 0.0;
  check(cspm_plane_cost_batch(ctx_, view, 1, xy, np, &cost), ctx_, "cspm_plane_cost_batch");
  return cost;
}

// ---------------------------------------------------------------- CSPatchMatch (cs_patchmatch.cc:3-109)
CSPatchMatch::CSPatchMatch(const Mat &l_img, const Mat &r_img, const int &max_dis, const int &dis_scale)
    : max_dis_(max_dis), dis_scale_(dis_scale), seed_(12345), schedule_(CSPM_SCHED_RASTER), rb_rounds_(1), rb_neighbours_(4), last_ctx_(NULL), own_ctx_(NULL), pending_ctx_(NULL), pending_pp_(false), speckle_size_(0), speckle_diff_(1.0), median_r_(0), smooth_() {
  CV_Assert(l_img.type() == CV_8UC3 && r_img.type() == CV_8UC3);  // cs_patchmatch.cc:8
  img_[kLeft] = l_img.clone();
  img_[kRight] = r_img.clone();
  wid_ = l_img.cols;
  hei_ = l_img.rows;
  for (int v = 0; v < kViewNum; ++v) dis_[v] = Mat::zeros(hei_, wid_, CV_8UC1);
}

// raw photographs of a calibrated rig: rectified here (RectifyPair), then the object is what the constructor above makes of the result
static std::pair<Mat, Mat> RectifiedPair(const cspm_rig &rig, const cspm_rectification &rect, const Mat &l_raw, const Mat &r_raw) {
  std::pair<Mat, Mat> out;
  RectifyPair(rig, rect, l_raw, r_raw, out.first, out.second, NULL, NULL);
  return out;
}
CSPatchMatch::CSPatchMatch(const Mat &l_raw, const Mat &r_raw, const cspm_rig &rig, const cspm_rectification &rect, const int &max_dis, const int &dis_scale)
    : CSPatchMatch(RectifiedPair(rig, rect, l_raw, r_raw), max_dis, dis_scale) {}
CSPatchMatch::CSPatchMatch(const std::pair<Mat, Mat> &rectified, const int &max_dis, const int &dis_scale)
    : CSPatchMatch(rectified.first, rectified.second, max_dis, dis_scale) {}

// A foreign IPlaneCost (i_plane_cost.h:28-33): the device owns the plane field, the random streams and the accept rules
// (cspm_fpm_*, csrc/cspm_foreign.h); every candidate is priced by the plugin's GetPlaneCost, exactly the calls the reference
// makes (cs_patchmatch.cc:144,181,191,200,208,269,334), batch by batch.  GetPlaneCost is const and re-entrant
// (the reference calls it from OpenMP threads): the batches are evaluated in parallel when this file is built with -fopenmp.
void CSPatchMatch::PatchMatchForeign(int iter_num, const IPlaneCost *plane_cost, bool use_pp) {
  if (!own_ctx_) {
    check(cspm_create(&own_ctx_, DeviceSlot::current().device()), NULL, "cspm_create");  // the calling thread's GPU
    DevicePlaneCost::adopt(own_ctx_);
  }
  cspm_ctx *ctx = own_ctx_;
  const Mat l = img_[kLeft].clone(), r = img_[kRight].clone();
  check(cspm_set_images(ctx, l.data, r.data, l.cols, l.rows, l.step), ctx, "cspm_set_images");
  check(cspm_fpm_begin(ctx, wid_, hei_, max_dis_), ctx, "cspm_fpm_begin");
  cspm_pm_params p;
  cspm_pm_default_params(&p);
  p.seed = seed_;
  if (schedule_ != CSPM_SCHED_RASTER) throw std::runtime_error("CSPatchMatch: a foreign IPlaneCost runs the raster schedule only");
  const size_t cap = (size_t)2 * wid_ * hei_;
  std::vector<int> xy(2 * cap), view(cap);
  std::vector<double> plane(6 * cap), cost(cap);
  auto batch = [&](int phase, int iter, int step) {
    int n = 0;
    check(cspm_fpm_candidates(ctx, phase, iter, step, &p, &n, xy.data(), view.data(), plane.data()), ctx, "cspm_fpm_candidates");
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64)
#endif
    for (int i = 0; i < n; ++i) {
      cost[i] = 0.0;
      if (xy[2 * i] < 0) continue;  // no such candidate (first sweep row / column, proposal outside the image)
      const double *q = &plane[6 * (size_t)i];
      Plane pl;
      pl.set_norm(Point3d(q[0], q[1], q[2]));
      pl.set_param(Vec3d(q[3], q[4], q[5]));
      cost[i] = plane_cost->GetPlaneCost(xy[2 * i], xy[2 * i + 1], pl, view[i] == 0 ? kLeft : kRight);
    }
    check(cspm_fpm_commit(ctx, cost.data()), ctx, "cspm_fpm_commit");
  };
  int steps = 0;
  for (double z = max_dis_ / 2.0; z >= 0.1; z /= 2.0) ++steps;  // kZStopThres_ (cs_patchmatch.h:146), :299-301,342
  batch(CSPM_FPM_INIT, 0, 0);                                   // cs_patchmatch.cc:55
  for (int it = 0; it < iter_num; ++it) {                       // :65-102
    for (int k = 1; k <= wid_ + hei_ - 2; ++k) batch(CSPM_FPM_SPATIAL, it, k);
    for (int v = 0; v < kViewNum; ++v) batch(CSPM_FPM_VIEW, it, v);
    for (int st = 0; st < steps; ++st) batch(CSPM_FPM_REFINE, it, st);
  }
  if (use_pp) {  // PostProcessing reads the level-0 images of a cost object: the cheapest one provides them
    // (cspm_build_cost_img refuses max_dis > width, include/cspm.h: the fused GRD object holds the same images)
    if (max_dis_ <= wid_) check(cspm_build_cost_img(ctx, max_dis_, 35, 0, 0.0), ctx, "cspm_build_cost_img");
    else check(cspm_build_cost_grd(ctx, max_dis_, 35, 0, 0.0), ctx, "cspm_build_cost_grd");
    ApplyPostFilters(ctx);
    check(cspm_postprocess(ctx, dis_scale_, dis_[kLeft].data, dis_[kRight].data, dis_[kLeft].step), ctx, "cspm_postprocess");
  } else {
    for (int v = 0; v < kViewNum; ++v)
      check(cspm_get_disparity_u8(ctx, v, dis_scale_, dis_[v].data, dis_[v].step), ctx, "cspm_get_disparity_u8");
  }
  last_ctx_ = ctx;
}

CSPatchMatch::~CSPatchMatch() {
  if (own_ctx_) {
    DevicePlaneCost::disown(own_ctx_);
    cspm_destroy(own_ctx_);
  }
}

void CSPatchMatch::PatchMatchBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  if (pending_ctx_) throw std::runtime_error("CSPatchMatch::PatchMatchBegin: the previous run has not been ended");
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) {
    PatchMatchForeign(iter_num, plane_cost, use_pp);
    return;
  }
  cspm_ctx *ctx = dev->device_ctx();
  cspm_pm_params p;
  cspm_pm_default_params(&p);
  p.seed = seed_;
  p.schedule = schedule_;
  p.rb_rounds = rb_rounds_;
  p.rb_neighbours = rb_neighbours_;
  check(cspm_patchmatch(ctx, iter_num, &p), ctx, "cspm_patchmatch");  // asynchronous: enqueued on the context's stream
  pending_ctx_ = ctx;
  pending_pp_ = use_pp;
}

void CSPatchMatch::PatchMatchEnd() {
  cspm_ctx *ctx = pending_ctx_;
  if (!ctx) return;  // nothing pending (a foreign IPlaneCost finished inside Begin)
  pending_ctx_ = NULL;
  if (!DevicePlaneCost::is_live(ctx)) throw std::runtime_error("CSPatchMatch::PatchMatchEnd: the plane cost the run was started on has been deleted");
  if (pending_pp_) {  // PostProcessing (cs_patchmatch.cc:105-107)
    ApplyPostFilters(ctx);
    check(cspm_postprocess(ctx, dis_scale_, dis_[kLeft].data, dis_[kRight].data, dis_[kLeft].step), ctx, "cspm_postprocess");
  } else {            // PlaneToDisp (cs_patchmatch.cc:103)
    for (int v = 0; v < kViewNum; ++v)
      check(cspm_get_disparity_u8(ctx, v, dis_scale_, dis_[v].data, dis_[v].step), ctx, "cspm_get_disparity_u8");
  }
  last_ctx_ = ctx;
}

void CSPatchMatch::LocalStereoBegin(const int &ca_method, const IPlaneCost *plane_cost, const bool &use_pp) {
  if (pending_ctx_) throw std::runtime_error("CSPatchMatch::LocalStereoBegin: the previous run has not been ended");
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::LocalStereo needs one of this library's PreSSPC / PreCSPC costs");
  cspm_ctx *ctx = dev->device_ctx();
  check(cspm_local_stereo(ctx, ca_method), ctx, "cspm_local_stereo");  // asynchronous: enqueued on the context's stream
  pending_ctx_ = ctx;
  pending_pp_ = use_pp;
}

void CSPatchMatch::LocalStereo(const int &ca_method, const IPlaneCost *plane_cost, const bool &use_pp) {
  LocalStereoBegin(ca_method, plane_cost, use_pp);
  PatchMatchEnd();
}

void CSPatchMatch::SetPlanes(const RefView &view, const std::vector<Plane> &planes) {
  if (planes.size() != (size_t)wid_ * hei_) throw std::runtime_error("CSPatchMatch::SetPlanes: one plane per pixel (wid x hei) expected");
  start_planes_[view] = planes;
}

// SetPlanes' fields into the context (their costs are re-scored before anything compares against them)
void CSPatchMatch::WriteStartPlanes(cspm_ctx *ctx) {
  for (int v = 0; v < kViewNum; ++v) {
    if (start_planes_[v].empty()) continue;
    const size_t n = start_planes_[v].size();
    std::vector<double> np(6 * n), cost(n, 0.0);
    for (size_t i = 0; i < n; ++i) {
      const Vec3d nv = start_planes_[v][i].norm();
      const Vec3d pv = start_planes_[v][i].param();
      np[6 * i] = nv[0]; np[6 * i + 1] = nv[1]; np[6 * i + 2] = nv[2];
      np[6 * i + 3] = pv[0]; np[6 * i + 4] = pv[1]; np[6 * i + 5] = pv[2];
    }
    check(cspm_set_planes(ctx, v, np.data(), cost.data()), ctx, "cspm_set_planes");
    start_planes_[v].clear();
  }
}

void CSPatchMatch::PatchMatchFromBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::PatchMatchFrom needs one of this library's device costs (a foreign IPlaneCost runs cold only: PatchMatch)");
  cspm_ctx *ctx = dev->device_ctx();
  if (pending_ctx_ && pending_ctx_ != ctx) throw std::runtime_error("CSPatchMatch::PatchMatchFromBegin: the previous run has not been ended");
  WriteStartPlanes(ctx);
  cspm_pm_params p;
  cspm_pm_default_params(&p);
  p.seed = seed_;
  p.schedule = schedule_;
  p.rb_rounds = rb_rounds_;
  p.rb_neighbours = rb_neighbours_;
  check(cspm_patchmatch_warm(ctx, iter_num, &p), ctx, "cspm_patchmatch_warm");  // asynchronous: enqueued on the context's stream
  pending_ctx_ = ctx;
  pending_pp_ = use_pp;
}

void CSPatchMatch::AddCandidates(const RefView &view, const std::vector<Plane> &planes) {
  const size_t n = (size_t)wid_ * hei_;
  if (planes.size() != n) throw std::runtime_error("CSPatchMatch::AddCandidates: one plane per pixel (wid x hei) expected");
  Candidates c;
  c.norm_param.resize(6 * n);
  for (size_t i = 0; i < n; ++i) {
    const Vec3d nv = planes[i].norm();
    const Vec3d pv = planes[i].param();
    double *q = &c.norm_param[6 * i];
    q[0] = nv[0]; q[1] = nv[1]; q[2] = nv[2];
    q[3] = pv[0]; q[4] = pv[1]; q[5] = pv[2];
  }
  candidates_[view].push_back(c);
}

void CSPatchMatch::AddCandidateDisparity(const RefView &view, const Mat &disp) {
  if (disp.cols != wid_ || disp.rows != hei_ || (disp.type() != CV_32FC1 && disp.type() != CV_64FC1))
    throw std::runtime_error("CSPatchMatch::AddCandidateDisparity: a CV_32FC1 or CV_64FC1 map of the image size expected");
  const size_t n = (size_t)wid_ * hei_;
  Candidates c;
  c.norm_param.assign(6 * n, 0.0);
  c.mask.assign(n, 0);
  for (int y = 0; y < hei_; ++y)
    for (int x = 0; x < wid_; ++x) {
      const double d = disp.type() == CV_32FC1 ? (double)disp.at<float>(y, x) : disp.at<double>(y, x);
      const size_t i = (size_t)y * wid_ + x;
      if (!std::isfinite(d) || d < 0.0) continue;  // no candidate
      c.norm_param[6 * i + 2] = 1.0;  // the fronto-parallel plane (0, 0, 1, 0, 0, d)
      c.norm_param[6 * i + 5] = d;
      c.mask[i] = 1;
    }
  candidates_[view].push_back(c);
}

void CSPatchMatch::AddCandidateDisparity(const RefView &view, const Mat &disp, const cspm_fit_params &params) {
  if (disp.cols != wid_ || disp.rows != hei_ || (disp.type() != CV_32FC1 && disp.type() != CV_64FC1))
    throw std::runtime_error("CSPatchMatch::AddCandidateDisparity: a CV_32FC1 or CV_64FC1 map of the image size expected");
  const size_t n = (size_t)wid_ * hei_;
  std::vector<double> d(n);
  std::vector<uint8_t> valid(n);
  for (int y = 0; y < hei_; ++y)
    for (int x = 0; x < wid_; ++x) {
      const size_t i = (size_t)y * wid_ + x;
      d[i] = disp.type() == CV_32FC1 ? (double)disp.at<float>(y, x) : disp.at<double>(y, x);
      valid[i] = std::isfinite(d[i]) && d[i] >= 0.0;  // what the fronto-parallel overload takes as a candidate
    }
  Candidates c;
  c.norm_param.resize(6 * n);
  c.mask.resize(n);
  const Mat &g = img_[view];
  check(cspm_fit_planes_host(DevicePlaneCost::device, d.data(), valid.data(), g.data, g.step, wid_, hei_, max_dis_, &params, c.norm_param.data(),
                             c.mask.data()), NULL, "cspm_fit_planes_host");
  candidates_[view].push_back(c);
}

void CSPatchMatch::FitPlanes(const IPlaneCost *plane_cost, const cspm_fit_params &params, const bool &merge) {
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::FitPlanes needs one of this library's device costs");
  cspm_ctx *ctx = dev->device_ctx();
  if (pending_ctx_ && pending_ctx_ != ctx) throw std::runtime_error("CSPatchMatch::FitPlanes: the previous run has not been ended");
  check(cspm_fit_planes(ctx, &params, merge ? 1 : 0), ctx, "cspm_fit_planes");  // asynchronous: enqueued on the context's stream
}

void CSPatchMatch::SegmentPlanes(const IPlaneCost *plane_cost, const cspm_seg_params &params, const bool &merge) {
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::SegmentPlanes needs one of this library's device costs");
  cspm_ctx *ctx = dev->device_ctx();
  if (pending_ctx_ && pending_ctx_ != ctx) throw std::runtime_error("CSPatchMatch::SegmentPlanes: the previous run has not been ended");
  check(cspm_segment_planes(ctx, &params, merge ? 1 : 0), ctx, "cspm_segment_planes");  // asynchronous: enqueued on the context's stream
}

void CSPatchMatch::SeededBegin(bool keep, int iter_num, const IPlaneCost *plane_cost, bool use_pp) {
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::PatchMatchSeeded / PatchMatchKeep need one of this library's device costs (a foreign IPlaneCost runs cold only: PatchMatch)");
  cspm_ctx *ctx = dev->device_ctx();
  if (pending_ctx_ && pending_ctx_ != ctx) throw std::runtime_error("CSPatchMatch::PatchMatchSeededBegin / PatchMatchKeepBegin: the previous run has not been ended");
  cspm_pm_params p;
  cspm_pm_default_params(&p);
  p.seed = seed_;
  p.schedule = schedule_;
  p.rb_rounds = rb_rounds_;
  p.rb_neighbours = rb_neighbours_;
  if (keep) {
    WriteStartPlanes(ctx);
    check(cspm_pm_init_keep(ctx, &p), ctx, "cspm_pm_init_keep");
  } else {
    check(cspm_pm_init(ctx, &p), ctx, "cspm_pm_init");
  }
  for (int v = 0; v < kViewNum; ++v) {
    for (size_t k = 0; k < candidates_[v].size(); ++k) {
      const Candidates &c = candidates_[v][k];
      check(cspm_merge_planes_host(ctx, v, c.norm_param.data(), c.mask.empty() ? NULL : c.mask.data()), ctx, "cspm_merge_planes_host");
    }
    candidates_[v].clear();
  }
  check(cspm_patchmatch_warm(ctx, iter_num, &p), ctx, "cspm_patchmatch_warm");  // asynchronous: enqueued on the context's stream
  pending_ctx_ = ctx;
  pending_pp_ = use_pp;
}

void CSPatchMatch::PatchMatchSeededBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  SeededBegin(false, iter_num, plane_cost, use_pp);
}
void CSPatchMatch::PatchMatchSeeded(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  SeededBegin(false, iter_num, plane_cost, use_pp);
  PatchMatchEnd();
}
void CSPatchMatch::PatchMatchKeepBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  SeededBegin(true, iter_num, plane_cost, use_pp);
}
void CSPatchMatch::PatchMatchKeep(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  SeededBegin(true, iter_num, plane_cost, use_pp);
  PatchMatchEnd();
}

void CSPatchMatch::PatchMatchCarriedBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp, const CSPatchMatch &prev,
                                          const cspm_calib &prev_calib, const cspm_calib &calib, const double *R, const double *t,
                                          const cspm_carry_params *params) {
  const IDevicePlaneCost *dev = dynamic_cast<const IDevicePlaneCost *>(plane_cost);
  if (!dev) throw std::runtime_error("CSPatchMatch::PatchMatchCarried needs one of this library's device costs (a foreign IPlaneCost runs cold only: PatchMatch)");
  cspm_ctx *ctx = dev->device_ctx();
  if (pending_ctx_ && pending_ctx_ != ctx) throw std::runtime_error("CSPatchMatch::PatchMatchCarriedBegin: the previous run has not been ended");
  if (!prev.last_ctx_ || prev.pending_ctx_) throw std::runtime_error("CSPatchMatch::PatchMatchCarried: the previous matcher has no finished run");
  if (!DevicePlaneCost::is_live(prev.last_ctx_)) throw std::runtime_error("CSPatchMatch::PatchMatchCarried: the plane cost the previous matcher ran on has been deleted");
  cspm_pm_params p;
  cspm_pm_default_params(&p);
  p.seed = seed_;
  p.schedule = schedule_;
  p.rb_rounds = rb_rounds_;
  p.rb_neighbours = rb_neighbours_;
  check(cspm_pm_init(ctx, &p), ctx, "cspm_pm_init");
  check(cspm_carry_planes(ctx, prev.last_ctx_, &prev_calib, &calib, R, t, params, 1), ctx, "cspm_carry_planes");
  check(cspm_patchmatch_warm(ctx, iter_num, &p), ctx, "cspm_patchmatch_warm");  // asynchronous: enqueued on the context's stream
  pending_ctx_ = ctx;
  pending_pp_ = use_pp;
}

void CSPatchMatch::PatchMatchCarried(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp, const CSPatchMatch &prev,
                                     const cspm_calib &prev_calib, const cspm_calib &calib, const double *R, const double *t,
                                     const cspm_carry_params *params) {
  PatchMatchCarriedBegin(iter_num, plane_cost, use_pp, prev, prev_calib, calib, R, t, params);
  PatchMatchEnd();
}

void CSPatchMatch::PatchMatchFrom(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  PatchMatchFromBegin(iter_num, plane_cost, use_pp);
  PatchMatchEnd();
}

void CSPatchMatch::PatchMatch(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp) {
  PatchMatchBegin(iter_num, plane_cost, use_pp);
  PatchMatchEnd();
}

void CSPatchMatch::disparity(const RefView &view, std::vector<double> *out) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::disparity before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::disparity: the plane cost PatchMatch ran on has been deleted");
  out->resize((size_t)wid_ * hei_);
  check(cspm_get_disparity_f64(last_ctx_, view, out->data()), last_ctx_, "cspm_get_disparity_f64");
}

void CSPatchMatch::PostProcessedDisparity(std::vector<double> *l_out, std::vector<double> *r_out) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::PostProcessedDisparity before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::PostProcessedDisparity: the plane cost PatchMatch ran on has been deleted");
  if (!l_out && !r_out) return;
  std::vector<double> unwanted;  // the library post-processes both views in one call
  std::vector<double> *outs[kViewNum] = {l_out ? l_out : &unwanted, r_out ? r_out : &unwanted};
  for (int v = 0; v < kViewNum; ++v) outs[v]->resize((size_t)wid_ * hei_);
  ApplyPostFilters(last_ctx_);
  check(cspm_postprocess_f64(last_ctx_, outs[kLeft]->data(), outs[kRight]->data(), NULL, NULL), last_ctx_, "cspm_postprocess_f64");
}

size_t CSPatchMatch::Reproject(const RefView &view, const cspm_calib &calib, const cspm_geom_params &params, int source, const cspm_fit_params *fit,
                               std::vector<double> *depth, std::vector<double> *xyz, std::vector<double> *normal, std::vector<uint8_t> *keep,
                               std::vector<cspm_point> *cloud) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::Reproject before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::Reproject: the plane cost PatchMatch ran on has been deleted");
  const size_t n = (size_t)wid_ * hei_;
  if (depth) depth->resize(n);
  if (xyz) xyz->resize(3 * n);
  if (normal) normal->resize(3 * n);
  if (keep) keep->resize(n);
  if (cloud) cloud->resize(n);
  if (source == CSPM_GEOM_PP) ApplyPostFilters(last_ctx_);
  unsigned int count = 0;
  check(cspm_reproject(last_ctx_, view, source, &calib, &params, fit, depth ? depth->data() : NULL, xyz ? xyz->data() : NULL,
                       normal ? normal->data() : NULL, keep ? keep->data() : NULL, cloud ? cloud->data() : NULL, cloud ? n : 0, &count),
        last_ctx_, "cspm_reproject");
  if (cloud) cloud->resize(count);
  return count;
}

size_t CSPatchMatch::Mesh(const RefView &view, const cspm_calib &calib, const cspm_geom_params &params, const cspm_mesh_params &mesh_params, int source,
                          const cspm_fit_params *fit, std::vector<cspm_point> *vertices, std::vector<cspm_face> *faces, std::vector<uint8_t> *quad) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::Mesh before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::Mesh: the plane cost PatchMatch ran on has been deleted");
  const size_t n = (size_t)wid_ * hei_, max_faces = 2 * (size_t)(wid_ - 1) * (size_t)(hei_ - 1);
  if (vertices) vertices->resize(n);
  if (faces) faces->resize(max_faces);
  if (quad) quad->resize(n);
  if (source == CSPM_GEOM_PP) ApplyPostFilters(last_ctx_);
  unsigned int nv = 0, nf = 0;
  check(cspm_mesh(last_ctx_, view, source, &calib, &params, fit, &mesh_params, vertices ? vertices->data() : NULL, vertices ? n : 0,
                  faces ? faces->data() : NULL, faces ? max_faces : 0, quad ? quad->data() : NULL, &nv, &nf),
        last_ctx_, "cspm_mesh");
  if (vertices) vertices->resize(nv);
  if (faces) faces->resize(nf);
  return nf;
}

void CSPatchMatch::Synthesize(double t, const cspm_synth_params &params, int source, Mat *bgr, std::vector<double> *disp, std::vector<uint8_t> *mask) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::Synthesize before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::Synthesize: the plane cost PatchMatch ran on has been deleted");
  const size_t n = (size_t)wid_ * hei_;
  if (bgr) bgr->create(hei_, wid_, CV_8UC3);
  if (disp) disp->resize(n);
  if (mask) mask->resize(n);
  if (source == CSPM_GEOM_PP) ApplyPostFilters(last_ctx_);
  check(cspm_synthesize(last_ctx_, source, &params, t, bgr ? bgr->ptr<unsigned char>(0) : NULL, bgr ? bgr->step : 0, disp ? disp->data() : NULL,
                        mask ? mask->data() : NULL),
        last_ctx_, "cspm_synthesize");
}

void CSPatchMatch::SetSpeckleFilter(int max_size, double max_diff) {
  if (max_size < 0 || !(max_diff >= 0.0) || !std::isfinite(max_diff))
    throw std::runtime_error("CSPatchMatch::SetSpeckleFilter: max_size >= 0 and a finite max_diff >= 0 expected");
  speckle_size_ = max_size;
  speckle_diff_ = max_diff;
}

// a context serves one cost object after the other (and, parked, one pair after the other): every post-processing sets what it wants
void CSPatchMatch::ApplyPostFilters(cspm_ctx *ctx) const {
  check(cspm_set_pp_speckle(ctx, speckle_size_, speckle_diff_), ctx, "cspm_set_pp_speckle");
  check(cspm_set_pp_median(ctx, median_r_), ctx, "cspm_set_pp_median");
  check(cspm_set_pp_smooth(ctx, &smooth_), ctx, "cspm_set_pp_smooth");
}

void CSPatchMatch::SetSmoothing(const cspm_smooth_params *params) {
  if (!params || params->lambda == 0.0) {
    smooth_.lambda = 0.0;
    return;
  }
  const cspm_smooth_params &p = *params;
  if (!(p.lambda >= 0.0) || !std::isfinite(p.lambda) || !(p.sigma_color > 0.0) || !std::isfinite(p.sigma_color) || p.iterations < 1 || p.iterations > 8 ||
      !(p.fill_conf >= 0.0 && p.fill_conf <= 1.0))
    throw std::runtime_error("CSPatchMatch::SetSmoothing: lambda >= 0, sigma_color > 0 (both finite), iterations 1 .. 8 and fill_conf in [0, 1] expected");
  smooth_ = p;
}

// include/cspm.h S over the device smoother: the Mats' rows are packed first (clone), dst may be src
void SmoothDisparity(const Mat &src, const Mat *conf, const Mat *guide, const cspm_smooth_params *params, int max_dis, Mat &dst) {
  if (src.empty() || src.type() != CV_64FC1) throw std::runtime_error("SmoothDisparity: a CV_64FC1 disparity map expected");
  if (conf && (conf->type() != CV_64FC1 || conf->rows != src.rows || conf->cols != src.cols))
    throw std::runtime_error("SmoothDisparity: the confidences must be a CV_64FC1 map of the disparity map's size");
  if (guide && (guide->type() != CV_8UC3 || guide->rows != src.rows || guide->cols != src.cols))
    throw std::runtime_error("SmoothDisparity: the guide must be a CV_8UC3 image of the disparity map's size");
  const Mat d = src.clone(), c = conf ? conf->clone() : Mat(), g = guide ? guide->clone() : Mat();
  Mat tmp(src.rows, src.cols, CV_64FC1);
  check(cspm_smooth_disparity_host(DeviceSlot::current().device(), d.ptr<double>(0), conf ? c.ptr<double>(0) : NULL, guide ? g.ptr<unsigned char>(0) : NULL,
                                   src.cols, src.rows, params, max_dis, tmp.ptr<double>(0)),
        NULL, "SmoothDisparity");
  dst = tmp;
}

void SegmentImage(const Mat &img, Mat &labels, const cspm_seg_params *params) {
  if (img.empty() || img.type() != CV_8UC3) throw std::runtime_error("SegmentImage: a CV_8UC3 image expected");
  Mat tmp(img.rows, img.cols, CV_32SC1);
  check(cspm_segment_host(DeviceSlot::current().device(), img.data, img.step, img.cols, img.rows, params, tmp.ptr<int32_t>(0), NULL, NULL), NULL,
        "SegmentImage");
  labels = tmp;
}

void SegmentPlanes(const Mat &disp, const Mat *valid, const Mat &labels, const cspm_seg_params *params, int max_dis, std::vector<Plane> *planes, Mat *fitted,
                   std::vector<double> *seg_abc) {
  if (disp.empty() || disp.type() != CV_64FC1) throw std::runtime_error("SegmentPlanes: a CV_64FC1 disparity map expected");
  if (labels.type() != CV_32SC1 || labels.rows != disp.rows || labels.cols != disp.cols)
    throw std::runtime_error("SegmentPlanes: the labels must be a CV_32SC1 map of the disparity map's size");
  if (valid && (valid->type() != CV_8UC1 || valid->rows != disp.rows || valid->cols != disp.cols))
    throw std::runtime_error("SegmentPlanes: the mask must be a CV_8UC1 map of the disparity map's size");
  const Mat d = disp.clone(), l = labels.clone(), v = valid ? valid->clone() : Mat();  // packed rows
  const size_t n = (size_t)disp.rows * disp.cols;
  cspm_seg_params p;
  cspm_seg_default_params(&p);
  if (params) p = *params;
  const int K = cspm_segment_count(disp.cols, disp.rows, p.step);
  std::vector<double> np(6 * n), abc(K > 0 ? 3 * (size_t)K : 0);
  Mat fit(disp.rows, disp.cols, CV_8UC1);
  check(cspm_segment_planes_host(DeviceSlot::current().device(), d.ptr<double>(0), valid ? v.ptr<unsigned char>(0) : NULL, l.ptr<int32_t>(0), disp.cols,
                                 disp.rows, max_dis, &p, K > 0 ? abc.data() : NULL, NULL, np.data(), fit.ptr<unsigned char>(0)),
        NULL, "SegmentPlanes");
  if (planes) {
    planes->resize(n);
    for (size_t i = 0; i < n; ++i) {
      Plane pl;
      pl.set_norm(Point3d(np[6 * i], np[6 * i + 1], np[6 * i + 2]));
      pl.set_param(Vec3d(np[6 * i + 3], np[6 * i + 4], np[6 * i + 5]));
      (*planes)[i] = pl;
    }
  }
  if (fitted) *fitted = fit;
  if (seg_abc) seg_abc->swap(abc);
}

void CSPatchMatch::SetMedianFilter(int r) {
  if (r < 0 || r > CSPM_MEDIAN_MAX_RADIUS) throw std::runtime_error("CSPatchMatch::SetMedianFilter: a radius of 0 (off) .. 7 expected");
  median_r_ = r;
}

// commfunc.cc:11-25 over the device filter (include/cspm.h M8).  src and dst may be the same Mat, as in the reference's own call.
void MedianFilter(const Mat &src, Mat &dst, int r) {
  CV_Assert(src.depth() == CV_8U);
  Mat tmp(src.rows, src.cols, src.type());
  check(cspm_median_filter_u8_host(DeviceSlot::current().device(), src.data, src.step, src.cols, src.rows, src.channels(), r, tmp.data, tmp.step), NULL,
        "MedianFilter");
  dst = tmp;
}

void CSPatchMatch::planes(const RefView &view, std::vector<Plane> *out, std::vector<double> *min_cost) const {
  if (!last_ctx_) throw std::runtime_error("CSPatchMatch::planes before PatchMatch");
  if (!DevicePlaneCost::is_live(last_ctx_)) throw std::runtime_error("CSPatchMatch::planes: the plane cost PatchMatch ran on has been deleted");
  const size_t n = (size_t)wid_ * hei_;
  std::vector<double> np(6 * n), cost(n);
  check(cspm_get_planes(last_ctx_, view, np.data(), cost.data()), last_ctx_, "cspm_get_planes");
  if (out) {
    out->resize(n);
    for (size_t i = 0; i < n; ++i) {
      Plane pl;
      pl.set_norm(Point3d(np[6 * i], np[6 * i + 1], np[6 * i + 2]));
      pl.set_param(Vec3d(np[6 * i + 3], np[6 * i + 4], np[6 * i + 5]));
      (*out)[i] = pl;
    }
  }
  if (min_cost) *min_cost = cost;
}
