// cspm_api.hip -- host side of libcspm_hip.so: the C ABI declared in include/cspm.h.
// Owns device memory, builds the plane-cost object (PreSSPC / PreCSPC) on the device and drives the
// PatchMatch kernels.  No CPU fallback anywhere: without a usable gfx950 device every call fails.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "cspm_kernels.h"
#include "cspm_pool.h"
#include "cspm_pp.h"
#include "cspm_speckle.h"
#include "cspm_median.h"
#include "cspm_smooth.h"
#include "cspm_fit.h"
#include "cspm_seg.h"
#include "cspm_geom.h"
#include "cspm_mesh.h"
#include "cspm_fuse.h"
#include "cspm_tsdf.h"
#include "cspm_tsdf_mesh.h"
#include "cspm_register.h"
#include "cspm_carry.h"
#include "cspm_synth.h"
#include "cspm_rect.h"
#include "cspm_ca.h"

using namespace cspm;

namespace {

thread_local std::string g_create_error;  // error of a failed cspm_create, per calling thread (cspm_last_error(NULL))

struct TimingRec {
  int kclass;
  hipEvent_t a, b;
  long long evals;
};

// the allocator pair of every DevPool of this file
int dev_alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
void dev_free(void *p) { (void)hipFree(p); }

}  // namespace

// every extern "C" entry that touches HIP runs on the ctx's device (ON_DEVICE), a one-shot host entry on the device it names (OneShot),
// and leaves the caller's current device as it found it
struct DevGuard {
  int prev = -1;
  bool ok = true;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    else prev = -1;
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// who built the cost object: cspm_begin_cost (uploaded volumes), cspm_build_cost_grd / _cen / _img (GrdPC / CSPC: no cells, no volumes) / _cengrd
enum CostKind { kKindNone = -1, kKindForeign = 0, kKindGrd = 1, kKindCen = 2, kKindImg = 3, kKindCenGrd = 4 };

// what the buffers of a cost object were sized for: an identical request reuses them (no hipMalloc / hipFree per pair).
// `kind` is also THE kind of the context's cost object (alloc_cost sets it, free_cost clears it); whether its cells come from volumes
// or are computed on the fly is Cost::fused
struct CostKey {
  int W = 0, H = 0, max_dis = 0, wnd = 0, scale_num = -1, with_vol = 0, with_pairs = 0, with_cvol = 0, with_px8 = 0;
  CostKind kind = kKindNone;
  bool operator==(const CostKey &o) const {
    return W == o.W && H == o.H && max_dis == o.max_dis && wnd == o.wnd && scale_num == o.scale_num && with_vol == o.with_vol && kind == o.kind &&
           with_pairs == o.with_pairs && with_cvol == o.with_cvol && with_px8 == o.with_px8;
  }
};

// an asynchronous output (cspm_disparity_u8_device / cspm_postprocess_device / cspm_postprocess_f64_device)
enum OutKind { kOutDisp, kOutPost8, kOutPostF64 };  // PlaneToDisp of one view, the 8-bit PostProcessing, the sub-pixel one
struct OutReq { OutKind kind; int view, dis_scale; void *o0, *o1; };

// WHEN A RUN IS REPEATED AFTER A SWEEP TIMEOUT.  A persistent raster sweep that gives up waiting raises a sticky error word, which the
// next call that synchronises with the host anyway looks at (check_sweep).  A timeout is slowness, not a wrong result: when exactly ONE
// whole run (cspm_patchmatch / cspm_patchmatch_warm) began since the last check and nothing tainted it, it is repeated with per-diagonal
// launches, and so are the outputs enqueued behind it; anything else is an error.  Only the operations below touch the fields.
// The two taints differ on purpose:
//   taint()               stays until the next check that finds a sweep pending.  For what no whole run can stand for: the single phases
//                         cspm_pm_init / _spatial / _view / _refine, cspm_rescore_planes, cspm_set_planes (the caller's costs) and
//                         cspm_fpm_begin (a foreign cost drives the field).
//   taint_unchecked_run() counts only behind a run that has not been checked: its inputs (alloc_cost, set_images_impl) or its planes
//                         (cspm_local_stereo, cspm_upsample_planes, cspm_merge_planes, cspm_merge_planes_host, cspm_pm_init_keep) are no
//                         longer what it ran on.  In front of a run they are its start -- a warm run snapshots it -- and taint nothing.
// Known limit: take() is not called while no sweep is pending, so a taint() outlives its call and blocks the repeat of the NEXT run:
// a timeout behind cspm_pm_init or cspm_set_planes + cspm_patchmatch_warm is an error, behind cspm_pm_init_keep or cspm_local_stereo +
// cspm_patchmatch_warm it is repeated.
struct Repeat {
  struct Record {
    int runs = 0;  // whole runs begun since the last check
    bool tainted = false;
    bool warm = false;  // the last run was cspm_patchmatch_warm: a repeat starts from warm_snap, not from the init
    int iters = 0;
    cspm_pm_params params{};
    std::vector<OutReq> outs;
  };
  // a whole run begins; the outputs behind an earlier run go, that run can no longer be repeated (two runs unchecked = an error)
  void begin_run(bool warm, int iters, const cspm_pm_params &params) {
    r_.warm = warm; r_.iters = iters; r_.params = params;
    r_.outs.clear();
    ++r_.runs;
  }
  void sweep_enqueued() { pending_ = true; }  // a persistent sweep's error word has not been checked yet
  bool pending() const { return pending_; }
  void taint() { r_.tainted = true; }
  void taint_unchecked_run() { r_.tainted = r_.tainted || r_.runs > 0; }
  // while a sweep is pending: a later request for the same kind of map into the same buffers replaces the earlier one
  void remember_output(const OutReq &q) {
    for (auto it = r_.outs.begin(); it != r_.outs.end(); ++it)
      if (it->kind == q.kind && it->o0 == q.o0 && it->o1 == q.o1 && (q.kind != kOutDisp || it->view == q.view)) { r_.outs.erase(it); break; }
    r_.outs.push_back(q);
  }
  // the pending sweep has been checked: what ran since the check before, and a clean record
  Record take() {
    const Record out = r_;
    r_ = Record{};
    pending_ = false;
    return out;
  }

 private:
  bool pending_ = false;
  Record r_;
};

struct cspm_ctx {
  int device = 0, ncu = 256;
  // persistent sweep: workgroups launched per CU (env CSPM_SWEEP_WG).  2..6 take the same time when the pair is alone (the sweep
  // is bound by its dependency chain; 1 is 43 % slower); the resident workgroups mostly wait, and every one of them holds
  // registers another pair's refinement could use: with three pairs in flight 2 gives 222.7 ms per pair, 3 gives 228.1.
  int sweep_wg_per_cu = 0;           // 0 = the default, 2: a CU evaluates two sweep pixels at full speed -- with three resident AND computing (the dataflow sweep) a pixel takes 23 us instead of 9
  int sweep_bands = 1;               // row bands of the persistent sweep (env CSPM_SWEEP_BANDS, up to 8; 1 = one queue for the whole image: the default,
                                     // bands help only the paired-cell volumes)
  int sweep_bands_built = 0;         // what d_sweep_start was filled for
  int refine_chunk = 64;  // PlaneRefinement halving steps per launch (tuning knob, env CSPM_REFINE_CHUNK)
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::string err;
  // device memory: one pool per lifetime owns every allocation the context keeps (DESIGN.md "Context memory")
  DevPool mem_images{dev_alloc, dev_free};  // img0, stage: until the geometry changes
  DevPool mem_cost{dev_alloc, dev_free};    // the cost object: until free_cost
  DevPool mem_field{dev_alloc, dev_free};   // the plane field and what is "kept with the field": until free_field
  DevPool mem_rect{dev_alloc, dev_free};    // the rectification: until free_rect
  DevPool mem_ca{dev_alloc, dev_free};      // local-stereo scratch: until ca_ensure meets a new key or the geometry changes
  DevPool mem_tsdf{dev_alloc, dev_free};    // the TSDF volume: from cspm_tsdf_begin until cspm_tsdf_end, whatever the fusion views do
  DevPool mem_fuse{dev_alloc, dev_free};    // the fusion views: from cspm_fuse_begin until cspm_fuse_end, whatever the geometry does
  // images
  int W = 0, H = 0;
  uint32_t *img0[2] = {nullptr, nullptr};
  uint8_t *stage = nullptr;  // host-image staging buffer (cspm_set_images), 3*W*H bytes, kept
  size_t stage_bytes = 0;
  // cost object
  bool cost_alloc = false, cost_ready = false;
  Cost cost{};
  int max_dis = 0, wnd = 0;
  double scale_wgt[CSPM_MAX_LEVELS] = {0};
  double host_max_cost[2 * CSPM_MAX_LEVELS] = {0};
  CostKey cost_key;
  bool max_cost_fetched = false;  // host_max_cost mirrors d_maxcost
  int *d_early_ok = nullptr;      // device flag: every max_cost (and, for uploaded volumes, every min) is >= 0
  uint8_t *cen_gray[2][CSPM_MAX_LEVELS] = {{nullptr}};
  double *d_lut = nullptr, *d_lut_a = nullptr, *d_maxcost = nullptr;
  long long opt_cengrd_fused = 0; // CSPM_OPT_CENGRD_FUSED
  const uint32_t *cen_code[2][CSPM_MAX_LEVELS] = {{nullptr}};
  long long opt_grd_volumes = 0; // CSPM_OPT_GRD_VOLUMES
  long long opt_sweep_pairs = 0;   // CSPM_OPT_SWEEP_PAIRS: 0 = never (default: measured no faster), 1 = when they fit
  long long sweep_pairs_limit = 4LL << 30;  // bytes of paired-cell volumes a context may hold (env CSPM_SWEEP_PAIRS_MAX_MB)
  bool sweep_pairs = false;      // this cost object carries Level::vol2: the raster sweep reads paired cells (kSrcVol2)
  long long opt_table_volumes = 1;          // CSPM_OPT_TABLE_VOLUMES: device-cell volumes for the row engine's DMA-filled tables, when they fit
  long long table_volumes_limit = 48LL << 30; // bytes of such volumes a context may hold (env CSPM_TABLE_VOLUMES_MAX_MB): 288 GB of HBM per GPU, a few contexts in flight
  long long opt_sweep_packed = 0;           // CSPM_OPT_SWEEP_PACKED: 1 = the raster sweep of a fused GRD cost reads packed 8-byte elements (kSrcGrd8); 0 (default: measured
                                            // 8 % slower -- the sweep is latency-bound and the unpacking adds VALU work to every step) = the 12-byte elements
  bool sweep_packed = false;                // this cost object carries Level::px8
  unsigned int *d_px8_bad = nullptr;        // device counter: gradients k_make_px8 could not pack (must stay 0)
  double volumes_mem_fraction = 0.5;        // of the memory hipMemGetInfo reports free when a cost object is allocated, the share the optional volumes (cvol, vol2) may take (env CSPM_VOLUMES_MEM_FRACTION)
  long long optional_volume_fallbacks = 0;  // times a hipMalloc of an optional volume failed and the pair went on without (CSPM_OPT_VOLUME_FALLBACKS)
  bool optional_missing = false;            // the current cost object wanted optional volumes and runs without them
  long long optional_reuses = 0;            // pairs that reused it since
  long long volume_retry_pairs = 16;        // CSPM_OPT_VOLUME_RETRY_PAIRS: ask again for the volumes every so many reuses (0 = never)
  int fault_volume_alloc = 0;               // fault injection for the tests: the n-th optional-volume allocation of this context fails (CSPM_OPT_FAULT_VOLUME_ALLOC, a test hook: nothing in the environment reaches it)
  int sweep_grid_cap = 0;                   // CSPM_OPT_SWEEP_GRID, a test hook: 0 = the library's grid, else at most max(this, bands) workgroups in the persistent sweep
  unsigned long long *d_maxkeys = nullptr;
  int row_claim = -1;  // row kernels: -1 = claimed column bands for launches of several rounds (default), 0 / 1 = never / always (env CSPM_ROW_CLAIM, tests)
  unsigned int *d_rowq = nullptr;  // row kernels: the eight claim counters of a launch that claims its items (cspm_rows.h row_item)
  // plane field
  bool field_alloc = false;
  bool field_consistent = false;  // every min_cost was computed from the stored plane by this cost object (not by cspm_set_planes)
  double *field_mem = nullptr;
  Field f[2]{};
  ViewCand vc{nullptr, nullptr, nullptr, nullptr};
  long long opt_sweep_fold = 0;  // CSPM_OPT_SWEEP_FOLD: cross-scale sweep workgroups of levels - 1 waves, the last level folded onto them (for contexts that share their GPU)
  long long opt_view_sort = 1;  // CSPM_OPT_VIEW_SORT: view propagation evaluates a row's proposals in the order of their target column
  uint8_t *d_dis[2] = {nullptr, nullptr};
  uint8_t *d_valid[2] = {nullptr, nullptr};  // post-processing: left-right consistency flags
  unsigned int *d_todo = nullptr;            // post-processing: per view n indices of inconsistent pixels, then the two counts
  double *d_pp[2] = {nullptr, nullptr};      // sub-pixel post-processing (cspm_postprocess_f64): the two f64 maps, allocated by its first call and kept
  int pp_speckle_size = 0;                   // cspm_set_pp_speckle: 0 = no speckle filter (no launch, no scratch)
  double pp_speckle_diff = 1.0;
  int *d_speckle = nullptr;                  // speckle filter: per view n parents, then per view n counts, then the removed-pixel counter; allocated by the first filtered call and kept
  int pp_median = 0;                         // cspm_set_pp_median: radius of the final median filter, 0 = none (no launch, no second buffer)
  uint8_t *d_med8[2] = {nullptr, nullptr};   // median filter: the second 8-bit buffer per view; swapped with d_dis by every filtered call.  Allocated by the first one and kept
  double *d_med64 = nullptr;                 // median filter: the second pair of f64 maps (one allocation, like d_pp); swapped with d_pp[0]
  cspm_smooth_params pp_smooth = {0.0, 20.0, 3, 0.25};  // cspm_set_pp_smooth: lambda == 0 = no smoothing (no launch, no scratch)
  double *d_smooth = nullptr;                // smoothing: N, M and ct of both views (one allocation of 6 maps), then the table; allocated by the first smoothed call and kept
  std::vector<double> smooth_lut;            // the host's copy of the uploaded exp(-k / sigma) table
  double smooth_lut_sigma = 0.0;             // ... and the sigma it was computed for (0 = none yet)
  bool speckle_ran = false;                  // the last post-processing enqueued ran the filter (CSPM_OPT_PP_SPECKLE_REMOVED reads its counter)
  // persistent raster sweep (k_spatial_sweep)
  unsigned int *d_sweep_ctrl = nullptr, *d_sweep_start = nullptr;
  unsigned long long *d_sweep_gran = nullptr;  // persistent sweep: 12 data-tagged granules per pixel and view (cspm_chain.h)
  unsigned int *d_sweep_ready = nullptr, *d_sweep_qctl = nullptr;  // dataflow sweep (k_spatial_flow): final predecessors per pixel; queue control words
  unsigned long long *d_sweep_queue = nullptr;                      // ... and its queue of ready pixels
  long long opt_sweep_flow = 0;  // CSPM_OPT_SWEEP_FLOW: 1 = the persistent raster sweep is scheduled by dataflow (k_spatial_flow), 0 (default: measured faster) = by ordered claims (k_spatial_sweep)
  unsigned int sweep_epoch = 0;
  long long opt_raster_launches = 0;  // CSPM_OPT_RASTER_LAUNCHES
  long long sweep_timeout_ms = 3000;  // CSPM_OPT_SWEEP_TIMEOUT_MS (env CSPM_SWEEP_TIMEOUT_MS): bound of one wait for a predecessor pixel
  Repeat repeat;                      // when a run is repeated after a sweep timeout
  double *warm_snap = nullptr;        // the starting field of the last warm run (both views, 7 arrays each), kept with the field
  double *cand_mem = nullptr;         // cspm_merge_planes_host, cspm_fit_planes, cspm_segment_planes: one view's candidate planes (6 arrays) and, behind them, its mask bytes (ensure_cand); allocated by the first such call and kept with the field
  double *fit_mem = nullptr;          // cspm_fit_planes: both views' disparity snapshots (2 arrays) and, behind them, the exp(-k/10) table; allocated by the first such call and kept with the field
  char *seg_mem = nullptr;            // cspm_segment_planes: both views' disparity snapshots and labels, then centres, counts and segment planes for the finest grid (step 4); allocated by the first such call and kept with the field
  bool seg_ran = false;               // cspm_get_segments: seg_mem holds the labels of a call
  double *geom_disp = nullptr;        // cspm_reproject: the CSPM_GEOM_RAW disparity map (1 array); allocated by the first such call and kept with the field
  double *geom_fit = nullptr;         // cspm_reproject with a fit: the fitted planes (6 arrays) and, behind them, the exp(-k/10) table
  unsigned int *geom_counts = nullptr;  // cspm_reproject: the kept pixels per workgroup, then the total
  uint8_t *mesh_bytes = nullptr;      // cspm_mesh: keep and Q (2 byte maps); allocated by the first such call and kept with the field
  uint32_t *mesh_map = nullptr;       // cspm_mesh: the pixel -> vertex map, then the vertex and the face counts per workgroup, each with its total
  double *synth_disp = nullptr;       // cspm_synthesize: both views' CSPM_GEOM_RAW disparity maps (2 arrays); allocated by the first such call and kept with the field
  uint32_t *carry_mem = nullptr;      // cspm_carry_planes into this context: a 64-bit depth key, then a 32-bit winner per pixel (3 words each); allocated by the first such call and kept with the field
  // depth-map fusion (cspm_fuse_*): the slots of max_views views of fuse_w x fuse_h, kept in mem_fuse
  bool fuse_on = false;
  int fuse_w = 0, fuse_h = 0, fuse_max = 0, fuse_views = 0;
  unsigned long long fuse_image_mask = 0;          // bit k: view k came with an image
  bool fuse_normals = false, fuse_images = false;  // the views pushed so far carry normals / at least one of them an image
  double *fuse_depth = nullptr, *fuse_normal = nullptr;  // per view w*h depths; three planes of w*h normals
  uint32_t *fuse_pix = nullptr;                          // per view w*h packed pixels, 0 in a view without an image
  uint8_t *fuse_bytes = nullptr;                         // used of all views, then S of all views
  FuseCam *fuse_cams = nullptr;                          // the camera table
  std::vector<FuseCam> fuse_cams_host;                   // ... and the host's copy of it, max_views rows
  double *reg_mem = nullptr;                             // registration scratch (cspm_fuse_register): partials, pose row, records; allocated by the first call
  // TSDF fusion (cspm_tsdf_*): the volume's three planes and the extraction's counts, kept in mem_tsdf
  bool tsdf_on = false, tsdf_coloured = false;           // coloured: a view with an image has been integrated since the last clear
  TsdfVol tsdf{};
  long long tsdf_nvox = 0;
  unsigned int *tsdf_counts = nullptr;                   // crossings per workgroup, then the total
  unsigned int *tsdf_first = nullptr;                    // cspm_tsdf_mesh (section 29), from its first call: a voxel's first vertex number
  unsigned int *tsdf_fcounts = nullptr;                  //   and the triangles per workgroup, then the total
  unsigned int *fuse_counts = nullptr;                   // kept pixels per workgroup of every pass, the total, the kept pixels per view
  // rectification (cspm_set_rectification): kept until the context goes or the rectification is dropped
  bool rect_on = false;
  cspm_rig rect_rig{};
  cspm_rectification rect{};
  double *rect_map[2] = {nullptr, nullptr};     // per view: the planes sx, sy (2 * w*h doubles) ...
  uint8_t *rect_valid[2] = {nullptr, nullptr};  // ... and the valid bytes
  uint8_t *rect_stage = nullptr;                // cspm_set_images_raw: the raw pair's bytes (host sources only), allocated by the first such call
  uint32_t *rect_rawpix = nullptr;              // cspm_set_images_raw(_device): the raw pair as packed words (k_pack_bgr)
  uint8_t *rect_out = nullptr;                  // ... and the rectified 8UC3 pair cspm_set_images_device's path consumes
  double *diffuse_snap = nullptr;     // CSPM_SCHED_DIFFUSE: the round's snapshot (both views, the 6 plane arrays each), allocated by the first such propagation and kept with the field
  long long sweep_fallbacks = 0;      // how often that happened (cspm_get_option)
  // CSPatchMatch over a foreign IPlaneCost (cspm_fpm_*): candidate buffers and what the pending batch was
  FpmCand fpm{nullptr, nullptr, nullptr, nullptr};
  long long fpm_cap = 0;
  int fpm_phase = -1, fpm_iter = 0, fpm_step = 0, fpm_inc = 1;
  long long fpm_count = 0;
  cspm_pm_params fpm_params{};
  // local stereo (cspm_local_stereo): scratch kept between pairs of the same geometry
  long long ca_key[4] = {0, 0, 0, 0};  // W, H, max_dis, levels
  double *ca_gn = nullptr, *ca_t = nullptr, *ca_s = nullptr, *ca_raw = nullptr, *ca_out = nullptr, *ca_best = nullptr;
  int *ca_bestd = nullptr;
  double *ca_vol[CSPM_MAX_LEVELS] = {nullptr};
  unsigned long long *ca_keys = nullptr;
  CaGuideT ca_gt{nullptr, nullptr, nullptr, nullptr};
  int ca_nb = 0;
  // timing
  bool timing = false;
  std::vector<TimingRec> recs;
  std::vector<hipEvent_t> pool;
  double acc_ms[CSPM_K_COUNT] = {0};
  long long acc_launch[CSPM_K_COUNT] = {0}, acc_evals[CSPM_K_COUNT] = {0};
};

namespace {

int fail(cspm_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  else g_create_error = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                            \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return fail(ctx, CSPM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

// run the rest of the enclosing scope on the context's device (DevGuard); ON_DEVICE_ID: before a context exists
#define ON_DEVICE_ID(ctx, dev) \
  DevGuard guard_(dev);        \
  if (!guard_.ok) return fail(ctx, CSPM_ERR_HIP, "hipSetDevice failed")
#define ON_DEVICE(ctx) ON_DEVICE_ID(ctx, (ctx)->device)

// n elements (at least one) from `pool`.  dalloc: into a slot the pool remembers -- nothing happens when it is set already, and the pool
// nulls it when it frees the memory.  dalloc_local: always, into a pointer the pool does not remember (a local, a member of Cost).
inline int alloc_status(cspm_ctx *c, int e) {
  return e ? fail(c, CSPM_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString((hipError_t)e)) : CSPM_OK;
}
template <class T>
int dalloc(cspm_ctx *c, DevPool &pool, T **slot, size_t n) { return alloc_status(c, pool.get(slot, n)); }
template <class T>
int dalloc_local(cspm_ctx *c, DevPool &pool, T **p, size_t n, size_t lead = 0) { return alloc_status(c, pool.add(p, n, lead)); }

// channel-major planes (six slabs of n values, as the device holds a field) into the interleaved records of the ABI, and back
void interleave_planes(const double *planar, size_t n, double *np_out) {
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 6; ++k) np_out[6 * i + k] = planar[k * n + i];
}
void deinterleave_planes(const double *np, size_t n, double *planar_out) {
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 6; ++k) planar_out[k * n + i] = np[6 * i + k];
}

// six slabs of n doubles behind one base: the plane arrays of a field without its costs, to read (SnapField) or to fit into (FitOut)
struct Slabs6 {
  double *p[6];
  SnapField snap() const { return SnapField{p[0], p[1], p[2], p[3], p[4], p[5]}; }
  FitOut fit_out(uint8_t *fitted, int keep_unfitted) const { return FitOut{p[0], p[1], p[2], p[3], p[4], p[5], fitted, keep_unfitted}; }
};
inline Slabs6 six_slabs(double *b, size_t n) { return Slabs6{{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n}}; }

// the candidate buffer cand_mem of cspm_merge_planes_host, cspm_fit_planes and cspm_segment_planes: one view's candidate planes and, behind
// them, its mask bytes (48 + 1 bytes per pixel); allocated by the first call that needs it and kept with the field
struct CandBuf {
  Slabs6 planes;
  uint8_t *mask;
  FitOut fit_out() const { return planes.fit_out(mask, 0); }  // a non-node's planes become NaN, its mask byte 0
  CandField field(int view, bool masked = true) const {       // the one-view candidate field do_merge reads
    CandField cf{};
    cf.s[view] = planes.snap();
    cf.mask[view] = masked ? mask : nullptr;
    return cf;
  }
};
int ensure_cand(cspm_ctx *c, CandBuf *out) {
  const size_t n = (size_t)c->W * c->H;
  const int rc = dalloc(c, c->mem_field, &c->cand_mem, 6 * n + (n + 7) / 8);
  if (!rc) *out = CandBuf{six_slabs(c->cand_mem, n), reinterpret_cast<uint8_t *>(c->cand_mem + 6 * n)};
  return rc;
}

hipEvent_t get_event(cspm_ctx *c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

// bracket a launch with events when timing is on
struct Timed {
  cspm_ctx *c;
  TimingRec r{};
  bool on;
  Timed(cspm_ctx *ctx, int kclass, long long evals) : c(ctx), on(ctx->timing) {
    if (!on) return;
    r.kclass = kclass;
    r.evals = evals;
    r.a = get_event(c);
    r.b = get_event(c);
    (void)hipEventRecord(r.a, c->stream);
  }
  ~Timed() {
    if (!on) return;
    (void)hipEventRecord(r.b, c->stream);
    c->recs.push_back(r);
  }
};

int drain_timing(cspm_ctx *c) {
  if (c->recs.empty()) return CSPM_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto &r : c->recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    c->acc_ms[r.kclass] += ms;
    c->acc_launch[r.kclass] += 1;
    c->acc_evals[r.kclass] += r.evals;
    c->pool.push_back(r.a);
    c->pool.push_back(r.b);
  }
  c->recs.clear();
  return CSPM_OK;
}

// row engine: one wave per 64-pixel run of an image row, kRowWaves waves per workgroup, grid a multiple of 8 (XCD bands)
// a row-kernel launch: claimed column bands when it runs for several rounds of resident waves, interleaved row blocks otherwise
// (cspm_rows.h row_item); workgroups of kRowWaves waves, grid a multiple of 8
inline bool row_claimed(const cspm_ctx *c, int views) {
  const long long items = row_items(c->W, c->H, views);
  if (items >= (1LL << 31)) return false;
  if (c->row_claim >= 0) return c->row_claim != 0;
  return items >= 2LL * c->ncu * 12;  // two rounds of the 12 waves a CU holds (a KITTI-size pair: every row kernel; a 450 x 375 pair: none)
}
inline unsigned row_grid(const cspm_ctx *c, int views) {
  const bool claimed = row_claimed(c, views);
  long long per_xcd = (row_items_per_xcd(c->W, c->H, views, claimed) + kRowWaves - 1) / kRowWaves;
  if (claimed) per_xcd += per_xcd / 4 + 1;  // the surplus workgroups of the XCDs that finish first take over the others' bands
  return (unsigned)(per_xcd * 8);
}
inline int row_cap(const cspm_ctx *c) { return strip_capacity(c->max_dis, c->cost.half); }
inline int row_ocap(const cspm_ctx *c) { return own_capacity(c->cost.half); }
inline size_t row_shmem(const cspm_ctx *c) { return sizeof(LutMem) + (size_t)kRowWaves * wave_lds_bytes(row_cap(c), row_ocap(c)); }

// the claim counters of the next row-kernel launch, zeroed on the stream right before it (launches of a context are serial on its
// stream: one set suffices); none for a launch of interleaved row blocks
inline RowQueue next_row_queue(cspm_ctx *c, int views) {
  if (!row_claimed(c, views)) return RowQueue{nullptr};
  (void)hipMemsetAsync(c->d_rowq, 0, 8 * sizeof(unsigned int), c->stream);
  return RowQueue{c->d_rowq};
}

inline unsigned eval_grid(long long items) {
  long long nb = (items + (kEvalBlock / kWave) - 1) / (kEvalBlock / kWave);
  nb = (nb + 7) / 8 * 8;
  if (nb < 8) nb = 8;
  return (unsigned)nb;
}
inline unsigned ew_grid(long long n, int block = 256) { return (unsigned)((n + block - 1) / block); }
inline unsigned stride_grid(long long n, int block = 256) { return (unsigned)std::min<long long>((n + block - 1) / block, 256 * 16); }

void free_cost(cspm_ctx *c) {
  c->mem_cost.release();
  c->cost_alloc = c->cost_ready = false;
  c->cost_key = CostKey{};
  memset(&c->cost, 0, sizeof c->cost);
}
// the pool's release nulls every pointer it gave out; what else describes the memory is reset here
void free_field(cspm_ctx *c) {
  c->mem_field.release();
  c->d_pp[1] = nullptr;  // lies in d_pp[0]'s allocation
  c->field_alloc = c->seg_ran = c->speckle_ran = false;
  c->smooth_lut_sigma = 0.0;
  c->fpm_cap = 0;
  c->fpm_phase = -1;
}
void free_rect(cspm_ctx *c) {
  c->mem_rect.release();
  c->rect_on = false;
}
void free_ca(cspm_ctx *c) {
  c->mem_ca.release();
  c->ca_nb = 0;
}
void free_images(cspm_ctx *c) {
  c->mem_images.release();
  c->stage_bytes = 0;
  c->W = c->H = 0;
}
// the geometry changes (the caller has synchronised the stream): everything sized by W x H goes
void free_geometry(cspm_ctx *c) {
  free_cost(c);
  free_field(c);
  free_ca(c);
  free_images(c);
}

void small_inverse_row0(int S, const double A[CSPM_MAX_LEVELS][CSPM_MAX_LEVELS], double *w);
// pre_cs_pc.cc:86-109: scale_wgt[s] = inv(tridiag(lambda))(0,s); Mat::inv() = cv::invert(DECOMP_LU): closed form for
// n <= 3, otherwise LU with partial pivoting and reciprocal pivots (OpenCV 2.4 LUImpl), identity right-hand side.
int scale_weights(int S, double lambda, double *w) {
  if (S < 1 || S > CSPM_MAX_LEVELS) return -1;
  double A[CSPM_MAX_LEVELS][CSPM_MAX_LEVELS] = {{0}}, B[CSPM_MAX_LEVELS][CSPM_MAX_LEVELS] = {{0}};
  for (int s = 0; s < S; ++s) {
    B[s][s] = 1.0;
    if (S == 1) { A[0][0] = 1 + lambda; break; }
    if (s == 0) { A[s][s] = 1 + lambda; A[s][s + 1] = -lambda; }
    else if (s == S - 1) { A[s][s] = 1 + lambda; A[s][s - 1] = -lambda; }
    else { A[s][s] = 1 + 2 * lambda; A[s][s - 1] = -lambda; A[s][s + 1] = -lambda; }
  }
  if (S <= 3) {  // cv::invert's closed-form path
    small_inverse_row0(S, A, w);
    return 0;
  }
  const double eps = DBL_EPSILON * 100;
  for (int i = 0; i < S; ++i) {
    int k = i;
    for (int j = i + 1; j < S; ++j)
      if (std::fabs(A[j][i]) > std::fabs(A[k][i])) k = j;
    if (std::fabs(A[k][i]) < eps) return -2;
    if (k != i) {
      for (int j = i; j < S; ++j) std::swap(A[i][j], A[k][j]);
      for (int j = 0; j < S; ++j) std::swap(B[i][j], B[k][j]);
    }
    const double d = -1 / A[i][i];
    for (int j = i + 1; j < S; ++j) {
      const double alpha = A[j][i] * d;
      for (int q = i + 1; q < S; ++q) A[j][q] += alpha * A[i][q];
      for (int q = 0; q < S; ++q) B[j][q] += alpha * B[i][q];
    }
    A[i][i] = -d;
  }
  for (int i = S - 1; i >= 0; --i)
    for (int j = 0; j < S; ++j) {
      double s = B[i][j];
      for (int q = i + 1; q < S; ++q) s -= A[i][q] * B[q][j];
      B[i][j] = s * A[i][i];
    }
  for (int s = 0; s < S; ++s) w[s] = B[0][s];
  return 0;
}

// cv::invert(DECOMP_LU) of OpenCV 2.4 takes a closed-form path for n <= 3 (det2 / det3 and cofactors times 1/det);
// only the first row of the inverse is needed (pre_cs_pc.cc:105-108).  Restated from the OpenCV 2.4 sources
// from memory -- not verifiable in this image.
void small_inverse_row0(int S, const double A[CSPM_MAX_LEVELS][CSPM_MAX_LEVELS], double *w) {
  if (S == 1) {
    w[0] = 1. / A[0][0];
  } else if (S == 2) {
    double d = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    d = 1. / d;
    w[0] = A[1][1] * d;
    w[1] = -A[0][1] * d;
  } else {
    double d = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
               A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    d = 1. / d;
    w[0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) * d;
    w[1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * d;
    w[2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * d;
  }
}

// (re)run the pyramid of both views into the level images (pre_cs_pc.cc:36-55)
void launch_pyramid(cspm_ctx *c) {
  Cost &cd = c->cost;
  for (int s = 0; s < cd.levels; ++s) {
    Level &L = cd.lv[s];
    for (int v = 0; v < 2; ++v) {
      Timed t(c, CSPM_K_MISC, 0);
      uint32_t *img = const_cast<uint32_t *>(L.pix[v]);
      if (s == 0) {
        hipLaunchKernelGGL(k_pad_u32, dim3(ew_grid((long long)L.Wp * L.H)), dim3(256), 0, c->stream, c->img0[v], L.W, L.H, L.Wp, L.pad, img);
      } else {
        const Level &P = cd.lv[s - 1];
        hipLaunchKernelGGL(k_pyrdown, dim3(ew_grid((long long)L.Wp * L.H)), dim3(256), 0, c->stream, P.pix[v], P.W, P.H, P.Wp, P.pad,
                           img, L.W, L.H, L.Wp, L.pad);
      }
    }
  }
}

// allocate the (padded) pyramid images, the per-kind side arrays (gradients / census codes) and, when `with_vol`, the
// cost volumes; fill Cost (everything except gradients / volume contents / max_cost).  An identical request (same
// image size, max_dis, window, levels, kind, volumes) reuses every buffer: no allocator call, no host synchronisation.
int alloc_cost(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda, bool with_vol, CostKind kind, bool want_pairs = false,
               bool want_cvol = false) {
  if (!c->img0[0]) return fail(c, CSPM_ERR_STATE, "cspm_set_images must precede cost construction");
  if (max_dis < 1 || wnd_size < 1 || wnd_size > kMaxWnd || scale_num < 0 || scale_num > CSPM_MAX_LEVELS)
    return fail(c, CSPM_ERR_ARG, "bad max_dis / wnd_size / scale_num");
  // paired-cell volumes for the raster sweep (kSrcVol2): only when every level's indices fit the sweep's 28-bit element offsets
  // and 24-bit slab size and the whole set stays under the context's budget (C3: 2.2 GB; C5 would need 56 GB and keeps the fused sweep)
  bool with_pairs = false;
  long long pairs_bytes = 0, cvol_bytes = 0;
  if (want_pairs) {
    long long bytes = 0;
    bool fits = true;
    int W = c->W, H = c->H, D = max_dis;
    for (int s = 0; s < (scale_num > 0 ? scale_num : 1); ++s) {
      if (s > 0) { H = (H + 1) / 2; W = (W + 1) / 2; D = D / 2; }
      const long long slab = (long long)W * H;
      if (slab >= (1LL << 24) || slab * std::max(D, 1) >= (1LL << 28)) fits = false;
      bytes += 2 * slab * std::max(D, 2) * 16;
    }
    with_pairs = fits && bytes <= c->sweep_pairs_limit;
    pairs_bytes = bytes;
  }
  // device-cell volumes for the row engine's DMA-filled tables: C3 1.2 GB, a 3000 x 2000 D = 256 pair 30 GB (each level's volume
  // must stay below 4 GiB per 16 disparities: the DMA's 32-bit offsets span the slabs of one table)
  bool with_cvol = false;
  const int cvpad_all = wnd_size / 2 + 2;
  if (want_cvol) {
    long long bytes = 0;
    bool fits32 = true;
    int W = c->W, H = c->H, D = max_dis;
    for (int s = 0; s < (scale_num > 0 ? scale_num : 1); ++s) {
      if (s > 0) { H = (H + 1) / 2; W = (W + 1) / 2; D = D / 2; }
      bytes += 2LL * (D + 1) * H * (W + 2 * cvpad_all) * 8;
      if ((long long)H * (W + 2 * cvpad_all) * 8 * std::min(D + 1, 64) >= (1LL << 32)) fits32 = false;  // the usual tables of <= 64 slabs within 32-bit offsets (the device checks every table's real span: cspm_rows.h span32)
    }
    with_cvol = fits32 && bytes <= c->table_volumes_limit;
    cvol_bytes = bytes;
  }
  CostKey key;
  key.W = c->W; key.H = c->H; key.max_dis = max_dis; key.wnd = wnd_size; key.scale_num = scale_num; key.with_vol = with_vol; key.kind = kind;
  key.with_pairs = with_pairs;
  key.with_cvol = with_cvol;
  const bool with_px8 = kind == kKindGrd && !with_vol && c->opt_sweep_packed != 0;
  key.with_px8 = with_px8;
  // the side arrays of a kind, per level and view: gradients (GRD, CENGRD: what the cell kernels read; the tap engines of a fused cost too), GRD's
  // paired elements, 8-bit gray (census input; GrdPC / CSPC's x-gradient input), census codes, and the census elements the tap engines read
  // for fused census cells (CEN always; CENGRD with CSPM_OPT_CENGRD_FUSED: `with_vol` is part of the reuse key).  The colour elements L.px
  // (window weights) every kind has
  const bool need_grd = kind == kKindGrd || kind == kKindCenGrd, need_px16 = kind == kKindGrd;
  const size_t grd_slack = kind == kKindGrd ? 64 : 0;  // a strip's last DMA piece may start inside the last row
  const bool need_gray = kind == kKindImg || kind == kKindCen || kind == kKindCenGrd, need_code = kind == kKindCen || kind == kKindCenGrd;
  const bool need_pc = kind == kKindCen || (kind == kKindCenGrd && !with_vol);
  bool reuse = c->cost_alloc && key == c->cost_key;
  // A cost object that wanted optional volumes and did not get them (free-memory veto, failed hipMalloc) is reused as it is, but not for
  // ever: every volume_retry_pairs-th reuse allocates afresh and asks again, so that one transient shortage -- another context was
  // building its own volumes at that moment -- does not leave this context on the slower path until its geometry changes.
  if (reuse && c->optional_missing && c->volume_retry_pairs > 0 && ++c->optional_reuses >= c->volume_retry_pairs) reuse = false;
  if (!reuse) {
    free_cost(c);
    c->optional_reuses = 0;
    c->optional_missing = false;
  }
  Cost &cd = c->cost;
  c->cost_ready = false;
  c->max_cost_fetched = false;
  c->field_consistent = false;  // stored min_costs belong to the previous cost object: only InitRandomPlane re-establishes them
  c->repeat.taint_unchecked_run();  // its inputs are being replaced
  int rc;
  if (!reuse) {
    cd.cs = scale_num > 0;
    cd.levels = cd.cs ? scale_num : 1;
    cd.half = wnd_size / 2;
    cd.n = 2 * cd.half + 1;
    cd.T = cd.n * cd.n;
    c->max_dis = max_dis;
    c->wnd = wnd_size;
    // pre_cs_pc.cc:36-55
    int W = c->W, H = c->H, D = max_dis;
    for (int s = 0; s < cd.levels; ++s) {
      if (s > 0) { H = (H + 1) / 2; W = (W + 1) / 2; D = D / 2; }
      Level &L = cd.lv[s];
      L.W = W; L.H = H; L.D = D;
      L.pad = D + cd.half + 8;  // cspm_device.h: window overrun and disparity range stay inside the padding
      L.Wp = W + 2 * L.pad;
      if ((long long)L.Wp * H * 12 >= (1LL << 31) || L.Wp * 12 >= (1 << 23))
        return fail(c, CSPM_ERR_ARG, "image too large for the 32-bit / 24-bit element offsets of the tap engine");
      const size_t px = (size_t)W * H, ppx = (size_t)L.Wp * H;
      for (int v = 0; v < 2; ++v) {
        uint32_t *img;
        if ((rc = dalloc_local(c, c->mem_cost, &img, ppx))) return rc;
        PixG *pxg;
        if ((rc = dalloc_local(c, c->mem_cost, &pxg, ppx))) return rc;
        L.px[v] = pxg;
        L.px16[v] = nullptr;
        L.px8[v] = nullptr;
        L.pc[v] = nullptr;
        L.pix[v] = img;
        L.grd[v] = nullptr;
        L.vol[v] = nullptr;
        L.vol2[v] = nullptr;
        L.cvol[v] = nullptr;
        L.cvpad = cvpad_all;
        L.cvW = W + 2 * cvpad_all;
        if (with_vol) {
          double *vol;
          // D+1 slabs and one guard slab behind them (clamped taps of a level with D == 1 form addresses in slabs 0 .. 2).  A level with
          // D == 0 (max_dis < 2^s) clamps to [-1, 1] (cspm_tap.h split_disp: med3(f, 1, D - 1)) and addresses slabs -1 .. 2: one more guard
          // slab on either side, the volume starts behind the first.  No tap of such a level is valid; the guard values are never used.
          const size_t lead = D < 1 ? px : 0;
          if ((rc = dalloc_local(c, c->mem_cost, &vol, (size_t)(D + 2) * px + lead, lead))) return rc;  // vol is `lead` behind what the pool frees
          L.vol[v] = vol;
        }
        if (need_grd) {
          double *g;
          if ((rc = dalloc_local(c, c->mem_cost, &g, ppx + grd_slack))) return rc;
          L.grd[v] = g;
        }
        if (need_px16) {
          uint4 *p16;
          if ((rc = dalloc_local(c, c->mem_cost, &p16, ppx + 64))) return rc;
          L.px16[v] = p16;
        }
        if (with_px8) {
          Pix8 *p8;
          if ((rc = dalloc_local(c, c->mem_cost, &p8, ppx + 64))) return rc;  // + slack: a pair load at the last element reads one element beyond
          L.px8[v] = p8;
        }
        if (need_gray && (rc = dalloc(c, c->mem_cost, &c->cen_gray[v][s], px))) return rc;
        if (need_code && (rc = dalloc(c, c->mem_cost, &c->cen_code[v][s], px * 3))) return rc;
        if (need_pc) {
          PixC *pc;
          if ((rc = dalloc_local(c, c->mem_cost, &pc, ppx))) return rc;
          L.pc[v] = pc;
        }
      }
    }
    // The OPTIONAL volumes come last: device-cell volumes for the DMA-filled tables and paired-cell volumes for the sweep are accelerators,
    // never a reason to fail a pair.  They are taken only from memory that is free NOW (at most `volumes_mem_fraction` of it: the
    // plane field, the sweep granules and the other contexts of the process still have to fit), and a hipMalloc that fails all the
    // same releases what this pass took and the pair runs with computed tables / the fused sweep -- the results are identical.
    if (with_cvol || with_pairs) {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const long long field_b = (long long)c->W * c->H * 2 * (14 + 3 + kGranPerPixel + 2) * 8;  // ensure_field's arrays, if not there yet
        long long avail = (long long)((double)free_b * c->volumes_mem_fraction) - (c->field_alloc ? 0 : field_b);
        if (with_cvol && cvol_bytes > avail) with_cvol = false;
        if (with_cvol) avail -= cvol_bytes;
        if (with_pairs && pairs_bytes > avail) with_pairs = false;
      }
    }
    const DevPool::Mark mandatory = c->mem_cost.mark();
    auto drop_optional = [&]() {  // give back whatever this pass allocated and run without either kind of volume
      c->mem_cost.rewind(mandatory);
      for (int s = 0; s < cd.levels; ++s)
        for (int v = 0; v < 2; ++v) cd.lv[s].cvol[v] = nullptr, cd.lv[s].vol2[v] = nullptr;
      (void)hipGetLastError();  // the out-of-memory error is handled: do not leave it as the runtime's sticky last error
      c->err.clear();
      c->optional_volume_fallbacks++;
    };
    for (int s = 0; s < cd.levels && (with_cvol || with_pairs); ++s) {
      Level &L = cd.lv[s];
      const size_t px = (size_t)L.W * L.H;
      for (int v = 0; v < 2 && (with_cvol || with_pairs); ++v) {
        if (with_cvol) {
          double *cv;
          const size_t ncv = (size_t)(L.D + 1) * L.H * L.cvW + 64;  // + slack: the last DMA piece of the last row may run 8 bytes over
          if ((c->fault_volume_alloc > 0 && --c->fault_volume_alloc == 0) || dalloc_local(c, c->mem_cost, &cv, ncv) != CSPM_OK) { drop_optional(); with_cvol = with_pairs = false; break; }
          HIPCHK(c, hipMemsetAsync(cv, 0, ncv * sizeof(double), c->stream));  // the pad columns stay 0.0; the image columns are rewritten per pair
          L.cvol[v] = cv;
        }
        if (with_pairs) {
          double2 *v2;  // slabs 0 .. D-1; a level with D < 2 is only ever addressed (slab 1), never used
          if ((c->fault_volume_alloc > 0 && --c->fault_volume_alloc == 0) || dalloc_local(c, c->mem_cost, &v2, (size_t)std::max(L.D, 2) * px) != CSPM_OK) { drop_optional(); with_cvol = with_pairs = false; break; }
          L.vol2[v] = v2;
        }
      }
    }
    c->optional_missing = (key.with_cvol && !with_cvol) || (key.with_pairs && !with_pairs);  // wanted, not held: asked for again later
    double lut[2 * kLutSize];
    for (int i = 0; i < kLutSize; ++i) {
      lut[i] = std::exp(-i * 1.0 / 10.0);  // WGT_GAMMA, pre_cs_pc.h:16
      double clrDiff = (double)i;          // sum of three |lC-rC|, an exact integer
      clrDiff *= 0.3333333333;
      clrDiff = clrDiff > 10.0 ? 10.0 : clrDiff;  // TAU_CLR
      lut[kLutSize + i] = 0.1 * clrDiff;   // ALPHA * clrDiff
    }
    if ((rc = dalloc(c, c->mem_cost, &c->d_lut, 2 * kLutSize))) return rc;
    c->d_lut_a = c->d_lut + kLutSize;
    if ((rc = dalloc(c, c->mem_cost, &c->d_maxcost, 2 * CSPM_MAX_LEVELS))) return rc;
    if ((rc = dalloc(c, c->mem_cost, &c->d_early_ok, 1))) return rc;
    if ((rc = dalloc(c, c->mem_cost, &c->d_px8_bad, 1))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_px8_bad, 0, sizeof(unsigned int), c->stream));
    if ((rc = dalloc(c, c->mem_cost, &c->d_maxkeys, 4 * CSPM_MAX_LEVELS))) return rc;
    HIPCHK(c, hipMemcpy(c->d_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    cd.lut = c->d_lut;
    cd.lut_a = c->d_lut_a;
    cd.max_cost = c->d_maxcost;
    cd.early_ok = c->d_early_ok;
    c->cost_key = key;
    c->cost_alloc = true;
  }
  launch_pyramid(c);
  HIPCHK(c, hipMemsetAsync(c->d_px8_bad, 0, sizeof(unsigned int), c->stream));  // per cost object, not per allocation
  // scale weights (pre_cs_pc.cc:86-109): host-side, per call (reg_lambda is not part of the buffer key)
  if (cd.cs) {
    if (scale_weights(cd.levels, reg_lambda, c->scale_wgt)) return fail(c, CSPM_ERR_ARG, "singular regularisation matrix");
  } else {
    c->scale_wgt[0] = 1.0;
  }
  for (int s = 0; s < cd.levels; ++s) cd.lv[s].wgt = c->scale_wgt[s];
  // max keys [0, 2L) start at 0 (= below every key), min keys [2L, 4L) at all-ones
  HIPCHK(c, hipMemsetAsync(c->d_maxkeys, 0, sizeof(unsigned long long) * 2 * CSPM_MAX_LEVELS, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_maxkeys + 2 * CSPM_MAX_LEVELS, 0xFF, sizeof(unsigned long long) * 2 * CSPM_MAX_LEVELS, c->stream));
  cd.fused = kSrcVolume;
  c->sweep_pairs = false;
  c->sweep_packed = false;
  return CSPM_OK;
}

// max_cost of every level/view from the reduced keys and the early-exit licence, all on the device: no host round trip.
// The early-exit proof (cspm_kernels.h level_cost) needs every term of the sum to be >= 0: scale weights (checked here),
// cell costs (GRD and census cells are >= 0 by construction; an uploaded volume is checked through its reduced MIN).
int finish_cost(cspm_ctx *c, bool check_min, double floor_val = -1.0) {
  Cost &cd = c->cost;
  int wgt_ok = 1;
  for (int s = 0; s < cd.levels; ++s)
    if (!(c->scale_wgt[s] >= 0.0)) wgt_ok = 0;
  hipLaunchKernelGGL(k_finish_cost, dim3(1), dim3(64), 0, c->stream, c->d_maxkeys, c->d_maxcost, 2 * CSPM_MAX_LEVELS, cd.levels, floor_val,
                     wgt_ok, check_min ? 1 : 0, c->d_early_ok);
  HIPCHK(c, hipGetLastError());
  c->cost_ready = true;
  return CSPM_OK;
}

int fetch_max_cost(cspm_ctx *c) {
  if (c->max_cost_fetched) return CSPM_OK;
  HIPCHK(c, hipMemcpyAsync(c->host_max_cost, c->d_maxcost, sizeof c->host_max_cost, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->max_cost_fetched = true;
  return CSPM_OK;
}

// The cell kernel of the context's cost kind for slabs d0 .. d0+n-1 of level s, view v: the cells go to `out` (null: none are stored),
// their max is reduced into `max_key` (null: not reduced).  `optional_volumes`: GRD's constructor also fills Level::vol2 / cvol, where held.
void launch_cells(cspm_ctx *c, int s, int v, int d0, int n, double *out, unsigned long long *max_key, bool optional_volumes = false) {
  const Level &L = c->cost.lv[s];
  const dim3 grid(stride_grid((long long)L.W * L.H * n)), block(256);
  const SrcU32 l{L.pix[0], L.Wp, L.pad}, r{L.pix[1], L.Wp, L.pad};
  switch (c->cost_key.kind) {
    case kKindGrd:
      hipLaunchKernelGGL((k_grd_volume<SrcU32, true>), grid, block, 0, c->stream, l, r, L.grd[0], L.grd[1], L.Wp, L.pad, L.W, L.H, d0, n, v, out, max_key,
                         optional_volumes ? (double2 *)L.vol2[v] : nullptr, optional_volumes ? (double *)L.cvol[v] : nullptr,
                         optional_volumes ? L.cvW : 0, optional_volumes ? L.cvpad : 0);
      break;
    case kKindCen:
      hipLaunchKernelGGL(k_cen_volume, grid, block, 0, c->stream, c->cen_code[0][s], c->cen_code[1][s], L.W, L.H, d0, n, v, out, max_key);
      break;
    case kKindCenGrd:
      hipLaunchKernelGGL(k_cengrd_volume<SrcU32>, grid, block, 0, c->stream, l, r, L.grd[0], L.grd[1], L.Wp, L.pad, c->cen_code[0][s], c->cen_code[1][s],
                         L.W, L.H, d0, n, v, out, max_key);
      break;
    default: break;  // uploaded volumes are read where they are; GrdPC / CSPC have no cells
  }
}

// the preparation launches of the constructors, each for level s, view v; g: the gradients to put into the colour elements, or null
void prep_gradient(cspm_ctx *c, const Level &L, int v) {
  hipLaunchKernelGGL(k_gradient<SrcU32>, dim3(ew_grid((long long)L.Wp * L.H)), dim3(256), 0, c->stream, SrcU32{L.pix[v], L.Wp, L.pad}, L.W, L.H, L.Wp,
                     L.pad, const_cast<double *>(L.grd[v]));
}
void prep_census(cspm_ctx *c, int s, int v) {
  const Level &L = c->cost.lv[s];
  const long long px = (long long)L.W * L.H;
  hipLaunchKernelGGL(k_gray8<SrcU32>, dim3(ew_grid(px)), dim3(256), 0, c->stream, SrcU32{L.pix[v], L.Wp, L.pad}, L.W, L.H, c->cen_gray[v][s]);
  hipLaunchKernelGGL(k_census, dim3(ew_grid(px)), dim3(256), 0, c->stream, c->cen_gray[v][s], L.W, L.H, const_cast<uint32_t *>(c->cen_code[v][s]));
}
void prep_aos(cspm_ctx *c, const Level &L, int v, const double *g) {
  const long long ppx = (long long)L.Wp * L.H;
  hipLaunchKernelGGL(k_make_aos, dim3(ew_grid(ppx)), dim3(256), 0, c->stream, L.pix[v], g, ppx, (PixG *)L.px[v]);
}
void prep_aos_cen(cspm_ctx *c, int s, int v) {
  const Level &L = c->cost.lv[s];
  hipLaunchKernelGGL(k_make_aos_cen, dim3(ew_grid((long long)L.Wp * L.H)), dim3(256), 0, c->stream, L.pix[v], c->cen_code[v][s], L.W, L.H, L.Wp, L.pad,
                     (PixC *)L.pc[v]);
}

// The constructors cspm_build_cost_grd / _cen / _cengrd / _img: per level the side arrays of both views, then the cells of both views
// (pre_cs_pc.cc:57-84) -- stored as volumes when `with_vol`, otherwise only their max is reduced (pre_cs_pc.cc:75-82) and the PatchMatch
// kernels compute cells on the fly.
int build_cost(cspm_ctx *c, CostKind kind, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  bool with_vol = false, want_pairs = false, want_cvol = false;
  int fused = kSrcImg;        // the cell source without volumes
  double floor_val = -1.0;    // finish_cost: max_cost when no cells exist
  switch (kind) {
    case kKindGrd:
      with_vol = c->opt_grd_volumes != 0;
      want_pairs = !with_vol && c->opt_sweep_pairs != 0;
      want_cvol = !with_vol && c->opt_table_volumes != 0;
      fused = kSrcGrd;
      break;
    case kKindCen:
      with_vol = c->opt_grd_volumes != 0;
      fused = kSrcCen;
      break;
    case kKindCenGrd:
      with_vol = c->opt_cengrd_fused == 0;
      fused = kSrcCenGrd;
      break;
    default: {  // kKindImg
      const double alpha = 0.1, tau_clr = 10.0, tau_grd = 2.0;
      floor_val = alpha * tau_clr + (1 - alpha) * tau_grd;
    }
  }
  int rc = alloc_cost(c, max_dis, wnd_size, scale_num, reg_lambda, with_vol, kind, want_pairs, want_cvol);
  if (rc == CSPM_ERR_HIP && kind == kKindCenGrd && with_vol)
    return fail(c, rc, "cspm_build_cost_cengrd: device allocation failed (" + c->err + "): the cost needs its f64 volumes on the device, there is no CPU fallback");
  if (rc) return rc;
  Cost &cd = c->cost;
  for (int s = 0; s < cd.levels; ++s) {
    Level &L = cd.lv[s];
    const long long px = (long long)L.W * L.H, ppx = (long long)L.Wp * L.H;
    for (int v = 0; v < 2; ++v) {
      Timed t(c, CSPM_K_GRD, 0);
      switch (kind) {
        case kKindGrd:  // gradients of both views per level (grd_cc.cpp:70-77)
          prep_gradient(c, L, v);
          prep_aos(c, L, v, L.grd[v]);
          // image v is the other view of view 1-v: the left view (0) reads the right image at x-f, x-f-1; the right view the left image at x+f, x+f+1
          hipLaunchKernelGGL(k_make_px16, dim3(ew_grid(ppx)), dim3(256), 0, c->stream, L.pix[v], L.grd[v], L.Wp, L.H, v == 1 ? -1 : 1, (uint4 *)L.px16[v]);
          if (L.px8[v])
            hipLaunchKernelGGL(k_make_px8, dim3(ew_grid(ppx)), dim3(256), 0, c->stream, L.pix[v], L.grd[v], ppx, (Pix8 *)L.px8[v], c->d_px8_bad);
          break;
        case kKindCen:
          prep_census(c, s, v);
          prep_aos_cen(c, s, v);
          prep_aos(c, L, v, nullptr);
          break;
        case kKindCenGrd:
          prep_gradient(c, L, v);
          prep_census(c, s, v);
          prep_aos(c, L, v, nullptr);
          if (!with_vol) prep_aos_cen(c, s, v);
          break;
        default:  // kKindImg: 8U gray and its x-gradient in the colour elements
          hipLaunchKernelGGL(k_gray8_u8, dim3(ew_grid(px)), dim3(256), 0, c->stream, L.pix[v], L.W, L.H, L.Wp, L.pad, c->cen_gray[v][s]);
          hipLaunchKernelGGL(k_make_aos_img, dim3(ew_grid(ppx)), dim3(256), 0, c->stream, L.pix[v], (const uint8_t *)c->cen_gray[v][s], L.W, L.H, L.Wp,
                             L.pad, (PixG *)L.px[v]);
      }
    }
    for (int v = 0; v < 2 && kind != kKindImg; ++v) {  // volumes when asked for (L.vol is null otherwise), their max always
      Timed t(c, CSPM_K_GRD, 0);
      launch_cells(c, s, v, 0, L.D + 1, (double *)L.vol[v], c->d_maxkeys + v * CSPM_MAX_LEVELS + s, true);
    }
  }
  HIPCHK(c, hipGetLastError());
  cd.fused = with_vol ? kSrcVolume : fused;
  c->sweep_pairs = cd.lv[0].vol2[0] != nullptr;                // GRD only: alloc_cost gives no other kind these buffers
  c->sweep_packed = !with_vol && cd.lv[0].px8[0] != nullptr;
  return finish_cost(c, false, floor_val);  // every cell of these kinds is >= 0 (CENGRD: G >= 0 and KAPPA*min(H, TAU_CEN) >= 0)
}

int ensure_field(cspm_ctx *c) {
  if (c->field_alloc) return CSPM_OK;
  const size_t n = (size_t)c->W * c->H;
  int rc;
  if ((rc = dalloc(c, c->mem_field, &c->field_mem, 14 * n))) return rc;
  for (int v = 0; v < 2; ++v) {
    double *base = c->field_mem + (size_t)v * 7 * n;
    c->f[v] = Field{base, base + n, base + 2 * n, base + 3 * n, base + 4 * n, base + 5 * n, base + 6 * n};
  }
  if ((rc = dalloc(c, c->mem_field, &c->vc.cost, n))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->vc.c, n))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->vc.cx, n))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->vc.perm, n))) return rc;
  for (int v = 0; v < 2; ++v) {
    if ((rc = dalloc(c, c->mem_field, &c->d_dis[v], n))) return rc;
    if ((rc = dalloc(c, c->mem_field, &c->d_valid[v], n))) return rc;
  }
  if ((rc = dalloc(c, c->mem_field, &c->d_todo, 2 * n + 2))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->d_rowq, 8))) return rc;
  // persistent sweep state: control words, per-pixel granules (tag zero = never written), diagonal start table
  if ((rc = dalloc(c, c->mem_field, &c->d_sweep_ctrl, 2 + kSweepMaxBands))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_sweep_ctrl, 0, (2 + kSweepMaxBands) * sizeof(unsigned int), c->stream));
  if ((rc = dalloc(c, c->mem_field, &c->d_sweep_gran, 2 * n * kGranPerPixel))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_sweep_gran, 0, sizeof(unsigned long long) * 2 * n * kGranPerPixel, c->stream));
  c->sweep_epoch = 0;
  {
    // per row band b (sweep rows [b*H/nb, (b+1)*H/nb)): start[k] = the band's items (both views) on anti-diagonals < k
    const int nd = c->W + c->H - 1;
    const int nb = std::max(1, std::min(std::min(c->sweep_bands, kSweepMaxBands), c->H));
    std::vector<unsigned int> start((size_t)nb * (nd + 1), 0);
    for (int b = 0; b < nb; ++b) {
      const int y0 = (int)((long long)b * c->H / nb), y1 = (int)((long long)(b + 1) * c->H / nb);
      unsigned int *st = start.data() + (size_t)b * (nd + 1);
      for (int k = 0; k < nd; ++k) {
        const int cnt = std::min(y1 - 1, k) - std::max(y0, k - (c->W - 1)) + 1;
        st[k + 1] = st[k] + 2u * (unsigned)std::max(cnt, 0);
      }
    }
    if ((rc = dalloc(c, c->mem_field, &c->d_sweep_start, start.size()))) return rc;
    HIPCHK(c, hipMemcpy(c->d_sweep_start, start.data(), start.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    c->sweep_bands_built = nb;
  }
  c->field_alloc = true;
  return CSPM_OK;
}

// dataflow sweep (CSPM_OPT_SWEEP_FLOW, off by default): predecessor counters (zeroed before every sweep), the queue of ready pixels
// (epoch-tagged entries: never cleared; at most one entry per pixel plus one reserved slot per waiting workgroup) and its control
// words -- 24 bytes per pixel that the default sweep never touches, so they are allocated by the first sweep that wants them
// (free_field releases them).
int ensure_flow(cspm_ctx *c) {
  if (c->d_sweep_ready && c->d_sweep_queue && c->d_sweep_qctl) return CSPM_OK;
  const size_t n = (size_t)c->W * c->H;
  int rc;
  if ((rc = dalloc(c, c->mem_field, &c->d_sweep_ready, 2 * n))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->d_sweep_queue, 2 * n + 65536))) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_sweep_queue, 0, sizeof(unsigned long long) * (2 * n + 65536), c->stream));
  if ((rc = dalloc(c, c->mem_field, &c->d_sweep_qctl, 4))) return rc;
  return CSPM_OK;
}

// the geometry and the two plane fields: all that the kernels which only read or convert planes look at
Pm field_pm(const cspm_ctx *c) {
  Pm pm{};
  pm.W = c->W; pm.H = c->H;
  pm.f[0] = c->f[0];
  pm.f[1] = c->f[1];
  return pm;
}
Pm make_pm(cspm_ctx *c, const cspm_pm_params *p) {
  Pm pm = field_pm(c);
  pm.max_dis = c->max_dis;
  pm.seed = p->seed;
  pm.rng_row_shared = p->rng_mode == CSPM_RNG_ROW_SHARED;
  pm.trust_cost = c->field_consistent ? 1 : 0;
  pm.use_thresh = p->early_exit ? 1 : 0;  // and-ed with the cost object's device-side licence (Cost::early_ok) in the kernels
  return pm;
}

const cspm_pm_params kDefaultParams = {12345ULL, CSPM_SCHED_RASTER, 1, 4, CSPM_RNG_PER_PIXEL, 1};

// preconditions of the entries that run on the plane field
int need_cost(cspm_ctx *c) {
  return c->cost_ready ? CSPM_OK : fail(c, CSPM_ERR_STATE, "no plane cost built (cspm_build_cost_grd / cspm_finish_cost)");
}
int need_field(cspm_ctx *c, const char *msg) { return c->field_alloc ? CSPM_OK : fail(c, CSPM_ERR_STATE, msg); }
const char *const kNoMergeTarget = "no plane field to merge into (cspm_pm_init, cspm_set_planes, cspm_local_stereo or an earlier run)";

int check_pm(cspm_ctx *c, const cspm_pm_params **p) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = need_cost(c)) return rc;
  if (!*p) *p = &kDefaultParams;
  if ((*p)->schedule != CSPM_SCHED_RASTER && (*p)->schedule != CSPM_SCHED_REDBLACK && (*p)->schedule != CSPM_SCHED_DIFFUSE)
    return fail(c, CSPM_ERR_ARG, "bad schedule");
  if ((*p)->schedule == CSPM_SCHED_DIFFUSE) {
    if ((*p)->rb_neighbours != 4 && (*p)->rb_neighbours != 8 && (*p)->rb_neighbours != 20)
      return fail(c, CSPM_ERR_ARG, "rb_neighbours must be 4, 8 or 20 under CSPM_SCHED_DIFFUSE");
  } else if ((*p)->rb_neighbours != 2 && (*p)->rb_neighbours != 4) return fail(c, CSPM_ERR_ARG, "rb_neighbours must be 2 or 4");
  if ((*p)->rb_rounds < 1) return fail(c, CSPM_ERR_ARG, "rb_rounds must be >= 1");
  return ensure_field(c);
}

// A launch gets 64 KB of dynamic LDS without asking; a wide disparity range (max_dis > ~290: two strip sets of 384 slots per wave)
// needs a little more -- gfx950 has 160 KB per CU -- and a kernel has to opt in once per instantiation.
template <class K>
inline void allow_lds(K kern, size_t shmem) {
  // always the device's whole 160 KB: the attribute belongs to the kernel, not to the launch, and two host threads (two contexts)
  // that set two different sizes for the same instantiation would race between one's attribute call and its launch
  if (shmem > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
#define LAUNCH_ONE(K, grid, block, shmem, ...)                                \
  do {                                                                       \
    allow_lds(K, shmem);                                                     \
    hipLaunchKernelGGL(K, grid, block, shmem, c->stream, __VA_ARGS__);       \
  } while (0)
#define LAUNCH_CS(kern, grid, block, shmem, ...)                                                                  \
  do {                                                                                                            \
    const int src_ = c->cost.fused;                                                                               \
    if (c->cost.cs) {                                                                                             \
      if (src_ == kSrcGrd) LAUNCH_ONE((kern<true, kSrcGrd>), grid, block, shmem, __VA_ARGS__);                    \
      else if (src_ == kSrcCen) LAUNCH_ONE((kern<true, kSrcCen>), grid, block, shmem, __VA_ARGS__);               \
      else if (src_ == kSrcCenGrd) LAUNCH_ONE((kern<true, kSrcCenGrd>), grid, block, shmem, __VA_ARGS__);         \
      else if (src_ == kSrcImg) LAUNCH_ONE((kern<true, kSrcImg>), grid, block, shmem, __VA_ARGS__);               \
      else LAUNCH_ONE((kern<true, kSrcVolume>), grid, block, shmem, __VA_ARGS__);                                 \
    } else {                                                                                                      \
      if (src_ == kSrcGrd) LAUNCH_ONE((kern<false, kSrcGrd>), grid, block, shmem, __VA_ARGS__);                   \
      else if (src_ == kSrcCen) LAUNCH_ONE((kern<false, kSrcCen>), grid, block, shmem, __VA_ARGS__);              \
      else if (src_ == kSrcCenGrd) LAUNCH_ONE((kern<false, kSrcCenGrd>), grid, block, shmem, __VA_ARGS__);        \
      else if (src_ == kSrcImg) LAUNCH_ONE((kern<false, kSrcImg>), grid, block, shmem, __VA_ARGS__);              \
      else LAUNCH_ONE((kern<false, kSrcVolume>), grid, block, shmem, __VA_ARGS__);                                \
    }                                                                                                             \
  } while (0)

// the raster sweep reads the paired-cell volumes when the cost object carries them (GRD, fused): same cells, same order, same bits
#define LAUNCH_SWEEP(kern, grid, block, shmem, ...)                                                              \
  do {                                                                                                            \
    if (c->sweep_pairs && c->cost.fused == kSrcGrd) {                                                             \
      if (c->cost.cs) LAUNCH_ONE((kern<true, kSrcVol2>), grid, block, shmem, __VA_ARGS__);                        \
      else LAUNCH_ONE((kern<false, kSrcVol2>), grid, block, shmem, __VA_ARGS__);                                  \
    } else if (c->sweep_packed && c->cost.fused == kSrcGrd) {                                                     \
      if (c->cost.cs) LAUNCH_ONE((kern<true, kSrcGrd8>), grid, block, shmem, __VA_ARGS__);                        \
      else LAUNCH_ONE((kern<false, kSrcGrd8>), grid, block, shmem, __VA_ARGS__);                                  \
    } else {                                                                                                      \
      LAUNCH_CS(kern, grid, block, shmem, __VA_ARGS__);                                                           \
    }                                                                                                             \
  } while (0)

// one row-engine launch over `views` views, timed as `kclass` with `evals` evaluations: the claim counters, then the kernel with the
// arguments every row kernel takes around its own (`pm` is the caller's)
#define LAUNCH_ROWS(kclass, evals, views, kern, ...)                                                                          \
  do {                                                                                                                        \
    Timed t_(c, kclass, evals);                                                                                               \
    const RowQueue rq_ = next_row_queue(c, views);                                                                            \
    LAUNCH_CS(kern, dim3(row_grid(c, views)), dim3(kRowBlock), row_shmem(c), c->cost, pm, rq_, ##__VA_ARGS__, row_cap(c), row_ocap(c)); \
  } while (0)

int do_init(cspm_ctx *c, const cspm_pm_params *p) {
  Pm pm = make_pm(c, p);
  LAUNCH_ROWS(CSPM_K_INIT, 2LL * c->W * c->H, 2, k_init);
  HIPCHK(c, hipGetLastError());
  c->field_consistent = true;
  return CSPM_OK;
}

// waves of a sweep workgroup: cross-scale -> one per pyramid level; single-scale -> one per chain pass of a full window
inline bool sweep_folded(const cspm_ctx *c) { return c->cost.cs && c->opt_sweep_fold != 0 && c->cost.levels >= 4; }
inline unsigned sweep_waves(const cspm_ctx *c) {
  if (sweep_folded(c)) return (unsigned)(c->cost.levels - 1);  // the last level is folded onto the waves of levels 1 .. (cspm_chain.h eval_pixel_pair)
  return c->cost.cs ? (unsigned)c->cost.levels : (unsigned)((c->cost.n + kChainRows - 1) / kChainRows);
}
inline size_t sweep_lds(const cspm_ctx *c) { return sweep_shared_bytes((int)sweep_waves(c) + (sweep_folded(c) ? 1 : 0)); }

int do_spatial(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  Pm pm = make_pm(c, p);
  const int inc = (iter % 2 == 0) ? 1 : -1;
  if (p->schedule == CSPM_SCHED_REDBLACK) {
    const long long items = 2LL * ((c->W + 1) / 2) * c->H;
    for (int r = 0; r < p->rb_rounds; ++r)
      for (int hs = 0; hs < 2; ++hs) {
        Timed t(c, CSPM_K_SPATIAL, items * p->rb_neighbours);
        LAUNCH_CS(k_spatial_rb, dim3(eval_grid(items)), dim3(kEvalBlock), 0, c->cost, pm, (hs + iter) & 1, inc, p->rb_neighbours);
      }
  } else if (p->schedule == CSPM_SCHED_DIFFUSE) {
    // per round: the twelve plane arrays go into the snapshot (one copy per view: a view's seventh array, min_cost, lies between
    // them and is no part of it), then one row-engine launch reads candidates from the snapshot only and writes the live field only
    static const signed char kOff4[4][2] = {CSPM_DIFFUSE_OFFSETS_4}, kOff8[8][2] = {CSPM_DIFFUSE_OFFSETS_8},
                             kOff20[20][2] = {CSPM_DIFFUSE_OFFSETS_20};
    const size_t n = (size_t)c->W * c->H;
    if (const int e = c->mem_field.get(&c->diffuse_snap, 12 * n))
      return fail(c, CSPM_ERR_HIP, "CSPM_SCHED_DIFFUSE: no memory for the snapshot of the plane fields (" + std::to_string(sizeof(double) * 12 * n) +
                                       " bytes): " + hipGetErrorString((hipError_t)e));
    Diffuse df{};
    df.K = p->rb_neighbours;
    const signed char(*off)[2] = df.K == 4 ? kOff4 : df.K == 8 ? kOff8 : kOff20;
    for (int k = 0; k < df.K; ++k) {
      df.off[k][0] = (signed char)(inc * off[k][0]);
      df.off[k][1] = (signed char)(inc * off[k][1]);
    }
    for (int v = 0; v < 2; ++v) df.s[v] = six_slabs(c->diffuse_snap + (size_t)v * 6 * n, n).snap();
    const long long items = 2LL * c->W * c->H;
    for (int r = 0; r < p->rb_rounds; ++r) {
      Timed t(c, CSPM_K_SPATIAL, items * df.K);  // the snapshot copies are part of the round's time: not LAUNCH_ROWS, which times the launch alone
      for (int v = 0; v < 2; ++v)
        HIPCHK(c, hipMemcpyAsync(c->diffuse_snap + (size_t)v * 6 * n, c->f[v].nx, sizeof(double) * 6 * n, hipMemcpyDeviceToDevice, c->stream));
      const RowQueue rq = next_row_queue(c, 2);
      LAUNCH_CS(k_spatial_diffuse, dim3(row_grid(c, 2)), dim3(kRowBlock), row_shmem(c), c->cost, pm, rq, df, row_cap(c), row_ocap(c));
    }
  } else if (!c->opt_raster_launches) {
    // one persistent launch per sweep: 2 workgroups of 8 waves per CU pull pixels in diagonal-major order
    Sweep sw{};
    sw.ctrl = c->d_sweep_ctrl;
    sw.gran[0] = c->d_sweep_gran;
    sw.gran[1] = c->d_sweep_gran + (size_t)c->W * c->H * kGranPerPixel;
    sw.start = c->d_sweep_start;
    sw.nbands = c->sweep_bands_built;
    sw.epoch = ++c->sweep_epoch;
    sw.total = 2u * (unsigned)c->W * (unsigned)c->H;
    sw.timeout_ticks = c->sweep_timeout_ms * 100000LL;  // the constant clock ticks at 100 MHz
    sw.trace = nullptr;
#ifdef CSPM_SWEEP_TRACE
    {
      static long long *d_trace = nullptr;
      if (!d_trace) { (void)hipMalloc((void **)&d_trace, sizeof(long long) * kTraceSlots * (size_t)sw.total); (void)hipMemset(d_trace, 0, sizeof(long long) * kTraceSlots * (size_t)sw.total); }
      sw.trace = d_trace;
      if (const char *path = getenv("CSPM_SWEEP_TRACE_FILE")) {
        static int sweep_no = 0;
        const int dump_after = getenv("CSPM_SWEEP_TRACE_SWEEP") ? atoi(getenv("CSPM_SWEEP_TRACE_SWEEP")) : 1;  // dump sweep n when sweep n+1 is about to start
        if (sweep_no++ == dump_after) {
          std::vector<long long> h((size_t)kTraceSlots * sw.total);
          (void)hipStreamSynchronize(c->stream);
          (void)hipMemcpy(h.data(), d_trace, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
          if (FILE *fp = fopen(path, "wb")) { fwrite(h.data(), sizeof(long long), h.size(), fp); fclose(fp); }
        }
      }
    }
#endif
    HIPCHK(c, hipMemsetAsync(c->d_sweep_ctrl + 2, 0, kSweepMaxBands * sizeof(unsigned int), c->stream));  // the claim counters; ctrl[1] is sticky
    const bool flow = c->opt_sweep_flow != 0 && (long long)c->W * c->H < (1LL << 30);
    if (flow) {
      int frc = ensure_flow(c);
      if (frc) return frc;
      sw.ready[0] = c->d_sweep_ready;
      sw.ready[1] = c->d_sweep_ready + (size_t)c->W * c->H;
      sw.queue = c->d_sweep_queue;
      sw.qctl = c->d_sweep_qctl;
      HIPCHK(c, hipMemsetAsync(c->d_sweep_ready, 0, sizeof(unsigned int) * 2 * (size_t)c->W * c->H, c->stream));
      HIPCHK(c, hipMemsetAsync(c->d_sweep_qctl, 0, 4 * sizeof(unsigned int), c->stream));
    }
    int ncu = c->ncu;
    // Workgroups per CU when the caller has not chosen (CSPM_OPT_SWEEP_WG = 0): 2 for a KITTI-size sweep -- bound by its dependency chain,
    // 19.3 / 18.5 ms with 2 / 3, while every resident workgroup holds registers other pairs' kernels want -- and 3 (the most five-wave
    // workgroups of 88 VGPRs a CU holds) once the anti-diagonals are wide enough for THROUGHPUT to bind: 1242 x 600 31.1 -> 27.1 ms,
    // 1600 x 1000 72.0 -> 58.5, 3000 x 2000 274.7 -> 214.8 (tools/exp_wg_threshold.py, profiles/r06_c5/).  Not for folded sweeps: their
    // caller shares the GPU, and with pairs in flight 2 per CU measured best.
    const bool wide = 2LL * std::min(c->W, c->H) >= 4LL * c->ncu && !sweep_folded(c);
    const int wg_per_cu = c->sweep_wg_per_cu > 0 ? c->sweep_wg_per_cu : (wide ? 3 : 2);
    // more workgroups than fit is harmless (unclaimed work is all a late workgroup needs); at least one per band, a multiple of
    // the bands so that every band gets the same number
    unsigned grid = (unsigned)std::max<long long>(sw.nbands, std::min<long long>((long long)sw.total, (long long)ncu * wg_per_cu));
    grid = (grid + (unsigned)sw.nbands - 1) / (unsigned)sw.nbands * (unsigned)sw.nbands;
    // CSPM_OPT_SWEEP_GRID (test hook): fewer workgroups, down to one per band and in uneven shares -- workgroup b serves band b mod nbands
    if (c->sweep_grid_cap > 0) grid = std::min(grid, (unsigned)std::max(c->sweep_grid_cap, sw.nbands));
    const unsigned waves = sweep_waves(c);
    {
      Timed t(c, CSPM_K_SPATIAL, (long long)sw.total * 2);
      if (flow) LAUNCH_SWEEP(k_spatial_flow, dim3(grid), dim3(waves * kWave), sweep_lds(c), c->cost, pm, sw, inc);
      else LAUNCH_SWEEP(k_spatial_sweep, dim3(grid), dim3(waves * kWave), sweep_lds(c), c->cost, pm, sw, inc);
    }
    c->repeat.sweep_enqueued();
  } else {
    for (int k = 1; k <= c->W + c->H - 2; ++k) {
      const int ys_lo = std::max(0, k - (c->W - 1)), ys_hi = std::min(c->H - 1, k);
      const long long items = 2LL * (ys_hi - ys_lo + 1);
      Timed t(c, CSPM_K_SPATIAL, items * 2);
      LAUNCH_SWEEP(k_spatial_diag, dim3((unsigned)items), dim3(sweep_waves(c) * kWave), sweep_lds(c), c->cost, pm, k, inc);
    }
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

int do_view(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  Pm pm = make_pm(c, p);
  const long long items = (long long)c->W * c->H;
  const size_t shmem = (size_t)c->W * (sizeof(unsigned long long) + sizeof(unsigned int));
  if (shmem > 160 * 1024) return fail(c, CSPM_ERR_ARG, "image too wide for the view-propagation row resolver");
  ViewCand vc = c->vc;
  const size_t sort_shmem = (size_t)(c->W + 1 + 256) * sizeof(unsigned int);
  if (!c->opt_view_sort || sort_shmem > 160 * 1024) vc.perm = nullptr;
  for (int v = 0; v < 2; ++v) {
    if (vc.perm) {
      Timed t(c, CSPM_K_MISC, 0);
      LAUNCH_ONE(k_view_sort, dim3(c->H), dim3(256), sort_shmem, pm, v, vc);
    }
    LAUNCH_ROWS(CSPM_K_VIEW, items, 1, k_view_eval, v, vc);
    {
      Timed t(c, CSPM_K_MISC, 0);
      LAUNCH_ONE(k_view_resolve, dim3(c->H), dim3(256), shmem, pm, v, iter % 2 == 0 ? 0 : 1, c->vc);
    }
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

int do_refine(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  Pm pm = make_pm(c, p);
  const long long items = 2LL * c->W * c->H;
  const double z_iter = c->max_dis / 2.0, n_iter = 1.0;  // cs_patchmatch.cc:95, cs_patchmatch.h:145
  int steps = 0;
  for (double z = z_iter; z >= 0.1; z /= 2.0) ++steps;   // kZStopThres_, cs_patchmatch.h:146
  // several halving steps per launch: a pixel's steps depend only on its own earlier steps, so the lane keeps its plane in
  // registers between them (c->refine_chunk steps per launch; one launch for all of them by default)
  double z = z_iter, nn = n_iter;
  for (int first = 0; first < steps; first += c->refine_chunk) {
    const int cnt = std::min(c->refine_chunk, steps - first);
    LAUNCH_ROWS(CSPM_K_REFINE, items * cnt, 2, k_refine, iter, first, cnt, z, nn);
    for (int k = 0; k < cnt; ++k) { z /= 2.0; nn /= 2.0; }
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

int run_iterations(cspm_ctx *c, int iter_num, const cspm_pm_params *p) {
  int rc;
  for (int i = 0; i < iter_num; ++i) {                 // :65-102
    if ((rc = do_spatial(c, i, p))) return rc;
    if ((rc = do_view(c, i, p))) return rc;
    if ((rc = do_refine(c, i, p))) return rc;
  }
  return CSPM_OK;
}

int run_patchmatch(cspm_ctx *c, int iter_num, const cspm_pm_params *p) {
  int rc;
  if ((rc = do_init(c, p))) return rc;                 // cs_patchmatch.cc:55
  return run_iterations(c, iter_num, p);
}

// the min_cost of every stored plane under the current cost object (k_rescore); makes the field consistent
int do_rescore(cspm_ctx *c) {
  Pm pm = make_pm(c, &kDefaultParams);  // k_rescore reads the field and the geometry only
  LAUNCH_ROWS(CSPM_K_INIT, 2LL * c->W * c->H, 2, k_rescore);
  HIPCHK(c, hipGetLastError());
  c->field_consistent = true;
  return CSPM_OK;
}

inline int ensure_consistent(cspm_ctx *c) { return c->field_consistent ? CSPM_OK : do_rescore(c); }

// candidate-field merging (k_merge / k_merge_keep) of views view0 .. view0 + views - 1: cf == nullptr is keep-init.
// The field has to be consistent (the callers re-score first) and stays so: an accepted candidate is stored with its own cost.
int do_merge(cspm_ctx *c, const CandField *cf, const cspm_pm_params *p, int view0, int views, long long evals) {
  Pm pm = make_pm(c, p);
  if (cf) LAUNCH_ROWS(CSPM_K_INIT, evals, views, k_merge, *cf, view0, views);
  else LAUNCH_ROWS(CSPM_K_INIT, evals, views, k_merge_keep, CandInit{}, view0, views);
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// both views' 7 arrays, field -> snapshot (save) or back (restore); the snapshot is allocated by the first warm run and kept
int warm_snapshot(cspm_ctx *c, bool save) {
  const size_t bytes = sizeof(double) * 14 * (size_t)c->W * c->H;
  if (int rc = dalloc(c, c->mem_field, &c->warm_snap, 14 * (size_t)c->W * c->H)) return rc;
  HIPCHK(c, hipMemcpyAsync(save ? c->warm_snap : c->field_mem, save ? c->field_mem : c->warm_snap, bytes, hipMemcpyDeviceToDevice, c->stream));
  return CSPM_OK;
}

// a warm run whose persistent sweep timed out: back to its (re-scored) starting field, then the same iterations again
int run_warm_retry(cspm_ctx *c, int iter_num, const cspm_pm_params *p) {
  int rc;
  if ((rc = warm_snapshot(c, false))) return rc;
  c->field_consistent = true;  // the snapshot was taken after the re-score
  return run_iterations(c, iter_num, p);
}

// The speckle filter's four launches (cspm_speckle.h) for `views` views (1 or 2) of w x h, n = w * h < 2^31.  scratch: views * n parents,
// then views * n counts.  size_out (one view only) may be null.
template <class T>
void speckle_launch(hipStream_t stream, const T *const *d, uint8_t *const *valid, int views, int w, int h, int max_size, double thr, int *scratch,
                    unsigned int *removed, int *size_out) {
  const long long n = (long long)w * h;
  SpkViews<T> vs;
  for (int v = 0; v < 2; ++v) {
    const int u = v < views ? v : 0;
    vs.v[v] = SpkView<T>{d[u], valid[u], scratch + u * n, scratch + (views + u) * n};
  }
  const unsigned tiles = (unsigned)(((w + kSpkTileW - 1) / kSpkTileW) * (long long)((h + kSpkTileH - 1) / kSpkTileH));
  const dim3 px_grid((unsigned)((n + 255) / 256), (unsigned)views);
  hipLaunchKernelGGL(k_speckle_tiles<T>, dim3(tiles, (unsigned)views), dim3(kSpkBlock), 0, stream, vs, w, h, thr);
  hipLaunchKernelGGL(k_speckle_borders<T>, px_grid, dim3(256), 0, stream, vs, w, h, thr);
  hipLaunchKernelGGL(k_speckle_sizes, px_grid, dim3(256), 0, stream, vs.v[0].parent, vs.v[1].parent, vs.v[0].cnt, vs.v[1].cnt, n);
  hipLaunchKernelGGL(k_speckle_apply, px_grid, dim3(256), 0, stream, vs.v[0].parent, vs.v[1].parent, vs.v[0].cnt, vs.v[1].cnt, vs.v[0].valid,
                     vs.v[1].valid, n, max_size, removed, size_out);
}

// plane fitting (cspm_fit.h)
const char *fit_params_error(const cspm_fit_params *p) {
  if (p->radius < 1 || p->radius > kFitMaxRadius) return "plane fit: radius must be 1 .. 17";
  if (p->min_support < 3) return "plane fit: min_support must be at least 3";
  if (!(p->max_diff >= 0.0)) return "plane fit: max_diff must be >= 0 (it may be +infinity)";
  return nullptr;
}
const cspm_fit_params kFitDefaults = {5, 1.5, 6, 1};
// lookup_exp_ once more (the cost object owns its own copy): exp(-k/10) by the host's libm
const double *fit_lut() {
  static double lut[kFitLut];
  static const bool filled = [] {
    for (int i = 0; i < kFitLut; ++i) lut[i] = std::exp(-i * 1.0 / 10.0);
    return true;
  }();
  (void)filled;
  return lut;
}
// one view: in.pix == nullptr means no guide
void fit_launch(hipStream_t stream, FitIn in, const FitOut &out, int w, int h, const cspm_fit_params *p, int max_dis) {
  const dim3 grid((unsigned)((w + kFitTileW - 1) / kFitTileW), (unsigned)((h + kFitTileH - 1) / kFitTileH));
  const size_t lds = fit_lds_bytes(p->radius);
  if (p->use_guide && in.pix)
    hipLaunchKernelGGL(k_fit_planes<true>, grid, dim3(kFitBlock), lds, stream, in, out, w, h, p->radius, p->max_diff, p->min_support, (double)max_dis);
  else
    hipLaunchKernelGGL(k_fit_planes<false>, grid, dim3(kFitBlock), lds, stream, in, out, w, h, p->radius, p->max_diff, p->min_support, (double)max_dis);
}
constexpr int kFitMaxRows = 65535 * kFitTileH;  // gridDim.y

// segment planes (cspm_seg.h)
const char *seg_params_error(const cspm_seg_params *p) {
  if (p->step < kSegMinStep || p->step > kSegMaxStep) return "segment planes: step must be 4 .. 64";
  if (p->compactness < 0 || p->compactness > 255) return "segment planes: compactness must be 0 .. 255";
  if (p->iters < 1 || p->iters > 16) return "segment planes: iters must be 1 .. 16";
  if (p->rounds < 0 || p->rounds > 8) return "segment planes: rounds must be 0 .. 8";
  if (p->min_support < 3) return "segment planes: min_support must be at least 3";
  if (!(p->tau >= 0.0)) return "segment planes: tau must be >= 0 (it may be +infinity)";
  return nullptr;
}
const cspm_seg_params kSegDefaults = {16, 20, 5, 1.0, 3, 6};
constexpr int kSegMaxRows = 65535 * kSegTileH;  // gridDim.y of k_seg_assign
inline SegGrid seg_grid(int w, int h, int s) { return SegGrid{w, h, s, (w + s - 1) / s, (h + s - 1) / s}; }
// the device records of a grid of K segments behind one another: centres (5 ints), counts (1 int), inliers (1 int), planes (4 doubles)
struct SegMem {
  int *cen, *counts, *inliers;
  double *planes;
  static size_t bytes(size_t K) { return K * (4 * sizeof(double) + 7 * sizeof(int)); }
  SegMem(void *base, size_t K) {
    planes = static_cast<double *>(base);  // the doubles first: aligned whatever K is
    cen = reinterpret_cast<int *>(planes + 4 * K);
    counts = cen + 5 * K;
    inliers = counts + K;
  }
};
// S on one view: T times ASSIGN then UPDATE
void seg_segment_launch(hipStream_t stream, const SegGrid &g, const uint32_t *pix, const cspm_seg_params *p, int *labels, const SegMem &m) {
  const int K = g.nx * g.ny, per = seg_per_block(g.s);
  const dim3 tiles((unsigned)((g.W + kSegTileW - 1) / kSegTileW), (unsigned)((g.H + kSegTileH - 1) / kSegTileH));
  hipLaunchKernelGGL(k_seg_init, dim3(ew_grid(K)), dim3(256), 0, stream, g, pix, m.cen);
  for (int t = 0; t < p->iters; ++t) {
    hipLaunchKernelGGL(k_seg_assign, tiles, dim3(kSegBlock), 0, stream, g, pix, m.cen, p->compactness, labels);
    hipLaunchKernelGGL(k_seg_update, dim3((unsigned)((K + per - 1) / per)), dim3(kSegBlock), 0, stream, g, pix, labels, m.cen, m.counts, per);
  }
}
// P on one view: the rounds of every segment, then the planes of every pixel
void seg_fit_launch(hipStream_t stream, const SegGrid &g, const SegFitIn &in, const cspm_seg_params *p, int max_dis, const SegMem &m, const FitOut &out) {
  const int K = g.nx * g.ny, per = seg_per_block(g.s);
  hipLaunchKernelGGL(k_seg_fit, dim3((unsigned)((K + per - 1) / per)), dim3(kSegBlock), 0, stream, g, in, p->tau, p->rounds, p->min_support, m.planes,
                     m.inliers, per);
  hipLaunchKernelGGL(k_seg_scatter, dim3(ew_grid((long long)g.W * g.H)), dim3(256), 0, stream, g, in.labels, m.planes, m.inliers, (double)max_dis, out);
}

// PostProcessing's speckle filter on c->d_valid, between LeftRightCheck and FillInvalid; nothing at all when off
template <class T>
int speckle_enqueue(cspm_ctx *c, const T *d0, const T *d1, double thr) {
  c->speckle_ran = c->pp_speckle_size > 0;
  if (!c->speckle_ran) return CSPM_OK;
  const long long n = (long long)c->W * c->H;
  if (n >= (1LL << 31)) return fail(c, CSPM_ERR_ARG, "image too large for the speckle filter's 32-bit labels");
  if (int rc = dalloc(c, c->mem_field, &c->d_speckle, 4 * (size_t)n + 1)) return rc;
  unsigned int *removed = (unsigned int *)(c->d_speckle + 4 * n);
  HIPCHK(c, hipMemsetAsync(removed, 0, sizeof(unsigned int), c->stream));
  const T *d[2] = {d0, d1};
  speckle_launch<T>(c->stream, d, c->d_valid, 2, c->W, c->H, c->pp_speckle_size, thr, c->d_speckle, removed, nullptr);
  return CSPM_OK;
}

// the reference's steps of postprocess_enqueue, timed as one CSPM_K_POST bracket
int postprocess_steps(cspm_ctx *c, int dis_scale) {
  const Pm pm = field_pm(c);
  const long long n = (long long)c->W * c->H;
  const Level &L0 = c->cost.lv[0];
  Timed t(c, CSPM_K_POST, 0);
  for (int v = 0; v < 2; ++v)  // PlaneToDisp (cs_patchmatch.cc:103)
    hipLaunchKernelGGL(k_plane_to_disp_u8, dim3(ew_grid(n)), dim3(256), 0, c->stream, pm, v, dis_scale, c->d_dis[v], (size_t)c->W);
  unsigned int *todo_cnt = c->d_todo + 2 * (size_t)n;
  HIPCHK(c, hipMemsetAsync(todo_cnt, 0, 2 * sizeof(unsigned int), c->stream));
  // LeftRightCheck of both views (:516) on the maps as PlaneToDisp left them
  hipLaunchKernelGGL(k_lr_check, dim3(ew_grid(2 * n)), dim3(256), 0, c->stream, c->d_dis[0], c->d_dis[1], c->W, c->H, dis_scale, c->d_valid[0],
                     c->d_valid[1]);
  if (int rc = speckle_enqueue<uint8_t>(c, c->d_dis[0], c->d_dis[1], c->pp_speckle_diff * (double)dis_scale)) return rc;
  // FillInvalid (:545): a workgroup per row and view
  if (fill_rows_shmem(c->W) > 160 * 1024) return fail(c, CSPM_ERR_ARG, "image too wide for the row scan of FillInvalid");
  LAUNCH_ONE(k_fill_rows<FillU8>, dim3(2u * (unsigned)c->H), dim3(kFillBlock), fill_rows_shmem(c->W), pm, (FillU8{dis_scale, c->d_dis[0], c->d_dis[1]}),
             c->d_valid[0], c->d_valid[1], c->d_todo, todo_cnt);
  // WeightedMedian(valid, 35, WMF_GAMMA) (:571-573): a wavefront per listed pixel; exp(-i/10) is the plane-cost LUT
  hipLaunchKernelGGL(k_weighted_median, dim3((unsigned)c->ncu * 8u), dim3(kMedianBlock), 0, c->stream, L0.pix[0], L0.pix[1], L0.Wp, L0.pad, c->W,
                     c->H, c->d_valid[0], c->d_valid[1], c->d_lut, c->d_dis[0], c->d_dis[1], c->d_todo, todo_cnt, 35 / 2);
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// The median filter's one launch (cspm_median.h) for `views` views (1 or 2) of w x h, 1 <= r <= CSPM_MEDIAN_MAX_RADIUS: radii 1 .. 3 have
// kernels of their own, the rest share the one that takes the radius as an argument.
inline unsigned median_tiles(int w, int h) { return (unsigned)(((w + kMedTileW - 1) / kMedTileW) * (long long)((h + kMedTileH - 1) / kMedTileH)); }
void median_launch_u8(hipStream_t stream, const uint8_t *const *src, uint8_t *const *dst, int views, size_t sstride, size_t dstride, int w, int h, int cn,
                      int r) {
  const dim3 grid(median_tiles(w, h), (unsigned)cn, (unsigned)views), block(kMedBlock);
  const int u = views - 1;
#define CSPM_MEDIAN_U8(RT) hipLaunchKernelGGL(k_median_u8<RT>, grid, block, 0, stream, src[0], src[u], dst[0], dst[u], sstride, dstride, w, h, cn, r)
  if (r == 1) CSPM_MEDIAN_U8(1);
  else if (r == 2) CSPM_MEDIAN_U8(2);
  else if (r == 3) CSPM_MEDIAN_U8(3);
  else CSPM_MEDIAN_U8(0);
#undef CSPM_MEDIAN_U8
}
void median_launch_f64(hipStream_t stream, const double *const *src, double *const *dst, int views, int w, int h, int r) {
  const dim3 grid(median_tiles(w, h), (unsigned)views), block(kMedBlock);
  const int u = views - 1;
  typedef unsigned long long Bits;
#define CSPM_MEDIAN_F64(RT) \
  hipLaunchKernelGGL(k_median_f64<RT>, grid, block, 0, stream, (const Bits *)src[0], (const Bits *)src[u], (Bits *)dst[0], (Bits *)dst[u], w, h, r)
  if (r == 1) CSPM_MEDIAN_F64(1);
  else if (r == 2) CSPM_MEDIAN_F64(2);
  else if (r == 3) CSPM_MEDIAN_F64(3);
  else CSPM_MEDIAN_F64(0);
#undef CSPM_MEDIAN_F64
}

// PostProcessing's last step: M8 of c->d_dis into the second buffers, which then are the maps; nothing at all when off
int median_u8_enqueue(cspm_ctx *c) {
  if (c->pp_median == 0) return CSPM_OK;
  for (int v = 0; v < 2; ++v)
    if (int rc = dalloc(c, c->mem_field, &c->d_med8[v], (size_t)c->W * c->H)) return rc;
  Timed t(c, CSPM_K_POST, 0);
  median_launch_u8(c->stream, c->d_dis, c->d_med8, 2, (size_t)c->W, (size_t)c->W, c->W, c->H, 1, c->pp_median);
  HIPCHK(c, hipGetLastError());
  for (int v = 0; v < 2; ++v) std::swap(c->d_dis[v], c->d_med8[v]);
  return CSPM_OK;
}
// the same on the sub-pixel maps: M64 of c->d_pp into the second pair
int median_f64_enqueue(cspm_ctx *c) {
  if (c->pp_median == 0) return CSPM_OK;
  const size_t n = (size_t)c->W * c->H;
  if (int rc = dalloc(c, c->mem_field, &c->d_med64, 2 * n)) return rc;
  double *dst[2] = {c->d_med64, c->d_med64 + n};
  Timed t(c, CSPM_K_POST, 0);
  median_launch_f64(c->stream, c->d_pp, dst, 2, c->W, c->H, c->pp_median);
  HIPCHK(c, hipGetLastError());
  std::swap(c->d_pp[0], c->d_med64);
  c->d_pp[1] = c->d_pp[0] + n;
  return CSPM_OK;
}

// Edge-aware global smoothing (cspm_smooth.h).  Defaults chosen, not tuned.
const cspm_smooth_params kSmoothDefaults = {100.0, 20.0, 3, 0.25};
const char *smooth_params_error(const cspm_smooth_params *p, bool with_fill_conf) {
  if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "smoothing: lambda must be finite and >= 0";
  if (!(p->sigma_color > 0.0) || !std::isfinite(p->sigma_color)) return "smoothing: sigma_color must be finite and > 0";
  if (p->iterations < 1 || p->iterations > kSmMaxIters) return "smoothing: iterations 1 .. 8";
  if (with_fill_conf && !(p->fill_conf >= 0.0 && p->fill_conf <= 1.0)) return "smoothing: fill_conf must lie in [0, 1]";
  return nullptr;
}
// LUT[k] = exp(-k / sigma) by the host's libm, like the fit's table
void smooth_lut_fill(double sigma, double *lut) {
  for (int k = 0; k < kSmLut; ++k) lut[k] = std::exp(-(double)k / sigma);
}
// S on `views` views (1 or 2) of w x h in place on d: init, T rounds of a horizontal and a vertical pass, finish.  lut == nullptr: no guide.
void smooth_launch(hipStream_t stream, double *const *d, const SmoothConf &cf, const SmoothPair &s, int views, int w, int h, const cspm_smooth_params *p,
                   double max_dis, const double *lut) {
  const long long n = (long long)w * h;
  const int u = views - 1, T = p->iterations;
  hipLaunchKernelGGL(k_smooth_init, dim3(ew_grid(n * views)), dim3(256), 0, stream, d[0], d[u], cf, s, n, views);
  double pow_T = 1.0;  // 4^T, exact
  for (int i = 0; i < T; ++i) pow_T *= 4.0;
  const dim3 rows((unsigned)((h + kSmRows - 1) / kSmRows), (unsigned)views), cols((unsigned)((w + kWave - 1) / kWave), (unsigned)views);
  for (int t = 1; t <= T; ++t) {
    double pow_t = 1.0;  // 4^(T - t)
    for (int i = 0; i < T - t; ++i) pow_t *= 4.0;
    const double lam = ((1.5 * pow_t) / (pow_T - 1.0)) * p->lambda;
    if (lut) {
      hipLaunchKernelGGL(k_smooth_rows<true>, rows, dim3(kWave), 0, stream, s, w, h, lam, lut);
      hipLaunchKernelGGL(k_smooth_cols<true>, cols, dim3(kWave), 0, stream, s, w, h, lam, lut);
    } else {
      hipLaunchKernelGGL(k_smooth_rows<false>, rows, dim3(kWave), 0, stream, s, w, h, lam, lut);
      hipLaunchKernelGGL(k_smooth_cols<false>, cols, dim3(kWave), 0, stream, s, w, h, lam, lut);
    }
  }
  hipLaunchKernelGGL(k_smooth_finish, dim3(ew_grid(n * views)), dim3(256), 0, stream, d[0], d[u], s, n, views, max_dis);
}

// the last step of the sub-pixel PostProcessing: S in place on c->d_pp, C from the final consistency masks; nothing at all when off
int smooth_f64_enqueue(cspm_ctx *c) {
  const cspm_smooth_params &p = c->pp_smooth;
  if (p.lambda == 0.0) return CSPM_OK;
  const size_t n = (size_t)c->W * c->H;
  if (int rc = dalloc(c, c->mem_field, &c->d_smooth, 6 * n + kSmLut)) return rc;  // a new one has no table: free_field zeroes smooth_lut_sigma
  double *d_lut = c->d_smooth + 6 * n;
  if (c->smooth_lut_sigma != p.sigma_color) {  // a new table: the stream is drained so that no earlier launch still reads the old one
    c->smooth_lut.resize(kSmLut);
    smooth_lut_fill(p.sigma_color, c->smooth_lut.data());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(d_lut, c->smooth_lut.data(), sizeof(double) * kSmLut, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->smooth_lut_sigma = p.sigma_color;
  }
  const Level &L0 = c->cost.lv[0];
  SmoothPair s;
  SmoothConf cf;
  for (int v = 0; v < 2; ++v) {
    s.v[v] = SmoothView{c->d_smooth + v * n, c->d_smooth + (2 + v) * n, c->d_smooth + (4 + v) * n, L0.pix[v]};
    cf.conf[v] = nullptr;
    cf.ok[v] = c->d_valid[v];
  }
  s.Wp = L0.Wp;
  s.pad = L0.pad;
  cf.fill_conf = p.fill_conf;
  Timed t(c, CSPM_K_POST, 0);
  smooth_launch(c->stream, c->d_pp, cf, s, 2, c->W, c->H, &p, (double)c->max_dis, d_lut);
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// PlaneToDisp + PostProcessing (cs_patchmatch.cc:103-107, 508-588) enqueued on the ctx stream; results in c->d_dis[v]
int postprocess_enqueue(cspm_ctx *c, int dis_scale) {
  if (int rc = postprocess_steps(c, dis_scale)) return rc;
  return median_u8_enqueue(c);
}

// PlaneToDisp of one view into a device buffer (u8, packed W*H), enqueued on the ctx stream
int enqueue_disp_u8(cspm_ctx *c, int view, int dis_scale, void *d_out) {
  const Pm pm = field_pm(c);
  {
    Timed t(c, CSPM_K_MISC, 0);
    hipLaunchKernelGGL(k_plane_to_disp_u8, dim3(ew_grid((long long)c->W * c->H)), dim3(256), 0, c->stream, pm, view, dis_scale,
                       (uint8_t *)d_out, (size_t)c->W);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// sub-pixel PostProcessing (cspm_pp.h) enqueued on the ctx stream; maps in c->d_pp[v], flags in c->d_valid[v].
// The 8-bit path's maps (c->d_dis) are not touched; the flags and the work list are scratch of whichever path runs.
int postprocess_f64_steps(cspm_ctx *c) {
  const long long n = (long long)c->W * c->H;
  if (int rc = dalloc(c, c->mem_field, &c->d_pp[0], 2 * (size_t)n)) return rc;
  c->d_pp[1] = c->d_pp[0] + n;
  if (fill_rows_shmem(c->W) > 160 * 1024) return fail(c, CSPM_ERR_ARG, "image too wide for the row scan of FillInvalid");
  const Pm pm = field_pm(c);
  const Level &L0 = c->cost.lv[0];
  Timed t(c, CSPM_K_POST, 0);
  for (int v = 0; v < 2; ++v)
    hipLaunchKernelGGL(k_plane_to_disp_f64, dim3(ew_grid(n)), dim3(256), 0, c->stream, pm, v, c->d_pp[v]);
  unsigned int *todo_cnt = c->d_todo + 2 * (size_t)n;
  HIPCHK(c, hipMemsetAsync(todo_cnt, 0, 2 * sizeof(unsigned int), c->stream));
  hipLaunchKernelGGL(k_lr_check_f64, dim3(ew_grid(2 * n)), dim3(256), 0, c->stream, c->d_pp[0], c->d_pp[1], c->W, c->H, c->d_valid[0], c->d_valid[1]);
  if (int rc = speckle_enqueue<double>(c, c->d_pp[0], c->d_pp[1], c->pp_speckle_diff)) return rc;
  LAUNCH_ONE(k_fill_rows<FillF64>, dim3(2u * (unsigned)c->H), dim3(kFillBlock), fill_rows_shmem(c->W), pm,
             (FillF64{(double)c->max_dis, c->d_pp[0], c->d_pp[1]}), c->d_valid[0], c->d_valid[1], c->d_todo, todo_cnt);
  hipLaunchKernelGGL(k_weighted_median_f64, dim3((unsigned)c->ncu * (unsigned)kPpGrid), dim3(kWave), 0, c->stream, L0.pix[0], L0.pix[1], L0.Wp, L0.pad,
                     c->W, c->H, c->d_valid[0], c->d_valid[1], c->d_lut, c->d_pp[0], c->d_pp[1], c->d_todo, todo_cnt);
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
int postprocess_f64_enqueue(cspm_ctx *c) {
  if (int rc = postprocess_f64_steps(c)) return rc;
  if (int rc = median_f64_enqueue(c)) return rc;
  return smooth_f64_enqueue(c);
}

// An asynchronous output, enqueued on the ctx stream: the map of one view, or both post-processed maps copied to the caller's buffers.
// request_output: when the run in front of it has an unchecked sweep the request is remembered -- a repeated run (sweep timeout) writes
// the map again from ITS planes, so the caller never reads a map of the aborted run after a successful check.
int enqueue_output(cspm_ctx *c, const OutReq &q) {
  if (q.kind == kOutDisp) return enqueue_disp_u8(c, q.view, q.dis_scale, q.o0);
  const bool f64 = q.kind == kOutPostF64;
  if (int rc = f64 ? postprocess_f64_enqueue(c) : postprocess_enqueue(c, q.dis_scale)) return rc;
  void *outs[2] = {q.o0, q.o1};
  const size_t bytes = (f64 ? sizeof(double) : 1) * (size_t)c->W * c->H;
  for (int v = 0; v < 2; ++v)
    HIPCHK(c, hipMemcpyAsync(outs[v], f64 ? (const void *)c->d_pp[v] : (const void *)c->d_dis[v], bytes, hipMemcpyDeviceToDevice, c->stream));
  return CSPM_OK;
}
int request_output(cspm_ctx *c, const OutReq &q) {
  if (c->repeat.pending()) c->repeat.remember_output(q);
  return enqueue_output(c, q);
}

// The run whose persistent sweep timed out, again with per-diagonal launches -- they need no inter-workgroup hand-off and give the same
// planes bit for bit -- and then the maps that were enqueued behind it: those were computed from the aborted run's planes.
int replay(cspm_ctx *c, const Repeat::Record &rec) {
  const long long keep = c->opt_raster_launches;
  c->opt_raster_launches = 1;
  int rc = rec.warm ? run_warm_retry(c, rec.iters, &rec.params) : run_patchmatch(c, rec.iters, &rec.params);
  c->opt_raster_launches = keep;
  for (size_t i = 0; rc == CSPM_OK && i < rec.outs.size(); ++i) rc = enqueue_output(c, rec.outs[i]);
  if (rc != CSPM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ++c->sweep_fallbacks;
  return CSPM_OK;
}

// A persistent sweep's bounded spins raise the STICKY error word ctrl[1] instead of hanging (later sweeps then drain at
// once).  It is looked at by every call that synchronises with the host anyway (cspm_synchronize, the getters, the
// single-phase entry cspm_pm_spatial): cspm_patchmatch itself stays asynchronous.  What a timeout leads to is Repeat's rule.
int check_sweep(cspm_ctx *c) {
  if (!c->repeat.pending()) return CSPM_OK;
  unsigned int ctrl[2] = {0, 0}, px8_bad = 0;
  HIPCHK(c, hipMemcpyAsync(ctrl, c->d_sweep_ctrl, sizeof ctrl, hipMemcpyDeviceToHost, c->stream));
  if (c->sweep_packed && c->cost_alloc && c->d_px8_bad)
    HIPCHK(c, hipMemcpyAsync(&px8_bad, c->d_px8_bad, sizeof px8_bad, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const Repeat::Record rec = c->repeat.take();
  // CSPM_OPT_SWEEP_PACKED: a gradient the 36-bit fixed-point field cannot hold was packed as 0 and the sweep read a wrong cell.  Cannot
  // happen for 8-bit images (cspm.h); if it ever does, the planes are wrong and the caller must hear about it, not only a counter.
  if (px8_bad)
    return fail(c, CSPM_ERR_HIP, "CSPM_OPT_SWEEP_PACKED: " + std::to_string(px8_bad) + " gradients could not be packed exactly; the raster sweep's planes are not valid");
  if (!ctrl[1]) return CSPM_OK;
  (void)hipMemsetAsync(c->d_sweep_ctrl, 0, 2 * sizeof(unsigned int), c->stream);
  if (rec.runs == 1 && !rec.tainted && c->cost_ready) return replay(c, rec);
  return fail(c, CSPM_ERR_HIP, "raster sweep timed out waiting for a predecessor pixel (inter-workgroup hand-off)");
}

// Work of `dst` that reads the planes of `src`, another context on the same device.
// source_check: a timed-out source run is repeated (or reported) before its planes are read.
int source_check(cspm_ctx *dst, cspm_ctx *src) {
  const int rc = check_sweep(src);
  return rc ? fail(dst, rc, "source context: " + src->err) : CSPM_OK;
}
// with_source: dst's stream waits for the source's work, `body` enqueues on dst's stream, and the source's later work (or its
// destruction) waits for that.  A HIP error is reported under `entry`; otherwise what body returned.
template <class Body>
int with_source(cspm_ctx *dst, cspm_ctx *src, const char *entry, Body body) {
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (auto &e : ev) HIPCHK(dst, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int rc = CSPM_OK;
  hipError_t e = hipEventRecord(ev[0], src->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev[0], 0);
  if (e == hipSuccess) {
    rc = body();
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], dst->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(src->stream, ev[1], 0);
  for (auto x : ev) (void)hipEventDestroy(x);
  if (e != hipSuccess) return fail(dst, CSPM_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
  return rc;
}

// ---- reprojection (cspm_geom.h) ---------------------------------------------------------------------------
const cspm_geom_params kGeomDefaults = {0.0, HUGE_VAL, 0.0, 0, 0};
const char *geom_args_error(const cspm_calib *k, const cspm_geom_params *g, int view) {
  if (!k) return "reprojection: no calibration";
  if (!std::isfinite(k->f) || !std::isfinite(k->cx) || !std::isfinite(k->cy) || !std::isfinite(k->baseline) || !std::isfinite(k->doffs))
    return "reprojection: the calibration must be finite";
  if (!(k->f > 0.0) || !(k->baseline > 0.0)) return "reprojection: f and baseline must be positive";
  if (!(g->z_near >= 0.0)) return "reprojection: z_near must be >= 0";
  if (!(g->z_far >= g->z_near)) return "reprojection: z_far must be >= z_near (it may be +infinity)";
  if (!(g->min_cos >= 0.0 && g->min_cos <= 1.0)) return "reprojection: min_cos must be in [0, 1]";
  if (view < 0 || view > 1) return "reprojection: view must be 0 or 1";
  return nullptr;
}
GeomCam geom_cam(const cspm_calib *k, const cspm_geom_params *g, int view) {
  GeomCam m{};
  m.f = k->f; m.cy = k->cy; m.baseline = k->baseline; m.doffs = k->doffs;
  m.cxv = k->cx + (double)view * k->doffs;
  m.fB = k->f * k->baseline;
  m.z_near = g->z_near; m.z_far = g->z_far; m.min_cos = g->min_cos;
  m.add_baseline = (g->left_frame && view == 1) ? 1 : 0;
  return m;
}
inline unsigned geom_blocks(long long n) { return (unsigned)((n + kGeomBlock - 1) / kGeomBlock); }
// the passes of G on one view: dense planes and keep; then, when a cloud or a count is wanted, the scan and the records.
// counts: geom_blocks(n) + 1 unsigned ints (the last one receives the total unless d_total names another place)
void geom_launch(hipStream_t stream, const GeomCam &cam, const GeomIn &in, const GeomOut &out, int w, int h, uint4 *cloud, size_t cap, bool want_count,
                 unsigned int *counts, unsigned int *d_total) {
  const long long n = (long long)w * h;
  const unsigned nb = geom_blocks(n);
  const bool slopes = in.a != nullptr;
  const bool compact = cloud != nullptr || want_count;
  unsigned int *cnt = compact ? counts : nullptr;
  if (slopes) hipLaunchKernelGGL(k_geom_dense<true>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, out, w, n, cnt);
  else hipLaunchKernelGGL(k_geom_dense<false>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, out, w, n, cnt);
  if (!compact) return;
  hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, stream, counts, (int)nb, d_total ? d_total : counts + nb);
  const unsigned int cap32 = (unsigned int)std::min<size_t>(cap, (size_t)n);
  if (!cloud || cap32 == 0) return;
  if (slopes) hipLaunchKernelGGL(k_geom_cloud<true>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, w, n, (const unsigned int *)counts, cloud, cap32);
  else hipLaunchKernelGGL(k_geom_cloud<false>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, w, n, (const unsigned int *)counts, cloud, cap32);
}

// the inputs of G on the stored field, shared by the reprojection and the mesh: geom_inputs_alloc before the timing bracket (scratch
// and, for CSPM_GEOM_PP, the post-processing with its own brackets), geom_inputs_launch inside it.
int geom_inputs_alloc(cspm_ctx *c, int source, const cspm_fit_params *fit) {
  int rc = CSPM_OK;
  const size_t n = (size_t)c->W * c->H;
  if (source == CSPM_GEOM_RAW && (rc = dalloc(c, c->mem_field, &c->geom_disp, n))) return rc;
  if (fit && !c->geom_fit) {
    if ((rc = dalloc(c, c->mem_field, &c->geom_fit, 6 * n + kFitLut))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->geom_fit + 6 * n, fit_lut(), sizeof(double) * kFitLut, hipMemcpyHostToDevice, c->stream));
  }
  if (source == CSPM_GEOM_PP && (rc = postprocess_f64_enqueue(c))) return rc;
  return CSPM_OK;
}
GeomIn geom_inputs_launch(cspm_ctx *c, int view, int source, const cspm_geom_params *g, const cspm_fit_params *fit) {
  const size_t n = (size_t)c->W * c->H;
  const Field &f = c->f[view];
  GeomIn in{};
  in.pix = c->img0[view];
  if (source == CSPM_GEOM_RAW) {
    hipLaunchKernelGGL(k_plane_to_disp_f64, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, field_pm(c), view, c->geom_disp);
    in.disp = c->geom_disp;
    in.a = f.a; in.b = f.b;
  } else {
    in.disp = c->d_pp[view];
    in.valid = g->consistent_only ? c->d_valid[view] : nullptr;
    in.a = f.a; in.b = f.b;
    in.slope_mask = c->d_valid[view];
  }
  if (fit) {
    double *b = c->geom_fit;
    fit_launch(c->stream, FitIn{in.disp, in.valid, c->img0[view], c->geom_fit + 6 * n}, six_slabs(b, n).fit_out(nullptr, 0), c->W, c->H, fit, c->max_dis);
    in.a = b + 3 * n; in.b = b + 4 * n;
    in.slope_mask = nullptr;
  }
  return in;
}

// cspm_reproject / cspm_reproject_device after their argument checks: the pending-run check, the inputs of the chosen source, the
// passes.  Every output is a device pointer; d_total == nullptr: the total goes behind the context's counts.
int reproject_enqueue(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, const GeomOut &out,
                      uint4 *cloud, size_t cap, bool want_count, unsigned int *d_total) {
  int rc = check_sweep(c);  // BEFORE the field is read: a run repeated after a sweep timeout must be the one the geometry comes from
  if (rc) return rc;
  const size_t n = (size_t)c->W * c->H;
  const unsigned nb = geom_blocks((long long)n);
  if ((rc = dalloc(c, c->mem_field, &c->geom_counts, (size_t)nb + 1))) return rc;
  if ((rc = geom_inputs_alloc(c, source, fit))) return rc;
  {
    Timed t(c, CSPM_K_MISC, (long long)n);
    const GeomIn in = geom_inputs_launch(c, view, source, g, fit);
    geom_launch(c->stream, geom_cam(calib, g, view), in, out, c->W, c->H, cloud, cap, want_count, c->geom_counts, d_total);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
// the checks cspm_reproject and cspm_reproject_device share; g and fit are defaulted / validated
int reproject_check(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params **g, const cspm_fit_params *fit) {
  if (!*g) *g = &kGeomDefaults;
  if (const char *msg = geom_args_error(calib, *g, view)) return fail(c, CSPM_ERR_ARG, msg);
  if (source != CSPM_GEOM_RAW && source != CSPM_GEOM_PP) return fail(c, CSPM_ERR_ARG, "reprojection: source must be CSPM_GEOM_RAW or CSPM_GEOM_PP");
  if (fit)
    if (const char *msg = fit_params_error(fit)) return fail(c, CSPM_ERR_ARG, msg);
  if (!c->img0[0]) return fail(c, CSPM_ERR_STATE, "cspm_set_images first");
  if (int rc = need_field(c, "no plane field to reproject (cspm_patchmatch, cspm_local_stereo, cspm_set_planes, ...)")) return rc;
  if ((source == CSPM_GEOM_PP || fit) && (!c->cost_alloc || !c->cost_ready || c->max_dis < 1))
    return fail(c, CSPM_ERR_STATE, "reprojection of the post-processed map or with a plane fit needs a cost object (its max_dis)");
  if ((long long)c->W * c->H >= (1LL << 31)) return fail(c, CSPM_ERR_ARG, "w * h must be below 2^31: cloud records hold 32-bit pixel indices");
  if (fit && c->H > kFitMaxRows) return fail(c, CSPM_ERR_ARG, "image too high for the plane fit");
  return CSPM_OK;
}

// ---- triangle meshes (cspm_mesh.h) ------------------------------------------------------------------------
static_assert(sizeof(cspm_face) == 12, "cspm_face is one 12-byte record");
const cspm_mesh_params kMeshDefaults = {1.0, 0};
const char *mesh_args_error(const cspm_mesh_params *m) {
  if (!(m->max_diff >= 0.0)) return "mesh: max_diff must be >= 0 (it may be +infinity)";
  return nullptr;
}
inline size_t mesh_max_faces(int w, int h) { return 2 * (size_t)(w - 1) * (size_t)(h - 1); }
// the unsigned ints behind the pixel -> vertex map: vertex counts per workgroup and their total, then the same for the faces
inline size_t mesh_count_words(unsigned nb) { return 2 * ((size_t)nb + 1); }
// the passes of M on one view.  maps: keep, Q and the vertex map; counts: mesh_count_words(nb) unsigned ints; the totals go behind
// their count arrays unless d_nv / d_nf name another place.
void mesh_launch(hipStream_t stream, const GeomCam &cam, const GeomIn &in, const cspm_mesh_params *m, int w, int h, const MeshMaps &maps, unsigned int *counts,
                 uint4 *vertices, size_t vertex_cap, uint32_t *faces, size_t face_cap, unsigned int *d_nv, unsigned int *d_nf) {
  const long long n = (long long)w * h;
  const unsigned nb = geom_blocks(n);
  const bool slopes = in.a != nullptr;
  const int all = m->all_vertices ? 1 : 0;
  unsigned int *vcounts = counts, *fcounts = counts + nb + 1;
  const GeomOut keep_only{nullptr, nullptr, nullptr, maps.keep};
  if (slopes) hipLaunchKernelGGL(k_geom_dense<true>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, keep_only, w, n, (unsigned int *)nullptr);
  else hipLaunchKernelGGL(k_geom_dense<false>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, keep_only, w, n, (unsigned int *)nullptr);
  if (slopes) hipLaunchKernelGGL(k_mesh_quad<true>, dim3(nb), dim3(kGeomBlock), 0, stream, in, (const uint8_t *)maps.keep, w, h, n, m->max_diff, maps.quad, fcounts);
  else hipLaunchKernelGGL(k_mesh_quad<false>, dim3(nb), dim3(kGeomBlock), 0, stream, in, (const uint8_t *)maps.keep, w, h, n, m->max_diff, maps.quad, fcounts);
  hipLaunchKernelGGL(k_mesh_use, dim3(nb), dim3(kGeomBlock), 0, stream, (const uint8_t *)maps.keep, (const uint8_t *)maps.quad, w, n, all, vcounts);
  hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, stream, vcounts, (int)nb, d_nv ? d_nv : vcounts + nb);
  hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, stream, fcounts, (int)nb, d_nf ? d_nf : fcounts + nb);
  const unsigned int vcap = vertices ? (unsigned int)std::min<size_t>(vertex_cap, (size_t)n) : 0u;
  const unsigned int fcap = faces ? (unsigned int)std::min<size_t>(face_cap, mesh_max_faces(w, h)) : 0u;
  if (vcap == 0 && fcap == 0) return;  // the counts alone; faces need the map of the vertex pass
  uint4 *vout = vcap ? vertices : nullptr;
  if (slopes)
    hipLaunchKernelGGL(k_mesh_vertex<true>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, (const uint8_t *)maps.keep, (const uint8_t *)maps.quad, w, n, all,
                       (const unsigned int *)vcounts, maps.vmap, vout, vcap);
  else
    hipLaunchKernelGGL(k_mesh_vertex<false>, dim3(nb), dim3(kGeomBlock), 0, stream, cam, in, (const uint8_t *)maps.keep, (const uint8_t *)maps.quad, w, n, all,
                       (const unsigned int *)vcounts, maps.vmap, vout, vcap);
  if (fcap == 0) return;
  hipLaunchKernelGGL(k_mesh_face, dim3(nb), dim3(kGeomBlock), 0, stream, (const uint8_t *)maps.quad, (const uint32_t *)maps.vmap, w, n,
                     (const unsigned int *)fcounts, faces, fcap);
}

// the checks cspm_mesh and cspm_mesh_device share: those of the reprojection, then the mesh parameters
int mesh_check(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params **g, const cspm_fit_params *fit, const cspm_mesh_params **m) {
  if (!*m) *m = &kMeshDefaults;
  if (const char *msg = mesh_args_error(*m)) return fail(c, CSPM_ERR_ARG, msg);
  return reproject_check(c, view, source, calib, g, fit);
}
// cspm_mesh / cspm_mesh_device after their checks: the pending-run check, the inputs of the chosen source by the reprojection's own
// code, the passes.  Every output is a device pointer; d_quad == nullptr: Q stays in the context's scratch.
int mesh_enqueue(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, const cspm_mesh_params *m,
                 uint4 *vertices, size_t vertex_cap, uint32_t *faces, size_t face_cap, uint8_t *d_quad, unsigned int *d_nv, unsigned int *d_nf) {
  int rc = check_sweep(c);  // BEFORE the field is read, as in reproject_enqueue
  if (rc) return rc;
  const size_t n = (size_t)c->W * c->H;
  const unsigned nb = geom_blocks((long long)n);
  if ((rc = dalloc(c, c->mem_field, &c->mesh_bytes, 2 * n))) return rc;
  if ((rc = dalloc(c, c->mem_field, &c->mesh_map, n + mesh_count_words(nb)))) return rc;
  if ((rc = geom_inputs_alloc(c, source, fit))) return rc;
  {
    Timed t(c, CSPM_K_MISC, (long long)n);
    const GeomIn in = geom_inputs_launch(c, view, source, g, fit);
    const MeshMaps maps{c->mesh_bytes, d_quad ? d_quad : c->mesh_bytes + n, c->mesh_map};
    mesh_launch(c->stream, geom_cam(calib, g, view), in, m, c->W, c->H, maps, c->mesh_map + n, vertices, vertex_cap, faces, face_cap, d_nv, d_nf);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// ---- view synthesis (cspm_synth.h) ------------------------------------------------------------------------
static_assert(kSynthMaxWidth == CSPM_SYNTH_MAX_WIDTH, "cspm.h states the widest row of the synthesis kernel");
const cspm_synth_params kSynthDefaults = {3, 1, 4.0, 1.0};
const char *synth_args_error(const cspm_synth_params *p, double t, int w, int h, bool want_bgr, size_t out_stride) {
  if (!(t >= 0.0 && t <= 1.0)) return "view synthesis: t must be in [0, 1]";
  if (p->views < 1 || p->views > 3) return "view synthesis: views must be 1, 2 or 3";
  if (!(p->max_stretch >= 1.0)) return "view synthesis: max_stretch must be >= 1";
  if (!(p->merge_diff >= 0.0)) return "view synthesis: merge_diff must be >= 0";
  if (w < 1 || h < 1) return "view synthesis: an empty image";
  if ((long long)w * h >= (1LL << 31)) return "view synthesis: w * h must be below 2^31";
  if (w > kSynthMaxWidth) return "view synthesis: the image is wider than CSPM_SYNTH_MAX_WIDTH";
  if (want_bgr && out_stride < (size_t)w * 3) return "view synthesis: out_stride is below 3 * w";
  return nullptr;
}
void synth_launch(hipStream_t stream, const SynthView &v0, const SynthView &v1, const cspm_synth_params *p, double t, const SynthOut &out, int w, int h) {
  SynthParams k{};
  k.sigma[0] = -t;
  k.sigma[1] = 1.0 - t;
  k.w0 = 1.0 - t;
  k.w1 = t;
  k.max_stretch = p->max_stretch;
  k.merge_diff = p->merge_diff;
  k.views = p->views;
  k.fill = p->fill ? 1 : 0;
  const size_t shmem = synth_lds_bytes(w);
  allow_lds(k_synth_row, shmem);
  hipLaunchKernelGGL(k_synth_row, dim3((unsigned)h), dim3(kSynthBlock), shmem, stream, v0, v1, k, out, w);
}
// the checks cspm_synthesize and cspm_synthesize_device share; p is defaulted / validated
int synthesize_check(cspm_ctx *c, int source, const cspm_synth_params **p, double t, bool want_bgr, size_t out_stride) {
  if (!*p) *p = &kSynthDefaults;
  if (source != CSPM_GEOM_RAW && source != CSPM_GEOM_PP) return fail(c, CSPM_ERR_ARG, "view synthesis: source must be CSPM_GEOM_RAW or CSPM_GEOM_PP");
  if (const char *msg = synth_args_error(*p, t, 1, 1, false, 0)) return fail(c, CSPM_ERR_ARG, msg);  // t and the parameters, before the state
  if (!c->img0[0]) return fail(c, CSPM_ERR_STATE, "cspm_set_images first");
  if (int rc = need_field(c, "no plane field to synthesise a view from (cspm_patchmatch, cspm_local_stereo, cspm_set_planes, ...)")) return rc;
  if (const char *msg = synth_args_error(*p, t, c->W, c->H, want_bgr, out_stride)) return fail(c, CSPM_ERR_ARG, msg);
  if (source == CSPM_GEOM_PP && (!c->cost_alloc || !c->cost_ready || c->max_dis < 1))
    return fail(c, CSPM_ERR_STATE, "view synthesis from the post-processed maps needs a cost object (its max_dis)");
  return CSPM_OK;
}
// after the checks: the pending-run check, the inputs of the chosen source, the launch.  Every output is a device pointer.
int synthesize_enqueue(cspm_ctx *c, int source, const cspm_synth_params *p, double t, const SynthOut &out) {
  int rc = check_sweep(c);  // BEFORE the field is read, as in reproject_enqueue
  if (rc) return rc;
  const size_t n = (size_t)c->W * c->H;
  if (source == CSPM_GEOM_RAW && (rc = dalloc(c, c->mem_field, &c->synth_disp, 2 * n))) return rc;
  if (source == CSPM_GEOM_PP && (rc = postprocess_f64_enqueue(c))) return rc;
  {
    Timed tm(c, CSPM_K_MISC, (long long)n);
    SynthView sv[2];
    for (int v = 0; v < 2; ++v) {
      sv[v] = SynthView{nullptr, nullptr, c->f[v].a, nullptr, c->img0[v]};
      if (source == CSPM_GEOM_RAW) {
        if (p->views >> v & 1)
          hipLaunchKernelGGL(k_plane_to_disp_f64, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, field_pm(c), v, c->synth_disp + (size_t)v * n);
        sv[v].disp = c->synth_disp + (size_t)v * n;
      } else {
        sv[v].disp = c->d_pp[v];
        sv[v].a_mask = c->d_valid[v];
      }
    }
    synth_launch(c->stream, sv[0], sv[1], p, t, out, c->W, c->H);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// ---- cost aggregation (cspm_ca.h) ----------------------------------------------------------------------------------------------
constexpr int kCaRadiusBox = 3, kCaRadiusGf = 9;  // BoxCA.cpp:11, GuidedFilter.h:24
inline int ca_min_size(int method) { return method == CSPM_CA_BOX ? 2 * kCaRadiusBox + 1 : (method == CSPM_CA_GF ? 2 * kCaRadiusGf + 1 : 17); }
inline const char *ca_name(int method) { return method == CSPM_CA_BOX ? "BOX" : (method == CSPM_CA_GF ? "GF" : "BF"); }

// device buffers of one aggregation: the guide (3 natural slabs), its GF terms (16 transposed slabs), the walks' scratch
// (t: max(9, 4 nb) slabs, s: 4 nb slabs) for batches of up to nb slices
struct CaWork {
  double *gn, *t, *s;
  CaGuideT gt;
  int nb;
};
inline size_t ca_t_slabs(int nb) { return (size_t)std::max(9, 4 * nb); }

// the guide-only terms of GF for the guide in w.gn (GuidedFilter.cpp:138-208, 248-263: N, mean_I, Sigma + eps, cofactors, 1/DET)
void ca_prepare_guide(cspm_ctx *c, int method, const CaWork &w, int W, int H) {
  if (method != CSPM_CA_GF) return;
  const size_t px = (size_t)W * H;
  Timed t(c, CSPM_K_MISC, 0);
  hipLaunchKernelGGL((k_ca_ywalk<9, CaInGuide>), dim3((W + kCaBlock - 1) / kCaBlock, 1), dim3(kCaBlock), 0, c->stream, CaInGuide{w.gn, px}, W, H,
                     kCaRadiusGf, w.t);
  hipLaunchKernelGGL((k_ca_xwalk<9, CaEpGuide>), dim3((H + kCaBlock - 1) / kCaBlock, 1), dim3(kCaBlock), 0, c->stream, (const double *)w.t, W, H,
                     kCaRadiusGf, CaEpGuide{w.gt, w.gn, W, H, kCaRadiusGf, (double)0.0001f});
}

// aggreCV's filter of n (<= w.nb) slices: src -> dst, n slabs of W x H each (src == dst allowed except for BF)
void ca_filter(cspm_ctx *c, int method, const CaWork &w, int W, int H, const double *src, int n, double *dst) {
  const size_t px = (size_t)W * H;
  const dim3 gy((W + kCaBlock - 1) / kCaBlock, n), gx((H + kCaBlock - 1) / kCaBlock, n);
  Timed t(c, CSPM_K_MISC, 0);
  if (method == CSPM_CA_BOX) {  // BoxCA.cpp:8-12
    hipLaunchKernelGGL((k_ca_ywalk<1, CaInPlain>), gy, dim3(kCaBlock), 0, c->stream, CaInPlain{src, 1, px}, W, H, kCaRadiusBox, w.t);
    hipLaunchKernelGGL((k_ca_xwalk<1, CaEpStore>), gx, dim3(kCaBlock), 0, c->stream, (const double *)w.t, W, H, kCaRadiusBox, CaEpStore{dst, W, px});
  } else if (method == CSPM_CA_GF) {  // GFCA.cpp:8-11, GuidedFilter.cpp:180-298
    hipLaunchKernelGGL((k_ca_ywalk<4, CaInGfP>), gy, dim3(kCaBlock), 0, c->stream, CaInGfP{src, w.gn, px}, W, H, kCaRadiusGf, w.t);
    hipLaunchKernelGGL((k_ca_xwalk<4, CaEpGfA>), gx, dim3(kCaBlock), 0, c->stream, (const double *)w.t, W, H, kCaRadiusGf, CaEpGfA{w.gt, w.s, W, H, kCaRadiusGf});
    hipLaunchKernelGGL((k_ca_ywalk<4, CaInPlain>), gy, dim3(kCaBlock), 0, c->stream, CaInPlain{w.s, 4, px}, W, H, kCaRadiusGf, w.t);
    hipLaunchKernelGGL((k_ca_xwalk<4, CaEpGfQ>), gx, dim3(kCaBlock), 0, c->stream, (const double *)w.t, W, H, kCaRadiusGf, CaEpGfQ{w.gt, dst, W, H, kCaRadiusGf});
  } else {  // BFCA.cpp:8-12
    hipLaunchKernelGGL(k_ca_bf, dim3(ew_grid((long long)px)), dim3(256), 0, c->stream, (const double *)w.gn, src, W, H, n, dst);
  }
}

// allocate a CaWork for images of up to px pixels and batches of nb slices; the pool does not remember *w, which may be a local
int ca_alloc_work(cspm_ctx *c, size_t px, int nb, CaWork *w, DevPool &pool) {
  int rc;
  double *gt;
  w->nb = nb;
  if ((rc = dalloc_local(c, pool, &w->gn, 3 * px)) || (rc = dalloc_local(c, pool, &gt, 16 * px)) ||
      (rc = dalloc_local(c, pool, &w->t, ca_t_slabs(nb) * px)) || (rc = dalloc_local(c, pool, &w->s, (size_t)4 * nb * px)))
    return rc;
  w->gt = CaGuideT{gt, gt + 3 * px, gt + 6 * px, gt + 15 * px};
  return CSPM_OK;
}

// slices per batch: the walks' scratch and the raw / aggregated batch (10 slabs per slice) within 6 GiB, 2 .. 128.  Large batches
// matter: a walk has one lane per column (or row) and slice, and a 1242 x 375 level walked in 32-slice batches keeps only ~190 waves
// busy in its X walks -- 85 ms per C3 pair for GF; the whole level 0 of a C3 pair in one batch takes 4.8 GB
inline int ca_batch(size_t px) { return (int)std::max<long long>(2, std::min<long long>(128, (6LL << 30) / (80LL * (long long)px))); }

// cells d0 .. d0+n-1 of level s, view v, as the cost object holds them: its volume, or the slab kernels cspm_get_cost_slab uses
const double *ca_raw_cells(cspm_ctx *c, int v, int s, int d0, int n, double *scratch) {
  const Level &L = c->cost.lv[s];
  const size_t px = (size_t)L.W * L.H;
  if (L.vol[v]) return L.vol[v] + (size_t)d0 * px;
  Timed t(c, CSPM_K_MISC, 0);
  launch_cells(c, s, v, d0, n, scratch, nullptr);
  return scratch;
}

// the context's local-stereo scratch for its current geometry (kept between pairs: no allocator call, no synchronisation)
int ca_ensure(cspm_ctx *c) {
  const Cost &cd = c->cost;
  const long long key[4] = {c->W, c->H, c->max_dis, cd.levels};
  if (c->ca_nb && std::equal(key, key + 4, c->ca_key)) return CSPM_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_ca(c);  // ca_nb == 0 until every buffer is there: a call that fails half-way leaves nothing the next one would use
  const size_t px = (size_t)c->W * c->H;
  const int nb = ca_batch(px);
  CaWork w;
  int rc;
  if ((rc = ca_alloc_work(c, px, nb, &w, c->mem_ca))) return rc;
  if ((rc = dalloc(c, c->mem_ca, &c->ca_raw, (size_t)nb * px)) || (rc = dalloc(c, c->mem_ca, &c->ca_out, (size_t)nb * px)) ||
      (rc = dalloc(c, c->mem_ca, &c->ca_best, px)) || (rc = dalloc(c, c->mem_ca, &c->ca_bestd, px)) ||
      (rc = dalloc(c, c->mem_ca, &c->ca_keys, CSPM_MAX_LEVELS)))
    return rc;
  for (int s = 1; s < cd.levels; ++s)
    if ((rc = dalloc(c, c->mem_ca, &c->ca_vol[s], (size_t)(cd.lv[s].D + 1) * cd.lv[s].W * cd.lv[s].H))) return rc;
  c->ca_gn = w.gn;
  c->ca_t = w.t;
  c->ca_s = w.s;
  c->ca_gt = w.gt;
  c->ca_nb = nb;
  std::copy(key, key + 4, c->ca_key);
  return CSPM_OK;
}

// Local stereo of one view (cspm.h): aggregate levels 1.. whole and keep them, then level 0 in batches of slices folded into the WTA
int ca_local_view(cspm_ctx *c, int method, int v) {
  const Cost &cd = c->cost;
  const CaWork w{c->ca_gn, c->ca_t, c->ca_s, c->ca_gt, c->ca_nb};
  const int nb = c->ca_nb;
  HIPCHK(c, hipMemsetAsync(c->ca_keys, 0, sizeof(unsigned long long) * CSPM_MAX_LEVELS, c->stream));
  CaLevels lv{};
  lv.levels = cd.levels;
  lv.cs = cd.cs;
  lv.max_key = c->ca_keys;
  for (int s = cd.levels - 1; s >= 0; --s) {
    const Level &L = cd.lv[s];
    lv.W[s] = L.W; lv.H[s] = L.H; lv.D[s] = L.D; lv.wgt[s] = c->scale_wgt[s];
    const size_t px = (size_t)L.W * L.H;
    {
      Timed t(c, CSPM_K_MISC, 0);
      hipLaunchKernelGGL(k_ca_guide_u32, dim3(ew_grid((long long)px)), dim3(256), 0, c->stream, L.pix[v], L.W, L.H, L.Wp, L.pad, w.gn);
    }
    if (L.D >= 1) ca_prepare_guide(c, method, w, L.W, L.H);
    if (s > 0) {
      double *A = c->ca_vol[s];
      lv.vol[s] = A;
      const double *raw0 = ca_raw_cells(c, v, s, 0, 1, A);  // slice 0 is left as it is (BoxCA.cpp:8, GFCA.cpp:8, BFCA.cpp:8)
      if (raw0 != A) HIPCHK(c, hipMemcpyAsync(A, raw0, sizeof(double) * px, hipMemcpyDeviceToDevice, c->stream));
      for (int d0 = 1; d0 <= L.D; d0 += nb) {
        const int n = std::min(nb, L.D + 1 - d0);
        ca_filter(c, method, w, L.W, L.H, ca_raw_cells(c, v, s, d0, n, c->ca_raw), n, A + (size_t)d0 * px);
      }
      Timed t(c, CSPM_K_MISC, 0);
      hipLaunchKernelGGL(k_ca_max, dim3(1024), dim3(256), 0, c->stream, (const double *)A, (long long)(L.D + 1) * (long long)px, c->ca_keys + s);
    } else {
      HIPCHK(c, hipMemsetAsync(c->ca_bestd, 0, sizeof(int) * px, c->stream));
      // slices d0 .. d0+n-1 give the costs of d = d0 .. d0+n-2 (each cost interpolates towards the next slice): batches overlap by one
      for (int d0 = 1; d0 <= L.D - 1;) {
        const int n = std::min(nb, L.D + 1 - d0);
        ca_filter(c, method, w, L.W, L.H, ca_raw_cells(c, v, 0, d0, n, c->ca_raw), n, c->ca_out);
        Timed t(c, CSPM_K_MISC, 0);
        hipLaunchKernelGGL(k_ca_wta, dim3(ew_grid((long long)px)), dim3(256), 0, c->stream, lv, (const double *)c->ca_out, d0, n, c->ca_best, c->ca_bestd);
        d0 += n - 1;
      }
      Timed t(c, CSPM_K_MISC, 0);
      hipLaunchKernelGGL(k_ca_planes, dim3(ew_grid((long long)px)), dim3(256), 0, c->stream, c->f[v], (long long)px, (const double *)c->ca_best,
                         (const int *)c->ca_bestd);
    }
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}

// ---- rectification (cspm_rect.h) ---------------------------------------------------------------------------
const cspm_rect_params kRectDefaults = {0.0, NAN, NAN, 0, 0};
inline bool all_finite(const double *p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}
const char *rig_error(const cspm_rig *rig) {
  if (!rig) return "rectification: no rig";
  for (int v = 0; v < 2; ++v) {
    if (!all_finite(&rig->cam[v].fx, 10)) return "rectification: the cameras must be finite";
    if (!(rig->cam[v].fx > 0.0) || !(rig->cam[v].fy > 0.0)) return "rectification: fx and fy must be positive";
  }
  if (!all_finite(rig->R, 9) || !all_finite(rig->T, 3)) return "rectification: R and T must be finite";
  if (rig->T[0] == 0.0 && rig->T[1] == 0.0 && rig->T[2] == 0.0) return "rectification: T is zero, the cameras share their centre";
  if (rig->raw_w < 1 || rig->raw_h < 1) return "rectification: the raw size must be at least 1 x 1";
  if ((long long)rig->raw_w * rig->raw_h >= (1LL << 31)) return "rectification: raw_w * raw_h must be below 2^31";
  return nullptr;
}
const char *rect_error(const cspm_rectification *r) {
  if (!r) return "rectification: no rectification (cspm_rectify_compute)";
  if (!all_finite(r->R0, 9) || !all_finite(r->R1, 9) || !std::isfinite(r->f) || !std::isfinite(r->cx) || !std::isfinite(r->cy) || !std::isfinite(r->baseline))
    return "rectification: the rectification must be finite";
  if (!(r->f > 0.0) || !(r->baseline > 0.0)) return "rectification: f and baseline must be positive";
  if (r->w < 1 || r->h < 1) return "rectification: the rectified size must be at least 1 x 1";
  if ((long long)r->w * r->h >= (1LL << 31)) return "rectification: w * h must be below 2^31";
  return nullptr;
}
inline void cross3(const double *p, const double *q, double *o) {
  o[0] = p[1] * q[2] - p[2] * q[1];
  o[1] = p[2] * q[0] - p[0] * q[2];
  o[2] = p[0] * q[1] - p[1] * q[0];
}
// the derivation of R (cspm.h "rectification"); the rig has passed rig_error
const char *rect_compute(const cspm_rig *rig, const cspm_rect_params *p, cspm_rectification *out) {
  const double *R = rig->R, *T = rig->T;
  double C1[3], e1[3], e2[3], e3[3], c[3];
  for (int j = 0; j < 3; ++j) C1[j] = -((R[j] * T[0] + R[3 + j] * T[1]) + R[6 + j] * T[2]);
  const double baseline = std::sqrt((C1[0] * C1[0] + C1[1] * C1[1]) + C1[2] * C1[2]);
  if (!(baseline > 0.0) || !std::isfinite(baseline)) return "rectification: the baseline is zero or not finite";
  for (int j = 0; j < 3; ++j) e1[j] = C1[j] / baseline;
  if (!(e1[0] > 0.0) || !(std::fabs(e1[0]) >= std::fabs(e1[1])) || !(std::fabs(e1[0]) >= std::fabs(e1[2])))
    return "rectification: camera 1 must be to the right of camera 0 and the rig horizontal (swap the cameras, or rotate the images)";
  const double zm[3] = {R[6], R[7], 1.0 + R[8]};
  cross3(zm, e1, c);
  const double len = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  if (!(len > 0.0) || !std::isfinite(len)) return "rectification: the mean optical axis is parallel to the baseline";
  for (int j = 0; j < 3; ++j) e2[j] = c[j] / len;
  cross3(e1, e2, e3);
  for (int j = 0; j < 3; ++j) { out->R0[j] = e1[j]; out->R0[3 + j] = e2[j]; out->R0[6 + j] = e3[j]; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out->R1[3 * i + j] = (out->R0[3 * i] * R[3 * j] + out->R0[3 * i + 1] * R[3 * j + 1]) + out->R0[3 * i + 2] * R[3 * j + 2];
  out->baseline = baseline;
  if (std::isinf(p->f) || std::isinf(p->cx) || std::isinf(p->cy)) return "rectification: f, cx and cy of the parameters must be finite or automatic";
  const cspm_camera *k = rig->cam;
  out->f = p->f > 0.0 ? p->f : 0.25 * (((k[0].fx + k[0].fy) + k[1].fx) + k[1].fy);
  out->w = p->w > 0 ? p->w : rig->raw_w;
  out->h = p->h > 0 ? p->h : rig->raw_h;
  if ((long long)out->w * out->h >= (1LL << 31)) return "rectification: w * h must be below 2^31";
  double q[2][2];
  for (int v = 0; v < 2; ++v) {
    const double *Rv = v ? out->R1 : out->R0;
    const double yn = ((double)(rig->raw_h - 1) / 2.0 - k[v].cy) / k[v].fy;
    const double xn = (((double)(rig->raw_w - 1) / 2.0 - k[v].cx) - k[v].skew * yn) / k[v].fx;
    double P[3];
    for (int i = 0; i < 3; ++i) P[i] = (Rv[3 * i] * xn + Rv[3 * i + 1] * yn) + Rv[3 * i + 2];
    q[v][0] = (out->f * P[0]) / P[2];
    q[v][1] = (out->f * P[1]) / P[2];
  }
  out->cx = std::isnan(p->cx) ? (double)(out->w - 1) / 2.0 - 0.5 * (q[0][0] + q[1][0]) : p->cx;
  out->cy = std::isnan(p->cy) ? (double)(out->h - 1) / 2.0 - 0.5 * (q[0][1] + q[1][1]) : p->cy;
  if (const char *msg = rect_error(out)) return msg;
  return nullptr;
}
RectView rect_view(const cspm_rig *rig, const cspm_rectification *r, int view) {
  RectView k;
  k.f = r->f; k.cx = r->cx; k.cy = r->cy;
  for (int i = 0; i < 9; ++i) k.r[i] = (view ? r->R1 : r->R0)[i];
  const cspm_camera &c = rig->cam[view];
  k.fx = c.fx; k.fy = c.fy; k.cxraw = c.cx; k.cyraw = c.cy; k.skew = c.skew;
  k.k1 = c.k1; k.k2 = c.k2; k.p1 = c.p1; k.p2 = c.p2; k.k3 = c.k3;
  k.raw_w = rig->raw_w; k.raw_h = rig->raw_h;
  return k;
}
inline void rect_map_launch(hipStream_t stream, const RectView &k, int w, int h, double *map, uint8_t *valid) {
  const long long n = (long long)w * h;
  hipLaunchKernelGGL(k_rect_map, dim3(ew_grid(n, kRectBlock)), dim3(kRectBlock), 0, stream, k, w, n, map, valid);
}
// raw_bgr (rows of raw_stride bytes) -> rawpix (packed words) -> dst (8UC3 rows of dst_stride bytes) through one view's map
inline void rect_remap_launch(hipStream_t stream, const uint8_t *raw_bgr, size_t raw_stride, int raw_w, int raw_h, uint32_t *rawpix, const double *map,
                              const uint8_t *valid, int w, int h, uint8_t *dst, size_t dst_stride) {
  hipLaunchKernelGGL(k_pack_bgr, dim3(ew_grid((long long)raw_w * raw_h)), dim3(256), 0, stream, raw_bgr, raw_stride, raw_w, raw_h, raw_w, 0, rawpix);
  const long long items = (((long long)w + kWave - 1) / kWave) * h;
  hipLaunchKernelGGL(k_rect_remap, dim3((unsigned)((items + kRectWaves - 1) / kRectWaves)), dim3(kRectBlock), 0, stream, map, valid, (const uint32_t *)rawpix,
                     raw_w, raw_h, w, h, dst, dst_stride);
}

// What an entry moves between caller memory and the device goes through a Staging on the context's stream: device
// temporaries, uploads, downloads and one latched status.  The first failure sticks in `rc` and turns every later member call into a
// no-op (a null pointer), so a body is straight-line code: stage, `if (S.rc) return S.finish();`, launch on S.c->stream, download,
// `return S.finish("what failed")`.  The temporaries are freed when the Staging goes, on every path.  No path returns while a copy to or
// from caller memory that this call enqueued is outstanding: a failure waits on the stream before it is latched, finish() waits, and
// whichever other way the body returns, ~Staging waits (a host buffer of the body's own that a copy uses is declared BEFORE the Staging).
// The message of a failure is the context's.  A context entry declares its Staging behind ON_DEVICE, so that the frees run on the
// buffers' device; a one-shot entry uses a OneShot.
struct Staging {
  cspm_ctx *c;
  int rc;
  DevPool bufs{dev_alloc, dev_free};  // freed when the Staging goes, behind ~Staging's wait
  bool broke = false;   // a launch or a download failed: finish() names it
  bool settled = true;  // no copy enqueued here since the last wait

  explicit Staging(cspm_ctx *ctx, int status = CSPM_OK) : c(ctx), rc(status) {}
  Staging(const Staging &) = delete;
  ~Staging() {
    if (!settled) wait();
  }
  bool wait() { return settled = hipStreamSynchronize(c->stream) == hipSuccess; }
  bool copied(hipError_t e) { return settled = false, e == hipSuccess; }  // the result of a copy that was just enqueued
  int latch(int status) {
    if (status && !rc && !settled) wait();
    return rc = rc ? rc : status;
  }
  int fail(int code, const char *msg) { return rc ? rc : latch(::fail(c, code, msg)); }
  // n elements on the device; null when !want
  template <class T>
  T *buf(size_t n, bool want = true) {
    T *p = nullptr;
    if (!rc && want) latch(dalloc_local(c, bufs, &p, n));
    return p;
  }
  template <class T>
  void put(T *dev, const T *host, size_t n) {
    if (!rc && !copied(hipMemcpyAsync(dev, host, sizeof(T) * n, hipMemcpyHostToDevice, c->stream))) fail(CSPM_ERR_HIP, "upload failed");
  }
  // `rows` rows of `row` bytes that lie `stride` bytes apart, `pitch` bytes apart on the device
  void put2d(void *dev, size_t pitch, const void *host, size_t stride, size_t row, size_t rows) {
    if (!rc && !copied(hipMemcpy2DAsync(dev, pitch, host, stride, row, rows, hipMemcpyHostToDevice, c->stream))) fail(CSPM_ERR_HIP, "upload failed");
  }
  void fill(void *dev, int byte, size_t bytes) {
    if (!rc && hipMemsetAsync(dev, byte, bytes, c->stream) != hipSuccess) fail(CSPM_ERR_HIP, "upload failed");
  }
  // a buffer holding host[0 .. n); null for a null host pointer
  template <class T>
  T *up(const T *host, size_t n) {
    T *p = buf<T>(n, host != nullptr);
    if (host) put(p, host, n);
    return p;
  }
  // the same for rows that lie `stride` bytes apart: packed on the device
  uint8_t *up2d(const uint8_t *host, size_t stride, size_t row, size_t rows) {
    uint8_t *p = buf<uint8_t>(row * rows, host != nullptr);
    if (host) put2d(p, row, host, stride, row, rows);
    return p;
  }
  // an 8UC3 image as the packed words the kernels read (k_pack_bgr); null for a null host pointer
  uint32_t *up_bgr(const uint8_t *host, size_t stride, int w, int h) {
    const uint8_t *bgr = up2d(host, stride, (size_t)w * 3, (size_t)h);
    uint32_t *pix = buf<uint32_t>((size_t)w * h, host != nullptr);
    if (host && !rc) hipLaunchKernelGGL(k_pack_bgr, dim3(ew_grid((long long)w * h)), dim3(256), 0, c->stream, bgr, (size_t)w * 3, w, h, w, 0, pix);
    return pix;
  }
  // downloads: nothing for a null host pointer or no elements, and nothing behind a launch that failed
  template <class T>
  void down(T *host, const void *dev, size_t n) {
    if (host && n && !rc && !broke) broke = hipGetLastError() != hipSuccess || !copied(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
  }
  void down2d(uint8_t *host, size_t stride, const uint8_t *dev, size_t row, size_t rows) {
    if (host && !rc && !broke)
      broke = hipGetLastError() != hipSuccess || !copied(hipMemcpy2DAsync(host, stride, dev, row, row, rows, hipMemcpyDeviceToHost, c->stream));
  }
  // waits for the launches and copies so far: `failed` is the message if one of them did not succeed
  int finish(const char *failed = "") {
    if (!rc && (broke || hipGetLastError() != hipSuccess || !wait())) fail(CSPM_ERR_HIP, failed);
    return rc;
  }
};

// A one-shot host entry (cspm_*_host: one kernel family alone on caller memory) checks its arguments, then stages on a OneShot: a
// temporary context on `device` and the Staging on it.  Everything between its construction and its destruction runs on that device; the
// caller's current device comes back when it goes.  The message of a failure stays behind as the thread's creation error
// (cspm_last_error(NULL)).
struct TempCtx {
  cspm_ctx *ctx = nullptr;
  int created;
  std::optional<DevGuard> guard;
  explicit TempCtx(int device) : created(cspm_create(&ctx, device)) {
    if (!created && !guard.emplace(device).ok) created = fail(ctx, CSPM_ERR_HIP, "hipSetDevice failed");
  }
  ~TempCtx() { cspm_destroy(ctx); }  // behind ~Staging; waits for the stream, then the guard goes
};
struct OneShot : TempCtx, Staging {
  explicit OneShot(int device) : TempCtx(device), Staging(ctx, created) {}
  int finish(const char *failed = "") {
    if (Staging::finish(failed) && c) g_create_error = c->err;
    return rc;
  }
};

// cspm_fit_planes and cspm_segment_planes behind their parameter checks: planes fitted to the stored field's own disparity maps replace
// the field or, with `merge`, are merged into it as candidates, view by view.  `scratch` allocates what the entry keeps and names the
// two disparity snapshots (n doubles per view); `fit_view(v, d, out)` enqueues the launches that fit view v's snapshot d into `out`.
template <class Scratch, class FitView>
int fit_stored_field(cspm_ctx *c, int merge, int max_rows, const char *too_high, Scratch scratch, FitView fit_view) {
  if (!c->img0[0]) return fail(c, CSPM_ERR_STATE, "cspm_set_images first");
  int rc;
  if ((rc = need_field(c, "no plane field to fit (cspm_local_stereo, cspm_set_planes, cspm_pm_init or an earlier run)"))) return rc;
  if (merge && (rc = need_cost(c))) return rc;
  if (c->max_dis < 1) return fail(c, CSPM_ERR_STATE, "no max_dis known: build a cost object (or cspm_fpm_begin) first");
  if (c->H > max_rows) return fail(c, CSPM_ERR_ARG, too_high);
  ON_DEVICE(c);
  const size_t n = (size_t)c->W * c->H;
  double *snap = nullptr;
  if ((rc = scratch(&snap))) return rc;
  CandBuf cand{};
  if (merge) {
    if ((rc = ensure_cand(c, &cand)) || (rc = ensure_consistent(c))) return rc;
  } else {
    c->field_consistent = false;  // min_cost still belongs to the planes that were replaced
  }
  c->repeat.taint_unchecked_run();  // it can no longer be repeated over these planes
  const Pm pm = field_pm(c);
  for (int v = 0; v < 2; ++v) {
    double *d = snap + (size_t)v * n;
    const Field &f = c->f[v];
    const FitOut out = merge ? cand.fit_out() : FitOut{f.nx, f.ny, f.nz, f.a, f.b, f.c, nullptr, 1};
    {
      Timed t(c, CSPM_K_MISC, (long long)n);
      hipLaunchKernelGGL(k_plane_to_disp_f64, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, pm, v, d);
      fit_view(v, d, out);
    }
    HIPCHK(c, hipGetLastError());
    if (merge) {
      const CandField cf = cand.field(v);
      if ((rc = do_merge(c, &cf, &kDefaultParams, v, 1, (long long)n))) return rc;
    }
  }
  return CSPM_OK;
}

// ---- depth-map fusion (cspm_fuse.h) -----------------------------------------------------------------------
static_assert(sizeof(FuseCam) == 15 * sizeof(double), "the camera table is 15 doubles per view");
static_assert(CSPM_FUSE_MAX_VIEWS == kFuseMaxViews, "cspm.h and cspm_fuse.h agree on the number of views");
const cspm_fuse_params kFuseDefaults = {2.0, 0.01, 0.0, 2, 1};
const char *fuse_params_error(const cspm_fuse_params *p) {
  if (!(p->max_reproj >= 0.0)) return "fusion: max_reproj must be >= 0";
  if (!(p->max_rel_depth >= 0.0)) return "fusion: max_rel_depth must be >= 0";
  if (!(p->min_cos >= 0.0 && p->min_cos <= 1.0)) return "fusion: min_cos must be in [0, 1]";
  if (p->min_views < 0 || p->min_views > kFuseMaxViews - 1) return "fusion: min_views must be in 0 .. 63";
  return nullptr;
}
const char *fuse_camera_error(double f, double cx, double cy, const double *R, const double *t) {
  if (!R || !t) return "fusion: no pose";
  bool finite = std::isfinite(f) && std::isfinite(cx) && std::isfinite(cy);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R[i]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(t[i]);
  if (!finite) return "fusion: the camera and its pose must be finite";
  if (!(f > 0.0)) return "fusion: f must be positive";
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(d) <= 1e-6)) return "fusion: R is not a rotation (max |R R^T - I| > 1e-6)";
    }
  return nullptr;
}
const char *fuse_size_error(int w, int h) {
  if (w < 1 || h < 1) return "fusion: w and h must be at least 1";
  if ((long long)w * h >= (1LL << 31)) return "w * h must be below 2^31: cloud records hold 32-bit pixel indices";
  return nullptr;
}
const char *fuse_maps_error(const double *depth, const uint8_t *bgr, size_t bgr_stride, int w) {
  if (!depth) return "fusion: no depth map";
  if (bgr && bgr_stride < (size_t)w * 3) return "fusion: bgr_stride is below 3 * w";
  return nullptr;
}
inline size_t fuse_count_words(int max_views, unsigned nb) { return (size_t)max_views * nb + 1 + (size_t)max_views; }

int fuse_begin(cspm_ctx *c, int w, int h, int max_views) {
  if (const char *msg = fuse_size_error(w, h)) return fail(c, CSPM_ERR_ARG, msg);
  if (max_views < 1 || max_views > kFuseMaxViews) return fail(c, CSPM_ERR_ARG, "fusion: max_views must be in 1 .. 64");
  if (c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin twice without cspm_fuse_end");
  const size_t n = (size_t)w * h, K = (size_t)max_views;
  int rc;
  if ((rc = dalloc(c, c->mem_fuse, &c->fuse_depth, K * n)) || (rc = dalloc(c, c->mem_fuse, &c->fuse_normal, K * 3 * n)) ||
      (rc = dalloc(c, c->mem_fuse, &c->fuse_pix, K * n)) || (rc = dalloc(c, c->mem_fuse, &c->fuse_bytes, 2 * K * n)) ||
      (rc = dalloc(c, c->mem_fuse, &c->fuse_cams, K)) ||
      (rc = dalloc(c, c->mem_fuse, &c->fuse_counts, fuse_count_words(max_views, geom_blocks((long long)n))))) {
    c->mem_fuse.release();
    return rc;
  }
  c->fuse_cams_host.assign(K, FuseCam{});
  c->fuse_on = true;
  c->fuse_w = w; c->fuse_h = h; c->fuse_max = max_views; c->fuse_views = 0;
  c->fuse_normals = c->fuse_images = false;
  c->fuse_image_mask = 0ull;
  return CSPM_OK;
}
void fuse_release(cspm_ctx *c) {
  c->mem_fuse.release();
  c->fuse_on = false;
  c->fuse_views = c->fuse_max = c->fuse_w = c->fuse_h = 0;
}
// what every push checks before it touches the slot: a begin, a free slot, a valid camera, normals in all views or in none
int fuse_slot_check(cspm_ctx *c, bool normals, double f, double cx, double cy, const double *R, const double *t) {
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (c->fuse_views >= c->fuse_max) return fail(c, CSPM_ERR_STATE, "fusion: every view slot is taken (max_views of cspm_fuse_begin)");
  if (const char *msg = fuse_camera_error(f, cx, cy, R, t)) return fail(c, CSPM_ERR_ARG, msg);
  if (c->fuse_views > 0 && normals != c->fuse_normals) return fail(c, CSPM_ERR_ARG, "fusion: normals in some views but not all");
  return CSPM_OK;
}
// the slot is filled: its row of the camera table goes up and the view counts
int fuse_slot_commit(cspm_ctx *c, bool normals, bool image, double f, double cx, double cy, const double *R, const double *t) {
  FuseCam &cam = c->fuse_cams_host[(size_t)c->fuse_views];  // lives as long as the slots: the copy may read it later
  cam.f = f; cam.cx = cx; cam.cy = cy;
  for (int i = 0; i < 9; ++i) cam.R[i] = R[i];
  for (int i = 0; i < 3; ++i) cam.t[i] = t[i];
  HIPCHK(c, hipMemcpyAsync(c->fuse_cams + c->fuse_views, &cam, sizeof cam, hipMemcpyHostToDevice, c->stream));
  c->fuse_normals = normals;
  c->fuse_images = c->fuse_images || image;
  if (image) c->fuse_image_mask |= 1ull << c->fuse_views;
  c->fuse_views += 1;
  return CSPM_OK;
}
// a view from caller memory (the caller runs on the context's device)
int fuse_push_maps(cspm_ctx *c, const double *depth, const double *normal, const uint8_t *bgr, size_t bgr_stride, double f, double cx, double cy,
                   const double *R, const double *t) {
  if (int rc = fuse_slot_check(c, normal != nullptr, f, cx, cy, R, t)) return rc;
  if (const char *msg = fuse_maps_error(depth, bgr, bgr_stride, c->fuse_w)) return fail(c, CSPM_ERR_ARG, msg);
  const int w = c->fuse_w, h = c->fuse_h;
  const size_t n = (size_t)w * h, k = (size_t)c->fuse_views;
  Staging S(c);
  S.put(c->fuse_depth + k * n, depth, n);
  if (normal) S.put(c->fuse_normal + k * 3 * n, normal, 3 * n);
  if (bgr) {
    const uint8_t *dbgr = S.up2d(bgr, bgr_stride, (size_t)w * 3, (size_t)h);
    if (!S.rc) hipLaunchKernelGGL(k_pack_bgr, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, dbgr, (size_t)w * 3, w, h, w, 0, c->fuse_pix + k * n);
  } else {
    S.fill(c->fuse_pix + k * n, 0, sizeof(uint32_t) * n);
  }
  if (S.finish("fusion: the upload of a view failed")) return S.rc;
  return fuse_slot_commit(c, normal != nullptr, bgr != nullptr, f, cx, cy, R, t);
}
// F over the views pushed so far; every output a device pointer or null
int fuse_enqueue(cspm_ctx *c, const cspm_fuse_params *p, uint4 *cloud, size_t cap, unsigned int *d_count, unsigned int *d_view_counts, uint8_t *d_state) {
  const int K = c->fuse_views, w = c->fuse_w, h = c->fuse_h;
  const long long n = (long long)w * h;
  const unsigned nb = geom_blocks(n);
  const FuseMaps maps{c->fuse_depth, c->fuse_normals ? c->fuse_normal : nullptr, c->fuse_images ? c->fuse_pix : nullptr, c->fuse_bytes,
                      c->fuse_bytes + (size_t)c->fuse_max * n};
  const FusePar par{p->max_reproj * p->max_reproj, p->max_rel_depth, p->min_cos, p->min_views, p->suppress ? 1 : 0};
  unsigned int *counts = c->fuse_counts, *total = d_count ? d_count : counts + (size_t)K * nb;  // behind the counts of the K passes
  {
    Timed t(c, CSPM_K_MISC, (long long)K * n);
    HIPCHK(c, hipMemsetAsync(maps.used, 0, (size_t)K * n, c->stream));
    for (int r = 0; r < K; ++r) {
      if (maps.normal) hipLaunchKernelGGL(k_fuse_view<true>, dim3(nb), dim3(kGeomBlock), 0, c->stream, (const FuseCam *)c->fuse_cams, maps, par, K, r, w, h, n, counts + (size_t)r * nb);
      else hipLaunchKernelGGL(k_fuse_view<false>, dim3(nb), dim3(kGeomBlock), 0, c->stream, (const FuseCam *)c->fuse_cams, maps, par, K, r, w, h, n, counts + (size_t)r * nb);
    }
    hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, c->stream, counts, (int)(K * nb), total);
    if (d_view_counts)
      hipLaunchKernelGGL(k_fuse_counts, dim3(1), dim3(kFuseMaxViews), 0, c->stream, (const unsigned int *)counts, (const unsigned int *)total, K, nb, d_view_counts);
    const unsigned int cap32 = (unsigned int)std::min<size_t>(cap, 0xFFFFFFFFull);  // ranks are 32-bit, like the count
    if (cloud && cap32 != 0) {
      if (maps.normal) hipLaunchKernelGGL(k_fuse_cloud<true>, dim3(nb, K), dim3(kGeomBlock), 0, c->stream, (const FuseCam *)c->fuse_cams, maps, par, K, w, h, n, (const unsigned int *)counts, cloud, cap32);
      else hipLaunchKernelGGL(k_fuse_cloud<false>, dim3(nb, K), dim3(kGeomBlock), 0, c->stream, (const FuseCam *)c->fuse_cams, maps, par, K, w, h, n, (const unsigned int *)counts, cloud, cap32);
    }
    if (d_state) HIPCHK(c, hipMemcpyAsync(d_state, maps.state, (size_t)K * n, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
int fuse_run_check(cspm_ctx *c, const cspm_fuse_params **p) {
  if (!*p) *p = &kFuseDefaults;
  if (const char *msg = fuse_params_error(*p)) return fail(c, CSPM_ERR_ARG, msg);
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (c->fuse_views < 1) return fail(c, CSPM_ERR_STATE, "fusion: no view has been pushed");
  return CSPM_OK;
}
// cspm_fuse_run behind its checks, on the context's device: host outputs
int fuse_run(cspm_ctx *c, const cspm_fuse_params *p, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out, unsigned int *view_counts_out,
             uint8_t *state_out) {
  const size_t K = (size_t)c->fuse_views, n = (size_t)c->fuse_w * c->fuse_h;
  const unsigned nb = geom_blocks((long long)n);
  const size_t cap = std::min(cloud_out ? cloud_cap : (size_t)0, K * n);
  unsigned int total = 0;  // in front of the Staging: a download writes it
  unsigned int *vcounts = c->fuse_counts + (size_t)c->fuse_max * nb + 1;
  Staging S(c);
  uint4 *dcloud = S.buf<uint4>(2 * cap, cap != 0);
  if (S.rc) return S.finish();
  if (int rc = fuse_enqueue(c, p, dcloud, cap, nullptr, view_counts_out ? vcounts : nullptr, nullptr)) return rc;
  S.down(&total, c->fuse_counts + K * nb, 1);
  if (S.finish("fusion kernels failed")) return S.rc;
  S.down(cloud_out, dcloud, std::min((size_t)total, cap));  // the count first, then the records that were written
  S.down(view_counts_out, vcounts, K);
  S.down(state_out, c->fuse_bytes + (size_t)c->fuse_max * n, K * n);
  if (S.finish("fusion download failed")) return S.rc;
  if (count_out) *count_out = total;
  return CSPM_OK;
}

// ---- TSDF fusion (cspm_tsdf.h) -------------------------------------------------------------------------------
static_assert(sizeof(cspm_tsdf_camera) == sizeof(FuseCam), "a raycast camera is a row of the camera table");
const cspm_tsdf_params kTsdfDefaults = {{0.0, 0.0, 0.0}, 0.0, 0, 0, 0, 0.0, 64.0, 0.0, 0.5};
const char *tsdf_params_error(const cspm_tsdf_params *p) {
  if (!p) return "tsdf: no parameters";
  if (!(std::isfinite(p->origin[0]) && std::isfinite(p->origin[1]) && std::isfinite(p->origin[2]) && std::isfinite(p->voxel) && p->voxel > 0.0))
    return "tsdf: the origin must be finite and voxel finite and > 0";
  if (p->nx < 1 || p->ny < 1 || p->nz < 1) return "tsdf: nx, ny and nz must be at least 1";
  if ((long long)p->nx * p->ny >= (1LL << 31) || (long long)p->nx * p->ny * p->nz >= (1LL << 31)) return "tsdf: nx * ny * nz must be below 2^31";
  if (!(std::isfinite(p->trunc) && p->trunc >= 0.0)) return "tsdf: trunc must be finite and > 0 (0 = 4 * voxel)";
  if (!(p->max_weight >= 1.0 && p->max_weight <= 16777216.0)) return "tsdf: max_weight must be in [1, 16777216]";
  if (!(p->min_cos >= 0.0 && p->min_cos <= 1.0)) return "tsdf: min_cos must be in [0, 1]";
  if (!(p->step_rel > 0.0 && p->step_rel <= 1.0)) return "tsdf: step_rel must be in (0, 1]";
  return nullptr;
}
const char *tsdf_camera_error(const cspm_tsdf_camera *k, double z_near) {
  if (!k) return "tsdf: no camera";
  if (const char *msg = fuse_camera_error(k->f, k->cx, k->cy, k->R, k->t)) return msg;
  if (!(std::isfinite(z_near) && z_near >= 0.0)) return "tsdf: z_near must be finite and >= 0";
  return nullptr;
}
inline FuseCam tsdf_cam(const cspm_tsdf_camera *k) {
  FuseCam cam;
  cam.f = k->f; cam.cx = k->cx; cam.cy = k->cy;
  for (int i = 0; i < 9; ++i) cam.R[i] = k->R[i];
  for (int i = 0; i < 3; ++i) cam.t[i] = k->t[i];
  return cam;
}
inline unsigned tsdf_blocks(long long nvox) { return (unsigned)((nvox + kTsdfBlock - 1) / kTsdfBlock); }

int tsdf_clear(cspm_ctx *c) {
  hipLaunchKernelGGL(k_tsdf_clear, dim3(tsdf_blocks(c->tsdf_nvox)), dim3(kTsdfBlock), 0, c->stream, c->tsdf, c->tsdf_nvox);
  HIPCHK(c, hipGetLastError());
  c->tsdf_coloured = false;
  return CSPM_OK;
}
void tsdf_release(cspm_ctx *c) {
  c->mem_tsdf.release();
  c->tsdf_on = c->tsdf_coloured = false;
  c->tsdf = TsdfVol{};
  c->tsdf_nvox = 0;
}
int tsdf_begin(cspm_ctx *c, const cspm_tsdf_params *p) {
  if (const char *msg = tsdf_params_error(p)) return fail(c, CSPM_ERR_ARG, msg);
  if (c->tsdf_on) return fail(c, CSPM_ERR_STATE, "tsdf: cspm_tsdf_begin twice without cspm_tsdf_end");
  const size_t nvox = (size_t)p->nx * p->ny * p->nz;
  TsdfVol &V = c->tsdf;  // its three pointers are the pool's slots
  int rc;
  if ((rc = dalloc(c, c->mem_tsdf, &V.D, nvox)) || (rc = dalloc(c, c->mem_tsdf, &V.W, nvox)) || (rc = dalloc(c, c->mem_tsdf, &V.C, nvox)) ||
      (rc = dalloc(c, c->mem_tsdf, &c->tsdf_counts, (size_t)tsdf_blocks((long long)nvox) + 1))) {
    c->mem_tsdf.release();
    return rc;
  }
  for (int a = 0; a < 3; ++a) V.origin[a] = p->origin[a];
  V.voxel = p->voxel;
  V.trunc = p->trunc == 0.0 ? 4.0 * p->voxel : p->trunc;
  V.max_weight = p->max_weight;
  V.min_cos = p->min_cos;
  V.step = p->step_rel * V.trunc;
  V.nx = p->nx; V.ny = p->ny; V.nz = p->nz;
  c->tsdf_nvox = (long long)nvox;
  c->tsdf_on = true;
  if ((rc = tsdf_clear(c))) tsdf_release(c);
  return rc;
}
int tsdf_state_check(cspm_ctx *c) { return c->tsdf_on ? CSPM_OK : fail(c, CSPM_ERR_STATE, "tsdf: cspm_tsdf_begin first"); }

// one fusion slot into the volume
int tsdf_integrate(cspm_ctx *c, int slot) {
  if (int rc = tsdf_state_check(c)) return rc;
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (slot < 0 || slot >= c->fuse_views) return fail(c, CSPM_ERR_STATE, "tsdf: no such fusion view");
  const int w = c->fuse_w, h = c->fuse_h;
  const long long n = (long long)w * h;
  const double *depth = c->fuse_depth + (size_t)slot * n, *normal = c->fuse_normal + (size_t)slot * 3 * n;
  const uint32_t *pix = c->fuse_pix + (size_t)slot * n;
  const bool normals = c->fuse_normals && c->tsdf.min_cos > 0.0, colour = ((c->fuse_image_mask >> slot) & 1ull) != 0;
  {
    Timed t(c, CSPM_K_MISC, c->tsdf_nvox);
    const dim3 grid(tsdf_blocks(c->tsdf_nvox)), block(kTsdfBlock);
#define TSDF_INTEGRATE(N, I) \
  hipLaunchKernelGGL((k_tsdf_integrate<N, I>), grid, block, 0, c->stream, (const FuseCam *)c->fuse_cams, slot, depth, normal, pix, w, h, n, c->tsdf, c->tsdf_nvox)
    if (normals && colour) TSDF_INTEGRATE(true, true);
    else if (normals) TSDF_INTEGRATE(true, false);
    else if (colour) TSDF_INTEGRATE(false, true);
    else TSDF_INTEGRATE(false, false);
#undef TSDF_INTEGRATE
  }
  HIPCHK(c, hipGetLastError());
  c->tsdf_coloured = c->tsdf_coloured || colour;
  return CSPM_OK;
}

// a raycast into device outputs
int tsdf_raycast_enqueue(cspm_ctx *c, const FuseCam &cam, int w, int h, double z_near, const TsdfRayOut &out) {
  {
    Timed t(c, CSPM_K_MISC, (long long)w * h);
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)((w + kTsdfTileW - 1) / kTsdfTileW), (unsigned)((h + kTsdfTileH - 1) / kTsdfTileH)), dim3(kTsdfBlock), 0,
                       c->stream, cam, c->tsdf, w, h, z_near, out);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
int tsdf_raycast_check(cspm_ctx *c, const cspm_tsdf_camera *k, int w, int h, double z_near, bool bgr, size_t stride) {
  if (const char *msg = tsdf_camera_error(k, z_near)) return fail(c, CSPM_ERR_ARG, msg);
  if (const char *msg = fuse_size_error(w, h)) return fail(c, CSPM_ERR_ARG, msg);
  if ((h + kTsdfTileH - 1) / kTsdfTileH > 65535) return fail(c, CSPM_ERR_ARG, "tsdf: h must be at most 524280");
  if (bgr && stride < (size_t)w * 3) return fail(c, CSPM_ERR_ARG, "tsdf: stride is below 3 * w");
  return tsdf_state_check(c);
}
int tsdf_raycast_host(cspm_ctx *c, const cspm_tsdf_camera *k, int w, int h, double z_near, double *depth_out, double *normal_out, uint8_t *bgr_out,
                      size_t stride, uint8_t *status_out) {
  const size_t n = (size_t)w * h;
  Staging S(c);
  TsdfRayOut out{};
  out.depth = S.buf<double>(n, depth_out != nullptr);
  out.normal = S.buf<double>(3 * n, normal_out != nullptr);
  out.bgr = S.buf<uint8_t>(3 * n, bgr_out != nullptr);
  out.bgr_stride = (size_t)w * 3;
  out.status = S.buf<uint8_t>(n, status_out != nullptr);
  if (S.rc) return S.finish();
  if (int rc = tsdf_raycast_enqueue(c, tsdf_cam(k), w, h, z_near, out)) return rc;
  S.down(depth_out, out.depth, n);
  S.down(normal_out, out.normal, 3 * n);
  S.down2d(bgr_out, stride, out.bgr, (size_t)w * 3, (size_t)h);
  S.down(status_out, out.status, n);
  return S.finish("tsdf: the raycast failed");
}

// the surface points; every output a device pointer or null
int tsdf_points_enqueue(cspm_ctx *c, uint4 *cloud, size_t cap, unsigned int *d_count) {
  const unsigned nb = tsdf_blocks(c->tsdf_nvox);
  unsigned int *counts = c->tsdf_counts, *total = d_count ? d_count : counts + nb;
  {
    Timed t(c, CSPM_K_MISC, c->tsdf_nvox);
    hipLaunchKernelGGL(k_tsdf_count, dim3(nb), dim3(kTsdfBlock), 0, c->stream, c->tsdf, c->tsdf_nvox, counts);
    hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, c->stream, counts, (int)nb, total);
    const unsigned int cap32 = (unsigned int)std::min<size_t>(cap, 0xFFFFFFFFull);
    if (cloud && cap32 != 0)
      hipLaunchKernelGGL(k_tsdf_points, dim3(nb), dim3(kTsdfBlock), 0, c->stream, c->tsdf, c->tsdf_nvox, (const unsigned int *)counts, cloud, cap32);
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
int tsdf_points_host(cspm_ctx *c, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out) {
  const unsigned nb = tsdf_blocks(c->tsdf_nvox);
  const size_t cap = std::min(cloud_out ? cloud_cap : (size_t)0, 3 * (size_t)c->tsdf_nvox);
  unsigned int total = 0;  // in front of the Staging: a download writes it
  Staging S(c);
  uint4 *dcloud = S.buf<uint4>(2 * cap, cap != 0);
  if (S.rc) return S.finish();
  if (int rc = tsdf_points_enqueue(c, dcloud, cap, nullptr)) return rc;
  S.down(&total, c->tsdf_counts + nb, 1);
  if (S.finish("tsdf: the extraction failed")) return S.rc;
  S.down(cloud_out, dcloud, std::min((size_t)total, cap));
  if (S.finish("tsdf: the download failed")) return S.rc;
  if (count_out) *count_out = total;
  return CSPM_OK;
}
int tsdf_get_volume(cspm_ctx *c, float *D_out, float *W_out, uint8_t *colour_out) {
  const size_t nvox = (size_t)c->tsdf_nvox;
  Staging S(c);
  S.down(D_out, c->tsdf.D, nvox);
  S.down(W_out, c->tsdf.W, nvox);
  S.down(reinterpret_cast<uint32_t *>(colour_out), c->tsdf.C, nvox);
  return S.finish("tsdf: the download failed");
}
int tsdf_set_volume(cspm_ctx *c, const float *D, const float *W, const uint8_t *colour) {
  const size_t nvox = (size_t)c->tsdf_nvox;
  Staging S(c);
  if (D) S.put(c->tsdf.D, D, nvox);
  if (W) S.put(c->tsdf.W, W, nvox);
  if (colour) S.put(c->tsdf.C, reinterpret_cast<const uint32_t *>(colour), nvox);
  if (S.finish("tsdf: the upload failed")) return S.rc;
  if (colour) c->tsdf_coloured = true;
  return CSPM_OK;
}

// MC (cspm_tsdf_mesh.h): the surface points as vertices and the faces over them; every output a device pointer or null
inline size_t tsdf_max_faces(const TsdfVol &V) {
  return V.nx < 2 || V.ny < 2 || V.nz < 2 ? 0 : (size_t)kMcMaxTris * (size_t)(V.nx - 1) * (size_t)(V.ny - 1) * (size_t)(V.nz - 1);
}
int tsdf_mesh_enqueue(cspm_ctx *c, uint4 *verts, size_t vcap, uint32_t *faces, size_t fcap, unsigned int *d_nv, unsigned int *d_nf) {
  const unsigned nb = tsdf_blocks(c->tsdf_nvox);
  int rc;
  if ((rc = dalloc(c, c->mem_tsdf, &c->tsdf_first, (size_t)c->tsdf_nvox)) || (rc = dalloc(c, c->mem_tsdf, &c->tsdf_fcounts, (size_t)nb + 1))) return rc;
  unsigned int *counts = c->tsdf_counts, *fcounts = c->tsdf_fcounts;
  {
    Timed t(c, CSPM_K_MISC, c->tsdf_nvox);
    const dim3 grid(nb), block(kTsdfBlock);
    hipLaunchKernelGGL(k_tsdf_count, grid, block, 0, c->stream, c->tsdf, c->tsdf_nvox, counts);
    hipLaunchKernelGGL(k_tsdf_mesh_count, grid, block, 0, c->stream, c->tsdf, c->tsdf_nvox, fcounts);
    hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, c->stream, counts, (int)nb, d_nv ? d_nv : counts + nb);
    hipLaunchKernelGGL(k_geom_scan, dim3(1), dim3(kGeomScanBlock), 0, c->stream, fcounts, (int)nb, d_nf ? d_nf : fcounts + nb);
    const unsigned int vcap32 = (unsigned int)std::min<size_t>(vcap, 0xFFFFFFFFull), fcap32 = (unsigned int)std::min<size_t>(fcap, 0xFFFFFFFFull);
    if (verts && vcap32 != 0)
      hipLaunchKernelGGL(k_tsdf_points, grid, block, 0, c->stream, c->tsdf, c->tsdf_nvox, (const unsigned int *)counts, verts, vcap32);
    if (faces && fcap32 != 0) {
      hipLaunchKernelGGL(k_tsdf_first, grid, block, 0, c->stream, c->tsdf, c->tsdf_nvox, (const unsigned int *)counts, c->tsdf_first);
      hipLaunchKernelGGL(k_tsdf_mesh_faces, grid, block, 0, c->stream, c->tsdf, c->tsdf_nvox, (const unsigned int *)fcounts, (const unsigned int *)c->tsdf_first,
                         faces, fcap32);
    }
  }
  HIPCHK(c, hipGetLastError());
  return CSPM_OK;
}
int tsdf_mesh_host(cspm_ctx *c, cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap, unsigned int *n_vertices_out,
                   unsigned int *n_faces_out) {
  const unsigned nb = tsdf_blocks(c->tsdf_nvox);
  const size_t vcap = std::min(vertices_out ? vertex_cap : (size_t)0, 3 * (size_t)c->tsdf_nvox);
  const size_t fcap = std::min(faces_out ? face_cap : (size_t)0, tsdf_max_faces(c->tsdf));
  unsigned int nv = 0, nf = 0;  // in front of the Staging: downloads write them
  Staging S(c);
  uint4 *dverts = S.buf<uint4>(2 * vcap, vcap != 0);
  uint32_t *dfaces = S.buf<uint32_t>(3 * fcap, fcap != 0);
  if (S.rc) return S.finish();
  if (int rc = tsdf_mesh_enqueue(c, dverts, vcap, dfaces, fcap, nullptr, nullptr)) return rc;
  S.down(&nv, c->tsdf_counts + nb, 1);
  S.down(&nf, c->tsdf_fcounts + nb, 1);
  if (S.finish("tsdf: the mesh extraction failed")) return S.rc;
  S.down(vertices_out, dverts, std::min((size_t)nv, vcap));  // the counts first, then the records that were written
  S.down(faces_out, dfaces, std::min((size_t)nf, fcap));
  if (S.finish("tsdf: the mesh download failed")) return S.rc;
  if (n_vertices_out) *n_vertices_out = nv;
  if (n_faces_out) *n_faces_out = nf;
  return CSPM_OK;
}

// ---- depth-view registration (cspm_register.h) ---------------------------------------------------------------
static_assert(CSPM_REG_MAX_ITERS == kRegMaxIters, "cspm.h and cspm_register.h agree on the number of iterations");
static_assert(sizeof(RegRec) == sizeof(cspm_reg_iter) && sizeof(RegRec) == 5 * sizeof(double), "an iteration record is 40 bytes on both sides");
const cspm_reg_params kRegDefaults = {8, 1, 0.5, 0.05, 0.0, 100, 1e-8};
const char *reg_params_error(const cspm_reg_params *p) {
  if (p->iters < 1 || p->iters > kRegMaxIters) return "registration: iters must be in 1 .. 64";
  if (p->stride < 1) return "registration: stride must be at least 1";
  if (!(p->max_dist >= 0.0)) return "registration: max_dist must be >= 0";
  if (!(p->huber >= 0.0)) return "registration: huber must be >= 0";
  if (!(p->min_cos >= 0.0 && p->min_cos <= 1.0)) return "registration: min_cos must be in [0, 1]";
  if (p->min_pairs < 0) return "registration: min_pairs must be >= 0";
  if (!(p->pivot_rel >= 0.0 && p->pivot_rel < 1.0)) return "registration: pivot_rel must be in [0, 1)";
  return nullptr;
}
const char *reg_mask_error(int src, unsigned long long targets, int views) {
  if (src < 0 || src >= views) return "registration: no such source view";
  const unsigned long long below = views >= 64 ? ~0ull : (1ull << views) - 1ull;
  if (targets == 0ull || (targets & ~below) || ((targets >> src) & 1ull)) return "registration: the targets must be other views that exist, at least one";
  return nullptr;
}
// the checks of cspm_fuse_register on a context with views; *start = the camera the loop begins with
int reg_check(cspm_ctx *c, int src, unsigned long long targets, const cspm_reg_params **p, const double *R0, const double *t0, FuseCam *start) {
  if (!*p) *p = &kRegDefaults;
  if (const char *msg = reg_params_error(*p)) return fail(c, CSPM_ERR_ARG, msg);
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (const char *msg = reg_mask_error(src, targets, c->fuse_views)) return fail(c, CSPM_ERR_ARG, msg);
  if (!c->fuse_normals) return fail(c, CSPM_ERR_STATE, "registration: the views carry no normals");
  *start = c->fuse_cams_host[(size_t)src];
  if (R0) for (int i = 0; i < 9; ++i) start->R[i] = R0[i];
  if (t0) for (int i = 0; i < 3; ++i) start->t[i] = t0[i];
  if (const char *msg = fuse_camera_error(start->f, start->cx, start->cy, start->R, start->t)) return fail(c, CSPM_ERR_ARG, msg);
  return CSPM_OK;
}
// R behind its checks, on the context's device; *start outlives the call's copies (the caller's local)
int reg_run(cspm_ctx *c, int src, unsigned long long targets, const cspm_reg_params *p, const FuseCam *start, int apply, double *R_out, double *t_out,
            cspm_reg_iter *iters_out) {
  const int w = c->fuse_w, h = c->fuse_h, K = c->fuse_views;
  const long long n = (long long)w * h;
  const int ws = (w + p->stride - 1) / p->stride, hs = (h + p->stride - 1) / p->stride;
  const long long samples = (long long)ws * hs;
  const size_t nb = (size_t)((samples + kRegBlock - 1) / kRegBlock);
  const size_t tail = sizeof(FuseCam) / sizeof(double) + (size_t)kRegMaxIters * sizeof(RegRec) / sizeof(double);
  const size_t all = (size_t)((n + kRegBlock - 1) / kRegBlock);  // the partials of stride 1: every call fits
  if (int rc = dalloc(c, c->mem_fuse, &c->reg_mem, tail + all * kRegSums)) return rc;
  FuseCam *pose = reinterpret_cast<FuseCam *>(c->reg_mem);
  RegRec *recs = reinterpret_cast<RegRec *>(c->reg_mem + sizeof(FuseCam) / sizeof(double));
  double *part = c->reg_mem + tail;
  const RegPar par{p->max_dist * p->max_dist, p->huber, p->min_cos, p->pivot_rel, (double)p->min_pairs, p->stride, ws, samples};
  FuseCam result;                 // in front of the Staging: downloads write them
  RegRec host_recs[kRegMaxIters];
  Staging S(c);
  S.put(pose, start, 1);
  if (S.rc) return S.finish();
  {
    Timed t(c, CSPM_K_MISC, (long long)p->iters * samples * (long long)__builtin_popcountll(targets));
    for (int it = 0; it < p->iters; ++it) {
      hipLaunchKernelGGL(k_reg_pairs, dim3((unsigned)nb), dim3(kRegBlock), 0, c->stream, (const FuseCam *)c->fuse_cams, (const FuseCam *)pose,
                         (const double *)c->fuse_depth, (const double *)c->fuse_normal, K, src, targets, w, h, n, par, part);
      hipLaunchKernelGGL(k_reg_solve, dim3(1), dim3(kRegBlock), 0, c->stream, (const double *)part, (int)nb, par, pose, recs + it);
    }
  }
  S.down(&result, pose, 1);
  S.down(host_recs, recs, (size_t)p->iters);
  if (S.finish("registration kernels failed")) return S.rc;
  if (apply) {
    c->fuse_cams_host[(size_t)src] = result;
    HIPCHK(c, hipMemcpyAsync(c->fuse_cams + src, &c->fuse_cams_host[(size_t)src], sizeof(FuseCam), hipMemcpyHostToDevice, c->stream));
  }
  if (R_out) for (int i = 0; i < 9; ++i) R_out[i] = result.R[i];
  if (t_out) for (int i = 0; i < 3; ++i) t_out[i] = result.t[i];
  if (iters_out) std::memcpy(iters_out, host_recs, sizeof(RegRec) * (size_t)p->iters);
  return CSPM_OK;
}

// ---- plane-field carry (cspm_carry.h) ----------------------------------------------------------------------
const cspm_carry_params kCarryDefaults = {1};
const char *carry_calib_error(const cspm_calib *k, int view) {
  if (!k) return "carry: no calibration";
  if (!std::isfinite(k->f) || !std::isfinite(k->cx) || !std::isfinite(k->cy) || !std::isfinite(k->baseline) || !std::isfinite(k->doffs))
    return "carry: the calibration must be finite";
  if (!(k->f > 0.0) || !(k->baseline > 0.0)) return "carry: f and baseline must be positive";
  if (view < 0 || view > 1) return "carry: view must be 0 or 1";
  return nullptr;
}
const char *carry_motion_error(const double *R, const double *t) {
  if (!R || !t) return "carry: no motion";
  bool finite = true;
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R[i]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(t[i]);
  if (!finite) return "carry: the motion must be finite";
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(d) <= 1e-6)) return "carry: R is not a rotation (max |R R^T - I| > 1e-6)";
    }
  return nullptr;
}
const char *carry_size_error(int w, int h) {
  if (w < 1 || h < 1) return "carry: w and h must be at least 1";
  if ((long long)w * h >= (1LL << 31)) return "carry: w * h must be below 2^31: winners are 32-bit pixel indices";
  return nullptr;
}
const char *carry_params_error(const cspm_carry_params *p) {
  if (p->fill != 0 && p->fill != 1) return "carry: fill must be 0 or 1";
  return nullptr;
}
inline CarryCam carry_cam(const cspm_calib *k, int view) {
  return CarryCam{k->f, k->cx + (double)view * k->doffs, k->cy, k->baseline, k->doffs, k->f * k->baseline};
}
inline CarryPar carry_par(const cspm_calib *sk, int sv, int ws, int hs, const cspm_calib *tk, int tv, int wt, int ht, double max_dis, const double *R,
                          const double *t, const cspm_carry_params *p) {
  CarryPar k{};
  k.s = carry_cam(sk, sv);
  k.t = carry_cam(tk, tv);
  for (int i = 0; i < 9; ++i) k.R[i] = R[i];
  for (int i = 0; i < 3; ++i) k.tr[i] = t[i];
  k.max_dis = max_dis;
  k.ws = ws; k.hs = hs; k.wt = wt; k.ht = ht;
  k.fill = p->fill;
  return k;
}

}  // namespace

// =================================================================================================
extern "C" {

int cspm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cspm_create(cspm_ctx **out, int device) {
  if (!out) return CSPM_ERR_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, CSPM_ERR_HIP, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count=0"));
  if (device < 0 || device >= n) return fail(nullptr, CSPM_ERR_ARG, "device index out of range");
  ON_DEVICE_ID(nullptr, device);
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail(nullptr, CSPM_ERR_HIP, hipGetErrorString(e));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(nullptr, CSPM_ERR_HIP, std::string("libcspm_hip is built for gfx950 only, device is ") + prop.gcnArchName);
  cspm_ctx *c = new cspm_ctx();
  c->device = device;
  c->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char *e = getenv("CSPM_REFINE_CHUNK")) c->refine_chunk = std::max(1, atoi(e));
  if (const char *e = getenv("CSPM_SWEEP_WG")) c->sweep_wg_per_cu = std::max(1, atoi(e));
  if (const char *e = getenv("CSPM_ROW_CLAIM")) c->row_claim = atoi(e) < 0 ? -1 : (atoi(e) ? 1 : 0);
  if (const char *e = getenv("CSPM_SWEEP_BANDS")) c->sweep_bands = std::max(1, std::min(kSweepMaxBands, atoi(e)));
  if (const char *e = getenv("CSPM_SWEEP_PAIRS")) c->opt_sweep_pairs = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_TABLE_VOLUMES")) c->opt_table_volumes = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_TABLE_VOLUMES_MAX_MB")) c->table_volumes_limit = std::max(0LL, atoll(e)) << 20;
  if (const char *e = getenv("CSPM_SWEEP_PACKED")) c->opt_sweep_packed = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_SWEEP_FLOW")) c->opt_sweep_flow = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_VIEW_SORT")) c->opt_view_sort = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_SWEEP_FOLD")) c->opt_sweep_fold = atoi(e) ? 1 : 0;
  if (const char *e = getenv("CSPM_VOLUMES_MEM_FRACTION")) c->volumes_mem_fraction = std::min(1.0, std::max(0.0, atof(e)));
  if (const char *e = getenv("CSPM_SWEEP_PAIRS_MAX_MB")) c->sweep_pairs_limit = std::max(0LL, atoll(e)) << 20;
  if (const char *e = getenv("CSPM_SWEEP_TIMEOUT_MS")) c->sweep_timeout_ms = std::min(3600000LL, std::max(0LL, atoll(e)));
  if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return fail(nullptr, CSPM_ERR_HIP, hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  *out = c;
  return CSPM_OK;
}

void cspm_destroy(cspm_ctx *c) {
  if (!c) return;
  DevGuard guard_(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (auto &r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  free_geometry(c);
  free_rect(c);
  fuse_release(c);
  tsdf_release(c);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char *cspm_last_error(const cspm_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int cspm_set_stream(cspm_ctx *c, void *s) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return CSPM_OK;
}

int cspm_get_stream(cspm_ctx *c, void **out) {
  if (!c || !out) return CSPM_ERR_ARG;
  *out = (void *)c->stream;
  return CSPM_OK;
}

int cspm_synchronize(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  int rc = check_sweep(c);  // also surfaces a timed-out raster sweep of an asynchronous cspm_patchmatch
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CSPM_OK;
}

// The work is enqueued on the ctx stream.  Device sources: the caller orders its producer before this call on the same
// stream (or synchronises); nothing here waits for the host.  Host sources: rows are gathered with a 2-D copy (a padded
// row is never read past 3*w bytes) into a staging buffer the ctx keeps.
static int set_images_impl(cspm_ctx *c, const void *l, const void *r, int w, int h, size_t stride, bool on_device) {
  if (!c) return CSPM_ERR_ARG;
  if (!l || !r || w < 1 || h < 1 || stride < (size_t)w * 3) return fail(c, CSPM_ERR_ARG, "bad image arguments");
  ON_DEVICE(c);
  if (w != c->W || h != c->H) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_geometry(c);
    int rc;
    for (int v = 0; v < 2; ++v)
      if ((rc = dalloc(c, c->mem_images, &c->img0[v], (size_t)w * h))) return rc;
    c->W = w; c->H = h;
  } else {
    c->cost_ready = false;
  }
  c->field_consistent = false;
  c->repeat.taint_unchecked_run();  // its inputs are being replaced
  const void *src[2] = {l, r};
  const size_t row = (size_t)w * 3;
  if (!on_device && c->stage_bytes < 2 * row * h) {
    c->mem_images.drop(&c->stage);
    c->stage_bytes = 0;
    if (int rc = dalloc(c, c->mem_images, &c->stage, 2 * row * h)) return rc;
    c->stage_bytes = 2 * row * h;
  }
  Staging S(c);
  for (int v = 0; v < 2; ++v) {
    uint8_t *staged = on_device ? nullptr : c->stage + (size_t)v * row * h;
    if (staged) S.put2d(staged, row, src[v], stride, row, h);
    if (S.rc) return S.rc;
    Timed t(c, CSPM_K_MISC, 0);
    hipLaunchKernelGGL(k_pack_bgr, dim3(ew_grid((long long)w * h)), dim3(256), 0, c->stream, staged ? staged : (const uint8_t *)src[v], staged ? row : stride, w,
                       h, w, 0, c->img0[v]);
  }
  HIPCHK(c, hipGetLastError());
  return on_device ? CSPM_OK : S.finish("image upload failed");  // the caller may reuse its host buffers
}

int cspm_set_images(cspm_ctx *c, const uint8_t *l, const uint8_t *r, int w, int h, size_t stride) { return set_images_impl(c, l, r, w, h, stride, false); }
int cspm_set_images_device(cspm_ctx *c, const void *l, const void *r, int w, int h, size_t stride) { return set_images_impl(c, l, r, w, h, stride, true); }

int cspm_set_option(cspm_ctx *c, int key, long long value) {
  if (!c) return CSPM_ERR_ARG;
  switch (key) {
    case CSPM_OPT_GRD_VOLUMES: c->opt_grd_volumes = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_RASTER_LAUNCHES: c->opt_raster_launches = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_PAIRS: c->opt_sweep_pairs = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_TABLE_VOLUMES: c->opt_table_volumes = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_PACKED: c->opt_sweep_packed = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_FLOW: c->opt_sweep_flow = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_CENGRD_FUSED: c->opt_cengrd_fused = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_WG: c->sweep_wg_per_cu = value < 0 ? 0 : (value > 16 ? 16 : (int)value); return CSPM_OK;
    case CSPM_OPT_VIEW_SORT: c->opt_view_sort = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_FOLD: c->opt_sweep_fold = value ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_FAULT_VOLUME_ALLOC: c->fault_volume_alloc = value < 0 ? 0 : (int)value; return CSPM_OK;
    case CSPM_OPT_SWEEP_GRID: c->sweep_grid_cap = value < 0 ? 0 : (value > (1LL << 20) ? (1 << 20) : (int)value); return CSPM_OK;
    case CSPM_OPT_VOLUME_RETRY_PAIRS: c->volume_retry_pairs = value < 0 ? 0 : value; return CSPM_OK;
    case CSPM_OPT_SWEEP_TIMEOUT_MS:
      if (value < 0 || value > 3600000) return fail(c, CSPM_ERR_ARG, "sweep timeout out of range");
      c->sweep_timeout_ms = value;
      return CSPM_OK;
    default: return fail(c, CSPM_ERR_ARG, "unknown option");
  }
}

int cspm_set_pp_speckle(cspm_ctx *c, int max_size, double max_diff) {
  if (!c) return CSPM_ERR_ARG;
  if (max_size < 0 || !(max_diff >= 0.0) || !std::isfinite(max_diff)) return fail(c, CSPM_ERR_ARG, "speckle filter: max_size >= 0 and a finite max_diff >= 0");
  c->pp_speckle_size = max_size;
  c->pp_speckle_diff = max_diff;
  return CSPM_OK;
}
int cspm_set_pp_median(cspm_ctx *c, int r) {
  if (!c) return CSPM_ERR_ARG;
  if (r < 0 || r > CSPM_MEDIAN_MAX_RADIUS) return fail(c, CSPM_ERR_ARG, "median filter: radius 0 (off) .. CSPM_MEDIAN_MAX_RADIUS");
  c->pp_median = r;
  return CSPM_OK;
}
int cspm_get_pp_median(cspm_ctx *c, int *r) {
  if (!c || !r) return CSPM_ERR_ARG;
  *r = c->pp_median;
  return CSPM_OK;
}
int cspm_smooth_default_params(cspm_smooth_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kSmoothDefaults;
  return CSPM_OK;
}
int cspm_set_pp_smooth(cspm_ctx *c, const cspm_smooth_params *p) {
  if (!c) return CSPM_ERR_ARG;
  if (!p || p->lambda == 0.0) {  // off: the other values stay as they were
    c->pp_smooth.lambda = 0.0;
    return CSPM_OK;
  }
  if (const char *msg = smooth_params_error(p, true)) return fail(c, CSPM_ERR_ARG, msg);
  c->pp_smooth = *p;
  return CSPM_OK;
}
int cspm_get_pp_smooth(cspm_ctx *c, cspm_smooth_params *p, int *on) {
  if (!c) return CSPM_ERR_ARG;
  if (p) *p = c->pp_smooth;
  if (on) *on = c->pp_smooth.lambda != 0.0;
  return CSPM_OK;
}
int cspm_get_pp_speckle(cspm_ctx *c, int *max_size, double *max_diff) {
  if (!c) return CSPM_ERR_ARG;
  if (max_size) *max_size = c->pp_speckle_size;
  if (max_diff) *max_diff = c->pp_speckle_diff;
  return CSPM_OK;
}

int cspm_get_option(cspm_ctx *c, int key, long long *value) {
  if (!c || !value) return CSPM_ERR_ARG;
  switch (key) {
    case CSPM_OPT_GRD_VOLUMES: *value = c->opt_grd_volumes; return CSPM_OK;
    case CSPM_OPT_RASTER_LAUNCHES: *value = c->opt_raster_launches; return CSPM_OK;
    case CSPM_OPT_SWEEP_TIMEOUT_MS: *value = c->sweep_timeout_ms; return CSPM_OK;
    case CSPM_OPT_SWEEP_FALLBACKS: *value = c->sweep_fallbacks; return CSPM_OK;
    case CSPM_OPT_DEVICE_BYTES:
      *value = (long long)(c->mem_images.bytes() + c->mem_cost.bytes() + c->mem_field.bytes() + c->mem_rect.bytes() + c->mem_ca.bytes() + c->mem_fuse.bytes() + c->mem_tsdf.bytes());
      return CSPM_OK;
    case CSPM_OPT_SWEEP_PAIRS: *value = c->opt_sweep_pairs; return CSPM_OK;
    case CSPM_OPT_TABLE_VOLUMES: *value = c->opt_table_volumes; return CSPM_OK;
    case CSPM_OPT_TABLE_VOLUMES_ACTIVE: *value = (c->cost_alloc && c->cost.lv[0].cvol[0]) ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_SWEEP_PAIRS_ACTIVE: *value = c->sweep_pairs ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_VOLUME_FALLBACKS: *value = c->optional_volume_fallbacks; return CSPM_OK;
    case CSPM_OPT_VOLUME_RETRY_PAIRS: *value = c->volume_retry_pairs; return CSPM_OK;
    case CSPM_OPT_VIEW_SORT: *value = c->opt_view_sort; return CSPM_OK;
    case CSPM_OPT_SWEEP_FOLD: *value = c->opt_sweep_fold; return CSPM_OK;
    case CSPM_OPT_SWEEP_PACKED: *value = c->opt_sweep_packed; return CSPM_OK;
    case CSPM_OPT_SWEEP_FLOW: *value = c->opt_sweep_flow; return CSPM_OK;
    case CSPM_OPT_SWEEP_WG: *value = c->sweep_wg_per_cu; return CSPM_OK;
    case CSPM_OPT_SWEEP_PACKED_ACTIVE: *value = c->sweep_packed ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_CENGRD_FUSED: *value = c->opt_cengrd_fused; return CSPM_OK;
    case CSPM_OPT_CENGRD_FUSED_ACTIVE: *value = (c->cost_alloc && c->cost.fused == kSrcCenGrd) ? 1 : 0; return CSPM_OK;
    case CSPM_OPT_PP_SPECKLE_REMOVED: {  // synchronises: pixels the speckle filter took out of both masks in the last post-processing
      if (c->pp_speckle_size == 0 || !c->speckle_ran || !c->d_speckle) { *value = 0; return CSPM_OK; }  // off, or nothing filtered yet
      DevGuard guard_(c->device);
      if (!guard_.ok) return fail(c, CSPM_ERR_HIP, "hipSetDevice failed");
      if (int rc = check_sweep(c)) return rc;  // a repeated run replays the post-processing behind it: the count is the replay's
      unsigned int removed = 0;
      HIPCHK(c, hipMemcpyAsync(&removed, c->d_speckle + 4 * (size_t)c->W * c->H, sizeof removed, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *value = removed;
      return CSPM_OK;
    }
    case CSPM_OPT_SWEEP_PACKED_BAD: {  // synchronises: gradients the packer could not represent (always 0 for 8-bit images)
      if (!c->cost_alloc || !c->d_px8_bad) { *value = 0; return CSPM_OK; }
      DevGuard guard_(c->device);
      unsigned int bad = 0;
      HIPCHK(c, hipMemcpyAsync(&bad, c->d_px8_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      *value = bad;
      return CSPM_OK;
    }
    default: return fail(c, CSPM_ERR_ARG, "unknown option");
  }
}

// GRD cells: stored as volumes when CSPM_OPT_GRD_VOLUMES, otherwise only their max is reduced and the PatchMatch kernels recompute them
int cspm_build_cost_grd(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  return build_cost(c, kKindGrd, max_dis, wnd_size, scale_num, reg_lambda);
}

// `new PreSSPC/PreCSPC(l, r, max_dis, wnd, [scale_num,] new CenCC, [reg_lambda])`: census volumes of every level
// built on the device (cc/cen_cc.cc:4-137), then read by the PatchMatch kernels like any CCMethod's volumes.
int cspm_build_cost_cen(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  return build_cost(c, kKindCen, max_dis, wnd_size, scale_num, reg_lambda);
}

// CENGRD (include/cspm.h): per level the gradients of cspm_build_cost_grd and the census codes of
// cspm_build_cost_cen, then ONE kernel per view that writes every cell fma(KAPPA, min(H, TAU_CEN), G) and reduces the max.  Volume-sourced
// by default: the PatchMatch kernels, local stereo and cspm_get_cost_slab read the volumes like any CCMethod's.  With CSPM_OPT_CENGRD_FUSED
// the kernel only reduces the max, no volume exists, and the tap engines compute the cells from Level::pc and Level::grd (kSrcCenGrd).
int cspm_build_cost_cengrd(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  return build_cost(c, kKindCenGrd, max_dis, wnd_size, scale_num, reg_lambda);
}

// `new GrdPC(l, r, max_dis, wnd)` (scale_num == 0; plane_cost/grd_pc.cc:11-66) / `new CSPC(l, r, max_dis, wnd, scale_num,
// reg_lambda)` (cspc.cc:11-93): pyramid, 8U gray and its x-gradient per level; no volumes, no CCMethod.  max_cost_ has no
// counterpart in these classes: the "impossible disparity" cost is a constant (grd_pc.cc:131-132, cspc.cc:150-152).
// max_dis > width is refused: HandleBorder (commfunc.h:129-145) wraps a column ONCE, so q_x + q_disp up to width - 1 + max_dis leaves
// ceil_x - width >= width and the reference reads I_ohter_y / G_other_y beyond the row (grd_pc.cc:153-165, cspc.cc:153-166) -- there is
// no value to reproduce.  With max_dis <= width every level stays in range (D_s = floor(D / 2^s) <= W_s = ceil(W / 2^s)).
int cspm_build_cost_img(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  if (!c) return CSPM_ERR_ARG;
  if (c->img0[0] && max_dis > c->W)
    return fail(c, CSPM_ERR_ARG, "cspm_build_cost_img: max_dis must not exceed the image width (the reference's single wrap-around leaves the row)");
  return build_cost(c, kKindImg, max_dis, wnd_size, scale_num, reg_lambda);
}

// ---- rectification (cspm.h "rectification") ----
int cspm_rect_default_params(cspm_rect_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kRectDefaults;
  return CSPM_OK;
}

int cspm_rectify_compute(const cspm_rig *rig, const cspm_rect_params *params, cspm_rectification *rect_out, cspm_calib *calib_out) {
  if (const char *msg = rig_error(rig)) return fail(nullptr, CSPM_ERR_ARG, msg);
  cspm_rectification r;
  if (const char *msg = rect_compute(rig, params ? params : &kRectDefaults, &r)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (rect_out) *rect_out = r;
  if (calib_out) *calib_out = cspm_calib{r.f, r.cx, r.cy, r.baseline, 0.0};
  return CSPM_OK;
}

// R alone on caller memory: the launches cspm_set_rectification and cspm_set_images_raw enqueue, on one view.  Arguments first, then the device.
int cspm_rectify_host(int device, const cspm_rig *rig, const cspm_rectification *rect, int view, const uint8_t *raw, size_t raw_stride, uint8_t *bgr_out,
                      size_t out_stride, double *map_out, uint8_t *valid_out) {
  if (const char *msg = rig_error(rig)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = rect_error(rect)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (view < 0 || view > 1) return fail(nullptr, CSPM_ERR_ARG, "rectification: view must be 0 or 1");
  if (bgr_out && !raw) return fail(nullptr, CSPM_ERR_ARG, "rectification: a remapped image needs the raw image");
  if (bgr_out && raw_stride < (size_t)rig->raw_w * 3) return fail(nullptr, CSPM_ERR_ARG, "rectification: raw_stride is below 3 * raw_w");
  if (bgr_out && out_stride < (size_t)rect->w * 3) return fail(nullptr, CSPM_ERR_ARG, "rectification: out_stride is below 3 * w");
  OneShot S(device);
  const int w = rect->w, h = rect->h, rw = rig->raw_w, rh = rig->raw_h;
  const size_t n = (size_t)w * h, rn = (size_t)rw * rh;
  double *dmap = S.buf<double>(2 * n);
  uint8_t *dvalid = S.buf<uint8_t>(n);
  uint8_t *draw = S.up2d(bgr_out ? raw : nullptr, raw_stride, (size_t)rw * 3, rh);
  uint32_t *dpix = S.buf<uint32_t>(rn, bgr_out != nullptr);
  uint8_t *dout = S.buf<uint8_t>(3 * n, bgr_out != nullptr);
  if (S.rc) return S.finish();
  rect_map_launch(S.c->stream, rect_view(rig, rect, view), w, h, dmap, dvalid);
  if (bgr_out) rect_remap_launch(S.c->stream, draw, (size_t)rw * 3, rw, rh, dpix, dmap, dvalid, w, h, dout, (size_t)w * 3);
  S.down(map_out, dmap, 2 * n);
  S.down(valid_out, dvalid, n);
  S.down2d(bgr_out, out_stride, dout, (size_t)w * 3, h);
  return S.finish("rectification kernels failed");
}

int cspm_set_rectification(cspm_ctx *c, const cspm_rig *rig, const cspm_rectification *rect) {
  if (!c) return CSPM_ERR_ARG;
  if (!rig) {  // back to a context without a rectification
    if (!c->rect_on && !c->rect_map[0]) return CSPM_OK;
    ON_DEVICE(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_rect(c);
    return CSPM_OK;
  }
  if (const char *msg = rig_error(rig)) return fail(c, CSPM_ERR_ARG, msg);
  if (const char *msg = rect_error(rect)) return fail(c, CSPM_ERR_ARG, msg);
  if (c->rect_on && memcmp(&c->rect_rig, rig, sizeof *rig) == 0 && memcmp(&c->rect, rect, sizeof *rect) == 0) return CSPM_OK;  // one rig, many pairs
  ON_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_rect(c);
  const size_t n = (size_t)rect->w * rect->h;
  int rc;
  for (int v = 0; v < 2; ++v)
    if ((rc = dalloc(c, c->mem_rect, &c->rect_map[v], 2 * n)) || (rc = dalloc(c, c->mem_rect, &c->rect_valid[v], n))) {
      free_rect(c);
      return rc;
    }
  {
    Timed t(c, CSPM_K_MISC, 2 * (long long)n);
    for (int v = 0; v < 2; ++v) rect_map_launch(c->stream, rect_view(rig, rect, v), rect->w, rect->h, c->rect_map[v], c->rect_valid[v]);
  }
  HIPCHK(c, hipGetLastError());
  c->rect_rig = *rig;
  c->rect = *rect;
  c->rect_on = true;
  return CSPM_OK;
}

int cspm_get_rect_map(cspm_ctx *c, int view, double *xy_out, uint8_t *valid_out) {
  if (!c) return CSPM_ERR_ARG;
  if (view < 0 || view > 1) return fail(c, CSPM_ERR_ARG, "rectification: view must be 0 or 1");
  if (!c->rect_on) return fail(c, CSPM_ERR_STATE, "no rectification stored (cspm_set_rectification)");
  ON_DEVICE(c);
  const size_t n = (size_t)c->rect.w * c->rect.h;
  Staging S(c);
  S.down(xy_out, c->rect_map[view], 2 * n);
  S.down(valid_out, c->rect_valid[view], n);
  return S.finish("rectification map download failed");
}

// both raw images through the stored maps into the rectified 8UC3 pair, which then takes cspm_set_images_device's path
static int set_images_raw_impl(cspm_ctx *c, const void *l, const void *r, size_t stride, bool on_device) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->rect_on) return fail(c, CSPM_ERR_STATE, "raw images need a stored rectification (cspm_set_rectification)");
  const int rw = c->rect_rig.raw_w, rh = c->rect_rig.raw_h, w = c->rect.w, h = c->rect.h;
  if (!l || !r || stride < (size_t)rw * 3) return fail(c, CSPM_ERR_ARG, "bad raw image arguments: two images with rows of at least 3 * raw_w bytes, the rig's size");
  ON_DEVICE(c);
  const size_t rn = (size_t)rw * rh, n = (size_t)w * h, raw_row = (size_t)rw * 3, row = (size_t)w * 3;
  int rc;
  if ((rc = dalloc(c, c->mem_rect, &c->rect_rawpix, 2 * rn))) return rc;
  if ((rc = dalloc(c, c->mem_rect, &c->rect_out, 2 * 3 * n))) return rc;
  if (!on_device && (rc = dalloc(c, c->mem_rect, &c->rect_stage, 2 * 3 * rn))) return rc;
  const uint8_t *d_src[2] = {(const uint8_t *)l, (const uint8_t *)r};
  const size_t d_stride = on_device ? stride : raw_row;
  Staging S(c);  // a host source: whatever fails behind an upload that was enqueued, the caller may reuse its buffers when this returns
  for (int v = 0; v < 2 && !on_device; ++v) {
    uint8_t *dst = c->rect_stage + (size_t)v * 3 * rn;
    S.put2d(dst, raw_row, d_src[v], stride, raw_row, rh);
    d_src[v] = dst;
  }
  if (S.rc) return S.rc;
  {
    Timed t(c, CSPM_K_MISC, 2 * (long long)n);
    for (int v = 0; v < 2; ++v)
      rect_remap_launch(c->stream, d_src[v], d_stride, rw, rh, c->rect_rawpix + (size_t)v * rn, c->rect_map[v], c->rect_valid[v], w, h,
                        c->rect_out + (size_t)v * 3 * n, row);
  }
  HIPCHK(c, hipGetLastError());
  if ((rc = set_images_impl(c, c->rect_out, c->rect_out + 3 * n, w, h, row, true))) return rc;
  return on_device ? CSPM_OK : S.finish("raw image upload failed");
}

int cspm_set_images_raw(cspm_ctx *c, const uint8_t *l, const uint8_t *r, size_t stride) { return set_images_raw_impl(c, l, r, stride, false); }
int cspm_set_images_raw_device(cspm_ctx *c, const void *l, const void *r, size_t stride) { return set_images_raw_impl(c, l, r, stride, true); }

// CCMethod::buildCV / buildRightCV on host buffers (cc_method.h:31-32): the cells of slabs 0 .. maxDis-1 from CV_64FC3 images
static int build_cv_host(CostKind kind, int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis, int right_view, double *vol_out) {
  if (!l_rgb || !r_rgb || !vol_out || w < 1 || h < 1 || maxDis < 1) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  OneShot S(device);
  cspm_ctx *c = S.c;
  const size_t px = (size_t)w * h;
  const bool need_grd = kind != kKindCen, need_code = kind != kKindGrd;
  double *d[2], *grd[2];
  uint8_t *gray[2];
  uint32_t *code[2];
  const double *src[2] = {l_rgb, r_rgb};
  for (int v = 0; v < 2; ++v) {
    d[v] = S.up(src[v], px * 3);
    grd[v] = S.buf<double>(px, need_grd);
    gray[v] = S.buf<uint8_t>(px, need_code);
    code[v] = S.buf<uint32_t>(px * 3, need_code);
  }
  double *vol = S.buf<double>(px * maxDis);
  // k_grd_volume<SrcF64, false> reduces its max: it gets a zeroed key, the other two kernels none
  unsigned long long *key = S.buf<unsigned long long>(1, kind == kKindGrd);
  if (key) S.fill(key, 0, sizeof *key);
  if (S.rc) return S.finish();
  const dim3 ew(ew_grid((long long)px)), grid(stride_grid((long long)px * maxDis)), block(256);
  for (int v = 0; v < 2; ++v) {
    if (need_grd) hipLaunchKernelGGL(k_gradient<SrcF64>, ew, block, 0, c->stream, SrcF64{d[v], w}, w, h, w, 0, grd[v]);
    if (need_code) {
      hipLaunchKernelGGL(k_gray8<SrcF64>, ew, block, 0, c->stream, SrcF64{d[v], w}, w, h, gray[v]);
      hipLaunchKernelGGL(k_census, ew, block, 0, c->stream, gray[v], w, h, code[v]);
    }
  }
  const SrcF64 l{d[0], w}, r{d[1], w};
  const char *what;
  if (kind == kKindGrd) {
    what = "GRD volume kernel failed";
    hipLaunchKernelGGL((k_grd_volume<SrcF64, false>), grid, block, 0, c->stream, l, r, grd[0], grd[1], w, 0, w, h, 0, maxDis, right_view, vol, key);
  } else if (kind == kKindCen) {
    what = "census volume kernel failed";
    hipLaunchKernelGGL(k_cen_volume, grid, block, 0, c->stream, code[0], code[1], w, h, 0, maxDis, right_view, vol, (unsigned long long *)nullptr);
  } else {
    what = "CENGRD volume kernel failed";
    hipLaunchKernelGGL(k_cengrd_volume<SrcF64>, grid, block, 0, c->stream, l, r, grd[0], grd[1], w, 0, code[0], code[1], w, h, 0, maxDis, right_view, vol,
                       (unsigned long long *)nullptr);
  }
  S.down(vol_out, vol, px * maxDis);
  return S.finish(what);
}

// GrdCC::buildCV / buildRightCV on host buffers
int cspm_grd_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis, int right_view, double *vol_out) {
  return build_cv_host(kKindGrd, device, l_rgb, r_rgb, w, h, maxDis, right_view, vol_out);
}

// CenCC::buildCV / buildRightCV on host buffers (cc_method.h:31-32, cc/cen_cc.cc:4-137)
int cspm_cen_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis, int right_view, double *vol_out) {
  return build_cv_host(kKindCen, device, l_rgb, r_rgb, w, h, maxDis, right_view, vol_out);
}

// CenGrdCC::buildCV / buildRightCV on host buffers: the CENGRD cells (include/cspm.h) from CV_64FC3 images, gradients as
// cspm_grd_build_cv_host derives them, census codes as cspm_cen_build_cv_host does
int cspm_cengrd_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis, int right_view, double *vol_out) {
  return build_cv_host(kKindCenGrd, device, l_rgb, r_rgb, w, h, maxDis, right_view, vol_out);
}

int cspm_begin_cost(cspm_ctx *c, int max_dis, int wnd_size, int scale_num, double reg_lambda) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  int rc = alloc_cost(c, max_dis, wnd_size, scale_num, reg_lambda, true, kKindForeign);
  if (rc) return rc;
  for (int s = 0; s < c->cost.levels; ++s)
    for (int v = 0; v < 2; ++v) {
      const Level &L = c->cost.lv[s];
      HIPCHK(c, hipMemsetAsync((void *)L.vol[v], 0, sizeof(double) * (size_t)(L.D + 1) * L.W * L.H, c->stream));  // Mat::zeros, pre_cs_pc.cc:52
      hipLaunchKernelGGL(k_make_aos, dim3(ew_grid((long long)L.Wp * L.H)), dim3(256), 0, c->stream, L.pix[v], (const double *)nullptr,
                         (long long)L.Wp * L.H, (PixG *)L.px[v]);
    }
  return CSPM_OK;
}

int cspm_upload_cost_slab(cspm_ctx *c, int view, int level, int d, const double *slab, size_t stride_elems) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->cost_alloc || c->cost_key.kind != kKindForeign) return fail(c, CSPM_ERR_STATE, "cspm_begin_cost first");
  if (view < 0 || view > 1 || level < 0 || level >= c->cost.levels || !slab) return fail(c, CSPM_ERR_ARG, "bad view/level/slab");
  const Level &L = c->cost.lv[level];
  if (d < 0 || d > L.D || stride_elems < (size_t)L.W) return fail(c, CSPM_ERR_ARG, "bad slab index or stride");
  ON_DEVICE(c);
  double *dst = (double *)L.vol[view] + (size_t)d * L.W * L.H;
  Staging S(c);
  S.put2d(dst, sizeof(double) * L.W, slab, sizeof(double) * stride_elems, sizeof(double) * L.W, L.H);
  if (S.finish("cost slab upload failed")) return S.rc;  // caller may reuse the slab buffer
  c->cost_ready = false;
  return CSPM_OK;
}

int cspm_finish_cost(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->cost_alloc || c->cost_key.kind != kKindForeign) return fail(c, CSPM_ERR_STATE, "cspm_begin_cost first");
  ON_DEVICE(c);
  HIPCHK(c, hipMemsetAsync(c->d_maxkeys, 0, sizeof(unsigned long long) * 2 * CSPM_MAX_LEVELS, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_maxkeys + 2 * CSPM_MAX_LEVELS, 0xFF, sizeof(unsigned long long) * 2 * CSPM_MAX_LEVELS, c->stream));
  for (int s = 0; s < c->cost.levels; ++s)
    for (int v = 0; v < 2; ++v) {
      const Level &L = c->cost.lv[s];
      const long long cells = (long long)(L.D + 1) * L.W * L.H;
      Timed t(c, CSPM_K_GRD, 0);
      hipLaunchKernelGGL(k_volume_max, dim3(2048), dim3(256), 0, c->stream, L.vol[v], cells, c->d_maxkeys + v * CSPM_MAX_LEVELS + s,
                         c->d_maxkeys + 2 * CSPM_MAX_LEVELS + v * CSPM_MAX_LEVELS + s);
    }
  HIPCHK(c, hipGetLastError());
  c->max_cost_fetched = false;
  return finish_cost(c, true);  // a foreign volume may hold negative cells: the early exit is licensed only when its min is >= 0
}

int cspm_get_levels(const cspm_ctx *c) { return (c && c->cost_alloc) ? c->cost.levels : 0; }

int cspm_get_level_dims(const cspm_ctx *c, int level, int *w, int *h, int *max_disp) {
  if (!c || !c->cost_alloc || level < 0 || level >= c->cost.levels) return CSPM_ERR_ARG;
  if (w) *w = c->cost.lv[level].W;
  if (h) *h = c->cost.lv[level].H;
  if (max_disp) *max_disp = c->cost.lv[level].D;
  return CSPM_OK;
}

int cspm_get_level_image(cspm_ctx *c, int view, int level, uint8_t *out) {
  if (!c || !out) return CSPM_ERR_ARG;
  if (!c->cost_alloc || view < 0 || view > 1 || level < 0 || level >= c->cost.levels) return fail(c, CSPM_ERR_ARG, "bad view/level");
  ON_DEVICE(c);
  const Level &L = c->cost.lv[level];
  const size_t px = (size_t)L.W * L.H;
  Staging S(c);
  uint8_t *tmp = S.buf<uint8_t>(px * 3);
  if (S.rc) return S.finish();
  hipLaunchKernelGGL(k_unpack_bgr, dim3(ew_grid((long long)px)), dim3(256), 0, c->stream, L.pix[view], L.W, L.H, L.Wp, L.pad, tmp);
  S.down(out, tmp, px * 3);
  return S.finish("level image download failed");
}

int cspm_get_cost_slab(cspm_ctx *c, int view, int level, int d, double *out) {
  if (!c || !out) return CSPM_ERR_ARG;
  if (!c->cost_alloc || view < 0 || view > 1 || level < 0 || level >= c->cost.levels) return fail(c, CSPM_ERR_ARG, "bad view/level");
  const Level &L = c->cost.lv[level];
  if (d < 0 || d > L.D) return fail(c, CSPM_ERR_ARG, "bad slab index");
  ON_DEVICE(c);
  const size_t px = (size_t)L.W * L.H;
  Staging S(c);
  const double *src = L.vol[view] ? L.vol[view] + (size_t)d * px : nullptr;
  if (!src) {
    if (c->cost_key.kind == kKindImg) return fail(c, CSPM_ERR_STATE, "GrdPC / CSPC have no cost volumes");
    // fused cost: materialise the requested slab with the volume kernel
    double *tmp = S.buf<double>(px);
    if (S.rc) return S.finish();
    launch_cells(c, level, view, d, 1, tmp, nullptr);
    src = tmp;
  }
  S.down(out, src, px);
  return S.finish("cost slab download failed");
}

int cspm_get_max_cost(cspm_ctx *c, int view, int level, double *out) {
  if (!c || !out) return CSPM_ERR_ARG;
  if (!c->cost_ready || view < 0 || view > 1 || level < 0 || level >= c->cost.levels) return fail(c, CSPM_ERR_STATE, "cost not ready or bad view/level");
  ON_DEVICE(c);
  int rc = fetch_max_cost(c);
  if (rc) return rc;
  *out = c->host_max_cost[view * CSPM_MAX_LEVELS + level];
  return CSPM_OK;
}

int cspm_get_scale_weights(const cspm_ctx *c, double *out) {
  if (!c || !out || !c->cost_alloc) return CSPM_ERR_ARG;
  for (int s = 0; s < c->cost.levels; ++s) out[s] = c->scale_wgt[s];
  return CSPM_OK;
}

// CAMethod::aggreCV on host buffers (ca_method.h:23; BoxCA.cpp, GFCA.cpp, BFCA.cpp): slices 1 .. n_slices-1 filtered in place
int cspm_aggregate_cv_host(int device, int method, const double *guide, int w, int h, int n_slices, double *vol) {
  if (method < CSPM_CA_BOX || method > CSPM_CA_BF) return fail(nullptr, CSPM_ERR_ARG, "unknown aggregation method (CSPM_CA_BOX / GF / BF)");
  if (!guide || !vol || w < 1 || h < 1 || n_slices < 1) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  if (n_slices > 1 && std::min(w, h) < ca_min_size(method))
    return fail(nullptr, CSPM_ERR_ARG, std::string(ca_name(method)) + " needs min(w, h) >= " + std::to_string(ca_min_size(method)) + ", the slabs are " +
                                           std::to_string(w) + "x" + std::to_string(h));
  if (n_slices == 1) return CSPM_OK;
  OneShot S(device);
  cspm_ctx *c = S.c;
  const size_t px = (size_t)w * h;
  const int nb = ca_batch(px);
  std::vector<double> gn(3 * px);  // channel-major, the values as given
  for (size_t i = 0; i < px; ++i)
    for (int k = 0; k < 3; ++k) gn[k * px + i] = guide[3 * i + k];
  CaWork wk;
  if (!S.rc) S.latch(ca_alloc_work(c, px, nb, &wk, S.bufs));
  S.put(wk.gn, gn.data(), 3 * px);
  double *dv = S.up(vol + px, (size_t)(n_slices - 1) * px);
  double *dout = S.buf<double>((size_t)nb * px);
  if (S.rc) return S.finish();
  ca_prepare_guide(c, method, wk, w, h);
  for (int d0 = 0; d0 < n_slices - 1 && !S.rc; d0 += nb) {
    const int n = std::min(nb, n_slices - 1 - d0);
    ca_filter(c, method, wk, w, h, dv + (size_t)d0 * px, n, dout);
    if (hipMemcpyAsync(dv + (size_t)d0 * px, dout, sizeof(double) * n * px, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) S.fail(CSPM_ERR_HIP, "copy failed");
  }
  S.down(vol + px, dv, (size_t)(n_slices - 1) * px);
  return S.finish("aggregation kernels failed");
}

// the speckle filter alone on caller maps: the launches PostProcessing enqueues, on one view
int cspm_filter_speckles_host(int device, const double *disp, const uint8_t *valid, int w, int h, int max_size, double max_diff, uint8_t *valid_out,
                              int32_t *size_out) {
  if (!disp || !valid_out || w < 1 || h < 1 || max_size < 0 || !(max_diff >= 0.0)) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  const long long n = (long long)w * h;
  if (n >= (1LL << 31)) return fail(nullptr, CSPM_ERR_ARG, "w * h must be below 2^31: labels are 32-bit pixel indices");
  OneShot S(device);
  double *dd = S.up(disp, (size_t)n);
  uint8_t *dv = valid ? S.up(valid, (size_t)n) : S.buf<uint8_t>((size_t)n);
  if (!valid) S.fill(dv, 1, (size_t)n);
  int *scratch = S.buf<int>(3 * (size_t)n + 1);  // parents, counts, n(p), the removed-pixel counter
  if (scratch) S.fill(scratch + 3 * n, 0, sizeof(int));
  if (S.rc) return S.finish();
  const double *d[1] = {dd};
  uint8_t *v[1] = {dv};
  speckle_launch<double>(S.c->stream, d, v, 1, w, h, max_size, max_diff, scratch, (unsigned int *)(scratch + 3 * n), scratch + 2 * n);
  S.down(valid_out, dv, (size_t)n);
  S.down(size_out, scratch + 2 * n, (size_t)n);
  return S.finish("speckle filter kernels failed");
}

// the plane fit alone on caller maps: the launch cspm_fit_planes enqueues, on one view
int cspm_fit_default_params(cspm_fit_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kFitDefaults;
  return CSPM_OK;
}

int cspm_fit_planes_host(int device, const double *disp, const uint8_t *valid, const uint8_t *guide_bgr, size_t guide_stride, int w, int h, int max_dis,
                         const cspm_fit_params *p, double *np_out, uint8_t *fitted_out) {
  if (!p) p = &kFitDefaults;
  if (const char *msg = fit_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!disp || !np_out || w < 1 || h < 1 || h > kFitMaxRows || max_dis < 0 || (guide_bgr && guide_stride < (size_t)w * 3))
    return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  OneShot S(device);
  const size_t n = (size_t)w * h;
  const bool guided = guide_bgr && p->use_guide;
  double *dd = S.up(disp, n), *dout = S.buf<double>(6 * n);
  uint8_t *dfit = S.buf<uint8_t>(n), *dv = S.up(valid, n);
  double *dlut = S.up(guided ? fit_lut() : nullptr, (size_t)kFitLut);
  uint32_t *dpix = S.up_bgr(guided ? guide_bgr : nullptr, guide_stride, w, h);
  if (S.rc) return S.finish();
  fit_launch(S.c->stream, FitIn{dd, dv, dpix, dlut}, six_slabs(dout, n).fit_out(dfit, 0), w, h, p, max_dis);
  std::vector<double> hst(6 * n);
  S.down(hst.data(), dout, 6 * n);
  S.down(fitted_out, dfit, n);
  if (S.finish("plane fit kernel failed")) return S.rc;
  interleave_planes(hst.data(), n, np_out);
  return CSPM_OK;
}

// the segmentation and the segment fit alone on caller memory: the launches cspm_segment_planes enqueues, on one view
int cspm_seg_default_params(cspm_seg_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kSegDefaults;
  return CSPM_OK;
}

int cspm_segment_count(int w, int h, int step) {
  if (w < 1 || h < 1 || step < kSegMinStep || step > kSegMaxStep) return CSPM_ERR_ARG;
  const long long K = (long long)((w + step - 1) / step) * ((h + step - 1) / step);
  return K < (1LL << 31) ? (int)K : CSPM_ERR_ARG;
}

int cspm_segment_host(int device, const uint8_t *bgr, size_t stride, int w, int h, const cspm_seg_params *p, int32_t *labels_out, int32_t *centres_out,
                      int32_t *counts_out) {
  if (!p) p = &kSegDefaults;
  if (const char *msg = seg_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!bgr || !labels_out || w < 1 || h < 1 || h > kSegMaxRows || stride < (size_t)w * 3 || (long long)w * h >= (1LL << 31))
    return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  OneShot S(device);
  const size_t n = (size_t)w * h;
  const SegGrid g = seg_grid(w, h, p->step);
  const size_t K = (size_t)g.nx * g.ny;
  uint32_t *dpix = S.up_bgr(bgr, stride, w, h);
  int *dlab = S.buf<int>(n);
  const SegMem m(S.buf<uint8_t>(SegMem::bytes(K)), K);
  if (S.rc) return S.finish();
  seg_segment_launch(S.c->stream, g, dpix, p, dlab, m);
  S.down(labels_out, dlab, n);
  S.down(centres_out, m.cen, 5 * K);
  S.down(counts_out, m.counts, K);
  return S.finish("segmentation kernels failed");
}

int cspm_segment_planes_host(int device, const double *disp, const uint8_t *valid, const int32_t *labels, int w, int h, int max_dis, const cspm_seg_params *p,
                             double *seg_planes_out, int32_t *inliers_out, double *np_out, uint8_t *fitted_out) {
  if (!p) p = &kSegDefaults;
  if (const char *msg = seg_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!disp || !labels || !np_out || w < 1 || h < 1 || max_dis < 0 || (long long)w * h >= (1LL << 31)) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  const SegGrid g = seg_grid(w, h, p->step);
  const size_t n = (size_t)w * h, K = (size_t)g.nx * g.ny;
  for (int y = 0; y < h; ++y)  // the 3 x 3 property: what makes the owners' window scans complete
    for (int x = 0; x < w; ++x) {
      const int32_t k = labels[(size_t)y * w + x];
      if (k < 0 || (size_t)k >= K || std::abs(k % g.nx - x / g.s) > 1 || std::abs(k / g.nx - y / g.s) > 1)
        return fail(nullptr, CSPM_ERR_ARG, "segment planes: a label is no segment of the 3 x 3 cells around its pixel");
    }
  OneShot S(device);
  double *dd = S.up(disp, n), *dout = S.buf<double>(6 * n);
  int *dlab = S.up(labels, n);
  uint8_t *dv = S.up(valid, n), *dfit = S.buf<uint8_t>(n);
  const SegMem m(S.buf<uint8_t>(SegMem::bytes(K)), K);
  if (S.rc) return S.finish();
  seg_fit_launch(S.c->stream, g, SegFitIn{dd, dv, dlab}, p, max_dis, m, six_slabs(dout, n).fit_out(dfit, 0));
  std::vector<double> hst(6 * n), hseg(4 * K);
  S.down(hst.data(), dout, 6 * n);
  S.down(hseg.data(), m.planes, 4 * K);
  S.down(inliers_out, m.inliers, K);
  S.down(fitted_out, dfit, n);
  if (S.finish("segment fit kernels failed")) return S.rc;
  interleave_planes(hst.data(), n, np_out);
  if (seg_planes_out)
    for (size_t k = 0; k < K; ++k) {
      seg_planes_out[3 * k] = hseg[4 * k];
      seg_planes_out[3 * k + 1] = hseg[4 * k + 1];
      seg_planes_out[3 * k + 2] = hseg[4 * k + 3];
    }
  return CSPM_OK;
}

// the median filter alone on caller memory: the launch PostProcessing enqueues, on one image
int cspm_median_filter_u8_host(int device, const uint8_t *src, size_t src_stride, int w, int h, int channels, int r, uint8_t *dst, size_t dst_stride) {
  if (!src || !dst || src == dst || w < 1 || h < 1 || channels < 1 || channels > 4 || r < 1 || r > CSPM_MEDIAN_MAX_RADIUS)
    return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  const size_t row = (size_t)w * channels;
  if (src_stride < row || dst_stride < row) return fail(nullptr, CSPM_ERR_ARG, "a stride is below w * channels");
  OneShot S(device);
  uint8_t *ds = S.up2d(src, src_stride, row, (size_t)h), *dd = S.buf<uint8_t>(row * h);  // packed rows on the device
  if (S.rc) return S.finish();
  const uint8_t *s1[1] = {ds};
  uint8_t *d1[1] = {dd};
  median_launch_u8(S.c->stream, s1, d1, 1, row, row, w, h, channels, r);
  S.down2d(dst, dst_stride, dd, row, (size_t)h);
  return S.finish("median filter kernel failed");
}

int cspm_median_filter_f64_host(int device, const double *src, int w, int h, int r, double *dst) {
  if (!src || !dst || src == dst || w < 1 || h < 1 || r < 1 || r > CSPM_MEDIAN_MAX_RADIUS) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  OneShot S(device);
  const size_t n = (size_t)w * h;
  double *ds = S.up(src, n), *dd = S.buf<double>(n);
  if (S.rc) return S.finish();
  const double *s1[1] = {ds};
  double *d1[1] = {dd};
  median_launch_f64(S.c->stream, s1, d1, 1, w, h, r);
  S.down(dst, dd, n);
  return S.finish("median filter kernel failed");
}

// the smoother alone on caller memory: the launches PostProcessing enqueues, on one view
int cspm_smooth_disparity_host(int device, const double *disp, const double *conf, const uint8_t *guide_bgr, int w, int h, const cspm_smooth_params *p,
                               int max_dis, double *out) {
  if (!p) p = &kSmoothDefaults;
  if (const char *msg = smooth_params_error(p, false)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!disp || !out || out == disp || w < 1 || h < 1 || max_dis < 0) return fail(nullptr, CSPM_ERR_ARG, "bad arguments");
  const size_t n = (size_t)w * h;
  if (conf)
    for (size_t i = 0; i < n; ++i)
      if (!(conf[i] >= 0.0 && conf[i] <= 1.0)) return fail(nullptr, CSPM_ERR_ARG, "smoothing: a confidence outside [0, 1] or a NaN");
  OneShot S(device);
  std::vector<double> lut(kSmLut);
  smooth_lut_fill(p->sigma_color, lut.data());
  double *dd = S.up(disp, n), *work = S.buf<double>(3 * n), *dconf = S.up(conf, n);
  double *dlut = S.up(guide_bgr ? lut.data() : nullptr, (size_t)kSmLut);
  uint32_t *dpix = S.up_bgr(guide_bgr, (size_t)w * 3, w, h);
  if (S.rc) return S.finish();
  SmoothPair s;
  s.v[0] = s.v[1] = SmoothView{work, work + n, work + 2 * n, dpix};
  s.Wp = w;
  s.pad = 0;
  const SmoothConf cf{{dconf, dconf}, {nullptr, nullptr}, 0.0};
  double *d1[1] = {dd};
  smooth_launch(S.c->stream, d1, cf, s, 1, w, h, p, (double)max_dis, dlut);
  S.down(out, dd, n);
  return S.finish("smoothing kernels failed");
}

// local stereo over the ctx's cost object (cspm.h): asynchronous on the ctx stream like cspm_patchmatch
int cspm_local_stereo(cspm_ctx *c, int method) {
  if (!c) return CSPM_ERR_ARG;
  if (method < CSPM_CA_BOX || method > CSPM_CA_BF) return fail(c, CSPM_ERR_ARG, "unknown aggregation method (CSPM_CA_BOX / GF / BF)");
  if (!c->cost_alloc || !c->cost_ready) return fail(c, CSPM_ERR_STATE, "local stereo needs a cost object (cspm_build_cost_grd / _cen / _cengrd / cspm_finish_cost)");
  if (c->cost_key.kind == kKindImg) return fail(c, CSPM_ERR_STATE, "GrdPC / CSPC costs have no cost cells to aggregate");
  const Cost &cd = c->cost;
  if (cd.lv[0].D < 2) return fail(c, CSPM_ERR_ARG, "local stereo needs max_dis >= 2");
  for (int s = 0; s < cd.levels; ++s)
    if (cd.lv[s].D >= 1 && std::min(cd.lv[s].W, cd.lv[s].H) < ca_min_size(method))
      return fail(c, CSPM_ERR_ARG, std::string(ca_name(method)) + " needs min(w, h) >= " + std::to_string(ca_min_size(method)) + "; level " +
                                       std::to_string(s) + " is " + std::to_string(cd.lv[s].W) + "x" + std::to_string(cd.lv[s].H));
  ON_DEVICE(c);
  int rc;
  if ((rc = ensure_field(c)) || (rc = ca_ensure(c))) return rc;
  c->field_consistent = false;  // min_cost is the local-stereo cost, not the plane cost of this cost object
  c->repeat.taint_unchecked_run();  // it can no longer be repeated over these planes
  for (int v = 0; v < 2; ++v)
    if ((rc = ca_local_view(c, method, v))) return rc;
  return CSPM_OK;
}

int cspm_plane_cost_batch(cspm_ctx *c, int view, int n, const int *xy, const double *np, double *out) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->cost_ready) return fail(c, CSPM_ERR_STATE, "no plane cost built");
  if (view < 0 || view > 1 || n < 0 || (n && (!xy || !np || !out))) return fail(c, CSPM_ERR_ARG, "bad arguments");
  if (n == 0) return CSPM_OK;
  for (int i = 0; i < n; ++i)
    if (xy[2 * i] < 0 || xy[2 * i] >= c->W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= c->H) return fail(c, CSPM_ERR_ARG, "pixel outside the image");
  ON_DEVICE(c);
  Staging S(c);
  int *dxy = S.buf<int>((size_t)2 * n);
  double *dnp = S.buf<double>((size_t)6 * n), *dout = S.buf<double>((size_t)n);
  S.put(dxy, xy, (size_t)2 * n);
  S.put(dnp, np, (size_t)6 * n);
  if (S.rc) return S.finish();
  LAUNCH_CS(k_cost_batch, dim3(eval_grid(n)), dim3(kEvalBlock), 0, c->cost, view, n, dxy, dnp, dout);
  S.down(out, dout, (size_t)n);
  return S.finish("plane cost batch failed");
}

int cspm_pm_default_params(cspm_pm_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kDefaultParams;
  return CSPM_OK;
}

#define PM_ENTER()                                                            \
  if (!c) return CSPM_ERR_ARG;                                                \
  ON_DEVICE(c);                                                               \
  int rc = check_pm(c, &p);                                                   \
  if (rc) return rc

int cspm_pm_init(cspm_ctx *c, const cspm_pm_params *p) {
  PM_ENTER();
  c->repeat.taint();
  return do_init(c, p);
}
int cspm_pm_spatial(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  PM_ENTER();
  c->repeat.taint();
  if ((rc = do_spatial(c, iter, p))) return rc;
  return check_sweep(c);
}
int cspm_pm_view(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  PM_ENTER();
  c->repeat.taint();
  return do_view(c, iter, p);
}
int cspm_pm_refine(cspm_ctx *c, int iter, const cspm_pm_params *p) {
  PM_ENTER();
  c->repeat.taint();
  return do_refine(c, iter, p);
}

// Asynchronous: everything is enqueued on the ctx stream and the call returns.  A raster sweep that timed out is
// reported by the next synchronising call (cspm_synchronize or any getter).
int cspm_patchmatch(cspm_ctx *c, int iter_num, const cspm_pm_params *p) {
  PM_ENTER();
  if (iter_num < 0 || iter_num > 15) return fail(c, CSPM_ERR_ARG, "iter_num out of range");
  c->repeat.begin_run(false, iter_num, *p);
  return run_patchmatch(c, iter_num, p);
}

int cspm_rescore_planes(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  int rc;
  if ((rc = need_cost(c)) || (rc = need_field(c, "no plane field to re-score"))) return rc;
  ON_DEVICE(c);
  c->repeat.taint();
  return do_rescore(c);
}

// Asynchronous like cspm_patchmatch.  The starting field (re-scored when it is not consistent) is copied aside first, so that a
// persistent sweep that times out can be repeated from it by the next synchronising call.
int cspm_patchmatch_warm(cspm_ctx *c, int iter_num, const cspm_pm_params *p) {
  if (!c) return CSPM_ERR_ARG;
  if (int e = need_cost(c)) return e;
  if (int e = need_field(c, "no plane field to start from (cspm_set_planes, cspm_local_stereo, cspm_upsample_planes or an earlier run)")) return e;
  PM_ENTER();
  if (iter_num < 0 || iter_num > 15) return fail(c, CSPM_ERR_ARG, "iter_num out of range");
  if ((rc = ensure_consistent(c)) || (rc = warm_snapshot(c, true))) return rc;
  c->repeat.begin_run(true, iter_num, *p);
  return run_iterations(c, iter_num, p);
}

int cspm_upsample_planes(cspm_ctx *dst, cspm_ctx *src) {
  if (!dst || !src || dst == src) return CSPM_ERR_ARG;
  if (dst->device != src->device) return fail(dst, CSPM_ERR_ARG, "the two contexts are on different devices");
  if (!src->field_alloc) return fail(dst, CSPM_ERR_STATE, "the source context has no plane field");
  if (!dst->img0[0]) return fail(dst, CSPM_ERR_STATE, "cspm_set_images first");
  if (src->W != (dst->W + 1) / 2 || src->H != (dst->H + 1) / 2)
    return fail(dst, CSPM_ERR_ARG, "the source is " + std::to_string(src->W) + "x" + std::to_string(src->H) + ", one pyramid level below " +
                                       std::to_string(dst->W) + "x" + std::to_string(dst->H) + " is " + std::to_string((dst->W + 1) / 2) + "x" +
                                       std::to_string((dst->H + 1) / 2));
  ON_DEVICE(dst);
  int rc;
  if ((rc = source_check(dst, src)) || (rc = ensure_field(dst))) return rc;
  return with_source(dst, src, "cspm_upsample_planes", [&] {
    Timed t(dst, CSPM_K_MISC, 0);
    const long long n = (long long)dst->W * dst->H;
    for (int v = 0; v < 2; ++v)
      hipLaunchKernelGGL(k_upsample_planes, dim3(ew_grid(n)), dim3(256), 0, dst->stream, dst->f[v], src->f[v], dst->W, dst->H, src->W);
    dst->field_consistent = false;  // min_cost is stale until a re-score (cspm_patchmatch_warm does one)
    dst->repeat.taint_unchecked_run();
    return CSPM_OK;
  });
}

inline SnapField snap_of(const Field &f) { return SnapField{f.nx, f.ny, f.nz, f.a, f.b, f.c}; }

int cspm_merge_planes(cspm_ctx *dst, cspm_ctx *src) {
  if (!dst || !src || dst == src) return dst ? fail(dst, CSPM_ERR_ARG, "cspm_merge_planes needs two different contexts") : CSPM_ERR_ARG;
  if (dst->device != src->device) return fail(dst, CSPM_ERR_ARG, "the two contexts are on different devices");
  if (!src->field_alloc) return fail(dst, CSPM_ERR_STATE, "the source context has no plane field");
  if (!dst->img0[0]) return fail(dst, CSPM_ERR_STATE, "cspm_set_images first");
  if (int e = need_cost(dst)) return e;
  if (int e = need_field(dst, kNoMergeTarget)) return e;
  if (src->W != dst->W || src->H != dst->H)
    return fail(dst, CSPM_ERR_ARG, "the source is " + std::to_string(src->W) + "x" + std::to_string(src->H) + ", the destination " +
                                       std::to_string(dst->W) + "x" + std::to_string(dst->H));
  ON_DEVICE(dst);
  int rc;
  if ((rc = source_check(dst, src)) || (rc = ensure_consistent(dst))) return rc;
  return with_source(dst, src, "cspm_merge_planes", [&] {
    const CandField cf{{snap_of(src->f[0]), snap_of(src->f[1])}, {nullptr, nullptr}};
    dst->repeat.taint_unchecked_run();  // it can no longer be repeated over these planes
    return do_merge(dst, &cf, &kDefaultParams, 0, 2, 2LL * dst->W * dst->H);
  });
}

int cspm_merge_planes_host(cspm_ctx *c, int view, const double *np, const uint8_t *mask) {
  if (!c) return CSPM_ERR_ARG;
  if (view < 0 || view > 1 || !np) return fail(c, CSPM_ERR_ARG, "cspm_merge_planes_host: bad view or no candidate field");
  int rc;
  if ((rc = need_cost(c)) || (rc = need_field(c, kNoMergeTarget))) return rc;
  ON_DEVICE(c);
  const size_t n = (size_t)c->W * c->H;
  CandBuf cand;
  if ((rc = ensure_cand(c, &cand))) return rc;
  std::vector<double> h(6 * n);
  deinterleave_planes(np, n, h.data());
  long long evals = 0;  // pixels that have a candidate
  for (size_t i = 0; i < n; ++i) evals += (!mask || mask[i] != 0) && all_finite(np + 6 * i, 6);
  // the copies out of caller memory are complete when the call returns; the merge itself is asynchronous
  Staging S(c);
  S.put(c->cand_mem, h.data(), 6 * n);
  if (mask) S.put(cand.mask, mask, n);
  if (S.finish("candidate upload failed")) return S.rc;
  if ((rc = ensure_consistent(c))) return rc;
  const CandField cf = cand.field(view, mask != nullptr);
  c->repeat.taint_unchecked_run();
  return do_merge(c, &cf, &kDefaultParams, view, 1, evals);
}

// slanted planes fitted to the stored field's own disparity maps (cspm.h "plane fitting"); asynchronous on the ctx stream
int cspm_fit_planes(cspm_ctx *c, const cspm_fit_params *p, int merge) {
  if (!c) return CSPM_ERR_ARG;
  if (!p) p = &kFitDefaults;
  if (const char *msg = fit_params_error(p)) return fail(c, CSPM_ERR_ARG, msg);
  return fit_stored_field(
      c, merge, kFitMaxRows, "image too high for the plane fit",
      [&](double **snap) -> int {
        const size_t n = (size_t)c->W * c->H;
        if (!c->fit_mem) {
          if (int rc = dalloc(c, c->mem_field, &c->fit_mem, 2 * n + kFitLut)) return rc;
          HIPCHK(c, hipMemcpyAsync(c->fit_mem + 2 * n, fit_lut(), sizeof(double) * kFitLut, hipMemcpyHostToDevice, c->stream));
        }
        *snap = c->fit_mem;
        return CSPM_OK;
      },
      [&](int v, const double *d, const FitOut &out) {
        fit_launch(c->stream, FitIn{d, nullptr, c->img0[v], c->fit_mem + 2 * (size_t)c->W * c->H}, out, c->W, c->H, p, c->max_dis);
      });
}

// seg_mem: both views' disparity snapshots (2n doubles), then view v's n labels; seg_labels(c, 2) is where the SegMem begins
inline int *seg_labels(cspm_ctx *c, int v) { return reinterpret_cast<int *>(reinterpret_cast<double *>(c->seg_mem) + 2 * (size_t)c->W * c->H) + (size_t)v * c->W * c->H; }

// one robustly fitted plane per superpixel of the stored field's own disparity maps (cspm.h "segment planes"); asynchronous on the ctx stream
int cspm_segment_planes(cspm_ctx *c, const cspm_seg_params *p, int merge) {
  if (!c) return CSPM_ERR_ARG;
  if (!p) p = &kSegDefaults;
  if (const char *msg = seg_params_error(p)) return fail(c, CSPM_ERR_ARG, msg);
  return fit_stored_field(
      c, merge, kSegMaxRows, "image too high for the segmentation",
      [&](double **snap) -> int {
        const size_t n = (size_t)c->W * c->H;
        const SegGrid finest = seg_grid(c->W, c->H, kSegMinStep);
        const size_t Kmax = (size_t)finest.nx * finest.ny;
        if (!c->seg_mem)
          if (int rc = dalloc(c, c->mem_field, &c->seg_mem, 2 * n * (sizeof(double) + sizeof(int)) + SegMem::bytes(Kmax))) return rc;
        *snap = reinterpret_cast<double *>(c->seg_mem);
        return CSPM_OK;
      },
      [&](int v, const double *d, const FitOut &out) {
        const SegGrid g = seg_grid(c->W, c->H, p->step);
        int *lab = seg_labels(c, v);
        const SegMem m(seg_labels(c, 2), (size_t)g.nx * g.ny);  // 8-byte aligned: 2n ints behind 2n doubles
        c->seg_ran = true;
        seg_segment_launch(c->stream, g, c->img0[v], p, lab, m);
        seg_fit_launch(c->stream, g, SegFitIn{d, nullptr, lab}, p, c->max_dis, m, out);
      });
}

int cspm_get_segments(cspm_ctx *c, int view, int32_t *labels_out) {
  if (!c || view < 0 || view > 1 || !labels_out) return CSPM_ERR_ARG;
  if (!c->seg_mem || !c->seg_ran) return fail(c, CSPM_ERR_STATE, "no segmentation yet (cspm_segment_planes)");
  ON_DEVICE(c);
  Staging S(c);
  S.down(labels_out, seg_labels(c, view), (size_t)c->W * c->H);
  return S.finish("label download failed");
}

// G alone on caller maps: the launches cspm_reproject enqueues, on one view.  Arguments first, then the device.
int cspm_geom_default_params(cspm_geom_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kGeomDefaults;
  return CSPM_OK;
}

int cspm_reproject_host(int device, const cspm_calib *calib, const cspm_geom_params *g, int view, const double *disp, const uint8_t *valid, const double *slope_a,
                        const double *slope_b, const uint8_t *bgr, size_t bgr_stride, int w, int h, double *depth_out, double *xyz_out, double *normal_out,
                        uint8_t *keep_out, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out) {
  if (!g) g = &kGeomDefaults;
  if (const char *msg = geom_args_error(calib, g, view)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!disp || w < 1 || h < 1) return fail(nullptr, CSPM_ERR_ARG, "reprojection: no disparity map or an empty one");
  if ((long long)w * h >= (1LL << 31)) return fail(nullptr, CSPM_ERR_ARG, "w * h must be below 2^31: cloud records hold 32-bit pixel indices");
  if ((slope_a == nullptr) != (slope_b == nullptr)) return fail(nullptr, CSPM_ERR_ARG, "reprojection: the two slope maps come together or not at all");
  if (normal_out && !slope_a) return fail(nullptr, CSPM_ERR_ARG, "reprojection: normals need the slope maps");
  if (bgr && bgr_stride < (size_t)w * 3) return fail(nullptr, CSPM_ERR_ARG, "reprojection: bgr_stride is below 3 * w");
  OneShot S(device);
  const size_t n = (size_t)w * h;
  const unsigned nb = geom_blocks((long long)n);
  const size_t cap = std::min(cloud_out ? cloud_cap : (size_t)0, n);
  unsigned int *dcounts = S.buf<unsigned int>((size_t)nb + 1);
  double *ddepth = S.buf<double>(n, depth_out != nullptr), *dxyz = S.buf<double>(3 * n, xyz_out != nullptr);
  double *dnormal = S.buf<double>(3 * n, normal_out != nullptr);
  uint8_t *dkeep = S.buf<uint8_t>(n, keep_out != nullptr);
  uint4 *dcloud = S.buf<uint4>(2 * cap, cap != 0);
  double *dd = S.up(disp, n);
  uint8_t *dv = S.up(valid, n);
  double *da = S.up(slope_a, n), *db = S.up(slope_b, n);
  uint32_t *dpix = S.up_bgr(bgr, bgr_stride, w, h);
  if (S.rc) return S.finish();
  const bool want_count = count_out != nullptr || cloud_out != nullptr;
  geom_launch(S.c->stream, geom_cam(calib, g, view), GeomIn{dd, dv, da, db, nullptr, dpix}, GeomOut{ddepth, dxyz, dnormal, dkeep}, w, h, dcloud, cap, want_count,
              dcounts, nullptr);
  unsigned int total = 0;
  S.down(depth_out, ddepth, n);
  S.down(xyz_out, dxyz, 3 * n);
  S.down(normal_out, dnormal, 3 * n);
  S.down(keep_out, dkeep, n);
  S.down(want_count ? &total : nullptr, dcounts + nb, 1);
  if (S.finish("reprojection kernels failed")) return S.rc;
  S.down(cloud_out, dcloud, std::min((size_t)total, cap));  // the count first, then the records that were written
  if (S.finish("cloud download failed")) return S.rc;
  if (count_out) *count_out = total;
  return CSPM_OK;
}

// G on one view of the stored field (cspm.h "reprojection"): synchronous, host outputs
int cspm_reproject(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, double *depth_out,
                   double *xyz_out, double *normal_out, uint8_t *keep_out, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = reproject_check(c, view, source, calib, &g, fit);
  if (rc) return rc;
  ON_DEVICE(c);
  const size_t n = (size_t)c->W * c->H;
  const unsigned nb = geom_blocks((long long)n);
  const size_t cap = std::min(cloud_out ? cloud_cap : (size_t)0, n);
  unsigned int total = 0;  // in front of the Staging: a download writes it
  Staging S(c);
  double *ddepth = S.buf<double>(n, depth_out != nullptr), *dxyz = S.buf<double>(3 * n, xyz_out != nullptr), *dnormal = S.buf<double>(3 * n, normal_out != nullptr);
  uint8_t *dkeep = S.buf<uint8_t>(n, keep_out != nullptr);
  uint4 *dcloud = S.buf<uint4>(2 * cap, cap != 0);
  if (S.rc) return S.finish();
  const bool want_count = count_out != nullptr || cloud_out != nullptr;
  if ((rc = reproject_enqueue(c, view, source, calib, g, fit, GeomOut{ddepth, dxyz, dnormal, dkeep}, dcloud, cap, want_count, nullptr))) return rc;
  S.down(depth_out, ddepth, n);
  S.down(xyz_out, dxyz, 3 * n);
  S.down(normal_out, dnormal, 3 * n);
  S.down(keep_out, dkeep, n);
  S.down(want_count ? &total : nullptr, c->geom_counts + nb, 1);
  if (S.finish("reprojection download failed")) return S.rc;
  S.down(cloud_out, dcloud, std::min((size_t)total, cap));  // the count first, then the records that were written
  if (S.finish("cloud download failed")) return S.rc;
  if (count_out) *count_out = total;
  return CSPM_OK;
}

// the same with device-resident outputs: asynchronous on the ctx stream behind the pending-run check; not replayed (cspm.h)
int cspm_reproject_device(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, void *d_depth_out,
                          void *d_xyz_out, void *d_normal_out, void *d_keep_out, void *d_cloud_out, size_t cloud_cap, void *d_count_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = reproject_check(c, view, source, calib, &g, fit);
  if (rc) return rc;
  if (d_cloud_out && ((uintptr_t)d_cloud_out & 15u)) return fail(c, CSPM_ERR_ARG, "reprojection: the cloud buffer must be 16-byte aligned");
  ON_DEVICE(c);
  return reproject_enqueue(c, view, source, calib, g, fit, GeomOut{(double *)d_depth_out, (double *)d_xyz_out, (double *)d_normal_out, (uint8_t *)d_keep_out},
                           (uint4 *)d_cloud_out, d_cloud_out ? cloud_cap : 0, d_count_out != nullptr || d_cloud_out != nullptr, (unsigned int *)d_count_out);
}

// M alone on caller maps: the launches cspm_mesh enqueues, on one view.  Arguments first, then the device.
int cspm_mesh_default_params(cspm_mesh_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kMeshDefaults;
  return CSPM_OK;
}

int cspm_mesh_host(int device, const cspm_calib *calib, const cspm_geom_params *g, const cspm_mesh_params *m, int view, const double *disp, const uint8_t *valid,
                   const double *slope_a, const double *slope_b, const uint8_t *bgr, size_t bgr_stride, int w, int h, cspm_point *vertices_out, size_t vertex_cap,
                   cspm_face *faces_out, size_t face_cap, uint8_t *quad_out, unsigned int *n_vertices_out, unsigned int *n_faces_out) {
  if (!g) g = &kGeomDefaults;
  if (!m) m = &kMeshDefaults;
  if (const char *msg = geom_args_error(calib, g, view)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = mesh_args_error(m)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (!disp || w < 1 || h < 1) return fail(nullptr, CSPM_ERR_ARG, "mesh: no disparity map or an empty one");
  if ((long long)w * h >= (1LL << 31)) return fail(nullptr, CSPM_ERR_ARG, "w * h must be below 2^31: vertex records hold 32-bit pixel indices");
  if ((slope_a == nullptr) != (slope_b == nullptr)) return fail(nullptr, CSPM_ERR_ARG, "mesh: the two slope maps come together or not at all");
  if (bgr && bgr_stride < (size_t)w * 3) return fail(nullptr, CSPM_ERR_ARG, "mesh: bgr_stride is below 3 * w");
  OneShot S(device);
  const size_t n = (size_t)w * h;
  const unsigned nb = geom_blocks((long long)n);
  const size_t vcap = std::min(vertices_out ? vertex_cap : (size_t)0, n), fcap = std::min(faces_out ? face_cap : (size_t)0, mesh_max_faces(w, h));
  uint8_t *dbytes = S.buf<uint8_t>(2 * n);
  uint32_t *dmap = S.buf<uint32_t>(n + mesh_count_words(nb));
  uint4 *dverts = S.buf<uint4>(2 * vcap, vcap != 0);
  uint32_t *dfaces = S.buf<uint32_t>(3 * fcap, fcap != 0);
  double *dd = S.up(disp, n);
  uint8_t *dv = S.up(valid, n);
  double *da = S.up(slope_a, n), *db = S.up(slope_b, n);
  uint32_t *dpix = S.up_bgr(bgr, bgr_stride, w, h);
  if (S.rc) return S.finish();
  unsigned int *dcounts = dmap + n;
  mesh_launch(S.c->stream, geom_cam(calib, g, view), GeomIn{dd, dv, da, db, nullptr, dpix}, m, w, h, MeshMaps{dbytes, dbytes + n, dmap}, dcounts, dverts, vcap,
              dfaces, fcap, nullptr, nullptr);
  unsigned int nv = 0, nf = 0;
  S.down(quad_out, dbytes + n, n);
  S.down(&nv, dcounts + nb, 1);
  S.down(&nf, dcounts + 2 * (size_t)nb + 1, 1);
  if (S.finish("mesh kernels failed")) return S.rc;
  S.down(vertices_out, dverts, std::min((size_t)nv, vcap));  // the counts first, then the records that were written
  S.down(faces_out, dfaces, std::min((size_t)nf, fcap));
  if (S.finish("mesh download failed")) return S.rc;
  if (n_vertices_out) *n_vertices_out = nv;
  if (n_faces_out) *n_faces_out = nf;
  return CSPM_OK;
}

// M on one view of the stored field (cspm.h "triangle meshes"): synchronous, host outputs
int cspm_mesh(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, const cspm_mesh_params *m,
              cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap, uint8_t *quad_out, unsigned int *n_vertices_out,
              unsigned int *n_faces_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = mesh_check(c, view, source, calib, &g, fit, &m);
  if (rc) return rc;
  ON_DEVICE(c);
  const size_t n = (size_t)c->W * c->H;
  const unsigned nb = geom_blocks((long long)n);
  const size_t vcap = std::min(vertices_out ? vertex_cap : (size_t)0, n), fcap = std::min(faces_out ? face_cap : (size_t)0, mesh_max_faces(c->W, c->H));
  unsigned int nv = 0, nf = 0;  // in front of the Staging: downloads write them
  Staging S(c);
  uint4 *dverts = S.buf<uint4>(2 * vcap, vcap != 0);
  uint32_t *dfaces = S.buf<uint32_t>(3 * fcap, fcap != 0);
  if (S.rc) return S.finish();
  if ((rc = mesh_enqueue(c, view, source, calib, g, fit, m, dverts, vcap, dfaces, fcap, nullptr, nullptr, nullptr))) return rc;
  const unsigned int *dcounts = c->mesh_map + n;
  S.down(quad_out, c->mesh_bytes + n, n);
  S.down(&nv, dcounts + nb, 1);
  S.down(&nf, dcounts + 2 * (size_t)nb + 1, 1);
  if (S.finish("mesh download failed")) return S.rc;
  S.down(vertices_out, dverts, std::min((size_t)nv, vcap));  // the counts first, then the records that were written
  S.down(faces_out, dfaces, std::min((size_t)nf, fcap));
  if (S.finish("mesh record download failed")) return S.rc;
  if (n_vertices_out) *n_vertices_out = nv;
  if (n_faces_out) *n_faces_out = nf;
  return CSPM_OK;
}

// the same with device-resident outputs: asynchronous on the ctx stream behind the pending-run check; not replayed (cspm.h)
int cspm_mesh_device(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit,
                     const cspm_mesh_params *m, void *d_vertices_out, size_t vertex_cap, void *d_faces_out, size_t face_cap, void *d_quad_out,
                     void *d_n_vertices_out, void *d_n_faces_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = mesh_check(c, view, source, calib, &g, fit, &m);
  if (rc) return rc;
  if (d_vertices_out && ((uintptr_t)d_vertices_out & 15u)) return fail(c, CSPM_ERR_ARG, "mesh: the vertex buffer must be 16-byte aligned");
  if (d_faces_out && ((uintptr_t)d_faces_out & 3u)) return fail(c, CSPM_ERR_ARG, "mesh: the face buffer must be 4-byte aligned");
  if ((d_n_vertices_out && ((uintptr_t)d_n_vertices_out & 3u)) || (d_n_faces_out && ((uintptr_t)d_n_faces_out & 3u)))
    return fail(c, CSPM_ERR_ARG, "mesh: the counts must be 4-byte aligned");
  ON_DEVICE(c);
  return mesh_enqueue(c, view, source, calib, g, fit, m, (uint4 *)d_vertices_out, d_vertices_out ? vertex_cap : 0, (uint32_t *)d_faces_out,
                      d_faces_out ? face_cap : 0, (uint8_t *)d_quad_out, (unsigned int *)d_n_vertices_out, (unsigned int *)d_n_faces_out);
}

// F: the fusion views of a context, and the one-shot form on caller maps
int cspm_fuse_default_params(cspm_fuse_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kFuseDefaults;
  return CSPM_OK;
}

int cspm_fuse_begin(cspm_ctx *c, int w, int h, int max_views) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  return fuse_begin(c, w, h, max_views);
}

int cspm_fuse_end(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  ON_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  fuse_release(c);
  return CSPM_OK;
}

int cspm_fuse_view_count(const cspm_ctx *c) { return c && c->fuse_on ? c->fuse_views : -1; }

int cspm_fuse_push_maps(cspm_ctx *c, const double *depth, const double *normal, const uint8_t *bgr, size_t bgr_stride, double f, double cx, double cy,
                        const double *R, const double *t) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  return fuse_push_maps(c, depth, normal, bgr, bgr_stride, f, cx, cy, R, t);
}

// one view of the stored field: the preparation of cspm_reproject_device, G's dense pass straight into the slot, then k_fuse_store
int cspm_fuse_push(cspm_ctx *c, int view, int source, const cspm_calib *calib, const cspm_geom_params *g, const cspm_fit_params *fit, const double *R,
                   const double *t) {
  if (!c) return CSPM_ERR_ARG;
  int rc = reproject_check(c, view, source, calib, &g, fit);
  if (rc) return rc;
  cspm_geom_params own = *g;
  own.left_frame = 0;  // a view is stored in its own camera frame
  const double cx = calib->cx + (double)view * calib->doffs;
  double tv[3] = {0.0, 0.0, 0.0};
  if (R && t)
    for (int i = 0; i < 3; ++i) tv[i] = view == 1 ? t[i] + R[3 * i] * calib->baseline : t[i];
  if ((rc = fuse_slot_check(c, true, calib->f, cx, calib->cy, R, R && t ? tv : nullptr))) return rc;
  if (c->W != c->fuse_w || c->H != c->fuse_h) return fail(c, CSPM_ERR_STATE, "fusion: the context's images are not of the size given to cspm_fuse_begin");
  ON_DEVICE(c);
  if ((rc = check_sweep(c))) return rc;  // BEFORE the field is read, as in reproject_enqueue
  if ((rc = geom_inputs_alloc(c, source, fit))) return rc;
  const size_t n = (size_t)c->W * c->H, k = (size_t)c->fuse_views;
  double *depth = c->fuse_depth + k * n;
  uint8_t *keep = c->fuse_bytes + ((size_t)c->fuse_max + k) * n;  // the slot's S bytes: every run rewrites them
  {
    Timed tm(c, CSPM_K_MISC, (long long)n);
    const GeomIn in = geom_inputs_launch(c, view, source, &own, fit);
    geom_launch(c->stream, geom_cam(calib, &own, view), in, GeomOut{depth, nullptr, c->fuse_normal + k * 3 * n, keep}, c->W, c->H, nullptr, 0, false, nullptr,
                nullptr);
    hipLaunchKernelGGL(k_fuse_store, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, depth, (const uint8_t *)keep, (const uint32_t *)c->img0[view],
                       c->fuse_pix + k * n, (long long)n);
  }
  HIPCHK(c, hipGetLastError());
  return fuse_slot_commit(c, true, true, calib->f, cx, calib->cy, R, tv);
}

int cspm_fuse_run(cspm_ctx *c, const cspm_fuse_params *p, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out, unsigned int *view_counts_out,
                  uint8_t *state_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = fuse_run_check(c, &p)) return rc;
  ON_DEVICE(c);
  return fuse_run(c, p, cloud_out, cloud_cap, count_out, view_counts_out, state_out);
}

int cspm_fuse_run_device(cspm_ctx *c, const cspm_fuse_params *p, void *d_cloud_out, size_t cloud_cap, void *d_count_out, void *d_view_counts_out,
                         void *d_state_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = fuse_run_check(c, &p)) return rc;
  if (d_cloud_out && ((uintptr_t)d_cloud_out & 15u)) return fail(c, CSPM_ERR_ARG, "fusion: the cloud buffer must be 16-byte aligned");
  if (((uintptr_t)d_count_out & 3u) || ((uintptr_t)d_view_counts_out & 3u)) return fail(c, CSPM_ERR_ARG, "fusion: the counts must be 4-byte aligned");
  ON_DEVICE(c);
  return fuse_enqueue(c, p, (uint4 *)d_cloud_out, d_cloud_out ? cloud_cap : 0, (unsigned int *)d_count_out, (unsigned int *)d_view_counts_out,
                      (uint8_t *)d_state_out);
}

int cspm_fuse_depth_maps(int device, const cspm_fuse_params *p, const cspm_fuse_view *views, int n_views, int w, int h, cspm_point *cloud_out, size_t cloud_cap,
                         unsigned int *count_out, unsigned int *view_counts_out, uint8_t *state_out) {
  if (!p) p = &kFuseDefaults;
  if (const char *msg = fuse_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (n_views < 1 || n_views > kFuseMaxViews) return fail(nullptr, CSPM_ERR_ARG, "fusion: the number of views must be in 1 .. 64");
  if (!views) return fail(nullptr, CSPM_ERR_ARG, "fusion: no views");
  if (const char *msg = fuse_size_error(w, h)) return fail(nullptr, CSPM_ERR_ARG, msg);
  for (int k = 0; k < n_views; ++k) {
    const cspm_fuse_view &v = views[k];
    if (const char *msg = fuse_camera_error(v.f, v.cx, v.cy, v.R, v.t)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if (const char *msg = fuse_maps_error(v.depth, v.bgr, v.bgr_stride, w)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if ((v.normal != nullptr) != (views[0].normal != nullptr)) return fail(nullptr, CSPM_ERR_ARG, "fusion: normals in some views but not all");
  }
  OneShot S(device);
  if (S.rc) return S.finish();
  int rc = fuse_begin(S.c, w, h, n_views);
  for (int k = 0; k < n_views && !rc; ++k) {
    const cspm_fuse_view &v = views[k];
    rc = fuse_push_maps(S.c, v.depth, v.normal, v.bgr, v.bgr_stride, v.f, v.cx, v.cy, v.R, v.t);
  }
  if (!rc) rc = fuse_run(S.c, p, cloud_out, cloud_cap, count_out, view_counts_out, state_out);
  S.latch(rc);
  return S.finish("fusion failed");
}

// T: the TSDF volume of a context, and the one-shot form on caller maps
int cspm_tsdf_default_params(cspm_tsdf_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kTsdfDefaults;
  return CSPM_OK;
}

int cspm_tsdf_begin(cspm_ctx *c, const cspm_tsdf_params *p) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  return tsdf_begin(c, p);
}

int cspm_tsdf_clear(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  return tsdf_clear(c);
}

int cspm_tsdf_integrate(cspm_ctx *c, int slot) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  return tsdf_integrate(c, slot);
}

int cspm_tsdf_raycast(cspm_ctx *c, const cspm_tsdf_camera *camera, int w, int h, double z_near, double *depth_out, double *normal_out, uint8_t *bgr_out,
                      size_t stride, uint8_t *status_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_raycast_check(c, camera, w, h, z_near, bgr_out != nullptr, stride)) return rc;
  ON_DEVICE(c);
  return tsdf_raycast_host(c, camera, w, h, z_near, depth_out, normal_out, bgr_out, stride, status_out);
}

int cspm_tsdf_raycast_device(cspm_ctx *c, const cspm_tsdf_camera *camera, int w, int h, double z_near, void *d_depth_out, void *d_normal_out,
                             void *d_bgr_out, size_t stride, void *d_status_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_raycast_check(c, camera, w, h, z_near, d_bgr_out != nullptr, stride)) return rc;
  if (((uintptr_t)d_depth_out & 7u) || ((uintptr_t)d_normal_out & 7u)) return fail(c, CSPM_ERR_ARG, "tsdf: the depth and normal maps must be 8-byte aligned");
  ON_DEVICE(c);
  TsdfRayOut out{};
  out.depth = (double *)d_depth_out;
  out.normal = (double *)d_normal_out;
  out.bgr = (uint8_t *)d_bgr_out;
  out.bgr_stride = stride;
  out.status = (uint8_t *)d_status_out;
  return tsdf_raycast_enqueue(c, tsdf_cam(camera), w, h, z_near, out);
}

int cspm_tsdf_raycast_push(cspm_ctx *c, const cspm_tsdf_camera *camera, double z_near) {
  if (!c) return CSPM_ERR_ARG;
  if (const char *msg = tsdf_camera_error(camera, z_near)) return fail(c, CSPM_ERR_ARG, msg);
  if (int rc = tsdf_state_check(c)) return rc;
  if (int rc = fuse_slot_check(c, true, camera->f, camera->cx, camera->cy, camera->R, camera->t)) return rc;
  if ((c->fuse_h + kTsdfTileH - 1) / kTsdfTileH > 65535) return fail(c, CSPM_ERR_ARG, "tsdf: h must be at most 524280");
  ON_DEVICE(c);
  const size_t n = (size_t)c->fuse_w * c->fuse_h, k = (size_t)c->fuse_views;
  TsdfRayOut out{};
  out.depth = c->fuse_depth + k * n;
  out.normal = c->fuse_normal + k * 3 * n;
  out.pix = c->fuse_pix + k * n;
  if (int rc = tsdf_raycast_enqueue(c, tsdf_cam(camera), c->fuse_w, c->fuse_h, z_near, out)) return rc;
  return fuse_slot_commit(c, true, c->tsdf_coloured, camera->f, camera->cx, camera->cy, camera->R, camera->t);
}

int cspm_tsdf_points(cspm_ctx *c, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  return tsdf_points_host(c, cloud_out, cloud_cap, count_out);
}

int cspm_tsdf_points_device(cspm_ctx *c, void *d_cloud_out, size_t cloud_cap, void *d_count_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  if (d_cloud_out && ((uintptr_t)d_cloud_out & 15u)) return fail(c, CSPM_ERR_ARG, "tsdf: the cloud buffer must be 16-byte aligned");
  if ((uintptr_t)d_count_out & 3u) return fail(c, CSPM_ERR_ARG, "tsdf: the count must be 4-byte aligned");
  ON_DEVICE(c);
  return tsdf_points_enqueue(c, (uint4 *)d_cloud_out, d_cloud_out ? cloud_cap : 0, (unsigned int *)d_count_out);
}

int cspm_tsdf_get_volume(cspm_ctx *c, float *D_out, float *W_out, uint8_t *colour_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  return tsdf_get_volume(c, D_out, W_out, colour_out);
}

int cspm_tsdf_set_volume(cspm_ctx *c, const float *D, const float *W, const uint8_t *colour) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  return tsdf_set_volume(c, D, W, colour);
}

int cspm_tsdf_mesh(cspm_ctx *c, cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap, unsigned int *n_vertices_out,
                   unsigned int *n_faces_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  return tsdf_mesh_host(c, vertices_out, vertex_cap, faces_out, face_cap, n_vertices_out, n_faces_out);
}

int cspm_tsdf_mesh_device(cspm_ctx *c, void *d_vertices_out, size_t vertex_cap, void *d_faces_out, size_t face_cap, void *d_n_vertices_out,
                          void *d_n_faces_out) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  if (d_vertices_out && ((uintptr_t)d_vertices_out & 15u)) return fail(c, CSPM_ERR_ARG, "tsdf: the vertex buffer must be 16-byte aligned");
  if (d_faces_out && ((uintptr_t)d_faces_out & 3u)) return fail(c, CSPM_ERR_ARG, "tsdf: the face buffer must be 4-byte aligned");
  if (((uintptr_t)d_n_vertices_out & 3u) || ((uintptr_t)d_n_faces_out & 3u)) return fail(c, CSPM_ERR_ARG, "tsdf: the counts must be 4-byte aligned");
  ON_DEVICE(c);
  return tsdf_mesh_enqueue(c, (uint4 *)d_vertices_out, d_vertices_out ? vertex_cap : 0, (uint32_t *)d_faces_out, d_faces_out ? face_cap : 0,
                           (unsigned int *)d_n_vertices_out, (unsigned int *)d_n_faces_out);
}

int cspm_tsdf_end(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  if (int rc = tsdf_state_check(c)) return rc;
  ON_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  tsdf_release(c);
  return CSPM_OK;
}

// what both one-shot entries check before a device is opened, and the views into a cleared volume of the temporary context
static int tsdf_one_shot_check(const cspm_tsdf_params *p, const cspm_fuse_view *views, int n_views, int w, int h) {
  if (const char *msg = tsdf_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (n_views < 1 || n_views > kFuseMaxViews) return fail(nullptr, CSPM_ERR_ARG, "fusion: the number of views must be in 1 .. 64");
  if (!views) return fail(nullptr, CSPM_ERR_ARG, "fusion: no views");
  if (const char *msg = fuse_size_error(w, h)) return fail(nullptr, CSPM_ERR_ARG, msg);
  for (int k = 0; k < n_views; ++k) {
    const cspm_fuse_view &v = views[k];
    if (const char *msg = fuse_camera_error(v.f, v.cx, v.cy, v.R, v.t)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if (const char *msg = fuse_maps_error(v.depth, v.bgr, v.bgr_stride, w)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if ((v.normal != nullptr) != (views[0].normal != nullptr)) return fail(nullptr, CSPM_ERR_ARG, "fusion: normals in some views but not all");
  }
  return CSPM_OK;
}
static int tsdf_one_shot_integrate(cspm_ctx *c, const cspm_tsdf_params *p, const cspm_fuse_view *views, int n_views, int w, int h) {
  int rc = fuse_begin(c, w, h, n_views);
  if (!rc) rc = tsdf_begin(c, p);
  for (int k = 0; k < n_views && !rc; ++k) {
    const cspm_fuse_view &v = views[k];
    rc = fuse_push_maps(c, v.depth, v.normal, v.bgr, v.bgr_stride, v.f, v.cx, v.cy, v.R, v.t);
    if (!rc) rc = tsdf_integrate(c, k);
  }
  return rc;
}

int cspm_tsdf_mesh_depth_maps(int device, const cspm_tsdf_params *p, const cspm_fuse_view *views, int n_views, int w, int h, cspm_point *vertices_out,
                              size_t vertex_cap, cspm_face *faces_out, size_t face_cap, unsigned int *n_vertices_out, unsigned int *n_faces_out) {
  if (int rc = tsdf_one_shot_check(p, views, n_views, w, h)) return rc;
  OneShot S(device);
  if (S.rc) return S.finish();
  int rc = tsdf_one_shot_integrate(S.c, p, views, n_views, w, h);
  if (!rc) rc = tsdf_mesh_host(S.c, vertices_out, vertex_cap, faces_out, face_cap, n_vertices_out, n_faces_out);
  S.latch(rc);
  return S.finish("tsdf meshing failed");
}

int cspm_tsdf_depth_maps(int device, const cspm_tsdf_params *p, const cspm_fuse_view *views, int n_views, int w, int h, cspm_point *cloud_out, size_t cloud_cap,
                         unsigned int *count_out, float *D_out, float *W_out, uint8_t *colour_out) {
  if (int rc = tsdf_one_shot_check(p, views, n_views, w, h)) return rc;
  OneShot S(device);
  if (S.rc) return S.finish();
  int rc = tsdf_one_shot_integrate(S.c, p, views, n_views, w, h);
  if (!rc) rc = tsdf_points_host(S.c, cloud_out, cloud_cap, count_out);
  if (!rc) rc = tsdf_get_volume(S.c, D_out, W_out, colour_out);
  S.latch(rc);
  return S.finish("tsdf fusion failed");
}

// R: a fusion view registered against other fusion views, and the one-shot form on caller maps
int cspm_reg_default_params(cspm_reg_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kRegDefaults;
  return CSPM_OK;
}

int cspm_fuse_register(cspm_ctx *c, int src, unsigned long long targets, const cspm_reg_params *p, const double *R0, const double *t0, int apply,
                       double *R_out, double *t_out, cspm_reg_iter *iters_out) {
  if (!c) return CSPM_ERR_ARG;
  FuseCam start;
  if (int rc = reg_check(c, src, targets, &p, R0, t0, &start)) return rc;
  ON_DEVICE(c);
  return reg_run(c, src, targets, p, &start, apply, R_out, t_out, iters_out);
}

int cspm_fuse_get_pose(cspm_ctx *c, int slot, double *R_out, double *t_out) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (slot < 0 || slot >= c->fuse_views) return fail(c, CSPM_ERR_ARG, "fusion: no such view");
  const FuseCam &cam = c->fuse_cams_host[(size_t)slot];
  if (R_out) for (int i = 0; i < 9; ++i) R_out[i] = cam.R[i];
  if (t_out) for (int i = 0; i < 3; ++i) t_out[i] = cam.t[i];
  return CSPM_OK;
}

int cspm_fuse_set_pose(cspm_ctx *c, int slot, const double *R, const double *t) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->fuse_on) return fail(c, CSPM_ERR_STATE, "fusion: cspm_fuse_begin first");
  if (slot < 0 || slot >= c->fuse_views) return fail(c, CSPM_ERR_ARG, "fusion: no such view");
  FuseCam &cam = c->fuse_cams_host[(size_t)slot];  // lives as long as the slots: the copy may read it later
  if (const char *msg = fuse_camera_error(cam.f, cam.cx, cam.cy, R, t)) return fail(c, CSPM_ERR_ARG, msg);
  ON_DEVICE(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // an earlier copy may still read the row
  for (int i = 0; i < 9; ++i) cam.R[i] = R[i];
  for (int i = 0; i < 3; ++i) cam.t[i] = t[i];
  HIPCHK(c, hipMemcpyAsync(c->fuse_cams + slot, &cam, sizeof cam, hipMemcpyHostToDevice, c->stream));
  return CSPM_OK;
}

int cspm_register_depth_maps(int device, const cspm_reg_params *p, const cspm_fuse_view *views, int n_views, int w, int h, int src,
                             unsigned long long targets, double *R_out, double *t_out, cspm_reg_iter *iters_out) {
  if (!p) p = &kRegDefaults;
  if (const char *msg = reg_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (n_views < 1 || n_views > kFuseMaxViews) return fail(nullptr, CSPM_ERR_ARG, "fusion: the number of views must be in 1 .. 64");
  if (!views) return fail(nullptr, CSPM_ERR_ARG, "fusion: no views");
  if (const char *msg = fuse_size_error(w, h)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = reg_mask_error(src, targets, n_views)) return fail(nullptr, CSPM_ERR_ARG, msg);
  for (int k = 0; k < n_views; ++k) {
    const cspm_fuse_view &v = views[k];
    if (const char *msg = fuse_camera_error(v.f, v.cx, v.cy, v.R, v.t)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if (const char *msg = fuse_maps_error(v.depth, v.bgr, v.bgr_stride, w)) return fail(nullptr, CSPM_ERR_ARG, msg);
    if (!v.normal) return fail(nullptr, CSPM_ERR_ARG, "registration: the views carry no normals");
  }
  FuseCam start;  // in front of the OneShot: an upload reads it
  OneShot S(device);
  if (S.rc) return S.finish();
  int rc = fuse_begin(S.c, w, h, n_views);
  for (int k = 0; k < n_views && !rc; ++k) {
    const cspm_fuse_view &v = views[k];
    rc = fuse_push_maps(S.c, v.depth, v.normal, nullptr, 0, v.f, v.cx, v.cy, v.R, v.t);  // R reads no colours
  }
  if (!rc) rc = reg_check(S.c, src, targets, &p, nullptr, nullptr, &start);
  if (!rc) rc = reg_run(S.c, src, targets, p, &start, 0, R_out, t_out, iters_out);
  S.latch(rc);
  return S.finish("registration failed");
}

// C: a plane field carried into a moved camera, on caller memory and between two contexts
int cspm_carry_default_params(cspm_carry_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kCarryDefaults;
  return CSPM_OK;
}

int cspm_carry_relative_pose(const double *Rs, const double *ts, const double *Rt, const double *tt, double *R_out, double *t_out) {
  if (!Rs || !ts || !Rt || !tt || !R_out || !t_out) return fail(nullptr, CSPM_ERR_ARG, "carry: a pose is missing");
  double R[9], t[3];
  const double d[3] = {ts[0] - tt[0], ts[1] - tt[1], ts[2] - tt[2]};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (Rt[i] * Rs[j] + Rt[3 + i] * Rs[3 + j]) + Rt[6 + i] * Rs[6 + j];
    t[i] = (Rt[i] * d[0] + Rt[3 + i] * d[1]) + Rt[6 + i] * d[2];
  }
  for (int i = 0; i < 9; ++i) R_out[i] = R[i];  // through locals: an output may be one of the inputs
  for (int i = 0; i < 3; ++i) t_out[i] = t[i];
  return CSPM_OK;
}

int cspm_carry_plane_field(int device, const double *src_norm_param, const uint8_t *mask, const cspm_calib *src_calib, int src_view, int w_s, int h_s,
                           const cspm_calib *dst_calib, int dst_view, int w_t, int h_t, int max_dis, const double *R, const double *t,
                           const cspm_carry_params *p, double *norm_param_out, uint8_t *state_out, int32_t *source_out) {
  if (!p) p = &kCarryDefaults;
  if (const char *msg = carry_params_error(p)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_calib_error(src_calib, src_view)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_calib_error(dst_calib, dst_view)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_motion_error(R, t)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_size_error(w_s, h_s)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_size_error(w_t, h_t)) return fail(nullptr, CSPM_ERR_ARG, msg);
  if (max_dis < 0) return fail(nullptr, CSPM_ERR_ARG, "carry: max_dis must be >= 0");
  if (!src_norm_param) return fail(nullptr, CSPM_ERR_ARG, "carry: no source plane field");
  const size_t ns = (size_t)w_s * h_s, nt = (size_t)w_t * h_t;
  std::vector<double> abc(3 * ns), rec(norm_param_out ? 6 * nt : 0);  // in front of the OneShot: its copies read and write them
  for (size_t i = 0; i < ns; ++i)
    for (int k = 0; k < 3; ++k) abc[k * ns + i] = src_norm_param[6 * i + 3 + k];
  OneShot S(device);
  double *dabc = S.up(abc.data(), 3 * ns);
  uint8_t *dmask = S.up(mask, ns);
  uint32_t *dkey = S.buf<uint32_t>(3 * nt);
  double *dout = S.buf<double>(6 * nt);
  uint8_t *dstate = S.buf<uint8_t>(nt, state_out != nullptr);
  int *dsource = S.buf<int>(nt, source_out != nullptr);
  if (S.rc) return S.finish();
  const CarryPar k = carry_par(src_calib, src_view, w_s, h_s, dst_calib, dst_view, w_t, h_t, (double)max_dis, R, t, p);
  const Slabs6 o = six_slabs(dout, nt);
  if (carry_launch(S.c->stream, k, CarrySrc{dabc, dabc + ns, dabc + 2 * ns, dmask}, reinterpret_cast<unsigned long long *>(dkey),
                   CarryOut{o.p[0], o.p[1], o.p[2], o.p[3], o.p[4], o.p[5], dstate, dsource, 0}) != hipSuccess)
    return S.fail(CSPM_ERR_HIP, "carry kernels failed"), S.finish();
  S.down(rec.data(), dout, rec.size());
  S.down(state_out, dstate, nt);
  S.down(source_out, dsource, nt);
  if (S.finish("carry kernels failed")) return S.rc;
  if (norm_param_out) interleave_planes(rec.data(), nt, norm_param_out);
  return CSPM_OK;
}

int cspm_carry_planes(cspm_ctx *dst, cspm_ctx *src, const cspm_calib *src_calib, const cspm_calib *dst_calib, const double *R, const double *t,
                      const cspm_carry_params *p, int merge) {
  if (!dst || !src || dst == src) return dst ? fail(dst, CSPM_ERR_ARG, "cspm_carry_planes needs two different contexts") : CSPM_ERR_ARG;
  if (!p) p = &kCarryDefaults;
  if (const char *msg = carry_params_error(p)) return fail(dst, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_calib_error(src_calib, 0)) return fail(dst, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_calib_error(dst_calib, 0)) return fail(dst, CSPM_ERR_ARG, msg);
  if (const char *msg = carry_motion_error(R, t)) return fail(dst, CSPM_ERR_ARG, msg);
  if (dst->device != src->device) return fail(dst, CSPM_ERR_ARG, "the two contexts are on different devices");
  if (!src->field_alloc) return fail(dst, CSPM_ERR_STATE, "the source context has no plane field");
  if (!dst->img0[0]) return fail(dst, CSPM_ERR_STATE, "cspm_set_images first");
  if (merge) {
    if (int e = need_cost(dst)) return e;
  }
  if (int e = need_field(dst, kNoMergeTarget)) return e;
  if (dst->max_dis < 1) return fail(dst, CSPM_ERR_STATE, "no max_dis known: build a cost object (or cspm_fpm_begin) first");
  ON_DEVICE(dst);
  int rc;
  const size_t nt = (size_t)dst->W * dst->H;
  CandBuf cand{};
  if ((rc = source_check(dst, src)) || (rc = dalloc(dst, dst->mem_field, &dst->carry_mem, 3 * nt))) return rc;
  if (merge) {
    if ((rc = ensure_cand(dst, &cand)) || (rc = ensure_consistent(dst))) return rc;
  } else {
    dst->field_consistent = false;  // min_cost still belongs to the planes that were replaced
  }
  return with_source(dst, src, "cspm_carry_planes", [&]() -> int {
    dst->repeat.taint_unchecked_run();  // it can no longer be repeated over these planes
    for (int v = 0; v < 2; ++v) {
      // view 1's cameras sit one baseline to the right of view 0's: X_s0 = X_s1 + (B_s, 0, 0), X_t1 = X_t0 - (B_t, 0, 0)
      double tv[3] = {t[0], t[1], t[2]};
      if (v == 1) {
        for (int i = 0; i < 3; ++i) tv[i] = t[i] + R[3 * i] * src_calib->baseline;
        tv[0] = tv[0] - dst_calib->baseline;
      }
      const CarryPar k = carry_par(src_calib, v, src->W, src->H, dst_calib, v, dst->W, dst->H, (double)dst->max_dis, R, tv, p);
      const Field &sf = src->f[v], &df = dst->f[v];
      const CarryOut out = merge ? CarryOut{cand.planes.p[0], cand.planes.p[1], cand.planes.p[2], cand.planes.p[3], cand.planes.p[4], cand.planes.p[5],
                                            cand.mask, nullptr, 0}
                                 : CarryOut{df.nx, df.ny, df.nz, df.a, df.b, df.c, nullptr, nullptr, 1};
      {
        Timed tm(dst, CSPM_K_MISC, (long long)src->W * src->H);
        if (carry_launch(dst->stream, k, CarrySrc{sf.a, sf.b, sf.c, nullptr}, reinterpret_cast<unsigned long long *>(dst->carry_mem), out) != hipSuccess)
          return fail(dst, CSPM_ERR_HIP, "carry kernels failed");
      }
      if (merge) {
        const CandField cf = cand.field(v);
        if (int e = do_merge(dst, &cf, &kDefaultParams, v, 1, (long long)nt)) return e;
      }
    }
    return CSPM_OK;
  });
}

// N alone on caller maps: the launch cspm_synthesize enqueues.  Arguments first, then the device.
int cspm_synth_default_params(cspm_synth_params *p) {
  if (!p) return CSPM_ERR_ARG;
  *p = kSynthDefaults;
  return CSPM_OK;
}

int cspm_synthesize_host(int device, const cspm_synth_params *p, double t, const cspm_synth_view *view0, const cspm_synth_view *view1, int w, int h,
                         uint8_t *bgr_out, size_t out_stride, double *disp_out, uint8_t *mask_out) {
  if (!p) p = &kSynthDefaults;
  if (const char *msg = synth_args_error(p, t, w, h, bgr_out != nullptr, out_stride)) return fail(nullptr, CSPM_ERR_ARG, msg);
  const cspm_synth_view *in[2] = {view0, view1};
  for (int v = 0; v < 2; ++v) {
    if (!(p->views >> v & 1)) continue;
    if (!in[v] || !in[v]->disp || !in[v]->bgr) return fail(nullptr, CSPM_ERR_ARG, "view synthesis: a view that `views` names has no disparity map or no image");
    if (in[v]->stride < (size_t)w * 3) return fail(nullptr, CSPM_ERR_ARG, "view synthesis: an image stride is below 3 * w");
  }
  OneShot S(device);
  const size_t n = (size_t)w * h;
  SynthView sv[2] = {};
  for (int v = 0; v < 2; ++v) {
    if (!(p->views >> v & 1)) continue;
    double *dd = S.up(in[v]->disp, n);
    uint8_t *dv = S.up(in[v]->valid, n);
    double *da = S.up(in[v]->slope_a, n);
    sv[v] = SynthView{dd, dv, da, nullptr, S.up_bgr(in[v]->bgr, in[v]->stride, w, h)};
  }
  uint8_t *dout = S.buf<uint8_t>(3 * n, bgr_out != nullptr), *dmask = S.buf<uint8_t>(n, mask_out != nullptr);
  double *ddisp = S.buf<double>(n, disp_out != nullptr);
  if (S.rc) return S.finish();
  synth_launch(S.c->stream, sv[0], sv[1], p, t, SynthOut{dout, (size_t)w * 3, ddisp, dmask}, w, h);
  S.down2d(bgr_out, out_stride, dout, (size_t)w * 3, h);
  S.down(disp_out, ddisp, n);
  S.down(mask_out, dmask, n);
  return S.finish("view synthesis kernel failed");
}

// N on the stored field (cspm.h "view synthesis"): synchronous, host outputs
int cspm_synthesize(cspm_ctx *c, int source, const cspm_synth_params *p, double t, uint8_t *bgr_out, size_t out_stride, double *disp_out, uint8_t *mask_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = synthesize_check(c, source, &p, t, bgr_out != nullptr, out_stride);
  if (rc) return rc;
  ON_DEVICE(c);
  const size_t n = (size_t)c->W * c->H, row = (size_t)c->W * 3;
  Staging S(c);
  uint8_t *dout = S.buf<uint8_t>(3 * n, bgr_out != nullptr);
  double *ddisp = S.buf<double>(n, disp_out != nullptr);
  uint8_t *dmask = S.buf<uint8_t>(n, mask_out != nullptr);
  if (S.rc) return S.finish();
  if ((rc = synthesize_enqueue(c, source, p, t, SynthOut{dout, row, ddisp, dmask}))) return rc;
  S.down2d(bgr_out, out_stride, dout, row, c->H);
  S.down(disp_out, ddisp, n);
  S.down(mask_out, dmask, n);
  return S.finish("view synthesis download failed");
}

// the same with device-resident outputs: asynchronous on the ctx stream behind the pending-run check; not replayed (cspm.h)
int cspm_synthesize_device(cspm_ctx *c, int source, const cspm_synth_params *p, double t, void *d_bgr_out, size_t out_stride, void *d_disp_out,
                           void *d_mask_out) {
  if (!c) return CSPM_ERR_ARG;
  int rc = synthesize_check(c, source, &p, t, d_bgr_out != nullptr, out_stride);
  if (rc) return rc;
  ON_DEVICE(c);
  return synthesize_enqueue(c, source, p, t, SynthOut{(uint8_t *)d_bgr_out, out_stride, (double *)d_disp_out, (uint8_t *)d_mask_out});
}

int cspm_pm_init_keep(cspm_ctx *c, const cspm_pm_params *p) {
  const bool had_field = c && c->field_alloc;
  PM_ENTER();
  c->repeat.taint_unchecked_run();
  if (!had_field) return do_init(c, p);  // nothing to keep
  if ((rc = ensure_consistent(c))) return rc;
  return do_merge(c, nullptr, p, 0, 2, 2LL * c->W * c->H);
}

int cspm_get_planes(cspm_ctx *c, int view, double *np_out, double *cost_out) {
  if (!c || view < 0 || view > 1) return CSPM_ERR_ARG;
  if (!c->field_alloc) return fail(c, CSPM_ERR_STATE, "no plane field yet");
  ON_DEVICE(c);
  if (int rc = check_sweep(c)) return rc;
  const size_t n = (size_t)c->W * c->H;
  std::vector<double> h(7 * n);
  Staging S(c);
  S.down(h.data(), c->f[view].nx, 7 * n);
  if (S.finish("plane download failed")) return S.rc;
  if (np_out) interleave_planes(h.data(), n, np_out);
  if (cost_out) memcpy(cost_out, h.data() + 6 * n, sizeof(double) * n);
  return CSPM_OK;
}

int cspm_set_planes(cspm_ctx *c, int view, const double *np, const double *cost) {
  if (!c || view < 0 || view > 1 || !np || !cost) return CSPM_ERR_ARG;
  if (!c->img0[0]) return fail(c, CSPM_ERR_STATE, "cspm_set_images first");
  ON_DEVICE(c);
  int rc = ensure_field(c);
  if (rc) return rc;
  const size_t n = (size_t)c->W * c->H;
  std::vector<double> h(7 * n);
  deinterleave_planes(np, n, h.data());
  memcpy(h.data() + 6 * n, cost, sizeof(double) * n);
  Staging S(c);
  S.put(c->f[view].nx, h.data(), 7 * n);
  if (S.finish("plane upload failed")) return S.rc;
  c->field_consistent = false;  // min_cost is whatever the caller says: the sweep may not assume cost(plane) == min_cost
  c->repeat.taint();
  return CSPM_OK;
}

int cspm_disparity_u8_device(cspm_ctx *c, int view, int dis_scale, void *d_out) {
  if (!c || view < 0 || view > 1 || !d_out) return CSPM_ERR_ARG;
  if (!c->field_alloc) return fail(c, CSPM_ERR_STATE, "no plane field yet");
  ON_DEVICE(c);
  return request_output(c, OutReq{kOutDisp, view, dis_scale, d_out, nullptr});
}

int cspm_get_disparity_u8(cspm_ctx *c, int view, int dis_scale, uint8_t *out, size_t stride) {
  if (!c || !out || view < 0 || view > 1 || stride < (size_t)c->W) return CSPM_ERR_ARG;
  if (!c->field_alloc) return fail(c, CSPM_ERR_STATE, "no plane field yet");
  ON_DEVICE(c);
  int rc = check_sweep(c);  // BEFORE PlaneToDisp: a run repeated after a sweep timeout must be the one the map is computed from
  if (rc) return rc;
  if ((rc = enqueue_disp_u8(c, view, dis_scale, c->d_dis[view]))) return rc;
  Staging S(c);
  S.down2d(out, stride, c->d_dis[view], c->W, c->H);
  return S.finish("disparity download failed");
}

int cspm_get_disparity_f64(cspm_ctx *c, int view, double *out) {
  if (!c || view < 0 || view > 1 || !out) return CSPM_ERR_ARG;
  if (!c->field_alloc) return fail(c, CSPM_ERR_STATE, "no plane field yet");
  ON_DEVICE(c);
  if (int rc = check_sweep(c)) return rc;
  const Pm pm = field_pm(c);
  const size_t n = (size_t)c->W * c->H;
  hipLaunchKernelGGL(k_plane_to_disp_f64, dim3(ew_grid((long long)n)), dim3(256), 0, c->stream, pm, view, c->vc.cost);
  Staging S(c);
  S.down(out, c->vc.cost, n);
  return S.finish("disparity download failed");
}

int cspm_postprocess(cspm_ctx *c, int dis_scale, uint8_t *l_out, uint8_t *r_out, size_t stride) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->field_alloc || !c->cost_alloc) return fail(c, CSPM_ERR_STATE, "cspm_postprocess needs a finished PatchMatch");
  if (dis_scale < 1 || stride < (size_t)c->W || !l_out || !r_out) return fail(c, CSPM_ERR_ARG, "bad dis_scale / stride / outputs");
  ON_DEVICE(c);
  int rc = check_sweep(c);
  if (rc) return rc;
  if ((rc = postprocess_enqueue(c, dis_scale))) return rc;
  uint8_t *outs[2] = {l_out, r_out};
  Staging S(c);
  for (int v = 0; v < 2; ++v) S.down2d(outs[v], stride, c->d_dis[v], c->W, c->H);
  return S.finish("post-processing download failed");
}

// the same with device-resident outputs (W*H bytes each, packed rows): asynchronous like cspm_patchmatch
int cspm_postprocess_device(cspm_ctx *c, int dis_scale, void *d_l_out, void *d_r_out) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->field_alloc || !c->cost_alloc) return fail(c, CSPM_ERR_STATE, "cspm_postprocess_device needs a finished PatchMatch");
  if (dis_scale < 1 || !d_l_out || !d_r_out) return fail(c, CSPM_ERR_ARG, "bad dis_scale / outputs");
  ON_DEVICE(c);
  return request_output(c, OutReq{kOutPost8, 0, dis_scale, d_l_out, d_r_out});
}

// sub-pixel PostProcessing: the f64 maps and, where asked for, the left-right consistency flags
int cspm_postprocess_f64(cspm_ctx *c, double *l_out, double *r_out, uint8_t *l_valid_out, uint8_t *r_valid_out) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->field_alloc || !c->cost_alloc) return fail(c, CSPM_ERR_STATE, "cspm_postprocess_f64 needs a finished PatchMatch");
  if (!l_out || !r_out) return fail(c, CSPM_ERR_ARG, "bad outputs");
  ON_DEVICE(c);
  int rc = check_sweep(c);
  if (rc) return rc;
  if ((rc = postprocess_f64_enqueue(c))) return rc;
  const size_t n = (size_t)c->W * c->H;
  double *outs[2] = {l_out, r_out};
  uint8_t *flags[2] = {l_valid_out, r_valid_out};
  Staging S(c);
  for (int v = 0; v < 2; ++v) {
    S.down(outs[v], c->d_pp[v], n);
    S.down(flags[v], c->d_valid[v], n);
  }
  return S.finish("post-processing download failed");
}

// the same with device-resident outputs (W*H f64 each, packed rows): asynchronous like cspm_postprocess_device
int cspm_postprocess_f64_device(cspm_ctx *c, void *d_l_out, void *d_r_out) {
  if (!c) return CSPM_ERR_ARG;
  if (!c->field_alloc || !c->cost_alloc) return fail(c, CSPM_ERR_STATE, "cspm_postprocess_f64_device needs a finished PatchMatch");
  if (!d_l_out || !d_r_out) return fail(c, CSPM_ERR_ARG, "bad outputs");
  ON_DEVICE(c);
  return request_output(c, OutReq{kOutPostF64, 0, 0, d_l_out, d_r_out});
}

int cspm_enable_timing(cspm_ctx *c, int on) {
  if (!c) return CSPM_ERR_ARG;
  c->timing = on != 0;
  return CSPM_OK;
}
int cspm_reset_timing(cspm_ctx *c) {
  if (!c) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  int rc = drain_timing(c);
  for (int k = 0; k < CSPM_K_COUNT; ++k) { c->acc_ms[k] = 0; c->acc_launch[k] = 0; c->acc_evals[k] = 0; }
  return rc;
}
int cspm_get_timing(cspm_ctx *c, int k, long long *launches, double *total_ms, long long *evals) {
  if (!c || k < 0 || k >= CSPM_K_COUNT) return CSPM_ERR_ARG;
  ON_DEVICE(c);
  int rc = drain_timing(c);
  if (launches) *launches = c->acc_launch[k];
  if (total_ms) *total_ms = c->acc_ms[k];
  if (evals) *evals = c->acc_evals[k];
  return rc;
}

long long cspm_taps_per_view_pass(const cspm_ctx *c) {
  if (!c || !c->cost_alloc) return 0;
  long long total = 0;
  const Cost &cd = c->cost;
  for (int s = 0; s < cd.levels; ++s) {
    const Level &L = cd.lv[s];
    long long sx = 0, sy = 0;
    for (int x = 0; x < c->W; ++x) {
      const int cx = x >> s;
      sx += std::min(cx + cd.half, L.W - 1) - std::max(cx - cd.half, 0) + 1;
    }
    for (int y = 0; y < c->H; ++y) {
      const int cy = y >> s;
      sy += std::min(cy + cd.half, L.H - 1) - std::max(cy - cd.half, 0) + 1;
    }
    total += sx * sy;
  }
  return total;
}

// lane-taps the row engine EXECUTES for one evaluation of every pixel of one view: every lane of every 64-pixel wave walks
// all window columns of the window rows that lie inside the image (columns outside the image are executed with weight 0,
// the lanes past the end of an image row shadow its last pixel)
long long cspm_row_engine_taps_per_view_pass(const cspm_ctx *c) {
  if (!c || !c->cost_alloc) return 0;
  long long total = 0;
  const Cost &cd = c->cost;
  const long long lanes_per_row = (long long)((c->W + kWave - 1) / kWave) * kWave;
  for (int s = 0; s < cd.levels; ++s) {
    const Level &L = cd.lv[s];
    long long sy = 0;
    for (int y = 0; y < c->H; ++y) {
      const int cy = y >> s;
      sy += std::min(cy + cd.half, L.H - 1) - std::max(cy - cd.half, 0) + 1;
    }
    total += sy * lanes_per_row * cd.n;
  }
  return total;
}

#ifdef CSPM_COUNT_ALIVE
// debug build only: lanes alive after each pyramid level / lanes evaluated at each level, summed over every row-engine launch
int cspm_debug_alive(unsigned long long *out16, int reset) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(cspm::g_alive), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_alive), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
int cspm_debug_alive_hist(unsigned long long *out120, int reset) {  // [3 groups][8 levels][5 buckets]
  static unsigned long long z[120];
  if (hipMemcpyFromSymbol(out120, HIP_SYMBOL(cspm::g_alive_hist), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_alive_hist), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
#endif

// ---- CSPatchMatch over a foreign IPlaneCost: see cspm_foreign.h -----------------------------------------------------------
int cspm_fpm_begin(cspm_ctx *c, int w, int h, int max_dis) {
  if (!c) return CSPM_ERR_ARG;
  if (w < 1 || h < 1 || max_dis < 1) return fail(c, CSPM_ERR_ARG, "bad w / h / max_dis");
  ON_DEVICE(c);
  if (w != c->W || h != c->H) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_geometry(c);
    c->W = w; c->H = h;
  }
  if (c->cost_alloc && c->max_dis != max_dis) {  // its levels, strips and init range were sized for the old disparity range
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_cost(c);
  }
  c->max_dis = max_dis;
  c->field_consistent = false;
  c->repeat.taint();
  int rc = ensure_field(c);
  if (rc) return rc;
  const long long need = std::max(2LL * w * h, 4LL * std::min(w, h));  // a diagonal batch holds 4 per pixel (tiny images)
  if (c->fpm_cap < need) {
    if ((rc = dalloc(c, c->mem_field, &c->fpm.xy, (size_t)need * 2)) || (rc = dalloc(c, c->mem_field, &c->fpm.view, (size_t)need)) ||
        (rc = dalloc(c, c->mem_field, &c->fpm.plane, (size_t)need * 6)) || (rc = dalloc(c, c->mem_field, &c->fpm.cost, (size_t)need)))
      return rc;
    c->fpm_cap = need;
  }
  c->fpm_phase = -1;
  return CSPM_OK;
}

int cspm_fpm_candidates(cspm_ctx *c, int phase, int iter, int step, const cspm_pm_params *p, int *n_out, int *xy_out, int *view_out,
                        double *plane_out) {
  if (!c || !n_out || !xy_out || !view_out || !plane_out) return CSPM_ERR_ARG;
  if (!c->fpm_cap) return fail(c, CSPM_ERR_STATE, "cspm_fpm_begin first");
  if (!p) p = &kDefaultParams;
  if (p->schedule != CSPM_SCHED_RASTER) return fail(c, CSPM_ERR_ARG, "a foreign IPlaneCost runs the reference's raster schedule only");
  ON_DEVICE(c);
  Pm pm = make_pm(c, p);
  const long long n = (long long)c->W * c->H;
  long long count = 0;
  int inc = 1;
  switch (phase) {
    case CSPM_FPM_INIT:
    case CSPM_FPM_REFINE: {
      if (phase == CSPM_FPM_REFINE && (step < 0 || step > 64)) return fail(c, CSPM_ERR_ARG, "refinement step out of range");
      double z = c->max_dis / 2.0, nn = 1.0;  // cs_patchmatch.cc:95, cs_patchmatch.h:145; halved once per step (:342-343)
      for (int k = 0; k < step && k < 64; ++k) { z /= 2.0; nn /= 2.0; }
      if (phase == CSPM_FPM_REFINE && z < 0.1) return fail(c, CSPM_ERR_ARG, "refinement step out of range");
      count = 2 * n;
      hipLaunchKernelGGL(k_fpm_point_cand, dim3(ew_grid(count)), dim3(256), 0, c->stream, pm, c->fpm, phase == CSPM_FPM_REFINE ? 1 : 0, iter, step, z, nn);
      break;
    }
    case CSPM_FPM_VIEW:
      if (step < 0 || step > 1) return fail(c, CSPM_ERR_ARG, "view propagation: step = target view, 0 or 1");
      count = n;
      hipLaunchKernelGGL(k_fpm_view_cand, dim3(ew_grid(count)), dim3(256), 0, c->stream, pm, c->fpm, step);
      break;
    case CSPM_FPM_SPATIAL: {
      if (step < 0 || step > c->W + c->H - 2) return fail(c, CSPM_ERR_ARG, "spatial propagation: step = anti-diagonal, 0 .. w+h-2");
      inc = (iter % 2 == 0) ? 1 : -1;
      const int cnt = std::min(c->H - 1, step) - std::max(0, step - (c->W - 1)) + 1;
      count = 4LL * cnt;
      hipLaunchKernelGGL(k_fpm_diag_cand, dim3(ew_grid(2LL * cnt)), dim3(256), 0, c->stream, pm, c->fpm, step, inc);
      break;
    }
    default: return fail(c, CSPM_ERR_ARG, "unknown phase");
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(xy_out, c->fpm.xy, sizeof(int) * 2 * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(view_out, c->fpm.view, sizeof(int) * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(plane_out, c->fpm.plane, sizeof(double) * 6 * count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->fpm_phase = phase; c->fpm_iter = iter; c->fpm_step = step; c->fpm_inc = inc; c->fpm_count = count; c->fpm_params = *p;
  *n_out = (int)count;
  return CSPM_OK;
}

int cspm_fpm_commit(cspm_ctx *c, const double *cost) {
  if (!c || !cost) return CSPM_ERR_ARG;
  if (c->fpm_phase < 0) return fail(c, CSPM_ERR_STATE, "no candidate batch pending (cspm_fpm_candidates)");
  ON_DEVICE(c);
  Pm pm = make_pm(c, &c->fpm_params);
  const long long count = c->fpm_count;
  HIPCHK(c, hipMemcpyAsync(c->fpm.cost, cost, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
  switch (c->fpm_phase) {
    case CSPM_FPM_INIT:
    case CSPM_FPM_REFINE:
      hipLaunchKernelGGL(k_fpm_point_commit, dim3(ew_grid(count)), dim3(256), 0, c->stream, pm, c->fpm, c->fpm_phase == CSPM_FPM_REFINE ? 1 : 0);
      break;
    case CSPM_FPM_VIEW: {
      const size_t shmem = (size_t)c->W * (sizeof(unsigned long long) + sizeof(unsigned int));
      if (shmem > 160 * 1024) return fail(c, CSPM_ERR_ARG, "image too wide for the view-propagation row resolver");
      hipLaunchKernelGGL(k_fpm_view_commit, dim3(ew_grid(count)), dim3(256), 0, c->stream, pm, c->fpm, c->vc);
      LAUNCH_ONE(k_view_resolve, dim3(c->H), dim3(256), shmem, pm, c->fpm_step, c->fpm_iter % 2 == 0 ? 0 : 1, c->vc);
      break;
    }
    case CSPM_FPM_SPATIAL:
      hipLaunchKernelGGL(k_fpm_diag_commit, dim3(ew_grid(count / 2)), dim3(256), 0, c->stream, pm, c->fpm, c->fpm_step, c->fpm_inc);
      break;
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `cost` is the caller's buffer
  c->fpm_phase = -1;
  return CSPM_OK;
}

#ifdef CSPM_ROW_STATS
// debug build only (tools/row_stats.py): the row-engine statistics of cspm_rows.h g_rowstat
int cspm_debug_unionstat(unsigned long long *out64, int reset) {
  static unsigned long long z[64];
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(cspm::g_unionstat), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_unionstat), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
int cspm_debug_rowtime(unsigned long long *out64, int reset) {
  static unsigned long long z[64];
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(cspm::g_rowtime), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_rowtime), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
int cspm_debug_rangestats(unsigned long long *out1024, int reset) {
  static unsigned long long z[16 * 8 * 8];
  if (hipMemcpyFromSymbol(out1024, HIP_SYMBOL(cspm::g_rangestat), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_rangestat), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
// tools/row_paths.py: which leaf of level_rows' decision the level passes took, [2 views][16 slots][8 levels][128 leaves] (cspm_rows.h g_pathstat)
int cspm_debug_pathstats(unsigned long long *out32768, int reset) {
  static unsigned long long z[2 * 16 * 8 * cspm::kPathLeaves];
  if (hipMemcpyFromSymbol(out32768, HIP_SYMBOL(cspm::g_pathstat), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_pathstat), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
int cspm_debug_rowstats(unsigned long long *out1024, int reset) {
  static unsigned long long z[16 * 8 * 8];
  if (hipMemcpyFromSymbol(out1024, HIP_SYMBOL(cspm::g_rowstat), sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(cspm::g_rowstat), z, sizeof z) != hipSuccess) return CSPM_ERR_HIP;
  return CSPM_OK;
}
#endif

}  // extern "C"
