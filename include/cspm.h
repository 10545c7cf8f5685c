/*
 * cspm.h -- C ABI of libcspm_hip.so: the MI355X (gfx950) implementation of the PatchMatch-stereo
 * hot path of rookiepig/CrossScalePatchMatch (GRD plane cost, single-scale and cross-scale).
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference's
 * CSPM/ directory).  Conventions:
 *   - extern "C", plain pointers and sizes, no C++/torch types; int status: 0 = OK, < 0 = error
 *     (cspm_last_error() gives the text); no exceptions cross the boundary.
 *   - a cspm_ctx owns all device memory of ONE stereo pair on ONE GPU and ONE HIP stream; it is not
 *     thread-safe; use one ctx per host thread / stream.  Host buffers are caller-owned.
 *   - "view": 0 = left (kLeft), 1 = right (kRight)  (commfunc.h:29).
 *   - images are packed 8UC3 BGR, the layout cv::imread(CV_LOAD_IMAGE_COLOR) returns (main.cc:68-69).
 *   - the library has no CPU fallback: every call fails with CSPM_ERR_HIP when no gfx950 device is
 *     usable.
 */
#ifndef CSPM_H
#define CSPM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSPM_OK 0
#define CSPM_ERR_ARG (-1)   /* bad argument (the reference CV_Asserts or crashes) */
#define CSPM_ERR_HIP (-2)   /* HIP runtime error, no device, out of memory */
#define CSPM_ERR_STATE (-3) /* call order violated (e.g. patchmatch before a cost is built) */

#define CSPM_MAX_LEVELS 8

typedef struct cspm_ctx cspm_ctx;

/* SpatialPropagation schedule (cs_patchmatch.cc:163-216) */
#define CSPM_SCHED_RASTER 0   /* reference order: in-place raster sweep, run as an anti-diagonal wavefront */
#define CSPM_SCHED_REDBLACK 1 /* checkerboard half-steps (option: fewer dependencies, clearly lower quality) */
/* CSPM_SCHED_DIFFUSE (an addition): snapshot propagation.  One SpatialPropagation of iteration `iter` is
 * rb_rounds rounds.  A round copies both views' plane fields (the six doubles nx, ny, nz, a, b, c per pixel, no costs) into a
 * snapshot S; then every pixel (x, y) of every view v, independently of every other pixel, starts from m = its stored min_cost and
 * walks k = 0 .. K-1 in this order: (ox, oy) = inc * O_k with inc = +1 for even iter, -1 for odd iter; a neighbour (x+ox, y+oy)
 * outside the image is no candidate; otherwise the candidate is S[v][y+oy][x+ox] taken whole (normal and parameters as stored, nothing
 * re-anchored: how cs_patchmatch.cc:181-212 adopts a neighbour's Plane), cost = GetPlaneCost(x, y, candidate, v) in the device order,
 * and where cost < m (strict) the pixel's plane and min_cost become the candidate and its cost, and m = cost.
 * K = rb_neighbours is 4, 8 or 20 under this schedule; O_0 .. O_{K-1} as (ox, oy) are the first K entries of the lists below
 * (K = 20: the pattern of Galliani et al.'s Gipuma).  Needs a snapshot of 96 bytes per pixel, allocated by the first such call and
 * kept with the plane field.  No spin-waits, no timeout, every cost object; the foreign-IPlaneCost protocol stays raster-only. */
#define CSPM_SCHED_DIFFUSE 2
#define CSPM_DIFFUSE_MAX_NEIGHBOURS 20
#define CSPM_DIFFUSE_OFFSETS_4 {-1, 0}, {0, -1}, {1, 0}, {0, 1}
#define CSPM_DIFFUSE_OFFSETS_8 CSPM_DIFFUSE_OFFSETS_4, {-5, 0}, {0, -5}, {5, 0}, {0, 5}
#define CSPM_DIFFUSE_OFFSETS_20                                                                                     \
  CSPM_DIFFUSE_OFFSETS_4, {-3, 0}, {0, -3}, {3, 0}, {0, 3}, {-5, 0}, {0, -5}, {5, 0}, {0, 5}, {-1, -2}, {1, -2}, {2, -1}, \
      {2, 1}, {1, 2}, {-1, 2}, {-2, 1}, {-2, -1}

/* rng flags */
#define CSPM_RNG_PER_PIXEL 0
#define CSPM_RNG_ROW_SHARED 1 /* the USE_OMP per-row re-seeding quirk (cs_patchmatch.cc:129-131,308-310) */

typedef struct cspm_pm_params {
  uint64_t seed;     /* replaces RNG(time(NULL)), cs_patchmatch.cc:32 */
  int schedule;      /* CSPM_SCHED_* */
  int rb_rounds;     /* red-black / diffuse rounds per iteration (>= 1) */
  int rb_neighbours; /* 2 or 4; under CSPM_SCHED_DIFFUSE: 4, 8 or 20 */
  int rng_mode;      /* CSPM_RNG_* */
  int early_exit;    /* 1: stop a plane evaluation once its partial sum proves cost >= min_cost
                        (result-preserving; ignored when a scale weight or max_cost is negative) */
} cspm_pm_params;

/* ---- lifetime ------------------------------------------------------------------------------ */
int cspm_device_count(void);
int cspm_create(cspm_ctx **out, int device);
void cspm_destroy(cspm_ctx *ctx);
const char *cspm_last_error(const cspm_ctx *ctx); /* ctx may be NULL: error of a failed cspm_create */
/* run on a caller-provided hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream */
int cspm_set_stream(cspm_ctx *ctx, void *hip_stream);
/* the hipStream_t the ctx enqueues on (its own non-blocking stream unless cspm_set_stream replaced it): for callers that order their
 * own work against it (events, torch.cuda.ExternalStream).  The batch driver keeps one ctx-owned stream per pair in flight: streams a
 * framework hands out may share a hardware queue, and two pairs on one queue run one after the other. */
int cspm_get_stream(cspm_ctx *ctx, void **hip_stream_out);
int cspm_synchronize(cspm_ctx *ctx);

/* ---- images: PreSSPC/PreCSPC/CSPatchMatch constructors' (l_img, r_img) ----------------------
 * pre_ss_pc.cc:12-30, pre_cs_pc.cc:12-30, cs_patchmatch.cc:3-11.  stride in bytes (>= 3*w). */
int cspm_set_images(cspm_ctx *ctx, const uint8_t *l_bgr, const uint8_t *r_bgr, int w, int h, size_t stride);
/* same, from device memory already resident in HBM (bench / batch driver).  The copy kernels are enqueued on the ctx
 * stream and nothing waits for the host: the caller orders the PRODUCER of the buffers before this call (same stream,
 * an event the ctx stream waits on, or a synchronisation) and keeps them alive until the stream has passed the call. */
int cspm_set_images_device(cspm_ctx *ctx, const void *d_l_bgr, const void *d_r_bgr, int w, int h, size_t stride);

/* ---- plane cost construction ------------------------------------------------------------------
 * cspm_build_cost_grd = `new PreSSPC(l,r,max_dis,wnd,new GrdCC)` when scale_num == 0
 * (pre_ss_pc.cc:12-65) and `new PreCSPC(l,r,max_dis,wnd,scale_num,new GrdCC,reg_lambda)` when
 * scale_num >= 1 (pre_cs_pc.cc:12-115): pyramid, per-level GRD cost volumes of both views
 * (cc/grd_cc.cpp:60-154), max_cost, scale weights, exp LUT -- all on the device. */
int cspm_build_cost_grd(cspm_ctx *ctx, int max_dis, int wnd_size, int scale_num, double reg_lambda);
/* options (set before cspm_build_cost_grd).
 * CSPM_OPT_GRD_VOLUMES (applies to the GRD and the census cost): 0 (default) = cell costs are recomputed on the fly from the images and
 * gradients inside the PatchMatch kernels (bit-identical to reading GrdCC's volumes, no 1-30 GB cost
 * volume in HBM); 1 = materialise the d-major f64 volumes exactly as PreCSPC does (pre_cs_pc.cc:50-73)
 * and read them. */
#define CSPM_OPT_GRD_VOLUMES 1
/* CSPM_OPT_RASTER_LAUNCHES: 0 (default) = the reference-order raster sweep runs as ONE persistent launch whose
 * workgroups hand pixels over through per-pixel data-tagged granules (the final plane, polled directly); 1 = one launch per anti-diagonal (W+H-2 launches
 * per sweep; same results, kept as a cross-check). */
#define CSPM_OPT_RASTER_LAUNCHES 2
/* CSPM_OPT_SWEEP_TIMEOUT_MS (default 3000; 0 = every wait fails at once, for tests): how long a workgroup of the persistent sweep
 * waits for a predecessor pixel before the sweep gives up.  A timeout is slowness (shared GPU, profiler, many contexts in
 * flight), never a wrong result: when exactly one whole cspm_patchmatch ran since the last synchronising call, that call
 * repeats it with per-diagonal launches (identical planes) and reports success; otherwise it reports CSPM_ERR_HIP.
 * CSPM_OPT_SWEEP_FALLBACKS (read only): how many times that happened on this context. */
#define CSPM_OPT_SWEEP_TIMEOUT_MS 3
#define CSPM_OPT_SWEEP_FALLBACKS 4
/* CSPM_OPT_SWEEP_PAIRS (set before cspm_build_cost_grd; GRD with fused cells only; default 0): 1 = when they fit the context's
 * budget (4 GiB; a KITTI-size pair needs 2.2 GB, a 3000x2000 D=256 pair would need 56 GB and does without), the cost
 * constructor also materialises the GRD cells as PAIRS {cell(d), cell(d+1)} per (d, y, x) -- the two f64 cells a tap interpolates
 * between (pre_cs_pc.cc:171-176) -- and the raster sweep (SpatialPropagation, whose taps are gathers) reads one pair per tap instead
 * of recomputing two cells from three image gathers; every other kernel keeps the fused cells.  Same cells, same order: identical
 * planes.  Measured on MI355X: no faster than the fused sweep (20.4 vs 20.2 ms per sweep of a KITTI-size pair; the 16-byte gathers
 * into a 1 GB volume cost the L1 return path more than the three 12-byte image gathers they replace), hence off by default.
 * CSPM_OPT_SWEEP_PAIRS_ACTIVE (read only): 1 when the current cost object carries the pairs. */
#define CSPM_OPT_SWEEP_PAIRS 5
#define CSPM_OPT_SWEEP_PAIRS_ACTIVE 6
/* CSPM_OPT_TABLE_VOLUMES (set before cspm_build_cost_grd; GRD with fused cells only; default 1): when they fit the context's budget
 * (48 GiB -- the device has 288 GB; a KITTI-size pair needs 1.2 GB, a 3000x2000 D=256 pair 30 GB) the cost constructor also keeps the GRD
 * cells as d-major f64 volumes -- what PreCSPC keeps (pre_cs_pc.cc:50-73) -- and the row kernels (InitRandomPlane, ViewPropagation,
 * PlaneRefinement) fill their per-row cell tables from them by LDS-DMA instead of recomputing the cells, wherever a wave's lanes
 * agree on a narrow disparity range; everything else still computes cells on the fly.  Same cells: identical planes.  0 = never.
 * CSPM_OPT_TABLE_VOLUMES_ACTIVE (read only): 1 when the current cost object carries them.
 * Both kinds of optional volume (this one and CSPM_OPT_SWEEP_PAIRS) are accelerators, never a reason for a pair to fail: beyond the
 * per-context budgets they are taken only out of memory that hipMemGetInfo reports FREE when the cost object is allocated (at most
 * half of it, env CSPM_VOLUMES_MEM_FRACTION), and when a hipMalloc for one of them fails all the same the constructor releases them
 * and goes on with computed tables / the fused sweep -- identical results, as on a device with less HBM than MI355X's 288 GB.
 * CSPM_OPT_VOLUME_FALLBACKS (read only): how many times such an allocation failed on this context. */
#define CSPM_OPT_TABLE_VOLUMES 7
#define CSPM_OPT_TABLE_VOLUMES_ACTIVE 8
#define CSPM_OPT_VOLUME_FALLBACKS 9
/* CSPM_OPT_SWEEP_PACKED (set before cspm_build_cost_grd; GRD with fused cells only; default 0): 1 = the raster sweep (SpatialPropagation,
 * whose window taps are gathers) reads the level images as PACKED 8-byte pixels {36-bit fixed-point x-gradient, 24-bit colour} --
 * lossless: the gradient of an 8-bit image's f32 gray values (grd_cc.cpp:70-77) is a multiple of 2^-27 below 256 -- so that a tap's two
 * adjacent other-view pixels arrive with one 16-byte gather and its own pixel with one 8-byte gather (2 gathers / 24 B instead of
 * 3 / 36 B per tap through the CU's L1).  Same cells, same order: identical planes.  0 = the 12-byte pixels every other kernel reads.
 * Measured on MI355X: 8 % SLOWER (65.3 against 60.5 ms of sweeps per KITTI-size pair) although the microbenchmark confirms the L1 path
 * does a third less work -- the sweep is bound by the latency of its dependent steps, and unpacking adds instructions to each: off.
 * CSPM_OPT_SWEEP_PACKED_ACTIVE (read only): 1 when the current cost object carries the packed pixels.
 * CSPM_OPT_SWEEP_PACKED_BAD (read only; synchronises): pixels the packer could not represent exactly -- 0 by construction; counted per
 * cost object, and a non-zero count fails the next synchronising call with CSPM_ERR_HIP (the sweep would have read wrong cells). */
/* CSPM_OPT_SWEEP_FLOW (default 0; measured on MI355X: 1 is 35 % slower, 26.9 against 20.0 ms per sweep of a KITTI-size pair): how the
 * persistent raster sweep (CSPM_OPT_RASTER_LAUNCHES = 0) hands out its pixels.  1 = by dataflow:
 * every pixel counts its final predecessors and the workgroup that completes the count continues with it at once (the other ready
 * successor goes to a queue idle workgroups pop); 0 = workgroups claim pixels in diagonal-major order and wait for their predecessors.
 * The dependencies, hence the planes, are the same: the reference's in-place raster order (cs_patchmatch.cc:163-216). */
#define CSPM_OPT_SWEEP_FLOW 13
/* CSPM_OPT_SWEEP_WG (default 0 = the library chooses): workgroups of the persistent raster sweep launched per CU.  The library's choice is 2 --
 * a KITTI-size sweep is bound by its dependency chain (one: 29 instead of 20 ms per sweep; three: no faster) and every resident workgroup
 * holds registers another pair's kernels would use -- and 3 for images whose anti-diagonals are many times wider than the resident
 * workgroups (2 * min(w, h) >= 4 * CUs: 1242 x 600 27 instead of 31 ms per sweep, 3000 x 2000 215 instead of 275) unless CSPM_OPT_SWEEP_FOLD says that the GPU is
 * shared.  Any value gives identical planes. */
#define CSPM_OPT_SWEEP_WG 14
/* CSPM_OPT_VOLUME_RETRY_PAIRS (default 16; 0 = never): a cost object that wanted optional volumes and runs without them (free-memory veto
 * or a failed hipMalloc, see CSPM_OPT_TABLE_VOLUMES) asks for them again after this many pairs have reused it.
 * CSPM_OPT_FAULT_VOLUME_ALLOC (write only, TEST HOOK): the n-th optional-volume allocation of this context from now on fails as if
 * hipMalloc had returned out-of-memory; a set_option call, never the environment, so that no deployment can switch it on by accident. */
#define CSPM_OPT_VOLUME_RETRY_PAIRS 15
/* CSPM_OPT_VIEW_SORT (default 1): ViewPropagation (cs_patchmatch.cc:229-277) evaluates the proposals of a row in the order of their TARGET
 * column instead of their source column, so that the 64 proposals of a wavefront land next to each other in the target view even where
 * the source disparities jump (a depth edge); 0 = source order.  The accept rule (smallest cost, earliest in the reference's traversal
 * among equals, :256-272) is applied afterwards per target pixel and does not depend on the order of evaluation: identical planes. */
#define CSPM_OPT_VIEW_SORT 17
/* CSPM_OPT_SWEEP_FOLD (default 0; cross-scale costs with 4 or more levels): 1 = the raster sweep's workgroups have one wavefront FEWER than
 * the cost has pyramid levels -- four, one per SIMD, for the reference's five levels (main.cc:100) -- and the coarsest level is evaluated by
 * the wavefronts of levels 1.. after their own; 0 = one wavefront per level.  Same taps and sums: identical planes.  For callers that keep
 * TWO OR MORE pairs in flight on one GPU (contexts on separate streams): a CU that holds two four-wavefront sweep workgroups has room for
 * two workgroups of another pair's refinement where two five-wavefront ones leave room for one (of three), so the refinement beside a
 * sweep runs at 2/3 instead of 1/3 of its speed -- measured with 3 pairs in flight: 137.9 against 142.8 ms per KITTI-size pair.  A pair
 * that has the GPU to itself is slower folded (a sweep takes 23.0 instead of 20.2 ms: three wavefronts walk 5 window passes instead of 4).
 * With it, CSPM_OPT_SWEEP_WG stays at its default (2) also for three pairs in flight. */
#define CSPM_OPT_SWEEP_FOLD 18
#define CSPM_OPT_FAULT_VOLUME_ALLOC 16
#define CSPM_OPT_SWEEP_PACKED 10
#define CSPM_OPT_SWEEP_PACKED_ACTIVE 11
#define CSPM_OPT_SWEEP_PACKED_BAD 12
/* CSPM_OPT_CENGRD_FUSED (set before cspm_build_cost_cengrd; default 0): 0 = the CENGRD cost materialises its f64 volumes (see
 * cspm_build_cost_cengrd).  1 = no volume is allocated: the PatchMatch kernels compute the cell defined at cspm_build_cost_cengrd from the
 * level's colours, gradients and census codes as they go -- identical planes and costs, bit for bit -- and cspm_get_cost_slab, max_cost and
 * cspm_local_stereo compute the cells they need slab by slab.  The fused form holds 40 bytes per padded pixel (row stride W_s + 2 * (D_s +
 * wnd_size / 2 + 8)) and 13 per image pixel, per level and view; the volume form 24 and 13 + 8 * (D_s + 2).  The option is part of what a
 * cost object's buffers are reused for: changing it between two builds rebuilds.  The GRD-only accelerators (CSPM_OPT_TABLE_VOLUMES,
 * CSPM_OPT_SWEEP_PAIRS, CSPM_OPT_SWEEP_PACKED) do not apply; their _ACTIVE keys read 0.
 * CSPM_OPT_CENGRD_FUSED_ACTIVE (read only): 1 when the current cost object is a fused CENGRD one. */
#define CSPM_OPT_CENGRD_FUSED 19
#define CSPM_OPT_CENGRD_FUSED_ACTIVE 20
/* CSPM_OPT_PP_SPECKLE_REMOVED (read only; synchronises): pixels the speckle filter (cspm_set_pp_speckle) took out of the two consistency
 * masks, both views together, in the context's last post-processing; 0 when that ran without the filter. */
#define CSPM_OPT_PP_SPECKLE_REMOVED 21
/* CSPM_OPT_DEVICE_BYTES (read only; does not synchronise): the device memory the context holds, in bytes: the sum of the sizes it asked
 * of the allocator for the images, the cost object, the plane field with everything kept beside it, the rectification and the
 * local-stereo scratch.  Requested sizes (the allocator's rounding is not in it); the temporaries an entry stages caller memory
 * through are freed before it returns and are not counted.  0 for a fresh context; a pair that reuses every buffer leaves it unchanged. */
#define CSPM_OPT_DEVICE_BYTES 22
/* CSPM_OPT_SWEEP_GRID (write only, TEST HOOK; default 0 = the library's choice, see CSPM_OPT_SWEEP_WG): any other value caps the grid of
 * the persistent raster sweep at max(value, row bands) workgroups.  On an image small enough for a test the library's grid gives every
 * workgroup a handful of unrelated pixels; a grid of one workgroup per row band makes each workgroup walk its band pixel by pixel, so
 * that consecutive turns of its item loop are a pixel and its direct successor.  Any value gives identical planes.  A set_option call,
 * never the environment, like CSPM_OPT_FAULT_VOLUME_ALLOC. */
#define CSPM_OPT_SWEEP_GRID 23
int cspm_get_option(cspm_ctx *ctx, int key, long long *value);
int cspm_set_option(cspm_ctx *ctx, int key, long long value);
/* The same constructors with `new CenCC` (main.cc:43-45; cc/cen_cc.cc:4-137): 9x9 census codes of every level built on
 * the device; Hamming cells are computed on the fly from the codes (default) or materialised as f64 volumes
 * (CSPM_OPT_GRD_VOLUMES = 1), exactly like the GRD cost. */
int cspm_build_cost_cen(cspm_ctx *ctx, int max_dis, int wnd_size, int scale_num, double reg_lambda);
/* CENGRD (an addition): census and GRD blended per cell.  The reference reserves the slot -- GetCCType("CG") /
 * "BSM", main.cc:47-54 -- and defines nothing behind it; this is the library's own definition:
 *     cell = fma(CSPM_CENGRD_KAPPA, min(H, CSPM_CENGRD_TAU), G)
 * G = the GRD cell the device reads (what cspm_get_cost_slab returns after cspm_build_cost_grd: myCostGrd with its last multiply-add
 * contracted, border branch included), H = the census cell of cspm_build_cost_cen at the same (view, level, x, y, d) (80 where the
 * other view is outside).  KAPPA is a power of two and min(H, TAU) an integer, so the cell is G + KAPPA*min(H, TAU) rounded once.
 * Both constants are documented defaults, chosen, not tuned: the census part spans [0, 2.0], the GRD part [0, 2.8].
 * Same contract as the constructors above (everything on the ctx stream, buffers reused for an unchanged geometry, scale_num == 0 =
 * single scale).  By default the cost is volume-sourced -- d-major f64 volumes of D_s + 1 slabs per level and view, as
 * CSPM_OPT_GRD_VOLUMES = 1 gives the other two; that option has no effect here -- so every consumer of a cost object works on it
 * unchanged.  Volumes that do not fit fail the call with CSPM_ERR_HIP; CSPM_OPT_CENGRD_FUSED = 1 builds the same cost without them. */
#define CSPM_CENGRD_KAPPA 0.0625 /* 2^-4 */
#define CSPM_CENGRD_TAU 32.0
int cspm_build_cost_cengrd(cspm_ctx *ctx, int max_dis, int wnd_size, int scale_num, double reg_lambda);
/* The two volume-free IPlaneCost implementations the reference also ships (not instantiated by its main.cc):
 *   scale_num == 0 -> `new GrdPC(l_img, r_img, max_disp, wnd_size)`                          plane_cost/grd_pc.h:27-29, grd_pc.cc:11-66
 *   scale_num >= 1 -> `new CSPC(l_img, r_img, max_disp, wnd_size, scale_num, reg_lambda)`    plane_cost/cspc.h:21-23,  cspc.cc:11-93
 * GetPlaneCost (grd_pc.cc:72-176, cspc.cc:107-183) interpolates the other view's colour and 8U-gray x-gradient at the
 * real-valued column x -+ q_disp (wrap-around HandleBorder) instead of interpolating pre-computed cells; the "impossible
 * disparity" cost is the constant COST_ALPHA*TAU_CLR + (1-COST_ALPHA)*TAU_GRD.  cspm_get_cost_slab is an error for these.
 * max_dis > image width is refused with CSPM_ERR_ARG: HandleBorder (commfunc.h:129-145) wraps a column once, so with a disparity
 * beyond the width floor_x / ceil_x stay outside [0, width) and the reference reads past the row (grd_pc.cc:153-165,
 * cspc.cc:153-166); the other cost kinds take such a pair. */
int cspm_build_cost_img(cspm_ctx *ctx, int max_dis, int wnd_size, int scale_num, double reg_lambda);
/* Foreign CCMethod plugins (cc_method.h:31-32): allocate like the constructors above, then upload
 * the host volumes the plugin filled slab by slab, then finalize (max_cost reduction). */
int cspm_begin_cost(cspm_ctx *ctx, int max_dis, int wnd_size, int scale_num, double reg_lambda);
int cspm_upload_cost_slab(cspm_ctx *ctx, int view, int level, int d, const double *slab, size_t stride_elems);
int cspm_finish_cost(cspm_ctx *ctx);
/* introspection of what the constructor built (parity hooks) */
int cspm_get_levels(const cspm_ctx *ctx);
int cspm_get_level_dims(const cspm_ctx *ctx, int level, int *w, int *h, int *max_disp);
int cspm_get_level_image(cspm_ctx *ctx, int view, int level, uint8_t *bgr_out);     /* packed w*h*3 */
int cspm_get_cost_slab(cspm_ctx *ctx, int view, int level, int d, double *slab_out); /* packed w*h */
int cspm_get_max_cost(cspm_ctx *ctx, int view, int level, double *out);
int cspm_get_scale_weights(const cspm_ctx *ctx, double *out /* levels */);

/* CCMethod::buildCV / buildRightCV on host buffers (cc_method.h:31-32, cc/grd_cc.cpp:60-154):
 * l_rgb/r_rgb are h*w*3 doubles (CV_64FC3, RGB, 0..255), vol_out receives maxDis slabs of h*w. */
int cspm_grd_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis,
                           int right_view, double *vol_out);

/* CenCC::buildCV / buildRightCV on host buffers (cc/cen_cc.cc:4-70, 72-137), same contract as above */
int cspm_cen_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis,
                           int right_view, double *vol_out);

/* The same boundary for the CENGRD cells (class CenGrdCC of the host layer): input contract of the two entries above, cells as
 * defined at cspm_build_cost_cengrd -- the device form of G here too, so that there is one definition. */
int cspm_cengrd_build_cv_host(int device, const double *l_rgb, const double *r_rgb, int w, int h, int maxDis,
                              int right_view, double *vol_out);

/* ---- IPlaneCost::GetPlaneCost, batched (plane_cost/i_plane_cost.h:28-33) ----------------------
 * xy: 2 ints per item; plane: 6 doubles per item = Plane::norm() then Plane::param().
 * The cost is computed in the DEVICE ORDER: the same terms as the reference's serial sum in the
 * "ROWTREE7" association, with five multiply-adds per tap contracted into fmas (disparity, the last step of a GRD cell x2,
 * interpolation, accumulation); differs from the reference's SSE2 arithmetic by rounding only, <= 1e-12 relative. */
int cspm_plane_cost_batch(cspm_ctx *ctx, int view, int n, const int *xy, const double *norm_param, double *cost_out);

/* ---- CSPatchMatch ------------------------------------------------------------------------------
 * cspm_patchmatch = CSPatchMatch::PatchMatch(iter_num, plane_cost, false) without PlaneToDisp
 * (cs_patchmatch.cc:51-102); max_dis / images are those of the ctx.  params == NULL: cspm_pm_default_params (raster
 * schedule).  ASYNCHRONOUS: the kernels are enqueued on the ctx stream and the call returns; an error inside the run
 * (a raster sweep whose inter-workgroup hand-off timed out) is reported by the next call that synchronises with the
 * host: cspm_synchronize or any cspm_get_* / cspm_postprocess. */
int cspm_pm_default_params(cspm_pm_params *p);
int cspm_patchmatch(cspm_ctx *ctx, int iter_num, const cspm_pm_params *p);
/* single phases (cs_patchmatch.cc:115-148, 163-216, 229-277, 292-345) for phase-by-phase parity */
int cspm_pm_init(cspm_ctx *ctx, const cspm_pm_params *p);
int cspm_pm_spatial(cspm_ctx *ctx, int iter, const cspm_pm_params *p);
int cspm_pm_view(cspm_ctx *ctx, int iter, const cspm_pm_params *p);
int cspm_pm_refine(cspm_ctx *ctx, int iter, const cspm_pm_params *p);
/* plane field in/out: 6 doubles per pixel (norm, param), row-major h*w; min_cost h*w doubles */
int cspm_get_planes(cspm_ctx *ctx, int view, double *norm_param_out, double *min_cost_out);
int cspm_set_planes(cspm_ctx *ctx, int view, const double *norm_param, const double *min_cost);
/* ---- warm starts (an addition: PatchMatch from a plane field that is already there) -------------
 * re-score: min_cost of every stored plane of both views under the ctx's cost object, the planes untouched; the same evaluation as
 * the random init's, so re-scoring the field cspm_pm_init just wrote gives its costs bit for bit.  Asynchronous on the ctx stream.
 * CSPM_ERR_STATE without a cost object or without a plane field.  Timed under CSPM_K_INIT. */
int cspm_rescore_planes(cspm_ctx *ctx);
/* cspm_patchmatch with the random init replaced by a re-score of the stored field (skipped when the field's min_costs already belong
 * to this cost object: after a run, cspm_pm_init or a re-score).  Iterations 0 .. iter_num-1: the random streams and sweep directions
 * of a cold run, so a warm run from the field cspm_pm_init wrote is the cold run.  Asynchronous like cspm_patchmatch, with the same
 * transparent repeat after a sweep timeout: the starting field is copied aside on the device (both views, 14 doubles per pixel,
 * allocated by the first warm run and kept with the field).  CSPM_ERR_STATE without a cost object or a plane field; CSPM_ERR_ARG
 * for iter_num outside 0 .. 15 or bad params. */
int cspm_patchmatch_warm(cspm_ctx *ctx, int iter_num, const cspm_pm_params *p);
/* one pyramid level up: dst is w x h, src (same device) holds a plane field of exactly ((w+1)/2, (h+1)/2).  Every pixel (x, y) of
 * both views takes src's plane at (x>>1, y>>1) with the normal, a and b as they are and c doubled (d(x,y) = 2 d_src(x/2, y/2)).
 * min_cost is left stale (the field is not consistent: cspm_patchmatch_warm re-scores it).  Checks src's sweep first (like a getter),
 * then is asynchronous on dst's stream, ordered after the work enqueued on src's stream; src's later work waits for the copy.
 * CSPM_ERR_STATE when src has no plane field or dst no images; CSPM_ERR_ARG for other sizes or two devices. */
int cspm_upsample_planes(cspm_ctx *dst, cspm_ctx *src);
/* ---- candidate fields (an addition): hypotheses that win only where they are better ---------------------------
 * MERGE.  A view has a candidate plane field C (six doubles per pixel, norm then param, the layout of cspm_get_planes) and optionally a
 * mask.  Every pixel (x, y), independently of every other pixel: m = its stored min_cost; the candidate is C[y][x] taken whole (nothing
 * is re-anchored: how CSPM_SCHED_DIFFUSE adopts a neighbour); cost = GetPlaneCost(x, y, candidate, view) in the device order; where
 * cost < m (strict) the pixel's plane and min_cost become the candidate and its cost.  A pixel whose mask byte is 0, or whose six
 * candidate values are not all finite, has no candidate and is left unchanged.  The evaluation stops early exactly as plane refinement's
 * does (early_exit of the default parameters and the cost object's licence): result-preserving.
 * KEEP-INIT.  The same rule with the candidate being the plane InitRandomPlane draws for (x, y, view) under the given parameters (seed,
 * rng_mode: the streams of cspm_pm_init); the stored plane stays on a tie.  The merge seen from the other side: the stored field is the
 * seed, the random field the challenger.
 * Both need m to be the stored plane's cost under the current cost object: a field that is not consistent (after cspm_set_planes,
 * cspm_local_stereo, cspm_upsample_planes, a new cost object) is re-scored first, the rule of cspm_patchmatch_warm; both leave the field
 * consistent.  cspm_pm_init -> merge(s) -> cspm_patchmatch_warm(n), and cspm_pm_init_keep -> cspm_patchmatch_warm(n), are therefore
 * whole pipelines: the warm call skips its re-score and runs iterations 0 .. n-1 with a cold run's streams from the merged field.
 * All three are asynchronous on the ctx stream and timed under CSPM_K_INIT, one evaluation per pixel that has a candidate.
 *
 * cspm_merge_planes: both views, candidates = src's stored plane field (its min_costs are not used).  Same w x h, same device, src != dst.
 * Checks src's sweep first (like a getter), then is ordered after the work enqueued on src's stream; src's later work waits for the
 * merge.  CSPM_ERR_STATE when src has no plane field or dst lacks images, a cost object or a plane field; CSPM_ERR_ARG for a size
 * mismatch, two devices or src == dst. */
int cspm_merge_planes(cspm_ctx *dst, cspm_ctx *src);
/* one view, candidates from caller memory: norm_param h*w*6 doubles, mask h*w bytes or NULL (every pixel).  They are copied into a
 * ctx-owned candidate buffer (48 + 1 bytes per pixel, allocated by the first such call and kept with the plane field); the host buffers
 * are free for reuse when the call returns.  CSPM_ERR_STATE without a cost object or a plane field; CSPM_ERR_ARG for a bad view or a
 * NULL norm_param. */
int cspm_merge_planes_host(cspm_ctx *ctx, int view, const double *norm_param, const uint8_t *mask);
/* keep-init over both views.  Without a plane field it is cspm_pm_init (nothing is there to keep); CSPM_ERR_STATE without a cost
 * object; params as for cspm_pm_init. */
int cspm_pm_init_keep(cspm_ctx *ctx, const cspm_pm_params *p);
/* ---- plane fitting (an addition): slanted planes from a disparity map --------------------------------------------
 * F(D, V, I, radius r, max_diff t, min_support m, use_guide, max_dis) -> (planes, fitted) on one view: D a w x h f64 map, V w x h bytes
 * (NULL = all 1), I an 8-bit BGR guide (absent: use_guide = 0).  A pixel is a NODE when V = 1 and D is finite.  For a node p = (x, y) the
 * window is visited j = -r .. r outer, i = -r .. r inner, q = (x+i, y+j); a tap CONTRIBUTES when q is inside the image, q is a node and
 * fabs(D[q] - D[p]) <= t (false for a NaN; t may be +infinity); the centre always contributes.  Per contributing tap:
 *     wq = LUT[|dB| + |dG| + |dR|], LUT[k] = exp(-k/10) computed on the host with libm (1.0 when use_guide = 0);
 *     e = D[q] - D[p];  u = (double)i;  v = (double)j;
 *     S = S + wq * t for the nine sums Sw, Su, Sv, Suu, Suv, Svv, Se, Sue, Sve with t = 1, u, v, u*u, u*v, v*v, e, u*e, v*e
 * -- every product and every sum one IEEE f64 operation, nothing contracted, serial in the visiting order; n = contributing taps.  Then
 *     C00 = Svv*Sw - Sv*Sv   C01 = Suv*Sw - Sv*Su   C02 = Suv*Sv - Svv*Su
 *     C11 = Suu*Sw - Su*Su   C12 = Suu*Sv - Suv*Su  C22 = Suu*Svv - Suv*Suv
 *     det = (Suu*C00 - Suv*C01) + Su*C02
 * The fit is DEGENERATE when n < m or !(det > 1e-6 * ((Suu*Svv)*Sw)) (Hadamard: 0 <= det <= Suu*Svv*Sw, so the ratio is a scale-free
 * measure of collinearity; 1e-6 is a stated condition, not a tuned value): then a = b = c0 = 0.  Otherwise, with three true divisions,
 *     a  = ((C00*Sue - C01*Sve) + C02*Se) / det
 *     b  = ((C11*Sve - C01*Sue) - C12*Se) / det
 *     c0 = ((C02*Sue - C12*Sve) + C22*Se) / det
 * Output: t = D[p] + c0;  z = t > 0 ? t : 0;  z = z < max_dis ? z : max_dis;  normal = (-a, -b, 1) * (1 / max(len, 1e-8)) with
 * len = sqrt((a*a + b*b) + 1) summed in that order (InitRandomPlane's normalisation);  plane = Plane(normal, (x, y, z)): the stored a, b, c
 * are derived from the normal like every other plane of a field;  fitted[p] = 1.  A non-node gets six NaNs and fitted = 0: exactly "no
 * candidate" for cspm_merge_planes_host.
 * Defaults (chosen, not tuned): radius 5, max_diff 1.5, min_support 6, use_guide 1.  Every entry returns CSPM_ERR_ARG for a radius outside
 * 1 .. 17, min_support < 3 or a negative or NaN max_diff.  params == NULL: the defaults. */
typedef struct cspm_fit_params {
  int radius;       /* window half-width, 1 .. 17 */
  double max_diff;  /* t: a tap contributes when its disparity is within t of the centre's; +infinity = every node */
  int min_support;  /* m >= 3: fewer contributing taps give the fronto-parallel plane */
  int use_guide;    /* 1: taps are weighted by colour similarity to the centre */
} cspm_fit_params;
int cspm_fit_default_params(cspm_fit_params *p);
/* the fit alone on caller maps, no context needed (like cspm_filter_speckles_host): disp w*h doubles, valid w*h bytes or NULL, guide_bgr
 * packed 8UC3 BGR rows of guide_stride bytes (>= 3*w) or NULL (implies use_guide = 0); norm_param_out w*h*6 doubles in the layout of
 * cspm_get_planes, fitted_out w*h bytes or NULL.  Synchronous.  CSPM_ERR_ARG also for max_dis < 0 or h > 262140. */
int cspm_fit_planes_host(int device, const double *disp, const uint8_t *valid, const uint8_t *guide_bgr, size_t guide_stride, int w, int h,
                         int max_dis, const cspm_fit_params *p, double *norm_param_out, uint8_t *fitted_out);
/* both views of the context's plane field: D = the stored field's a*x+b*y+c (what cspm_get_disparity_f64 returns), computed into scratch
 * first so that the fit reads a snapshot and never its own output; V all 1; I the view's level-0 image; max_dis the context's (that of
 * its last cost constructor or cspm_fpm_begin).
 * merge = 0: every fitted pixel's plane is replaced; min_cost is left stale and the field is not consistent (as after cspm_local_stereo
 * or cspm_upsample_planes: cspm_patchmatch_warm re-scores).
 * merge = 1: the fitted planes go into the candidate buffer of cspm_merge_planes_host with `fitted` as the mask and are merged by that
 * entry's rule, one view after the other; a field that is not consistent is re-scored first, and the field is left consistent.
 * Asynchronous on the ctx stream.  Timed under CSPM_K_MISC: one bracket per view around the snapshot and the fit, w*h evaluations each;
 * the merge launches under CSPM_K_INIT as in cspm_merge_planes_host.  A whole run in front of it that has not been checked can no longer be
 * repeated (as with cspm_local_stereo).  Scratch: two doubles per pixel and the table, allocated by the first call and kept with the
 * plane field.  CSPM_ERR_STATE without images, a plane field or a known max_dis, and with merge = 1 without a cost object. */
int cspm_fit_planes(cspm_ctx *ctx, const cspm_fit_params *p, int merge);
/* ---- segment planes (an addition): one robustly fitted plane per superpixel ----------------------------------------
 * Everything whose result could depend on the order of a sum is done in integers, so a device may reduce in any order and still give
 * exactly these results.
 *
 * SEGMENTATION S(I, step s, compactness m, iters T) -> labels: I an 8-bit BGR w x h image.  Grid nx = ceil(w/s), ny = ceil(h/s), K = nx*ny
 * segments; segment k = gy*nx + gx has HOME CELL (gx, gy).  A centre is five integers (cx, cy, cb, cg, cr) in 1/16 units; it starts as 16 *
 * the coordinates and colour of the pixel (min(w-1, gx*s + s/2), min(h-1, gy*s + s/2)).  T times ASSIGN, then UPDATE:
 *   ASSIGN: pixel (x, y) has home cell (min(nx-1, x/s), min(ny-1, y/s)); its candidates are the up-to-nine segments of the 3 x 3 cells around
 *     it that exist, visited gy outer, gx inner, ascending.  Dist = dc*s*s + ds*m*m in 64-bit integers with
 *     dc = (16B-cb)^2 + (16G-cg)^2 + (16R-cr)^2 and ds = (16x-cx)^2 + (16y-cy)^2; the label is the first candidate with the strictly smallest Dist.
 *   UPDATE: for every segment with n > 0 member pixels every centre component becomes (2*Sum + n) / (2*n) by integer division, Sum = the sum
 *     of 16 * the members' value (a mean rounded half up); a segment with n = 0 keeps its centre.
 * Outputs: labels, a w x h int32 map, from the last ASSIGN; the centres and member counts of the UPDATE after it.  Connectivity is NOT enforced:
 * a segment is a label set inside the 3 x 3 cells around its home cell (the 3 x 3 PROPERTY), possibly in several pieces, possibly empty.
 * Magnitudes: a member lies within 2s of its segment's home-cell origin and so does the centre, a pixel and a candidate's centre are less than
 * 3s <= 192 pixels apart: ds < 2 * (16*192)^2 < 2^25, ds*m*m < 2^41; dc <= 3 * (16*255)^2 < 2^26, dc*s*s < 2^38: Dist < 2^42.  A centre
 * component is at most 16 * max(w, h, 255) and is stored as an int32.
 *
 * SEGMENT FIT P(D, V, labels, s, max_dis, tau, rounds R, min_support) -> (segment planes, inliers, per-pixel planes, fitted): D a w x h f64
 * map, V w x h bytes (NULL = all 1), labels any map with the 3 x 3 property.  A pixel is a NODE when V != 0 and fabs(D) <= 32768 (false for NaN
 * and inf).  For segment k with home-cell origin (ox, oy) = (gx*s, gy*s) a member node has u = x - ox, v = y - oy (-s <= u, v < 2s) and
 * q = llrint(D * 65536.0).  The nine sums over the SELECTED member nodes are exact 64-bit integer sums
 *     Sw = n, Su, Sv, Suu, Suv, Svv, Se = sum q, Sue = sum u*q, Sve = sum v*q
 * (at most 9*64^2 < 2^16 nodes, |u|, |v| <= 2^7, |q| <= 2^31: every sum stays below 2^54, far below 2^63), each converted to double once.
 * Then the cofactors C00 .. C22, det and the degeneracy test of "plane fitting" above, verbatim -- degenerate when n < min_support or
 * !(det > 1e-6 * ((Suu*Svv)*Sw)) -- and, with three true divisions followed by an exact scaling by 2^-16,
 *     a  = (((C00*Sue - C01*Sve) + C02*Se) / det) * 2^-16   b = (((C11*Sve - C01*Sue) - C12*Se) / det) * 2^-16
 *     c0 = (((C02*Sue - C12*Sve) + C22*Se) / det) * 2^-16
 * Round 0 selects every member node.  Round r = 1 .. R selects the member nodes with fabs(D - ((a*u + b*v) + c0)) <= tau * 2^(R-r) under
 * the previous round's plane (u, v as doubles; every operation one IEEE f64 operation, nothing contracted; the threshold shrinks 4 tau, 2 tau,
 * tau at the defaults).  A degenerate round 0 leaves the segment UNFITTED; a degenerate later round ends the rounds and keeps the previous
 * plane.  inliers = the n of the last round that produced the plane (0 for an unfitted segment).
 * Per segment: (a, b, c) with c = (c0 - a*ox) - b*oy, so that d(x, y) = a*x + b*y + c; three NaNs when unfitted.
 * Per pixel of a fitted segment, node or not (a hole receives its segment's plane): t = (a*u + b*v) + c0;  z = t > 0 ? t : 0;
 * z = z < max_dis ? z : max_dis;  normal and Plane(normal, (x, y, z)) exactly as "plane fitting" builds them;  fitted = 1.  A pixel of an
 * unfitted segment gets six NaNs and fitted = 0: exactly "no candidate" for cspm_merge_planes_host.
 * Defaults (chosen, not tuned): step 16, compactness 20, iters 5, tau 1.0, rounds 3, min_support 6.  Every entry returns CSPM_ERR_ARG for a
 * step outside 4 .. 64, a compactness outside 0 .. 255, iters outside 1 .. 16, rounds outside 0 .. 8, min_support < 3 or a negative or NaN tau
 * (+infinity is allowed).  params == NULL: the defaults. */
typedef struct cspm_seg_params {
  int step;         /* s: the grid spacing in pixels, 4 .. 64 */
  int compactness;  /* m: the weight of position against colour, 0 .. 255 */
  int iters;        /* T: ASSIGN + UPDATE repetitions, 1 .. 16 */
  double tau;       /* the last round's inlier threshold in disparities; +infinity = every round is plain least squares */
  int rounds;       /* R: re-fits on the inliers, 0 .. 8; 0 = plain least squares */
  int min_support;  /* >= 3: a round with fewer selected nodes is degenerate */
} cspm_seg_params;
int cspm_seg_default_params(cspm_seg_params *p);
/* K = ceil(w/step) * ceil(h/step); CSPM_ERR_ARG for w or h < 1 or a step outside 4 .. 64 */
int cspm_segment_count(int w, int h, int step);
/* S alone on caller memory, no context needed, synchronous: bgr packed 8UC3 rows of `stride` bytes (>= 3*w); labels_out w*h int32;
 * centres_out K*5 int32 (cx, cy, cb, cg, cr per segment) or NULL; counts_out K int32 or NULL.  Only step, compactness and iters are used
 * (all six are validated).  CSPM_ERR_ARG also for h > 262140 or w*h >= 2^31. */
int cspm_segment_host(int device, const uint8_t *bgr, size_t stride, int w, int h, const cspm_seg_params *p, int32_t *labels_out,
                      int32_t *centres_out, int32_t *counts_out);
/* P alone on caller memory, synchronous: disp w*h doubles, valid w*h bytes or NULL, labels w*h int32 for the grid of p->step.  The labels are
 * checked on the host first: CSPM_ERR_ARG unless every label has the 3 x 3 property (the device scans only those cells).  seg_planes_out
 * K*3 doubles (a, b, c) or NULL, inliers_out K int32 or NULL, norm_param_out w*h*6 doubles in the layout of cspm_get_planes, fitted_out w*h
 * bytes or NULL.  CSPM_ERR_ARG also for max_dis < 0. */
int cspm_segment_planes_host(int device, const double *disp, const uint8_t *valid, const int32_t *labels, int w, int h, int max_dis,
                             const cspm_seg_params *p, double *seg_planes_out, int32_t *inliers_out, double *norm_param_out, uint8_t *fitted_out);
/* both views of the context's plane field: I = the view's level-0 image, D = a snapshot of the stored field's a*x+b*y+c (what
 * cspm_get_disparity_f64 returns), V all 1, max_dis the context's.
 * merge = 0: the planes of fitted segments replace the stored ones (a pixel of an unfitted segment keeps its plane); min_cost is left stale
 * and the field is not consistent (cspm_patchmatch_warm re-scores).
 * merge = 1: the planes go into the candidate buffer of cspm_merge_planes_host with `fitted` as the mask and are merged by that entry's
 * rule, one view after the other; a field that is not consistent is re-scored first, and the field is left consistent.
 * Asynchronous on the ctx stream.  Timed under CSPM_K_MISC: one bracket per view around the snapshot, S and P, w*h evaluations each; the
 * merge launches under CSPM_K_INIT as in cspm_merge_planes_host.  A whole run in front of it that has not been checked can no longer be
 * repeated (as with cspm_fit_planes).  Scratch: 12 bytes per pixel and view (snapshot and labels) and 60 bytes per segment of the finest
 * grid, allocated by the first call and kept with the plane field.  The state rules are those of cspm_fit_planes: CSPM_ERR_STATE without
 * images, a plane field or a known max_dis, and with merge = 1 without a cost object. */
int cspm_segment_planes(cspm_ctx *ctx, const cspm_seg_params *p, int merge);
/* the labels (w*h int32) of the last cspm_segment_planes call for one view; synchronising.  CSPM_ERR_STATE if there was none. */
int cspm_get_segments(cspm_ctx *ctx, int view, int32_t *labels_out);
/* PlaneToDisp + dis() (cs_patchmatch.cc:590-601, 111-113): saturate_u8(Round2Int(d*dis_scale)) */
int cspm_get_disparity_u8(cspm_ctx *ctx, int view, int dis_scale, uint8_t *out, size_t stride);
int cspm_get_disparity_f64(cspm_ctx *ctx, int view, double *out); /* unquantised a*x+b*y+c */
/* device-resident result (u8, packed w*h) for the batch driver.  Asynchronous; when the PatchMatch run in front of it is repeated
 * after a sweep timeout (CSPM_OPT_SWEEP_TIMEOUT_MS), the map is written again from the repeated run's planes before the
 * synchronising call returns success.
 * CONTRACT for every asynchronous output (this call, cspm_postprocess_device and cspm_postprocess_f64_device): the buffer must stay allocated, and its contents
 * must not be consumed, until a synchronising cspm_* call on this ctx (cspm_synchronize, any cspm_get_*, cspm_postprocess) has
 * returned CSPM_OK after the request.  Synchronising the stream or an event of your own is NOT enough: only the cspm_* call looks at
 * the sweep's error word, and if the sweep timed out the map that stream-side synchronisation sees was written from the aborted run
 * and is rewritten inside that cspm_* call.  Repeated requests for the same (buffer, kind) between two synchronising calls are
 * recorded once. */
int cspm_disparity_u8_device(cspm_ctx *ctx, int view, int dis_scale, void *d_out);
/* PostProcessing (cs_patchmatch.cc:508-588) on the 8-bit maps */
int cspm_postprocess(cspm_ctx *ctx, int dis_scale, uint8_t *l_out, uint8_t *r_out, size_t stride);
/* the same with device-resident outputs (u8, packed w*h each); asynchronous on the ctx stream like cspm_patchmatch --
 * PatchMatch(iter_num, plane_cost, use_pp = true) without leaving the device (cs_patchmatch.cc:103-107) */
int cspm_postprocess_device(cspm_ctx *ctx, int dis_scale, void *d_l_out, void *d_r_out);
/* sub-pixel PostProcessing (an addition): the reference's three steps -- left-right check, fill, weighted
 * median -- on the unquantised a*x+b*y+c of both views instead of the 8-bit maps.  Needs a plane field, a cost object and images,
 * like cspm_postprocess.  l_out / r_out: w*h doubles each (packed rows); valid pixels hold what cspm_get_disparity_f64 returns,
 * inconsistent ones the filled (clamped to [0, max_dis]) or median value.  l_valid_out / r_valid_out (w*h bytes each, 1 = the pixel
 * passed the left-right check) may be NULL.  Synchronises.  The 8-bit maps are untouched: cspm_postprocess before or after this
 * call gives what it gives alone, and vice versa. */
int cspm_postprocess_f64(cspm_ctx *ctx, double *l_out, double *r_out, uint8_t *l_valid_out, uint8_t *r_valid_out);
/* device-resident outputs (packed w*h f64 each), asynchronous on the ctx stream; the CONTRACT for asynchronous outputs above holds */
int cspm_postprocess_f64_device(cspm_ctx *ctx, void *d_l_out, void *d_r_out);

/* speckle filter (an addition), a step of all four post-processing entries above, between the left-right check
 * and the fill.  S(D, V, max_size, max_diff) -> V' on one view's map D and its consistency mask V: nodes are the pixels with V = 1; two
 * nodes are joined when they are 4-neighbours and |D[p] - D[q]| <= max_diff (in f64; false when either is NaN; pairwise, not against a
 * seed); n(p) = size of p's connected component, 0 for a non-node; V'[p] = V[p] && n(p) > max_size.  Fill and weighted median then see
 * V' as they see V without the filter (a removed pixel is filled, is medianed and does not vote), and the masks cspm_postprocess_f64
 * returns are V'.  The f64 entries filter the unquantised a*x+b*y+c maps; the 8-bit entries (double)byte with the threshold
 * max_diff * dis_scale (one f64 product).  max_size == 0 (the default; max_diff defaults to 1.0) = no filter: no launch, no memory.
 * Scratch: two int32 per pixel and view (and one counter), allocated by the first filtered post-processing and kept with the plane field.
 * Timed under CSPM_K_POST.  CSPM_ERR_ARG for max_size < 0 or a max_diff that is negative or not finite; the getter's outputs may be NULL. */
int cspm_set_pp_speckle(cspm_ctx *ctx, int max_size, double max_diff);
int cspm_get_pp_speckle(cspm_ctx *ctx, int *max_size, double *max_diff);
/* the filter alone on caller maps, no context needed: disp w*h doubles, valid w*h bytes (NULL = every pixel is a node), valid_out w*h
 * bytes = V', size_out (may be NULL) w*h int32 = n(p).  max_diff may be +infinity here (the mask's own components).  CSPM_ERR_ARG for
 * max_size < 0, a negative or NaN max_diff, or w*h >= 2^31 (labels are 32-bit pixel indices). */
int cspm_filter_speckles_host(int device, const double *disp, const uint8_t *valid, int w, int h, int max_size, double max_diff,
                              uint8_t *valid_out, int32_t *size_out);

/* median filter (an addition): the reference's MedianFilter (commfunc.cc:11-25; the call PostProcessing keeps
 * commented out, cs_patchmatch.cc:573-575), restated from its behaviour.  Window of radius r: the (2r+1)^2 taps
 * D[clamp(y+j, 0, h-1)][clamp(x+i, 0, w-1)], i, j in -r .. r (the border is replicated), defined for every w, h >= 1.
 *   M8(D, r), 8-bit, cn interleaved channels: out[y][x][c] = the tap of 0-based rank 2r^2 + 2r among the window's values of channel c.
 *   M64(D, r), f64: a NaN tap does not vote; a NaN centre stays as it is (the same bits); otherwise, with n >= 1 voting taps, the tap
 *     of 0-based rank (n - 1) / 2 (integer division: the lower median) in the total order of the order-preserving 64-bit key of the
 *     bit pattern (-inf < finite < +inf, -0.0 < +0.0).  The output is a tap's own bits: nothing is averaged or rounded.  Without
 *     NaNs the rank is 2r^2 + 2r, and M64 of integer-valued data equals M8.
 * Both read a snapshot, never their own output. */
#define CSPM_MEDIAN_MAX_RADIUS 7
/* M8 / M64 alone on caller memory, no context needed, synchronous.  u8: channels 1 .. 4, strides in bytes and >= w * channels; f64:
 * packed w*h maps.  r in 1 .. CSPM_MEDIAN_MAX_RADIUS.  CSPM_ERR_ARG for a radius or channels outside the range, a NULL buffer, a
 * stride below w * channels, w or h < 1, or src == dst. */
int cspm_median_filter_u8_host(int device, const uint8_t *src, size_t src_stride, int w, int h, int channels, int r, uint8_t *dst,
                               size_t dst_stride);
int cspm_median_filter_f64_host(int device, const double *src, int w, int h, int r, double *dst);
/* the filter as the LAST step of all four post-processing entries above, after the weighted median, on every pixel of both views:
 * cspm_postprocess and cspm_postprocess_device run M8 (one channel) on the 8-bit maps, the two f64 entries M64 on the f64 maps; the
 * consistency masks cspm_postprocess_f64 returns are not changed.  r = 0 (the default) = off: no launch, no memory, today's bytes.
 * The filter writes into a second buffer per view, which then is the map; it is allocated by the first filtered call and kept with the
 * plane field.  Timed under CSPM_K_POST as a bracket of its own.  CSPM_ERR_ARG for r outside 0 .. CSPM_MEDIAN_MAX_RADIUS or a NULL r. */
int cspm_set_pp_median(cspm_ctx *ctx, int r);
int cspm_get_pp_median(cspm_ctx *ctx, int *r);

/* edge-aware global smoothing (an addition): the fast global smoother on an f64 disparity map,
 * S(D, C, I, lambda, sigma, T, max_dis) -> O on one view.  D: w x h f64; C: w x h f64 confidences in [0, 1] (absent: all 1); I: an 8-bit BGR
 * guide (absent: every weight is 1.0).  A pixel is a node when D is finite; c[p] = C[p] at a node and 0.0 elsewhere; N[p] = c[p] * D[p] at a
 * node and 0.0 elsewhere; M[p] = c[p].
 * Weights: LUT[k] = exp(-k / sigma), k = 0 .. 765, by the host's libm; between horizontal neighbours (x, y) and (x+1, y) the weight is
 * LUT[|dB| + |dG| + |dR|], between vertical neighbours likewise.
 * Schedule: for t = 1 .. T, lambda_t = ((1.5 * 4^(T-t)) / (4^T - 1)) * lambda (exact powers, one division, one multiplication, on the host),
 * then a horizontal pass over every row and a vertical pass over every column.
 * A pass replaces N and M on each line of length n by the solution of one tridiagonal system with the two right-hand sides.  Per element i, with
 * wl the weight to i-1 and wr the weight to i+1:  a = -(lambda_t * wl), or 0.0 at i = 0;  cc = -(lambda_t * wr), or 0.0 at i = n-1;
 * b = (1.0 - a) - cc.  Forward, serial in i:  r = 1.0 / b, ct[0] = cc * r, ft[0] = F[0] * r;  for i >= 1  r = 1.0 / (b - ct[i-1] * a),
 * ct[i] = cc * r, ft[i] = (F[i] - ft[i-1] * a) * r.  Backward:  U[n-1] = ft[n-1], U[i] = ft[i] - ct[i] * U[i+1].  F is N for one right-hand side
 * and M for the other; ct and r are shared.  One true division per element; every product, sum and difference is one IEEE f64 operation,
 * nothing contracted; the serial order is part of the definition.  The system is strictly diagonally dominant: no pivoting, no singular case.
 * Output: O[p] = N[p] / M[p] where M[p] > 0 (false for a NaN), elsewhere D[p]'s own bits; where max_dis > 0 a quotient t is clamped as the
 * plane fit clamps: z = t > 0 ? t : 0; z = z < max_dis ? z : max_dis.  A non-node with a confident pixel in reach is filled: intended.
 * Defaults (chosen, not tuned): lambda 100, sigma_color 20, iterations 3, fill_conf 0.25. */
typedef struct cspm_smooth_params {
  double lambda;      /* >= 0 and finite; 0 switches cspm_set_pp_smooth off */
  double sigma_color; /* > 0 and finite */
  int iterations;     /* T, 1 .. 8 */
  double fill_conf;   /* cspm_set_pp_smooth only: the confidence of a pixel that failed the left-right check, in [0, 1] */
} cspm_smooth_params;
int cspm_smooth_default_params(cspm_smooth_params *p);
/* S alone on caller memory, no context needed (like cspm_filter_speckles_host), synchronous.  disp, out: packed w*h doubles; conf: w*h doubles
 * or NULL; guide_bgr: packed 8UC3 rows of 3*w bytes or NULL; params NULL = the defaults, fill_conf is ignored; max_dis 0 = no clamp.
 * CSPM_ERR_ARG, before a device is opened, for lambda < 0, NaN or infinite, sigma_color <= 0 or not finite, iterations outside 1 .. 8, a
 * confidence outside [0, 1] or NaN (the host scans the map), a NULL disp or out, w or h < 1, max_dis < 0, or out == disp. */
int cspm_smooth_disparity_host(int device, const double *disp, const double *conf, const uint8_t *guide_bgr, int w, int h,
                               const cspm_smooth_params *params, int max_dis, double *out);
/* S as the LAST step of cspm_postprocess_f64 and cspm_postprocess_f64_device, after the weighted median and after the median filter when
 * that is on, on both views: C = 1.0 where the view's final consistency mask (after the speckle filter) is 1 and fill_conf elsewhere, I = the
 * view's level-0 image, max_dis the context's.  The masks the entries return are not changed, and the CSPM_GEOM_PP / PP sources of
 * cspm_reproject* and cspm_synthesize* read the smoothed maps.  The 8-bit entries cspm_postprocess and cspm_postprocess_device are NOT
 * affected.  params NULL or lambda == 0 = off (the default): no launch, no memory, today's bytes.  Scratch (three maps per view and the
 * table) is allocated by the first smoothed call and kept with the plane field.  Timed under CSPM_K_POST as a bracket of its own.
 * CSPM_ERR_ARG as above, and for a fill_conf outside [0, 1].  The getter's outputs may be NULL; *on = 1 while smoothing is switched on. */
int cspm_set_pp_smooth(cspm_ctx *ctx, const cspm_smooth_params *params);
int cspm_get_pp_smooth(cspm_ctx *ctx, cspm_smooth_params *params, int *on);

/* ---- reprojection (an addition): metric depth, camera-space points, unit normals, a point cloud ---------------------
 * A plane in disparity space is a plane in 3-D: with x = f X/Z + cx, y = f Y/Z + cy, d + doffs = f B/Z the disparity plane d = a x + b y + c
 * is  a f X + b f Y + (a cx + b cy + c + doffs) Z = f B  -- exact, no finite differences.
 * G(calib, params, view v, D, V, A, Bs, I) on one view: D a w x h f64 disparity map, V w x h bytes (NULL = all 1), slopes A, Bs w x h f64
 * (NULL = no normals), I an 8-bit BGR image (NULL = no colour).  Every product, sum, quotient and square root is one IEEE f64 operation in
 * the association written here, nothing contracted, no reciprocal.  The host computes once cxv = cx + (double)v * doffs and fB = f * baseline.
 * Per pixel (x, y):
 *     t  = D + doffs
 *     ok = V != 0 && isfinite(D) && t > 0.0
 *     Z  = fB / t
 *     u  = (double)x - cxv          wv = (double)y - cy
 *     X  = (u * Z) / f              Y  = (wv * Z) / f
 *     if (left_frame && v == 1) X = X + baseline
 *     ok = ok && Z >= z_near && Z <= z_far
 * and with slopes
 *     n0  = A * f    n1 = Bs * f    n2 = (t - A*u) - Bs*wv
 *     len = sqrt((n0*n0 + n1*n1) + n2*n2)
 *     N   = (-n0/len, -n1/len, -n2/len)                       the unit normal facing the camera, three divisions
 *     cos = (f * t) / (len * sqrt((u*u + wv*wv) + f*f))       the cosine between the normal and the view ray
 * n . (u, wv, f) = f t, so cos > 0 whenever t > 0: a plane is never seen from behind.  A non-finite A or Bs gives NaN normals and a NaN
 * cos without a branch.  keep = ok && (no slopes || min_cos == 0.0 || cos >= min_cos); a NaN cos fails the test.
 * Dense outputs, each optional (NULL) and untouched when not requested: depth = Z where ok, NaN elsewhere; xyz = three w x h planes X, Y, Z,
 * NaN where !ok; normal = three planes, NaN where !ok (without slopes: CSPM_ERR_ARG); keep = w x h bytes.
 * Cloud: the kept pixels in raster order (y outer, x inner), one 32-byte cspm_point each: the six floats are (float) of the f64 values, round
 * to nearest (NaN stays NaN; without slopes the normal is NaN); pixel = y*w + x; b, g, r from the image and a = 255, without an image all
 * four bytes 0.  *count = the number of kept pixels whatever the capacity; when count > cloud_cap the first cloud_cap records in raster
 * order are written and the rest of the buffer is untouched; a NULL cloud asks for the count only; count_out may be NULL.  w*h < 2^31.
 * Calibration: valid when all five values are finite, f > 0 and baseline > 0.  Parameters (NULL = the defaults 0, +infinity, 0, 0, 0):
 * CSPM_ERR_ARG for a NaN or negative z_near, a z_far that is NaN or below z_near, a min_cos outside [0, 1]. */
typedef struct cspm_calib {
  double f;        /* focal length in pixels */
  double cx, cy;   /* principal point of view 0 */
  double baseline; /* any length unit: the outputs are in that unit */
  double doffs;    /* cx1 - cx0 */
} cspm_calib;
typedef struct cspm_geom_params {
  double z_near, z_far; /* ok only for z_near <= Z <= z_far (both inclusive) */
  double min_cos;       /* keep only pixels whose normal makes at least this cosine with the view ray; 0 = every ok pixel */
  int left_frame;       /* 1: view 1's points are moved into view 0's camera frame (X + baseline) */
  int consistent_only;  /* cspm_reproject(_device), CSPM_GEOM_PP: V = the left-right consistency mask instead of all 1 */
} cspm_geom_params;
typedef struct cspm_point {
  float x, y, z, nx, ny, nz;
  uint8_t b, g, r, a;
  uint32_t pixel;
} cspm_point;
int cspm_geom_default_params(cspm_geom_params *p);
/* G alone on caller memory, no context needed (like cspm_fit_planes_host), synchronous.  slope_a and slope_b come together or not at all;
 * bgr: packed 8UC3 rows of bgr_stride bytes (>= 3*w) or NULL.  Arguments are checked before a device is opened: CSPM_ERR_ARG for a bad
 * calibration, parameters or view, a NULL disp, w or h < 1, w*h >= 2^31, one slope map without the other, normal_out without slopes, or
 * a bgr_stride below 3*w. */
int cspm_reproject_host(int device, const cspm_calib *calib, const cspm_geom_params *params, int view, const double *disp, const uint8_t *valid,
                        const double *slope_a, const double *slope_b, const uint8_t *bgr, size_t bgr_stride, int w, int h, double *depth_out,
                        double *xyz_out, double *normal_out, uint8_t *keep_out, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out);
/* G on one view of the context's stored plane field; I = the view's level-0 image.  source:
 *   CSPM_GEOM_RAW  D = the field's a*x+b*y+c (what cspm_get_disparity_f64 returns) written into scratch; V all 1; slopes = the field's a, b.
 *   CSPM_GEOM_PP   D = the view's map of the sub-pixel post-processing (cspm_postprocess_f64, with the context's speckle and median
 *                  settings), which this call runs itself, by the path that entry takes, so that the map always belongs to the stored field;
 *                  V all 1, or the consistency mask that entry returns when consistent_only; slopes = the field's a, b where the pixel
 *                  passed the check (that mask) and NaN elsewhere: a filled pixel has a disparity but no plane of its own.
 * fit != NULL replaces the slopes of EVERY pixel by those of the plane fit F (cspm_fit_planes_host) applied to (D, V) with the level-0 image
 * as guide and the context's max_dis, computed into scratch; an unfitted pixel gets NaN slopes.
 * Like cspm_get_disparity_f64 the entry first checks a pending run, so it never reads planes of an aborted sweep.  Synchronous; host outputs.
 * Timed as one CSPM_K_MISC bracket per call with w*h evaluations (CSPM_GEOM_PP: behind the post-processing's own CSPM_K_POST brackets).
 * Scratch (a map, six fit planes and the counts) is allocated on first use and freed with the plane field.
 * CSPM_ERR_ARG for a bad view, source, calibration, parameters or fit parameters; CSPM_ERR_STATE without images
 * or a plane field, and without a cost object when source is CSPM_GEOM_PP or fit is given (these need max_dis). */
#define CSPM_GEOM_RAW 0
#define CSPM_GEOM_PP 1
int cspm_reproject(cspm_ctx *ctx, int view, int source, const cspm_calib *calib, const cspm_geom_params *params, const cspm_fit_params *fit,
                   double *depth_out, double *xyz_out, double *normal_out, uint8_t *keep_out, cspm_point *cloud_out, size_t cloud_cap,
                   unsigned int *count_out);
/* the same with device pointers for every output (d_cloud_out 16-byte aligned) and a device unsigned int for the count.  Makes the same
 * pending-run check on entry, then enqueues on the ctx stream and returns.  Deliberately NOT part of the deferred-output replay of the
 * asynchronous outputs above: a run enqueued BEHIND this call that times out and is repeated does not rewrite these buffers -- they hold
 * the geometry of the field as it was checked on entry, which is what was asked for. */
int cspm_reproject_device(cspm_ctx *ctx, int view, int source, const cspm_calib *calib, const cspm_geom_params *params,
                          const cspm_fit_params *fit, void *d_depth_out, void *d_xyz_out, void *d_normal_out, void *d_keep_out, void *d_cloud_out,
                          size_t cloud_cap, void *d_count_out);

/* ---- triangle meshes (an addition): a surface from one view's plane field --------------------------------------------
 * Neighbouring pixels are connected when each one's plane predicts the other's disparity, so a steep surface stays whole where the plain
 * difference test |D_p - D_q| <= tau tears it, and a real step is cut where a larger tau would bridge it.
 * M(calib, geom params, mesh params, view v, D, V, A, Bs, I): the inputs of one view are exactly those of G above, and
 * cspm_mesh_params { max_diff (tau), all_vertices }.  Every operation is one IEEE f64 operation in the association written here, nothing
 * contracted.
 * Candidate vertices: K(p) = G's keep of pixel p; a vertex sits at the pixel's point (X, Y, Z) of G with G's normal.
 * Slopes of the edge test: (a_p, b_p) = the pixel's (A, Bs) when both are finite, else (0, 0) (no slope maps, a slope mask of 0 on the
 * CSPM_GEOM_PP source, NaN or infinite slopes).
 * Edge predicate, for two kept pixels s, t at most one pixel apart in x and in y:
 *     pred(s,t) = (D_s + a_s * (double)(x_t - x_s)) + b_s * (double)(y_t - y_s)
 *     E(s,t)    = fabs(pred(s,t) - D_t) <= tau  &&  fabs(pred(t,s) - D_s) <= tau
 * E is symmetric and depends on the two end points only: an edge shared by two quads gets one answer.
 * Quads: one at every origin (x, y), 0 <= x < w-1, 0 <= y < h-1, with corners p00 = (x,y), p10 = (x+1,y), p01 = (x,y+1), p11 = (x+1,y+1):
 *     main_ok = K(p00) && K(p11);   anti_ok = K(p10) && K(p01)
 *     split = none   if !main_ok && !anti_ok
 *           = main   if main_ok && !anti_ok
 *           = anti   if anti_ok && !main_ok
 *           = (fabs(D00 - D11) <= fabs(D10 - D01)) ? main : anti     otherwise (a tie takes main)
 *     main:  T0 = (p00, p01, p11)   T1 = (p00, p11, p10)
 *     anti:  T0 = (p00, p01, p10)   T1 = (p10, p01, p11)
 * A triangle of the chosen split is emitted iff its three corners are kept and E holds on its three edges.  All four triangles have the
 * same orientation in the image plane; seen from the camera (x right, y down) the corners run counter-clockwise, so that the geometric
 * normal (P1 - P0) x (P2 - P0) faces the camera like G's normals.
 * Quad byte Q(x,y): bit 0 = T0 is emitted, bit 1 = T1 is emitted, bit 2 = the split is anti; 0 in the last column, the last row and for
 * split none.
 * Vertices: pixel p is a vertex iff K(p) && (all_vertices || p is a corner of an emitted triangle); numbered in raster order (y outer, x
 * inner); each one cspm_point built exactly as G's cloud record of that pixel (with all_vertices the vertices ARE G's cloud).
 * Faces: one 12-byte cspm_face each, in raster order of the quad origin, T0 before T1; v[] = the vertex numbers of the corners in the order
 * written above.
 * Counts and capacities: *n_vertices and *n_faces are reported whatever the capacities; when a count exceeds its capacity the first `cap`
 * records are written and the rest of the buffer is untouched.  Faces always carry full vertex numbers, so THE MESH IS COMPLETE ONLY WHEN
 * BOTH COUNTS FIT: a face may then name a vertex beyond vertex_cap.  NULL buffers ask for the counts only; the count pointers may be NULL.
 * w*h < 2^31.  An image with w == 1 or h == 1 has no quads and so no faces.
 * Parameters (NULL = the defaults 1.0, 0): CSPM_ERR_ARG for a NaN or negative max_diff; +infinity is allowed. */
typedef struct cspm_mesh_params {
  double max_diff;  /* tau of the edge predicate, in disparity units */
  int all_vertices; /* 1: every kept pixel is a vertex; 0: only the corners of emitted triangles */
} cspm_mesh_params;
typedef struct cspm_face {
  uint32_t v[3];
} cspm_face;
int cspm_mesh_default_params(cspm_mesh_params *p);
/* M alone on caller memory with a temporary context, synchronous; the inputs as for cspm_reproject_host.  quad_out: w*h bytes or NULL.
 * Arguments are checked before a device is opened: CSPM_ERR_ARG for what cspm_reproject_host refuses in these inputs and for a bad
 * max_diff. */
int cspm_mesh_host(int device, const cspm_calib *calib, const cspm_geom_params *geom_params, const cspm_mesh_params *mesh_params, int view,
                   const double *disp, const uint8_t *valid, const double *slope_a, const double *slope_b, const uint8_t *bgr, size_t bgr_stride,
                   int w, int h, cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap, uint8_t *quad_out,
                   unsigned int *n_vertices_out, unsigned int *n_faces_out);
/* M on one view of the context's stored plane field.  source, consistent_only and fit mean exactly what they mean in cspm_reproject, and
 * the inputs are prepared by the same code; the same pending-run check is made before the field is read.  Synchronous; host outputs.
 * Timed as one CSPM_K_MISC bracket per call with w*h evaluations (CSPM_GEOM_PP: behind the post-processing's own CSPM_K_POST brackets).
 * Scratch (keep and Q bytes, a 32-bit pixel -> vertex map and two count arrays) is allocated on first use and freed with the plane field.
 * The error classes of cspm_reproject, and CSPM_ERR_ARG for a bad max_diff. */
int cspm_mesh(cspm_ctx *ctx, int view, int source, const cspm_calib *calib, const cspm_geom_params *geom_params, const cspm_fit_params *fit,
              const cspm_mesh_params *mesh_params, cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap,
              uint8_t *quad_out, unsigned int *n_vertices_out, unsigned int *n_faces_out);
/* the same with device pointers for every output (vertices 16-byte aligned, faces and the counts 4-byte aligned; the two counts are device
 * unsigned ints).  Makes the same pending-run check on entry, then enqueues on the ctx stream and returns.  Like cspm_reproject_device
 * it is NOT part of the deferred-output replay, for the reason given there. */
int cspm_mesh_device(cspm_ctx *ctx, int view, int source, const cspm_calib *calib, const cspm_geom_params *geom_params, const cspm_fit_params *fit,
                     const cspm_mesh_params *mesh_params, void *d_vertices_out, size_t vertex_cap, void *d_faces_out, size_t face_cap,
                     void *d_quad_out, void *d_n_vertices_out, void *d_n_faces_out);

/* ---- view synthesis (an addition): the scene rendered from a camera between (or at) the two views ----------------------
 * A rectified warp never leaves its image row, and a slanted plane says how one source pixel stretches or compresses in the target view,
 * so a surface is rasterised exactly, without cracks, instead of splatting rounded disparities.
 * N(t, params, per view v in {0, 1}: D_v, V_v, A_v, I_v): D a w x h f64 disparity map, V w x h bytes (NULL = all 1), A the w x h f64 x-slope
 * of the pixel's plane (NULL = all 0; the y-slope is not needed: D is already the plane at the pixel and the warp stays in the row), I a
 * packed 8-bit BGR image.  t in [0, 1] is the fraction of the baseline from view 0 to view 1.  Every product, sum and quotient is one IEEE
 * f64 operation in the association written here, nothing contracted, no reciprocal.  The host computes once
 *     sigma_0 = -t        sigma_1 = 1.0 - t        w0 = 1.0 - t        w1 = t
 * Step 1, footprints.  For view v (sigma = sigma_v) and source pixel (x, y):
 *     usable = V != 0 && isfinite(D) && D >= 0.0
 *     a    = isfinite(A) ? A : 0.0
 *     g    = 1.0 + sigma * a                   target pixels one source pixel covers
 *     u    = (double)x + sigma * D
 *     half = 0.5 * g        lo = u - half        hi = u + half
 *     used = usable && g > 0.0 && g <= max_stretch
 *   A non-positive g is a surface seen from behind, a g above the cap one stretched beyond what its colours can fill.  A used pixel
 *   covers every integer x' with lo <= (double)x' < hi and 0 <= x' < w (half-open; lo and hi are the rounded values above), and there
 *     xs = (double)x + ((double)x' - u) / g    the source position
 *     d' = D + a * (xs - (double)x)            the plane's disparity there
 * Step 2, visibility.  Per view and target pixel the candidate with the greatest d' wins, in the total order of the order-preserving
 *   64-bit key of the bit pattern (as M64 above: -0.0 < +0.0; a candidate is never NaN); among bit-equal d' the smallest source x wins.
 *   In exact arithmetic two pixels of one view cannot tie; the rule makes the result independent of the execution order.  The result is
 *   Z_v(x') = d' and xs_v(x') of the winner, or a hole.
 * Step 3, colour.  fl = floor(xs), f = xs - fl, ia = clamp(fl, 0, w-1), ib = clamp(fl + 1, 0, w-1), and per channel
 *     C_v = (1.0 - f) * (double)I[y][ia] + f * (double)I[y][ib]
 * Step 4, merge.  Both views present and fabs(Z_0 - Z_1) <= merge_diff: C = w0 * C_0 + w1 * C_1 per channel, Z = w0 * Z_0 + w1 * Z_1,
 *   mask 3.  Both present otherwise: view 0 alone when Z_0 >= Z_1 (mask 1), else view 1 alone (mask 2).  One present: that view, mask 1 or
 *   2.  None: a hole, mask 0.
 * Step 5, fill, when `fill`.  A hole takes the nearest non-hole pixel of its row on either side; with both sides present the right one
 *   when its Z is smaller (Z_R < Z_L: the background, the reference's choice in FillInvalid, cs_patchmatch.cc:399-411) and the left one
 *   otherwise.  Colour and disparity are copied, the mask is 4.  A row without any non-hole pixel stays a hole.
 * Outputs, each optional (NULL) and untouched when not requested: a BGR 8-bit image with rows of out_stride bytes (bytes beyond 3*w of a
 * row are untouched), each channel the Round2Int (round half to even) of the f64 colour saturated to 0 .. 255, holes 0; an f64 disparity
 * map, NaN in holes; a u8 mask, 0 .. 4.
 * Parameters (NULL = the defaults).  The defaults are documented choices, not tuned values: no quality figure was optimised over them. */
#define CSPM_SYNTH_MAX_WIDTH 6784 /* a target row lives in one workgroup's LDS (24 bytes per pixel of 160 KiB); wider: CSPM_ERR_ARG */
typedef struct cspm_synth_params {
  int views;          /* bit mask of the source views used: 1 = view 0, 2 = view 1, 3 = both (the default) */
  int fill;           /* step 5 on (the default, 1) or off (0) */
  double max_stretch; /* a source pixel is used only when 0 < g <= max_stretch; >= 1, may be +infinity; default 4.0 */
  double merge_diff;  /* the views are blended where their disparities differ by at most this; >= 0, may be +infinity; default 1.0 */
} cspm_synth_params;
typedef struct cspm_synth_view {
  const double *disp;    /* D: w*h, packed rows */
  const uint8_t *valid;  /* V: w*h bytes or NULL */
  const double *slope_a; /* A: w*h or NULL */
  const uint8_t *bgr;    /* I: 8UC3 rows of `stride` bytes */
  size_t stride;         /* >= 3*w */
} cspm_synth_view;
int cspm_synth_default_params(cspm_synth_params *p);
/* N alone on caller memory, no context needed, synchronous.  view0 / view1 may be NULL when `views` does not name the view.  Arguments are
 * checked before a device is opened: CSPM_ERR_ARG for a t that is NaN or outside [0, 1], views outside 1 .. 3, a max_stretch that is NaN or
 * < 1, a merge_diff that is NaN or negative, a missing map or image of a view that `views` names, w or h < 1, w*h >= 2^31,
 * w > CSPM_SYNTH_MAX_WIDTH, an input stride of a named view below 3*w, or (with bgr_out) an out_stride below 3*w. */
int cspm_synthesize_host(int device, const cspm_synth_params *params, double t, const cspm_synth_view *view0, const cspm_synth_view *view1,
                         int w, int h, uint8_t *bgr_out, size_t out_stride, double *disp_out, uint8_t *mask_out);
/* N on the context's stored plane field; I = the level-0 images.  source as for cspm_reproject:
 *   CSPM_GEOM_RAW  D = the field's a*x+b*y+c of either view written into scratch, A = the field's a, V all 1.
 *   CSPM_GEOM_PP   D = the maps of the sub-pixel post-processing (cspm_postprocess_f64, with the context's speckle and median settings),
 *                  which this call runs itself; A = the field's a where the pixel passed the left-right check (the masks that entry
 *                  returns) and 0 elsewhere; V all 1.
 * Makes the same pending-run check on entry as cspm_reproject.  Synchronous; host outputs.  Timed as one CSPM_K_MISC bracket per call with
 * w*h evaluations (CSPM_GEOM_PP: behind the post-processing's own CSPM_K_POST brackets).  Scratch (two maps, CSPM_GEOM_RAW only) is
 * allocated on first use and freed with the plane field.  CSPM_ERR_ARG as above and for a bad source; CSPM_ERR_STATE without images or a
 * plane field, and without a cost object when source is CSPM_GEOM_PP. */
int cspm_synthesize(cspm_ctx *ctx, int source, const cspm_synth_params *params, double t, uint8_t *bgr_out, size_t out_stride,
                    double *disp_out, uint8_t *mask_out);
/* the same with device pointers for every output; enqueued on the ctx stream behind the pending-run check.  Like cspm_reproject_device it is
 * NOT part of the deferred-output replay. */
int cspm_synthesize_device(cspm_ctx *ctx, int source, const cspm_synth_params *params, double t, void *d_bgr_out, size_t out_stride,
                           void *d_disp_out, void *d_mask_out);

/* ---- depth-map fusion (an addition): one consistent point cloud from many views ----------------------------------
 * Everything above relates the two views of ONE pair.  A surface that is wrong in both of them passes the left-right check; what removes
 * it is agreement with a third viewpoint: the geometric consistency fusion of Gipuma ("fusibile") and COLMAP.
 * F(params, K views): view k = a w x h f64 depth map (along the optical axis, > 0; anything else is a hole), optionally three w x h planes
 * of unit normals in the camera frame (all views or none), optionally an 8-bit BGR image, a pinhole camera and a camera -> world pose.
 * 1 <= K <= 64 (CSPM_FUSE_MAX_VIEWS), all views w x h, w*h < 2^31.  Every product, sum, quotient, floor and square root is one IEEE f64
 * operation in the association written here, nothing contracted, no reciprocal.
 * Camera k is (f_k, cx_k, cy_k, R_k, t_k), R row-major (M[i][j] at entry 3*i+j), P_world = R P_cam + t.
 * cspm_fuse_params { max_reproj, max_rel_depth, min_cos, min_views, suppress }, defaults 2.0, 0.01, 0.0, 2, 1: 2 pixels and 1 % are
 * COLMAP's and Gipuma's values, min_cos = 0 switches the normal test off (a raw field's normals are noisy); chosen, not tuned.  The host
 * computes once mr2 = max_reproj * max_reproj.
 *     back(k, x, y, Z):  u = (double)x - cx_k;  wv = (double)y - cy_k;  X = (u*Z)/f_k;  Y = (wv*Z)/f_k          (G's association)
 *     world(k, X,Y,Z):   W[i] = ((R_k[i][0]*X + R_k[i][1]*Y) + R_k[i][2]*Z) + t_k[i]
 *     cam(k, W):         d = W - t_k (three subtractions);  Q[j] = (R_k[0][j]*d[0] + R_k[1][j]*d[1]) + R_k[2][j]*d[2]
 *     proj(k, Q):        fails unless Q[2] > 0.0;  pu = (f_k*Q[0])/Q[2] + cx_k;  pv = (f_k*Q[1])/Q[2] + cy_k
 *     rot(k, n):         N[i] = (R_k[i][0]*n[0] + R_k[i][1]*n[1]) + R_k[i][2]*n[2]
 * Pixel (x, y) of reference view r, Z = depth_r[y][x], m = y*w + x:
 *  1. !(isfinite(Z) && Z > 0.0): S = 0, nothing is emitted.
 *  2. suppress && used_r[m]: S = 0x80, nothing is emitted.
 *  3. P = world(r, back(r, x, y, Z)); SP = P; Nr = rot(r, n_r[m]); SN = Nr when its three components are finite, else (0,0,0);
 *     SC = (b, g, r) of the pixel as ints; c = 0.
 *  4. For k = 0 .. K-1, k != r, ascending:
 *       Q = cam(k, P); if proj(k, Q) fails, continue.
 *       fx = floor(pu + 0.5), fy = floor(pv + 0.5); continue unless fx >= 0.0 && fx <= (double)(w-1) && fy >= 0.0 && fy <= (double)(h-1)
 *       (tested on the doubles, a NaN fails; only then are they converted to int).
 *       Zk = depth_k[fy][fx]; continue unless it is finite and > 0.0.
 *       Pk = world(k, back(k, fx, fy, Zk)); Q2 = cam(r, Pk); if proj(r, Q2) fails, continue; it gives (pu2, pv2).
 *       ex = pu2 - (double)x, ey = pv2 - (double)y; continue unless ex*ex + ey*ey <= mr2.
 *       continue unless fabs(Q2[2] - Z) <= max_rel_depth * Z.
 *       With normals: Nk = rot(k, n_k[fy*w+fx]); when min_cos > 0.0, continue unless (Nr[0]*Nk[0] + Nr[1]*Nk[1]) + Nr[2]*Nk[2] >= min_cos
 *       (a NaN fails; the test is against the reference pixel's own normal, not the running sum).
 *       The view is consistent: c += 1; SP[i] = SP[i] + Pk[i]; SN[i] = SN[i] + Nk[i] iff Nk is all finite; SC += bgr_k; m_k = fy*w + fx.
 *  5. kept = c >= min_views;  S = c | (kept ? 0x40 : 0)   (c <= 63: the flags never collide).
 *  6. kept && suppress: used_k[m_k] = 1 for every consistent k.  Only kept pixels make marks.
 *  7. The record of a kept pixel: den = (double)(c+1); x, y, z = (float)(SP[i]/den); len = sqrt((SN0*SN0 + SN1*SN1) + SN2*SN2);
 *     nx, ny, nz = (float)(SN[i]/len) (a zero sum gives NaN; without normal maps the three are NaN); each colour byte
 *     (2*SC_i + (c+1)) / (2*(c+1)) in integer arithmetic, a = 255; without an image in ANY view all four bytes are 0, otherwise a view
 *     without an image contributes (0,0,0) to the sums; pixel = m.
 * Order: used is all 0 when a run begins; the views are processed as passes r = 0, 1, .., K-1.  Pass r reads only used_r and writes only
 * used_k, k != r, and every write stores 1: the result does not depend on scheduling.  With suppress == 0 the passes are independent.
 * Outputs: the cloud = all kept pixels in (view ascending, raster) order, one cspm_point each in WORLD coordinates; *count = their number
 * whatever the capacity, when count > cap the first cap records are written and the rest of the buffer is untouched; view_counts[K] = the
 * kept pixels per view; state = the S bytes, K*w*h, view-major.  Each output may be NULL.
 * CSPM_ERR_ARG: K outside 1 .. 64; f <= 0 or a non-finite camera value; max |R R^T - I| > 1e-6; a NaN or negative max_reproj or
 * max_rel_depth; a min_cos outside [0, 1]; a min_views outside 0 .. 63; normals in some views but not all; a bgr_stride below 3*w. */
#define CSPM_FUSE_MAX_VIEWS 64
typedef struct cspm_fuse_params {
  double max_reproj;    /* pixels: the forward-backward reprojection error a consistent view may have */
  double max_rel_depth; /* the relative depth difference it may have */
  double min_cos;       /* with normals: the least cosine between the two world normals; 0 = no normal test */
  int min_views;        /* a pixel is kept when at least this many OTHER views are consistent with it */
  int suppress;         /* 1: surface emitted from an earlier view is not emitted again */
} cspm_fuse_params;
typedef struct cspm_fuse_view {
  const double *depth;  /* w*h */
  const double *normal; /* three planes of w*h (the layout of cspm_reproject's normal_out) or NULL */
  const uint8_t *bgr;   /* 8UC3 rows of bgr_stride bytes or NULL */
  size_t bgr_stride;    /* >= 3*w when bgr is given */
  double f, cx, cy;
  double R[9], t[3];    /* camera -> world */
} cspm_fuse_view;
int cspm_fuse_default_params(cspm_fuse_params *p);
/* F alone on caller memory with a temporary context: begin, one cspm_fuse_push_maps per view, run.  Synchronous.  Every argument is
 * checked before a device is opened (the list above, and NULL views or depth, w or h < 1, w*h >= 2^31).  It is a one-shot entry like the
 * cspm_*_host entries; its name deliberately does not end in _host, because it takes the views of a whole scene, not one kernel family's
 * maps of one view. */
int cspm_fuse_depth_maps(int device, const cspm_fuse_params *params, const cspm_fuse_view *views, int n_views, int w, int h,
                         cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out, unsigned int *view_counts_out, uint8_t *state_out);
/* The fusion views of a context live in a pool of their own from cspm_fuse_begin to cspm_fuse_end (or cspm_destroy), whatever happens to the
 * image geometry, cost object and plane field in between: one context serves a video.  Per view and pixel the pool holds an 8-byte depth,
 * a 24-byte normal, a 4-byte colour and the bytes used and S.  CSPM_ERR_ARG for w or h < 1, w*h >= 2^31 or max_views outside 1 .. 64;
 * CSPM_ERR_STATE for a second begin without an end. */
int cspm_fuse_begin(cspm_ctx *ctx, int w, int h, int max_views);
/* appends one view of the context's STORED FIELD.  view, source, calib, geom_params (NULL = the defaults) and fit mean what they mean in
 * cspm_reproject_device and the inputs are prepared by the same code behind the same pending-run check; depth and normals land in the slot
 * without leaving the device.  The slot's depth is G's Z where G's keep holds and NaN elsewhere (so z_near, z_far and min_cos apply), the
 * normals are G's, the colour is the view's level-0 image.  left_frame is ignored: a view is stored in its own camera frame.  R, t is the
 * pose of the pair's view-0 rectified camera; for view == 1 the entry stores cx + doffs and t + R (baseline, 0, 0), so both views of a
 * pair can be pushed.  Asynchronous on the ctx stream.  CSPM_ERR_STATE without a begin, when the slots are full, or when the context's
 * current w x h differs from the begin's; CSPM_ERR_ARG for a bad pose, or when earlier views have no normals; otherwise the error classes
 * of cspm_reproject. */
int cspm_fuse_push(cspm_ctx *ctx, int view, int source, const cspm_calib *calib, const cspm_geom_params *geom_params, const cspm_fit_params *fit,
                   const double *R, const double *t);
/* appends one view from caller memory (another sensor's depth map, maps saved earlier); the maps as in cspm_fuse_view.  Synchronous. */
int cspm_fuse_push_maps(cspm_ctx *ctx, const double *depth, const double *normal, const uint8_t *bgr, size_t bgr_stride, double f, double cx,
                        double cy, const double *R, const double *t);
/* the number of views pushed since the begin; -1 without a begin */
int cspm_fuse_view_count(const cspm_ctx *ctx);
/* F over the views pushed so far.  Synchronous; host outputs.  It clears used first, so it may be called again with other parameters and
 * after further pushes.  Timed as one CSPM_K_MISC bracket with K*w*h evaluations.  CSPM_ERR_STATE without a begin or a view. */
int cspm_fuse_run(cspm_ctx *ctx, const cspm_fuse_params *params, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out,
                  unsigned int *view_counts_out, uint8_t *state_out);
/* the same with device pointers (the cloud 16-byte aligned, the count and the view counts 4-byte aligned unsigned ints); enqueues on the ctx
 * stream and returns.  Like cspm_reproject_device it is NOT part of the deferred-output replay, for the reason given there. */
int cspm_fuse_run_device(cspm_ctx *ctx, const cspm_fuse_params *params, void *d_cloud_out, size_t cloud_cap, void *d_count_out,
                         void *d_view_counts_out, void *d_state_out);
/* waits for the stream and frees the views.  CSPM_ERR_STATE without a begin. */
int cspm_fuse_end(cspm_ctx *ctx);

/* ---- depth-view registration (an addition): the poses the fusion needs, from the fusion views themselves ---------------
 * F needs every camera -> world pose to within its gates.  Each fusion view holds a metric depth map and an exact per-pixel normal, which is
 * all that projective point-to-plane registration (the tracking step of KinectFusion) needs: a Gauss-Newton loop that stays on the device.
 * The specification R.  Every product, sum, quotient, floor and fabs is one IEEE f64 operation in the association written here, nothing
 * contracted, no reciprocal, no trigonometry.  back, world, cam, proj and rot are F's.
 * Inputs: the views of the fusion pool (all with normals), a source slot s, a 64-bit target mask T (bit k = view k is a target; bit s clear,
 * at least one bit set, every set bit below the view count), a start pose (R, t) of the source, cspm_reg_params { iters, stride, max_dist,
 * huber, min_cos, min_pairs, pivot_rel }, defaults 8, 1, 0.5, 0.05, 0.0, 100, 1e-8: chosen, not tuned.  The host computes once
 * md2 = max_dist * max_dist.  Camera s below is (f_s, cx_s, cy_s) of the slot with the CURRENT (R, t).
 * Samples: source pixels (x, y) = (i*stride, j*stride), i < ws = ceil(w / stride), j < hs = ceil(h / stride); flat index q = j*ws + i.
 * One iteration, sample q, acc[0 .. 28] = 0.0:
 *   Z = depth_s[y][x]; nothing more unless Z is finite and > 0.0.  P = world(s, back(s, x, y, Z)); L[i] = P[i] - t[i].
 *   For each k in T, ascending:
 *     Q = cam(k, P); proj, the rounding fx, fy, the bounds test on the doubles and Zk = depth_k[fy][fx] finite and > 0.0: F's step 4.
 *     Pk = world(k, back(k, fx, fy, Zk)).  N = rot(k, n_k[fy*w + fx]); continue unless its three components are finite.
 *     d = Pk - P (three subtractions); continue unless (d0*d0 + d1*d1) + d2*d2 <= md2 (a NaN fails).
 *     When min_cos > 0.0: Ns = rot(s, n_s[y*w + x]); continue unless (Ns0*N0 + Ns1*N1) + Ns2*N2 >= min_cos (a NaN fails).
 *     r = (N0*d0 + N1*d1) + N2*d2.   J = (L1*N2 - L2*N1, L2*N0 - L0*N2, L0*N1 - L1*N0, N0, N1, N2).
 *     wt = 1.0 when huber == 0.0 or fabs(r) <= huber, else huber / fabs(r).   g_a = wt * J_a.
 *     acc[0 .. 20] += g_a * J_b for a <= b in row-major order; acc[21 + a] += g_a * r; acc[27] += (wt * r) * r; acc[28] += 1.0:
 *     each update one product and one addition into acc.
 * Reduction (the order is part of R): block B holds the samples [256 B, 256 B + 256), a missing sample is all 0.0.  Within a block, for
 * s = 128, 64, .., 1: v[i] = v[i] + v[i + s] for i < s.  Across blocks, lane j of 256 computes u_j = 0.0, then u_j = u_j + part[B] for
 * B = j, j + 256, .. ascending; the same tree over u gives A (21 entries), b (6), cost and pairs.
 * Solve: status 1 when pairs < (double)min_pairs.  Else LDL^T without pivoting, for j = 0 .. 5: D_j = A_jj - sum_{k<j} (L_jk*L_jk)*D_k, one
 * term subtracted at a time, k ascending; status 2 unless D_j > pivot_rel * A_jj (a NaN fails); L_ij = (A_ij - sum_{k<j} (L_ik*L_jk)*D_k) / D_j.
 * y_i = b_i - sum_{k<i} L_ik*y_k; z_i = y_i / D_i; xi_i = z_i - sum_{k>i} L_ki*xi_k for i = 5 .. 0; k ascending throughout.  Status 3 when
 * a component of xi is not finite.  xi = (om, v).
 * Update (status 0 only; otherwise the pose stays and the loop goes on): a = 0.5 * om; s = (a0*a0 + a1*a1) + a2*a2; p = 1.0 - s;
 * q = 1.0 + s; the Cayley map E = ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s), exactly orthogonal in exact arithmetic:
 *     E_ii = (p + 2.0*(a_i*a_i)) / q
 *     E_01 = (2.0*(a0*a1) - 2.0*a2) / q   E_02 = (2.0*(a0*a2) + 2.0*a1) / q   E_12 = (2.0*(a1*a2) - 2.0*a0) / q
 *     E_10 = (2.0*(a0*a1) + 2.0*a2) / q   E_20 = (2.0*(a0*a2) - 2.0*a1) / q   E_21 = (2.0*(a1*a2) + 2.0*a0) / q
 * R_ij <- (E_i0*R_0j + E_i1*R_1j) + E_i2*R_2j;  t_i <- t_i + v_i.
 * Outputs: the final R, t and one cspm_reg_iter per iteration: pairs, cost, rot2 = (om0*om0 + om1*om1) + om2*om2, trans2 likewise of v
 * (both 0.0 on a refused step), status.
 * CSPM_ERR_ARG: a bad slot or mask; iters or stride < 1; iters > CSPM_REG_MAX_ITERS; a NaN or negative max_dist or huber; a min_cos outside
 * [0, 1]; a pivot_rel outside [0, 1); a negative min_pairs; a start pose a push would refuse.  CSPM_ERR_STATE: no begin, or views without
 * normals.  Every output stays untouched on an error. */
#define CSPM_REG_MAX_ITERS 64
typedef struct cspm_reg_params {
  int iters;        /* Gauss-Newton iterations, all of them run: 1 .. CSPM_REG_MAX_ITERS */
  int stride;       /* every stride-th source pixel in x and y */
  double max_dist;  /* world units: the largest distance between a source point and its associated target point */
  double huber;     /* world units: residuals beyond it are down-weighted; 0 = plain least squares */
  double min_cos;   /* the least cosine between the source's and the target's world normal; 0 = no normal test */
  int min_pairs;    /* fewer pairs refuse the step (status 1) */
  double pivot_rel; /* a pivot D_j <= pivot_rel * A_jj refuses the step (status 2): the geometry does not fix all six freedoms */
} cspm_reg_params;
typedef struct cspm_reg_iter {
  double pairs, cost, rot2, trans2;
  int status; /* 0 = the step was taken; 1 = too few pairs; 2 = a pivot failed; 3 = a non-finite step */
} cspm_reg_iter;
int cspm_reg_default_params(cspm_reg_params *p);
/* R for slot src against the slots of `targets`.  Synchronous: iters x (k_reg_pairs, k_reg_solve) go on the ctx stream back to back, the host
 * waits once.  R0 / t0 NULL = the slot's own rotation / translation.  With apply != 0 the slot's row of the device camera table and its host
 * copy take the result.  R_out (9), t_out (3), iters_out (params->iters records) may each be NULL.  Scratch (the partial sums, the pose row,
 * the records) is allocated in the fusion pool by the first call.  Timed as one CSPM_K_MISC bracket with iters * ws * hs * |T| evaluations. */
int cspm_fuse_register(cspm_ctx *ctx, int src, unsigned long long targets, const cspm_reg_params *params, const double *R0, const double *t0,
                       int apply, double *R_out, double *t_out, cspm_reg_iter *iters_out);
/* the pose of a slot (the host's copy of the camera table); set_pose makes the pose checks of a push.  CSPM_ERR_ARG for a bad slot or pose,
 * CSPM_ERR_STATE without a begin. */
int cspm_fuse_get_pose(cspm_ctx *ctx, int slot, double *R_out, double *t_out);
int cspm_fuse_set_pose(cspm_ctx *ctx, int slot, const double *R, const double *t);
/* R alone on caller memory with a temporary context: begin, one cspm_fuse_push_maps per view, one registration of view src from its own
 * pose.  Every argument is checked before a device is opened: the list above (views without normals are CSPM_ERR_ARG here) and what
 * cspm_fuse_depth_maps checks in views, n_views, w, h. */
int cspm_register_depth_maps(int device, const cspm_reg_params *params, const cspm_fuse_view *views, int n_views, int w, int h, int src,
                             unsigned long long targets, double *R_out, double *t_out, cspm_reg_iter *iters_out);

/* ---- plane-field carry (an addition): a plane field moved into another camera: temporal starts for stereo video ------
 * A plane in disparity space is a plane in 3-D (G above), so a converged field can be moved across a rigid motion into another camera's
 * disparity space and pixel grid, with visibility resolved: frame i + 1 of a moving rig starts from frame i's planes.  For the pure
 * baseline shift it is the reference's view propagation (cs_patchmatch.cc:229-277) as a geometric operation.
 * The specification C.  Every product, sum, quotient, floor and square root is one IEEE f64 operation in the association written here,
 * nothing contracted, no reciprocal, no trigonometry.
 * A carry camera is {f, cxv, cy, B, doffs} of one view of a rectified pair: a cspm_calib and a view v, cxv = cx + (double)v * doffs (G's
 * cxv), B = baseline.  The host computes once per camera fB = f * B.  Subscript s is the source camera, t the target camera.
 * The motion (R, t), R row-major, maps source-camera to target-camera coordinates: X_t = R X_s + t.
 * Inputs: the source planes a, b, c on w_s x h_s (the param part of cspm_get_planes' records), an optional mask of w_s*h_s bytes, both
 * cameras, (R, t), the target size w_t x h_t, max_dis of the target, cspm_carry_params { fill }, default 1.
 * Splat, source pixel (x, y), m = y*w_s + x:
 *  1. No contender when the mask byte is 0 or one of a, b, c is not finite.
 *  2. D = (a*x + b*y) + c;  tt = D + doffs_s;  continue only when tt > 0.0 (a NaN fails).
 *     Z = fB_s / tt;  u = x - cxv_s;  wv = y - cy_s;  X = (u*Z) / f_s;  Y = (wv*Z) / f_s                           (G's association)
 *  3. Q[i] = ((R[i][0]*X + R[i][1]*Y) + R[i][2]*Z) + t[i];  continue only when Q[2] > 0.0.
 *     pu = (f_t*Q[0]) / Q[2] + cxv_t;  pv = (f_t*Q[1]) / Q[2] + cy_t;  fx = floor(pu + 0.5);  fy = floor(pv + 0.5);
 *     continue unless fx >= 0.0 && fx <= (double)(w_t-1) && fy >= 0.0 && fy <= (double)(h_t-1) (tested on the doubles, a NaN fails; only
 *     then are they converted to int: F's step 4).
 *  4. The 3-D plane is n . P = fB_s with n0 = a*f_s, n1 = b*f_s, n2 = ((a*cxv_s + b*cy_s) + c) + doffs_s.  Rotated:
 *     n'[i] = (R[i][0]*n0 + R[i][1]*n1) + R[i][2]*n2;  hq = fB_s + ((n'0*t[0] + n'1*t[1]) + n'2*t[2]);
 *     continue only when hq > 0.0 (a NaN fails): the target camera is on the plane's visible side.
 *  5. a' = (B_t*n'0) / hq;  b' = (B_t*n'1) / hq;  c' = (((fB_t*n'2) / hq - a'*cxv_t) - b'*cy_t) - doffs_t.
 *  6. continue unless a', b', c' are finite;  z = (a'*fx + b'*fy) + c';  continue only when z >= 0.0 && z <= max_dis (a NaN fails).
 *  The pixel is then a contender for target pixel g = fy*w_t + fx with depth Q[2].  Steps 4 and 5 do not depend on (x, y).
 * Winner of g: the contender with the smallest Q[2] (f64), then the smallest m: independent of scheduling.
 * Fill (fill = 1): a target pixel (x, y) without a winner looks at (x-1,y), (x+1,y), (x,y-1), (x,y+1) in that order, those inside the image
 *  that have a winner; for each, z = (a'*x + b'*y) + c' with that winner's (a', b', c') at its OWN (x, y); among those with
 *  z >= 0.0 && z <= max_dis it takes the smallest z (the background side), the first in the order on a tie.  Fill reads winners only,
 *  never filled pixels.
 * Output per target pixel (x, y) with its (a', b') and z (a winner's z is that of step 6):
 *     len = sqrt((a'*a' + b'*b') + 1.0);  inv = 1.0 / max(len, 1e-8);  normal = (-a'*inv, -b'*inv, 1.0*inv)
 *     plane = Plane(normal, (x, y, z)), exactly as cspm_fit_planes_host finishes; the record is six doubles, norm then param.
 *  State S: 1 = a winner, 2 = filled, 0 = none; a pixel of state 0 gets six NaNs ("no candidate" for cspm_merge_planes_host).
 *  source: the m of the source pixel whose plane the pixel took (its winner's, or for a filled pixel the chosen neighbour's winner's);
 *  -1 for state 0.
 * CSPM_ERR_ARG: a calibration the reprojection would refuse (non-finite, f <= 0, baseline <= 0) or a view outside 0 .. 1;
 * max |R R^T - I| > 1e-6 or a non-finite R or t; max_dis < 0; w or h < 1 or w*h >= 2^31 (source or target); fill outside 0 .. 1. */
typedef struct cspm_carry_params {
  int fill; /* 1 (default): a target pixel without a winner takes a neighbouring winner's plane; 0: it stays without a candidate */
} cspm_carry_params;
int cspm_carry_default_params(cspm_carry_params *p);
/* two camera -> world poses (P_world = R P_cam + t, row-major R) into the motion between the cameras, R = Rt^T Rs, t = Rt^T (ts - tt):
 *     R[i][j] = (Rt[0][i]*Rs[0][j] + Rt[1][i]*Rs[1][j]) + Rt[2][i]*Rs[2][j]
 *     d = ts - tt (three subtractions);  t[i] = (Rt[0][i]*d[0] + Rt[1][i]*d[1]) + Rt[2][i]*d[2]
 * Pure host code, no checks beyond NULL (CSPM_ERR_ARG); an output may alias an input. */
int cspm_carry_relative_pose(const double *Rs, const double *ts, const double *Rt, const double *tt, double *R_out, double *t_out);
/* C alone on caller memory with a temporary context, synchronous.  src_norm_param: w_s*h_s records of six doubles in the layout of
 * cspm_get_planes, of which only the param part (entries 3 .. 5) is read; mask w_s*h_s bytes or NULL.  Outputs, each optional:
 * norm_param_out w_t*h_t*6 doubles in the layout of cspm_get_planes, state_out w_t*h_t bytes, source_out w_t*h_t int32.  Every argument
 * is checked before a device is opened (the list above, and a NULL field); no output is touched on an error.  A one-shot entry like
 * cspm_fuse_depth_maps; its name does not end in _host because it relates two cameras, not one kernel family's maps of one view. */
int cspm_carry_plane_field(int device, const double *src_norm_param, const uint8_t *mask, const cspm_calib *src_calib, int src_view, int w_s,
                           int h_s, const cspm_calib *dst_calib, int dst_view, int w_t, int h_t, int max_dis, const double *R, const double *t,
                           const cspm_carry_params *params, double *norm_param_out, uint8_t *state_out, int32_t *source_out);
/* C from src's stored field into dst, both views; the contexts may differ in size.  (R, t) is the motion between the two VIEW-0 cameras;
 * view v of dst receives view v of src.  For v = 1 the entry shifts both cameras by their baselines itself (as cspm_fuse_push does):
 *     t1[i] = t[i] + R[i][0]*B_s for i = 0 .. 2, then t1[0] = t1[0] - B_t;   cxv = cx + doffs on both sides.
 * max_dis is dst's.
 *   merge = 1  the candidates go into the context's candidate buffer with S != 0 as the mask and are merged under
 *              cspm_merge_planes_host's rule, one view after the other; a field that is not consistent is re-scored first.
 *   merge = 0  pixels that have a candidate are replaced and the field is left not consistent, as cspm_fit_planes does.
 * Stream ordering and the pending-sweep check are those of cspm_merge_planes.  The keys and winners (12 bytes per pixel of dst) are
 * allocated by the first call, kept with dst's plane field and counted by CSPM_OPT_DEVICE_BYTES.  Timed as one CSPM_K_MISC bracket per
 * view with w_s*h_s evaluations; the merge under CSPM_K_INIT.  CSPM_ERR_ARG as above, for dst == src and for two devices;
 * CSPM_ERR_STATE when src has no plane field, dst no images, no plane field or no max_dis, and with merge when dst has no cost object. */
int cspm_carry_planes(cspm_ctx *dst, cspm_ctx *src, const cspm_calib *src_calib, const cspm_calib *dst_calib, const double *R, const double *t,
                      const cspm_carry_params *params, int merge);

/* ---- TSDF fusion (an addition): the fusion views averaged into one implicit surface --------------------------------
 * F ends in a point cloud and R registers a view against raw views.  A truncated signed distance volume (Curless & Levoy; KinectFusion)
 * averages every view into one surface that can be raycast from any pose into the (depth, normal, colour) triple a fusion slot holds --
 * an output and a target for cspm_fuse_register (frame to model) -- and whose zero level set is written out as oriented points.
 * The surface points with normals come in a defined order; the triangles over them (marching cubes) are the section "TSDF meshes" below.
 * The specification T.  Every product, sum, quotient, floor and square root is one IEEE f64 operation in the association written here,
 * nothing contracted, no reciprocal, no trigonometry.  back, world, cam, proj and rot are F's; lerp(a, b, t) = a + t*(b - a).
 * Volume: cspm_tsdf_params { origin[3], voxel, nx, ny, nz, trunc, max_weight, min_cos, step_rel }: voxel > 0, nx, ny, nz >= 1,
 * nx*ny*nz < 2^31, trunc > 0 (0, the default, = 4.0*voxel), 1 <= max_weight <= 2^24 (default 64; W stays an exact integer in f32),
 * min_cos in [0, 1] (default 0 = no test), step_rel in (0, 1] (default 0.5); chosen, not tuned.  The host computes once
 * step = step_rel * trunc.  Voxel (i, j, k) has flat index v = (k*ny + j)*nx + i and centre C[a] = origin[a] + ((double)idx_a + 0.5)*voxel.
 * State per voxel, 12 bytes: D (f32), W (f32), colour b, g, r and a byte has.  A cleared volume has D = 1, W = 0, colour bytes 0.
 * Integrate view k (a fusion slot), every voxel on its own:
 *  1. Q = cam(k, C); if proj(k, Q) fails, leave (behind).  fx = floor(pu + 0.5), fy = floor(pv + 0.5); leave (outside) unless
 *     fx >= 0.0 && fx <= (double)(w-1) && fy >= 0.0 && fy <= (double)(h-1) (on the doubles, F's step 4); m = fy*w + fx.
 *     Z = depth_k[m]; leave (hole) unless it is finite and > 0.0.
 *  2. sdf = Z - Q[2]; leave (occluded) unless sdf >= -trunc.
 *  3. With normal maps and min_cos > 0.0: (n0, n1, n2) = n_k[m]; (X, Y, Z) = back(k, fx, fy, Z);
 *     num = (n0*X + n1*Y) + n2*Z;  ln = sqrt((n0*n0 + n1*n1) + n2*n2);  ls = sqrt((X*X + Y*Y) + Z*Z);  c = (-num) / (ln*ls):
 *     the cosine between the pixel's normal and the direction from the surface point to the camera.  Leave (grazing) unless
 *     c >= min_cos (a NaN fails).
 *  4. d = sdf / trunc; if (d > 1.0) d = 1.0.  Wo = (double)W;  Wn = Wo + 1.0;  D = (float)(((double)D*Wo + d) / Wn);
 *     W = (float)(Wn > max_weight ? max_weight : Wn)   (D is read before it is written, Wo is the weight before the update).
 *  5. When view k has an image and sdf <= trunc: Wc = has ? Wo : 0.0; each of b, g, r = floor(((double)old*Wc + (double)new) / (Wc + 1.0) + 0.5)
 *     with new the byte of pixel m; has = 1.
 * Views are integrated in the order of the calls, one launch each; a voxel is owned by one lane: nothing depends on scheduling.
 * Raycast from a camera (f, cx, cy, R, t) into w x h maps, z_near finite and >= 0.  Pixel (x, y):
 *     dir = rot((((double)x - cx)/f, ((double)y - cy)/f, 1.0)), so the ray parameter lam IS the depth along the optical axis;
 *     P(lam)[a] = t[a] + lam*dir[a].
 *  Clip against the box of voxel CENTRES: when one of nx, ny, nz is below 2 the box is empty and the ray misses (status 0).  Otherwise
 *     l0 = z_near, l1 = +infinity; for a = x, y, z: lo = origin[a] + 0.5*voxel, hi = origin[a] + ((double)n_a - 0.5)*voxel; when
 *     dir[a] == 0.0 the ray misses unless lo <= t[a] <= hi; else ta = (lo - t[a])/dir[a], tb = (hi - t[a])/dir[a], swapped when ta > tb,
 *     if (ta > l0) l0 = ta, if (tb < l1) l1 = tb.  The ray misses (status 0) unless l0 <= l1.
 *  March lam_m = l0 + (double)m*step, m = 0, 1, .. while lam_m <= l1 (at most 2^20 samples).  A sample at P(lam_m):
 *     g[a] = (P[a] - origin[a])/voxel - 0.5;  c[a] = floor(g[a]);  fr[a] = g[a] - c[a];  it is KNOWN iff 0 <= c[a] <= n_a - 2 on every
 *     axis (on the doubles) and all eight corners (c + (dx, dy, dz)) have W > 0.  With d[dz][dy][dx] the corners' (double)D its value is
 *     val = lerp(lerp(lerp(d000, d001, fr0), lerp(d010, d011, fr0), fr1), lerp(lerp(d100, d101, fr0), lerp(d110, d111, fr0), fr1), fr2).
 *  An unknown sample forgets prev.  A known sample > 0 becomes prev.  A known sample cur <= 0 ends the ray: directly behind a known
 *  prev > 0 it is a hit, lam* = lam_prev + (step*prev)/(prev - cur); otherwise a miss with status 3 (a back face).  A ray that leaves
 *  the march without either is a miss with status 2.
 *  Hit: depth = lam*, status 1.  In the cell of P(lam*) (its c, fr, d as above) the analytic gradient of the interpolant is
 *     g0 = lerp(lerp(d001-d000, d011-d010, fr1), lerp(d101-d100, d111-d110, fr1), fr2)
 *     g1 = lerp(lerp(d010-d000, d011-d001, fr0), lerp(d110-d100, d111-d101, fr0), fr2)
 *     g2 = lerp(lerp(d100-d000, d101-d001, fr0), lerp(d110-d010, d111-d011, fr0), fr1)
 *     len = sqrt((g0*g0 + g1*g1) + g2*g2);  nw = g/len;  normal[j] = (R[0][j]*nw[0] + R[1][j]*nw[1]) + R[2][j]*nw[2]   (R^T nw).
 *  D grows towards the free space in front of a surface, so the normal points towards the camera that saw it, like G's normals (section
 *  19: they face the camera).  Colour: 0 when a corner has has = 0, else per channel floor(val(the corners' bytes) + 0.5).  When that cell
 *  is not known (the hit point may lie in another cell than both samples) the normal is NaN and the colour 0; depth and status stay.
 *  Miss: depth NaN, normal NaN, colour 0, status 0 (missed the box), 2 (ran out of the box) or 3 (met a back face).
 * Surface points: voxels v in flat order; for a voxel with W > 0 its +x, +y, +z neighbours in that order.  A neighbour inside the volume
 *  counts when it has W > 0 and exactly one of the two D is > 0.  Each counted neighbour gives one cspm_point in WORLD coordinates:
 *     t = Da/(Da - Db) on the (double)D of the voxel (a) and the neighbour (b);  x, y, z = (float)lerp(Ca[e], Cb[e], t);
 *     G_v[e] = (double)D(v + e) - (double)D(v - e), NaN when one of the two is outside the volume or has W = 0;
 *     G[e] = lerp(G_a[e], G_b[e], t);  len = sqrt((G0*G0 + G1*G1) + G2*G2);  nx, ny, nz = (float)(G[e]/len): one NaN component makes
 *     len, and with it all three, NaN; b, g, r = floor(lerp(colour_a, colour_b, t) + 0.5) and a = 255 when both have has = 1, else all
 *     four bytes 0; pixel = v.
 *  *count = their number whatever the capacity; when count > cap the first cap records are written, the rest of the buffer is untouched.
 * CSPM_ERR_ARG: parameters outside the ranges above ("tsdf: ..."), a NULL or bad camera (the fusion's messages), a bad z_near, w or
 * h < 1, w*h >= 2^31, a stride below 3*w.  CSPM_ERR_STATE: no cspm_tsdf_begin ("tsdf: cspm_tsdf_begin first"), a second begin, and for
 * cspm_tsdf_integrate no cspm_fuse_begin or a slot that holds no view. */
typedef struct cspm_tsdf_params {
  double origin[3];  /* the world corner of voxel (0, 0, 0) */
  double voxel;      /* edge length */
  int nx, ny, nz;
  double trunc;      /* truncation distance; 0 = 4 * voxel */
  double max_weight; /* a voxel's weight saturates here */
  double min_cos;    /* with normals: the least cosine between a pixel's normal and its view ray; 0 = no test */
  double step_rel;   /* the raycast's step as a fraction of trunc */
} cspm_tsdf_params;
typedef struct cspm_tsdf_camera {
  double f, cx, cy;
  double R[9], t[3]; /* camera -> world */
} cspm_tsdf_camera;
/* origin 0, voxel 0 and dims 0 (to be set), trunc 0, max_weight 64, min_cos 0, step_rel 0.5 */
int cspm_tsdf_default_params(cspm_tsdf_params *p);
/* The volume lives in a pool of its own from cspm_tsdf_begin to cspm_tsdf_end (or cspm_destroy), counted by CSPM_OPT_DEVICE_BYTES, whatever
 * happens to the fusion views in between; it starts cleared.  12 bytes per voxel and the extraction's counts.  CSPM_ERR_ARG for bad
 * parameters, CSPM_ERR_STATE ("tsdf: cspm_tsdf_begin twice without cspm_tsdf_end") for a second begin, CSPM_ERR_HIP without memory. */
int cspm_tsdf_begin(cspm_ctx *ctx, const cspm_tsdf_params *params);
/* D = 1, W = 0, colour 0.  Asynchronous on the ctx stream.  CSPM_ERR_STATE without a begin. */
int cspm_tsdf_clear(cspm_ctx *ctx);
/* integrates one fusion slot (its depth, normals, image and row of the camera table as they are on the device when the launch runs).
 * Asynchronous on the ctx stream.  Timed as one CSPM_K_MISC bracket with nx*ny*nz evaluations.  CSPM_ERR_STATE without a TSDF begin
 * ("tsdf: cspm_tsdf_begin first"), without a fusion begin ("fusion: cspm_fuse_begin first") or for a slot that holds no view
 * ("tsdf: no such fusion view"). */
int cspm_tsdf_integrate(cspm_ctx *ctx, int slot);
/* raycast into host maps, each optional: depth w*h f64, normal three planes of w*h f64, bgr 8UC3 rows of `stride` bytes, status w*h
 * bytes.  Synchronous.  Timed as one CSPM_K_MISC bracket with w*h evaluations.  CSPM_ERR_ARG for a NULL or bad camera, a bad z_near
 * ("tsdf: z_near must be finite and >= 0"), a bad size (the fusion's messages; h above 524280: "tsdf: h must be at most 524280"), a stride
 * below 3*w ("tsdf: stride is below 3 * w"); CSPM_ERR_STATE without a begin. */
int cspm_tsdf_raycast(cspm_ctx *ctx, const cspm_tsdf_camera *camera, int w, int h, double z_near, double *depth_out, double *normal_out,
                      uint8_t *bgr_out, size_t stride, uint8_t *status_out);
/* the same with device pointers (depth and normal 8-byte aligned); enqueues on the ctx stream and returns */
int cspm_tsdf_raycast_device(cspm_ctx *ctx, const cspm_tsdf_camera *camera, int w, int h, double z_near, void *d_depth_out, void *d_normal_out,
                             void *d_bgr_out, size_t stride, void *d_status_out);
/* raycast at the fusion pool's w x h INTO THE NEXT FUSION SLOT without leaving the device: the slot's depth (NaN where the ray
 * missed), normals, colour and camera.  The slot is a view like any other: a source and a target for cspm_fuse_register and cspm_fuse_run;
 * it counts as a view with an image when a view with an image has been integrated since the last clear.  Asynchronous.  The errors of the
 * raycast, and those of a push: CSPM_ERR_STATE without a fusion begin or a free slot, CSPM_ERR_ARG when earlier views have no normals. */
int cspm_tsdf_raycast_push(cspm_ctx *ctx, const cspm_tsdf_camera *camera, double z_near);
/* the surface points: cloud, capacity and count as in cspm_fuse_run.  Synchronous; host outputs, each optional.  Timed as one CSPM_K_MISC
 * bracket with nx*ny*nz evaluations.  CSPM_ERR_STATE without a begin. */
int cspm_tsdf_points(cspm_ctx *ctx, cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out);
/* the same with device pointers (the cloud 16-byte aligned, the count a 4-byte aligned unsigned int); enqueues and returns.  CSPM_ERR_ARG
 * ("tsdf: the cloud buffer must be 16-byte aligned", "tsdf: the count must be 4-byte aligned"). */
int cspm_tsdf_points_device(cspm_ctx *ctx, void *d_cloud_out, size_t cloud_cap, void *d_count_out);
/* downloads the volume in flat order, each output optional: D and W nx*ny*nz floats, colour 4 bytes per voxel (b, g, r, has).
 * Synchronous.  CSPM_ERR_STATE without a begin. */
int cspm_tsdf_get_volume(cspm_ctx *ctx, float *D_out, float *W_out, uint8_t *colour_out);
/* waits for the stream and frees the volume.  CSPM_ERR_STATE without a begin. */
int cspm_tsdf_end(cspm_ctx *ctx);
/* T alone on caller memory with a temporary context: fusion begin and TSDF begin, then per view one cspm_fuse_push_maps and one
 * cspm_tsdf_integrate in the order of `views`, the surface points and the volume (outputs as in cspm_tsdf_points and
 * cspm_tsdf_get_volume, each optional).  Synchronous.  Every argument is checked before a device is opened: the parameters, and what
 * cspm_fuse_depth_maps checks in views, n_views, w, h (with its messages). */
int cspm_tsdf_depth_maps(int device, const cspm_tsdf_params *params, const cspm_fuse_view *views, int n_views, int w, int h,
                         cspm_point *cloud_out, size_t cloud_cap, unsigned int *count_out, float *D_out, float *W_out, uint8_t *colour_out);

/* ---- TSDF meshes (an addition): the zero level set of the volume as triangles -----------------------------------------
 * T's surface points lie one on every sign change between 6-neighbours, which is where marching cubes puts its vertices.  The mesh reuses
 * them record for record, as cspm_mesh reuses the reprojection's points; what this section adds is connectivity.
 * The specification MC.  It holds no arithmetic of its own: predicates on T's D and W, and integers.
 * Cells and cases.  A cell (i, j, k) exists for 0 <= i <= nx-2, 0 <= j <= ny-2, 0 <= k <= nz-2; its eight corners are the voxels
 *  (i+dx, j+dy, k+dz), corner number c = dx | dy<<1 | dz<<2.  A volume with a dimension below 2 has no cells and so no faces.  A cell is
 *  KNOWN iff all eight corners have W > 0; an unknown cell emits nothing.  The case of a known cell has bit c set iff D(corner c) > 0.0f:
 *  the predicate of T's surface points, so a NaN or -0.0 corner is "not positive", as it is there.
 * Edges.  The cube edge along axis a whose lower corner has the offsets (u, w) on the two other axes, in increasing axis order, has the
 *  number e = 4*a + u + 2*w.  It belongs to the voxel at its lower corner and to axis a.  A sign-change edge of a known cell is by
 *  construction a counted neighbour of T's surface points (both W > 0, exactly one D > 0).
 * The table, derived and not typed (tools/gen_mc_table.py writes csrc/cspm_mc_table.h; tests/tsdfmesh_ref.py derives it again).
 *  Each of the six cube faces has its four corners in cyclic order, counter-clockwise seen from outside the cube in the right-handed frame
 *  x, y, z: for the face "axis a, side 1" with b = (a+1)%3, c = (a+2)%3 the (b, c) offsets run (0,0), (1,0), (1,1), (0,1); side 0 takes the
 *  reverse order.  Going round a face, every maximal run of positive corners is entered over one face edge (negative -> positive) and left
 *  over one (positive -> negative): next[entering edge] = leaving edge.  On a face with two diagonal positive corners each positive corner is
 *  thereby cut off on its own.  The rule looks only at the face's four signs, so the two cells that share a face always agree.  Every
 *  sign-change edge of the cube is entering on exactly one of its two faces and leaving on the other, so `next` is a permutation of the
 *  sign-change edges and falls into loops.  Take the loops in increasing order of their lowest edge number L0; follow next from there,
 *  L0, L1, .., L(m-1); emit the fan (L0, L(i+1), L(i)) for i = 1 .. m-2.  With this winding (v1 - v0) x (v2 - v0) points towards positive
 *  D: the free space, the direction of the surface points' own normals.  Case 1 gives (0, 8, 4), case 254 gives (0, 4, 8), case 0x69 gives
 *  (0,8,4), (1,11,5), (2,9,7), (3,10,6); 820 triangles over the 256 cases, at most 5 per cell.
 * Vertices: exactly the records of cspm_tsdf_points, in its order; vertex number = rank of the surface point.  The vertex on the edge
 *  (voxel u, axis a) has the number first[u] + the number of u's counted neighbours on the axes before a, first[u] being the number of
 *  surface points of all voxels before u in flat order.  Points on edges with no known cell around them stay in the list unreferenced.
 *  When D is exactly 0 at a corner several vertices coincide and some faces have zero area; they are emitted all the same, because the
 *  topology must stay closed.
 * Faces: one 12-byte cspm_face each; cells in flat order of their corner-0 voxel, within a cell the table's order, v[] the three vertex
 *  numbers in the table's order.
 * Counts and capacities are cspm_mesh's rule: both counts are reported whatever the capacities, the first `cap` records of each buffer are
 *  written and the rest is untouched.  Faces always carry full vertex numbers, so the mesh is complete only when both counts fit.  (Counts
 *  are 32-bit: a volume with more than 2^32 / 5 cells can overflow the face count.)
 * Memory: the first mesh call allocates first[] (4 bytes per voxel) and one count per 256 voxels, plus one, in the volume's pool; they are
 *  counted by CSPM_OPT_DEVICE_BYTES and freed with the volume.  A context that never meshes allocates and launches nothing new. */
/* the mesh of the volume into host buffers, each output optional (NULL buffers ask for the counts only).  Synchronous.  Timed as one
 * CSPM_K_MISC bracket with nx*ny*nz evaluations.  CSPM_ERR_STATE without a begin ("tsdf: cspm_tsdf_begin first"); CSPM_ERR_HIP without
 * memory or when a launch or a download fails ("tsdf: the mesh extraction failed", "tsdf: the mesh download failed"). */
int cspm_tsdf_mesh(cspm_ctx *ctx, cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap,
                   unsigned int *n_vertices_out, unsigned int *n_faces_out);
/* the same with device pointers, each optional; enqueues on the ctx stream and returns.  CSPM_ERR_STATE without a begin; CSPM_ERR_ARG
 * ("tsdf: the vertex buffer must be 16-byte aligned", "tsdf: the face buffer must be 4-byte aligned", "tsdf: the counts must be 4-byte
 * aligned"); CSPM_ERR_HIP without memory. */
int cspm_tsdf_mesh_device(cspm_ctx *ctx, void *d_vertices_out, size_t vertex_cap, void *d_faces_out, size_t face_cap, void *d_n_vertices_out,
                          void *d_n_faces_out);
/* the counterpart of cspm_tsdf_get_volume: uploads the planes that are given, as their bytes stand (D and W nx*ny*nz floats, colour 4 bytes
 * per voxel b, g, r, has); a NULL plane stays as it is.  Nothing is checked: a W that is no integer in [0, max_weight] is the caller's.  With
 * a colour plane the volume counts as coloured for cspm_tsdf_raycast_push.  Synchronous.  It keeps a model between sessions.
 * CSPM_ERR_STATE without a begin ("tsdf: cspm_tsdf_begin first"); CSPM_ERR_HIP when the upload fails ("tsdf: the upload failed"). */
int cspm_tsdf_set_volume(cspm_ctx *ctx, const float *D, const float *W, const uint8_t *colour);
/* MC alone on caller memory with a temporary context: what cspm_tsdf_depth_maps does up to the last integration, then the mesh (outputs
 * as in cspm_tsdf_mesh, each optional).  Synchronous.  Every argument is checked before a device is opened, with cspm_tsdf_depth_maps'
 * messages (CSPM_ERR_ARG); CSPM_ERR_HIP without a device or when the run fails ("tsdf meshing failed"). */
int cspm_tsdf_mesh_depth_maps(int device, const cspm_tsdf_params *params, const cspm_fuse_view *views, int n_views, int w, int h,
                              cspm_point *vertices_out, size_t vertex_cap, cspm_face *faces_out, size_t face_cap, unsigned int *n_vertices_out,
                              unsigned int *n_faces_out);

/* ---- rectification (an addition): a calibrated RAW pair undistorted and row-aligned on the device ----------------------
 * Every entry above that takes images assumes an undistorted, row-aligned pair, and cspm_reproject a cspm_calib of that pair.  This section
 * produces both from a rig description: two pinhole cameras with Brown-Conrady distortion and the pose of camera 1 in camera 0's frame.
 * The specification R.  Every product, sum, quotient and square root is one IEEE f64 operation in the association written here, nothing
 * contracted, no reciprocal, no trigonometry.  M[i][j] is entry 3*i + j of a row-major matrix.
 *
 * Derivation (host, cspm_rectify_compute): the axis construction of Fusiello et al. with the mean optical axis.
 *     C1[j]    = -((R[0][j]*T[0] + R[1][j]*T[1]) + R[2][j]*T[2])          the centre of camera 1 in camera 0's frame, -R^T T
 *     baseline = sqrt((C1[0]*C1[0] + C1[1]*C1[1]) + C1[2]*C1[2])
 *     e1       = C1 / baseline                                            three divisions
 *     zm       = (R[2][0], R[2][1], 1.0 + R[2][2])                        (0, 0, 1) + the third row of R: the sum of the two optical axes
 *     c        = zm x e1,  (p x q)[0] = p[1]*q[2] - p[2]*q[1], [1] = p[2]*q[0] - p[0]*q[2], [2] = p[0]*q[1] - p[1]*q[0]
 *     e2       = c / sqrt((c[0]*c[0] + c[1]*c[1]) + c[2]*c[2])            three divisions
 *     e3       = e1 x e2
 *     R0       = rows e1, e2, e3          R1[i][j] = (R0[i][0]*R[j][0] + R0[i][1]*R[j][1]) + R0[i][2]*R[j][2]         R1 = R0 R^T
 *   X_rect = R_v X_cam_v; camera 1's centre is (baseline, 0, 0) in the rectified frame.  CSPM_ERR_ARG unless e1[0] > 0, |e1[0]| >= |e1[1]| and
 *   |e1[0]| >= |e1[2]| (camera 1 is to the right of camera 0 and the rig is horizontal: otherwise the caller swaps the cameras), and
 *   when zm is parallel to e1.
 *   Projection.  params NULL or a field "automatic" (f not > 0; cx or cy NaN; w or h <= 0):
 *     f    = 0.25 * (((fx0 + fy0) + fx1) + fy1)            w, h = raw_w, raw_h
 *     per view v, from the centre pixel of the raw image through K_v^-1 (skew honoured, distortion ignored), rotated and projected:
 *       yn = ((double)(raw_h-1)/2.0 - cy_v) / fy_v         xn = (((double)(raw_w-1)/2.0 - cx_v) - skew_v*yn) / fx_v
 *       P[i] = (R_v[i][0]*xn + R_v[i][1]*yn) + R_v[i][2]   q_v = ((f*P[0]) / P[2], (f*P[1]) / P[2])
 *     cx = (double)(w-1)/2.0 - 0.5*(q_0.x + q_1.x)         cy = (double)(h-1)/2.0 - 0.5*(q_0.y + q_1.y)
 *   Both views share cx: the derived cspm_calib is {f, cx, cy, baseline, doffs = 0} and every point in front of the rig has a disparity >= 0.
 *   CSPM_ERR_ARG for any non-finite input (an infinite f, cx or cy in params included), fx or fy <= 0, T = 0, raw_w, raw_h, w or h < 1,
 *   w*h >= 2^31, or a derived f, cx or cy that is not finite (a centre ray with P[2] = 0).
 *
 * Map M_v(x, y) -> (sx, sy, front), on the device, r_ij = R_v[i][j] (applied transposed: the ray in camera v), cxraw = cx_v, cyraw = cy_v:
 *     u = ((double)x - cx) / f          wv = ((double)y - cy) / f
 *     X = (r00*u + r10*wv) + r20        Y = (r01*u + r11*wv) + r21        Z = (r02*u + r12*wv) + r22
 *     front = Z > 0.0
 *     a = X / Z    b = Y / Z    r2 = a*a + b*b
 *     rad = 1.0 + r2*(k1 + r2*(k2 + r2*k3))
 *     ad = a*rad + ((2.0*p1)*a*b + p2*(r2 + 2.0*a*a))
 *     bd = b*rad + (p1*(r2 + 2.0*b*b) + (2.0*p2)*a*b)
 *     sx = (fx*ad + skew*bd) + cxraw    sy = fy*bd + cyraw
 *   Rectified -> raw is the forward distortion model: no iteration anywhere.  valid = front && 0 <= sx <= raw_w-1 && 0 <= sy <= raw_h-1, every
 *   comparison false for NaN.  The stored map holds sx, sy as computed, also where they are invalid or NaN.
 *
 * Remap.  A valid pixel: x0 = (int)floor(sx), x1 = min(x0+1, raw_w-1), y0, y1 likewise, tx = sx - x0, ty = sy - y0 and per channel, the
 * four taps I[y][x] as doubles:
 *     top = I00 + tx*(I01 - I00)        bot = I10 + tx*(I11 - I10)        val = top + ty*(bot - top)
 *   the output byte is Round2Int(val) (round half to even) saturated to 0 .. 255.  An invalid pixel is (0, 0, 0) and its valid byte is 0. */
typedef struct cspm_camera {
  double fx, fy, cx, cy, skew; /* K = [fx skew cx; 0 fy cy; 0 0 1] */
  double k1, k2, p1, p2, k3;   /* Brown-Conrady: radial k1, k2, k3, tangential p1, p2 */
} cspm_camera;
typedef struct cspm_rig {
  cspm_camera cam[2];
  double R[9], T[3]; /* X1 = R*X0 + T, row-major R */
  int raw_w, raw_h;  /* both raw images */
} cspm_rig;
typedef struct cspm_rect_params {
  double f, cx, cy; /* f <= 0, NaN cx / cy: automatic */
  int w, h;         /* <= 0: automatic (the raw size) */
} cspm_rect_params;
typedef struct cspm_rectification {
  double R0[9], R1[9]; /* X_rect = Rv * X_camv */
  double f, cx, cy, baseline;
  int w, h;
} cspm_rectification;
/* everything automatic */
int cspm_rect_default_params(cspm_rect_params *p);
/* the derivation: pure host logic, answers without a GPU.  params may be NULL (all automatic); rect_out and calib_out are each optional.
 * The message of a CSPM_ERR_ARG is cspm_last_error(NULL)'s. */
int cspm_rectify_compute(const cspm_rig *rig, const cspm_rect_params *params, cspm_rectification *rect_out, cspm_calib *calib_out);
/* R alone on caller memory, no context needed, synchronous: the map of `view` and, with bgr_out, the remap of one raw image (packed 8UC3
 * rows of raw_stride bytes, rig->raw_w x rig->raw_h) into rect->w x rect->h rows of out_stride bytes (bytes beyond 3*w are untouched).
 * Each output is optional: map_out 2*w*h doubles (the plane sx, then the plane sy), valid_out w*h bytes.  Arguments are checked before a
 * device is opened: CSPM_ERR_ARG for a NULL rig or rect, a rig or rectification cspm_rectify_compute would refuse or could not have
 * produced (non-finite values, f <= 0, sizes < 1, w*h or raw_w*raw_h >= 2^31), a view outside 0 .. 1, bgr_out without raw, a raw_stride
 * below 3*raw_w or an out_stride below 3*w. */
int cspm_rectify_host(int device, const cspm_rig *rig, const cspm_rectification *rect, int view, const uint8_t *raw, size_t raw_stride,
                      uint8_t *bgr_out, size_t out_stride, double *map_out, uint8_t *valid_out);
/* builds both views' maps on the ctx stream and keeps them with the context (17 bytes per pixel and view) until the context goes or a
 * call with rig == NULL (then rect is ignored) drops them; a call with the rig and rectification already stored launches nothing.
 * One rig serves many pairs.  With no rectification stored no other entry changes a byte or a launch.  Argument checks as above. */
int cspm_set_rectification(cspm_ctx *ctx, const cspm_rig *rig, const cspm_rectification *rect);
/* the stored map of one view, layouts as cspm_rectify_host; each output optional.  Synchronous.  CSPM_ERR_STATE without a rectification. */
int cspm_get_rect_map(cspm_ctx *ctx, int view, double *xy_out, uint8_t *valid_out);
/* cspm_set_images with a RAW pair of the rig's size (rows of `stride` bytes, >= 3*raw_w): both images are remapped through the stored maps
 * on the ctx stream and the rectified rect.w x rect.h pair goes down exactly the path of cspm_set_images_device; afterwards the context
 * is in the state cspm_set_images would have left it in with the rectified bytes (cspm_get_level_image(ctx, v, 0, ...) returns them).
 * Synchronous like cspm_set_images.  The remap of both views is timed as one CSPM_K_MISC bracket.  Scratch (the packed raw pair and the
 * rectified 8UC3 pair) is allocated by the first call and kept with the rectification.  CSPM_ERR_STATE without a stored rectification;
 * CSPM_ERR_ARG for a NULL image or a stride below 3*raw_w. */
int cspm_set_images_raw(cspm_ctx *ctx, const uint8_t *l_raw, const uint8_t *r_raw, size_t stride);
/* the same from device memory, asynchronous, with the contract of cspm_set_images_device */
int cspm_set_images_raw_device(cspm_ctx *ctx, const void *d_l_raw, const void *d_r_raw, size_t stride);

/* ---- CSPatchMatch::PatchMatch over a FOREIGN IPlaneCost (plane_cost/i_plane_cost.h:28-33) ------------------------------
 * Any object with a GetPlaneCost(x, y, plane, view) that is not one of this library's device costs: the reference drives it
 * through the virtual call (call sites cs_patchmatch.cc:144,181,191,200,208,269,334).  Here the device keeps the plane field,
 * draws every candidate from the same random streams and applies the reference's accept rules; the CALLER evaluates the
 * candidates with its cost function -- the plugin contract, batched:
 *     cspm_fpm_begin(ctx, w, h, max_dis);                       plane field, no cost object, no images needed
 *     per batch:  cspm_fpm_candidates(...) -> n candidates {xy, view, plane};  cost[i] = GetPlaneCost(...) for xy[2i] >= 0;
 *                 cspm_fpm_commit(ctx, cost)
 *   phase CSPM_FPM_INIT    (iter, step ignored): InitRandomPlane, 2*w*h candidates                (:115-148)
 *   phase CSPM_FPM_SPATIAL (step = anti-diagonal 0 .. w+h-2 of the raster sweep of iteration iter): 2 per pixel, x- then
 *                           y-predecessor's plane, xy[2i] = -1 where the pixel has no such predecessor (:163-216)
 *   phase CSPM_FPM_VIEW    (step = target view): w*h candidates, one per source pixel of the other view (:229-277)
 *   phase CSPM_FPM_REFINE  (step = halving step 0 ..): 2*w*h candidates                            (:292-345)
 * Arrays must hold max(2*w*h, 4*min(w,h)) candidates.  Synchronous.  Afterwards cspm_get_planes / cspm_get_disparity_* / cspm_postprocess
 * (which needs cspm_set_images for the weighted median) read the result as usual. */
#define CSPM_FPM_INIT 0
#define CSPM_FPM_SPATIAL 1
#define CSPM_FPM_VIEW 2
#define CSPM_FPM_REFINE 3
int cspm_fpm_begin(cspm_ctx *ctx, int w, int h, int max_dis);
int cspm_fpm_candidates(cspm_ctx *ctx, int phase, int iter, int step, const cspm_pm_params *p, int *n_out, int *xy_out, int *view_out,
                        double *plane_out);
int cspm_fpm_commit(cspm_ctx *ctx, const double *cost);

/* ---- cost aggregation and local stereo (CAMethod, ca_method.h:8-25; ca_filter/) ------------------------------------------------
 * The three CAMethod implementations of the reference, applied to f64 slabs of h*w with a 3-channel f64 guide:
 *   CSPM_CA_BOX  BoxCA: BoxFilter(p, 3), the unnormalised 7x7 sum of two serial cumulative sums (BoxCA.cpp:5-13, GuidedFilter.cpp:29-122)
 *   CSPM_CA_GF   GFCA:  GuidedFilter(I, p, 9, 0.0001f), colour branch with FAST_INV (GFCA.cpp:5-12, GuidedFilter.cpp:131-299)
 *   CSPM_CA_BF   BFCA:  BilateralFilter(I, p, 35), colour branch, sig_sp 17.5, sig_clr 0.03, wrap-around borders (BFCA.cpp:5-13,
 *                       BilateralFilter.cpp:51-97); its weights use the device's f64 exp
 * Every op in the reference's order, no contraction.  A filtered slab needs min(w, h) >= 7 (BOX), 19 (GF), 17 (BF): below that the
 * reference indexes outside the image; such a call fails with CSPM_ERR_ARG. */
#define CSPM_CA_BOX 0
#define CSPM_CA_GF 1
#define CSPM_CA_BF 2
/* CAMethod::aggreCV on host buffers: guide h*w*3 doubles as given, vol n_slices slabs of h*w, slices 1.. filtered in place */
int cspm_aggregate_cv_host(int device, int method, const double *guide, int w, int h, int n_slices, double *vol);
/* local stereo over the ctx's cost object: both views' plane fields; asynchronous on the ctx stream like cspm_patchmatch.
 * PreSSPC / PreCSPC with a CAMethod between buildCV and the max-cost loop (pre_cs_pc.cc:57-84), then the cost of the fronto-parallel
 * plane of every d = 1 .. max_dis-1 with the window reduced to its centre (pre_cs_pc.cc:157-183, pre_ss_pc.cc:99-111), then
 * winner-take-all (the first d that reaches the minimum):
 *   - per view v and level s: aggreCV over the raw cells 0 .. D_s (those cspm_get_cost_slab returns) with maxDis = D_s + 1, guided by
 *     view v's level image, BGR -> RGB, each 8-bit value times (double)(1.0f/255.0f); M[v][s] = max(-1.0, max of the aggregated volume);
 *   - cost(d) = sum over s of c_s * w_s, c_s = M[v][s] where f = (int)(d halved s times) is <= 0 or >= D_s, else the linear
 *     interpolation between aggregated slices f and f+1 at (x>>s, y>>s);
 *   - plane = Plane(Vec3d(0,0,1), Point3d(x, y, d*)), min_cost = cost(d*).
 * The cost object is read, never written: cspm_get_disparity_*, cspm_postprocess(_device) and cspm_patchmatch work afterwards as usual.
 * CSPM_ERR_STATE without a cost object or with a GrdPC / CSPC cost (no cells); CSPM_ERR_ARG for a bad method or a level too small.
 * Its launches are timed under CSPM_K_MISC. */
int cspm_local_stereo(cspm_ctx *ctx, int method);

/* ---- measurement --------------------------------------------------------------------------------
 * When enabled, every kernel launch is bracketed by hipEvents on the ctx stream. */
#define CSPM_K_GRD 0      /* cost-volume construction kernels */
#define CSPM_K_INIT 1     /* plane cost evaluation: random init */
#define CSPM_K_SPATIAL 2  /* plane cost evaluation: spatial propagation */
#define CSPM_K_VIEW 3     /* plane cost evaluation: view propagation */
#define CSPM_K_REFINE 4   /* plane cost evaluation: plane refinement (the dominant kernel) */
#define CSPM_K_MISC 5     /* pyramid, resolve, disparity, ... */
#define CSPM_K_POST 6     /* PostProcessing: left-right check, fill, weighted median */
#define CSPM_K_COUNT 7
int cspm_enable_timing(cspm_ctx *ctx, int on);
int cspm_reset_timing(cspm_ctx *ctx);
/* launches, summed milliseconds and summed evaluated candidate planes of a kernel class */
int cspm_get_timing(cspm_ctx *ctx, int kclass, long long *launches, double *total_ms, long long *evals);
/* exact in-image window taps of ONE evaluation of every pixel of one view (sum over pixels, levels) */
long long cspm_taps_per_view_pass(const cspm_ctx *ctx);
/* lane-taps the row engine executes for the same pass (masked window columns and tail lanes included): the denominator of
 * "executed vs algorithmic taps" */
long long cspm_row_engine_taps_per_view_pass(const cspm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
