"""ctypes view of the C ABI in include/cspm.h (libcspm_hip.so).  Plumbing only -- all compute is in
the HIP library.  Fails loudly when the library is missing; there is no fallback path."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("CSPM_LIB") or os.path.join(_HERE, "libcspm_hip.so")  # CSPM_LIB: an alternative build of the same library (tuning experiments)

SCHED_RASTER, SCHED_REDBLACK, SCHED_DIFFUSE = 0, 1, 2  # DIFFUSE: rb_neighbours is 4, 8 or 20 (include/cspm.h)
RNG_PER_PIXEL, RNG_ROW_SHARED = 0, 1
K_GRD, K_INIT, K_SPATIAL, K_VIEW, K_REFINE, K_MISC, K_POST = range(7)
K_NAMES = ["grd", "init", "spatial", "view", "refine", "misc", "post"]
MAX_LEVELS = 8
OPT_GRD_VOLUMES = 1
OPT_RASTER_LAUNCHES = 2
OPT_SWEEP_TIMEOUT_MS = 3
OPT_SWEEP_FALLBACKS = 4
OPT_SWEEP_PAIRS = 5          # paired-cell volumes for the raster sweep: 0 never (default), 1 when they fit
OPT_SWEEP_PAIRS_ACTIVE = 6   # read only
OPT_TABLE_VOLUMES = 7        # device-cell volumes for the row kernels' DMA-filled tables: 1 when they fit (default), 0 never
OPT_TABLE_VOLUMES_ACTIVE = 8 # read only
OPT_SWEEP_PACKED = 10        # packed 8-byte pixels for the raster sweep (default 0: measured slower)
OPT_SWEEP_PACKED_ACTIVE = 11 # read only
OPT_SWEEP_PACKED_BAD = 12    # read only, synchronises: pixels the packer could not represent (0 by construction)
OPT_SWEEP_FLOW = 13          # persistent raster sweep scheduled by dataflow (1: measured slower) or by ordered claims (0, default)
OPT_SWEEP_WG = 14            # persistent sweep workgroups launched per CU; default 0 = the library chooses: 2, and 3 where 2 * min(w, h) >= 4 * CUs and OPT_SWEEP_FOLD is 0 (identical planes)
OPT_VOLUME_FALLBACKS = 9     # read only: hipMalloc failures of an optional volume this context survived
OPT_VOLUME_RETRY_PAIRS = 15  # a cost object that runs without the optional volumes it wanted asks again after this many reuses (default 16, 0 = never)
OPT_VIEW_SORT = 17           # view propagation evaluates a row's proposals in target-column order (default 1; identical planes either way)
OPT_SWEEP_FOLD = 18          # 1 = cross-scale sweep workgroups of levels - 1 waves, the coarsest level folded onto them; default 0, callers with two or more pairs in flight set 1 (identical planes)
OPT_FAULT_VOLUME_ALLOC = 16  # write only, TEST HOOK: the n-th optional-volume allocation from now on fails
OPT_SWEEP_GRID = 23          # write only, TEST HOOK: 0 = the library's grid (default), else the persistent sweep launches at most max(value, row bands) workgroups (identical planes)
OPT_CENGRD_FUSED = 19        # set before build_cost_cengrd: 1 = no volumes, the cells are computed inside the PatchMatch kernels (default 0; identical planes)
OPT_CENGRD_FUSED_ACTIVE = 20 # read only: the current cost object is a fused CENGRD one
OPT_PP_SPECKLE_REMOVED = 21  # read only, synchronises: pixels the speckle filter removed from both masks in the last post-processing
OPT_DEVICE_BYTES = 22        # read only, no synchronisation: bytes of device memory the context holds (requested sizes; staging temporaries not included)
MEDIAN_MAX_RADIUS = 7  # CSPM_MEDIAN_MAX_RADIUS: the median filter's window is at most 15 x 15
CA_BOX, CA_GF, CA_BF = 0, 1, 2  # cost aggregation: BoxCA, GFCA, BFCA (ca_filter/)
SYNTH_MAX_WIDTH = 6784  # CSPM_SYNTH_MAX_WIDTH: the widest image cspm_synthesize* takes (a target row lives in one workgroup's LDS)
GEOM_RAW, GEOM_PP = 0, 1  # cspm_reproject's source: the stored field's a*x+b*y+c, or the sub-pixel post-processed map
CENGRD_KAPPA, CENGRD_TAU = 0.0625, 32.0  # CSPM_CENGRD_KAPPA / CSPM_CENGRD_TAU: cell = fma(KAPPA, min(H, TAU), G)

# every symbol include/cspm.h declares
SYMBOLS = [
    "cspm_device_count", "cspm_create", "cspm_destroy", "cspm_last_error", "cspm_set_stream", "cspm_get_stream", "cspm_synchronize",
    "cspm_set_images", "cspm_set_images_device", "cspm_build_cost_grd", "cspm_build_cost_cen", "cspm_build_cost_cengrd", "cspm_build_cost_img", "cspm_cen_build_cv_host", "cspm_cengrd_build_cv_host", "cspm_set_option", "cspm_get_option", "cspm_begin_cost", "cspm_upload_cost_slab",
    "cspm_finish_cost", "cspm_get_levels", "cspm_get_level_dims", "cspm_get_level_image", "cspm_get_cost_slab",
    "cspm_get_max_cost", "cspm_get_scale_weights", "cspm_grd_build_cv_host", "cspm_plane_cost_batch",
    "cspm_pm_default_params", "cspm_patchmatch", "cspm_pm_init", "cspm_pm_spatial", "cspm_pm_view", "cspm_pm_refine",
    "cspm_get_planes", "cspm_set_planes", "cspm_get_disparity_u8", "cspm_get_disparity_f64",
    "cspm_disparity_u8_device", "cspm_postprocess", "cspm_postprocess_device", "cspm_postprocess_f64", "cspm_postprocess_f64_device",
    "cspm_enable_timing", "cspm_reset_timing", "cspm_get_timing",
    "cspm_taps_per_view_pass", "cspm_row_engine_taps_per_view_pass", "cspm_fpm_begin", "cspm_fpm_candidates", "cspm_fpm_commit",
    "cspm_aggregate_cv_host", "cspm_local_stereo", "cspm_rescore_planes", "cspm_patchmatch_warm", "cspm_upsample_planes",
    "cspm_merge_planes", "cspm_merge_planes_host", "cspm_pm_init_keep",
    "cspm_set_pp_speckle", "cspm_get_pp_speckle", "cspm_filter_speckles_host",
    "cspm_median_filter_u8_host", "cspm_median_filter_f64_host", "cspm_set_pp_median", "cspm_get_pp_median",
    "cspm_smooth_default_params", "cspm_smooth_disparity_host", "cspm_set_pp_smooth", "cspm_get_pp_smooth",
    "cspm_fit_default_params", "cspm_fit_planes_host", "cspm_fit_planes",
    "cspm_seg_default_params", "cspm_segment_count", "cspm_segment_host", "cspm_segment_planes_host", "cspm_segment_planes", "cspm_get_segments",
    "cspm_geom_default_params", "cspm_reproject_host", "cspm_reproject", "cspm_reproject_device",
    "cspm_mesh_default_params", "cspm_mesh_host", "cspm_mesh", "cspm_mesh_device",
    "cspm_synth_default_params", "cspm_synthesize_host", "cspm_synthesize", "cspm_synthesize_device",
    "cspm_fuse_default_params", "cspm_fuse_depth_maps", "cspm_fuse_begin", "cspm_fuse_push", "cspm_fuse_push_maps", "cspm_fuse_view_count",
    "cspm_fuse_run", "cspm_fuse_run_device", "cspm_fuse_end",
    "cspm_reg_default_params", "cspm_fuse_register", "cspm_fuse_get_pose", "cspm_fuse_set_pose", "cspm_register_depth_maps",
    "cspm_carry_default_params", "cspm_carry_relative_pose", "cspm_carry_plane_field", "cspm_carry_planes",
    "cspm_tsdf_default_params", "cspm_tsdf_begin", "cspm_tsdf_clear", "cspm_tsdf_integrate", "cspm_tsdf_raycast", "cspm_tsdf_raycast_device",
    "cspm_tsdf_raycast_push", "cspm_tsdf_points", "cspm_tsdf_points_device", "cspm_tsdf_get_volume", "cspm_tsdf_end", "cspm_tsdf_depth_maps",
    "cspm_tsdf_mesh", "cspm_tsdf_mesh_device", "cspm_tsdf_set_volume", "cspm_tsdf_mesh_depth_maps",
    "cspm_rect_default_params", "cspm_rectify_compute", "cspm_rectify_host", "cspm_set_rectification", "cspm_get_rect_map",
    "cspm_set_images_raw", "cspm_set_images_raw_device",
]


class CspmError(RuntimeError):
    pass


class PmParams(C.Structure):
    """struct cspm_pm_params"""
    _fields_ = [("seed", C.c_uint64), ("schedule", C.c_int), ("rb_rounds", C.c_int), ("rb_neighbours", C.c_int),
                ("rng_mode", C.c_int), ("early_exit", C.c_int)]


class FitParams(C.Structure):
    """struct cspm_fit_params"""
    _fields_ = [("radius", C.c_int), ("max_diff", C.c_double), ("min_support", C.c_int), ("use_guide", C.c_int)]


class SegParams(C.Structure):
    """struct cspm_seg_params"""
    _fields_ = [("step", C.c_int), ("compactness", C.c_int), ("iters", C.c_int), ("tau", C.c_double), ("rounds", C.c_int), ("min_support", C.c_int)]


class SmoothParams(C.Structure):
    """struct cspm_smooth_params"""
    _fields_ = [("lambda_", C.c_double), ("sigma_color", C.c_double), ("iterations", C.c_int), ("fill_conf", C.c_double)]


class Calib(C.Structure):
    """struct cspm_calib: a rectified pair (focal length in pixels, principal point of view 0, baseline, doffs = cx1 - cx0)"""
    _fields_ = [("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("baseline", C.c_double), ("doffs", C.c_double)]


class GeomParams(C.Structure):
    """struct cspm_geom_params"""
    _fields_ = [("z_near", C.c_double), ("z_far", C.c_double), ("min_cos", C.c_double), ("left_frame", C.c_int), ("consistent_only", C.c_int)]


class MeshParams(C.Structure):
    """struct cspm_mesh_params"""
    _fields_ = [("max_diff", C.c_double), ("all_vertices", C.c_int)]


class SynthParams(C.Structure):
    """struct cspm_synth_params"""
    _fields_ = [("views", C.c_int), ("fill", C.c_int), ("max_stretch", C.c_double), ("merge_diff", C.c_double)]


class SynthView(C.Structure):
    """struct cspm_synth_view: one source view of cspm_synthesize_host"""
    _fields_ = [("disp", C.POINTER(C.c_double)), ("valid", C.POINTER(C.c_uint8)), ("slope_a", C.POINTER(C.c_double)),
                ("bgr", C.POINTER(C.c_uint8)), ("stride", C.c_size_t)]


class FuseParams(C.Structure):
    """struct cspm_fuse_params"""
    _fields_ = [("max_reproj", C.c_double), ("max_rel_depth", C.c_double), ("min_cos", C.c_double), ("min_views", C.c_int), ("suppress", C.c_int)]


class FuseView(C.Structure):
    """struct cspm_fuse_view: one view of cspm_fuse_depth_maps (maps, pinhole camera, camera -> world pose)"""
    _fields_ = [("depth", C.POINTER(C.c_double)), ("normal", C.POINTER(C.c_double)), ("bgr", C.POINTER(C.c_uint8)), ("bgr_stride", C.c_size_t),
                ("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class RegParams(C.Structure):
    """struct cspm_reg_params"""
    _fields_ = [("iters", C.c_int), ("stride", C.c_int), ("max_dist", C.c_double), ("huber", C.c_double), ("min_cos", C.c_double),
                ("min_pairs", C.c_int), ("pivot_rel", C.c_double)]


class RegIter(C.Structure):
    """struct cspm_reg_iter: one Gauss-Newton iteration of a registration"""
    _fields_ = [("pairs", C.c_double), ("cost", C.c_double), ("rot2", C.c_double), ("trans2", C.c_double), ("status", C.c_int)]


REG_ITER = np.dtype(dict(names=["pairs", "cost", "rot2", "trans2", "status"], formats=["<f8", "<f8", "<f8", "<f8", "<i4"], offsets=[0, 8, 16, 24, 32],
                         itemsize=40))  # RegIter as a numpy record


class TsdfParams(C.Structure):
    """struct cspm_tsdf_params"""
    _fields_ = [("origin", C.c_double * 3), ("voxel", C.c_double), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("trunc", C.c_double),
                ("max_weight", C.c_double), ("min_cos", C.c_double), ("step_rel", C.c_double)]


class TsdfCamera(C.Structure):
    """struct cspm_tsdf_camera: a pinhole camera and its camera -> world pose"""
    _fields_ = [("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class CarryParams(C.Structure):
    """struct cspm_carry_params"""
    _fields_ = [("fill", C.c_int)]


class Camera(C.Structure):
    """struct cspm_camera: K = [fx skew cx; 0 fy cy; 0 0 1] and Brown-Conrady distortion"""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "skew", "k1", "k2", "p1", "p2", "k3")]


class Rig(C.Structure):
    """struct cspm_rig: two cameras, X1 = R*X0 + T (row-major R), the raw image size"""
    _fields_ = [("cam", Camera * 2), ("R", C.c_double * 9), ("T", C.c_double * 3), ("raw_w", C.c_int), ("raw_h", C.c_int)]


class RectParams(C.Structure):
    """struct cspm_rect_params: f <= 0, NaN cx / cy, w / h <= 0 = automatic"""
    _fields_ = [("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("w", C.c_int), ("h", C.c_int)]


class Rectification(C.Structure):
    """struct cspm_rectification: X_rect = Rv * X_camv, the common projection, the rectified size"""
    _fields_ = [("R0", C.c_double * 9), ("R1", C.c_double * 9), ("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("baseline", C.c_double), ("w", C.c_int), ("h", C.c_int)]


# struct cspm_point: one 32-byte cloud record
Point = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                  ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("pixel", "<u4")])
assert Point.itemsize == 32
# struct cspm_face: the three vertex numbers of one triangle
Face = np.dtype([("v", "<u4", 3)])
assert Face.itemsize == 12


def library_path():
    return _SO


def build_library(force=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)] + [os.path.join(_HERE, "..", "include", "cspm.h")]
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", src_dir, "-B"], stdout=subprocess.DEVNULL)
    return _SO


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise CspmError(f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(_SO)
    vp, dp, ip, u8p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    llp = C.POINTER(C.c_longlong)
    pp = C.POINTER(PmParams)
    fp = C.POINTER(FitParams)
    mp = C.POINTER(SmoothParams)
    qp, i32p = C.POINTER(SegParams), C.POINTER(C.c_int32)
    kp, gp, up = C.POINTER(Calib), C.POINTER(GeomParams), C.POINTER(C.c_uint)
    sp, svp = C.POINTER(SynthParams), C.POINTER(SynthView)
    mshp = C.POINTER(MeshParams)
    rgp, rpp, rcp = C.POINTER(Rig), C.POINTER(RectParams), C.POINTER(Rectification)
    fup, fuv = C.POINTER(FuseParams), C.POINTER(FuseView)
    tsp, tcp = C.POINTER(TsdfParams), C.POINTER(TsdfCamera)
    rgpp, rgip = C.POINTER(RegParams), C.POINTER(RegIter)
    cyp = C.POINTER(CarryParams)
    sig = {
        "cspm_device_count": (C.c_int, []),
        "cspm_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "cspm_destroy": (None, [vp]),
        "cspm_last_error": (C.c_char_p, [vp]),
        "cspm_set_stream": (C.c_int, [vp, vp]),
        "cspm_get_stream": (C.c_int, [vp, C.POINTER(vp)]),
        "cspm_synchronize": (C.c_int, [vp]),
        "cspm_set_images": (C.c_int, [vp, u8p, u8p, C.c_int, C.c_int, C.c_size_t]),
        "cspm_set_images_device": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_size_t]),
        "cspm_build_cost_grd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double]),
        "cspm_set_option": (C.c_int, [vp, C.c_int, C.c_longlong]),
        "cspm_get_option": (C.c_int, [vp, C.c_int, llp]),
        "cspm_build_cost_cen": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double]),
        "cspm_build_cost_cengrd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double]),
        "cspm_build_cost_img": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double]),
        "cspm_cen_build_cv_host": (C.c_int, [C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_cengrd_build_cv_host": (C.c_int, [C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_begin_cost": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double]),
        "cspm_upload_cost_slab": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp, C.c_size_t]),
        "cspm_finish_cost": (C.c_int, [vp]),
        "cspm_get_levels": (C.c_int, [vp]),
        "cspm_get_level_dims": (C.c_int, [vp, C.c_int, ip, ip, ip]),
        "cspm_get_level_image": (C.c_int, [vp, C.c_int, C.c_int, u8p]),
        "cspm_get_cost_slab": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_get_max_cost": (C.c_int, [vp, C.c_int, C.c_int, dp]),
        "cspm_get_scale_weights": (C.c_int, [vp, dp]),
        "cspm_grd_build_cv_host": (C.c_int, [C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_plane_cost_batch": (C.c_int, [vp, C.c_int, C.c_int, ip, dp, dp]),
        "cspm_pm_default_params": (C.c_int, [pp]),
        "cspm_patchmatch": (C.c_int, [vp, C.c_int, pp]),
        "cspm_pm_init": (C.c_int, [vp, pp]),
        "cspm_pm_spatial": (C.c_int, [vp, C.c_int, pp]),
        "cspm_pm_view": (C.c_int, [vp, C.c_int, pp]),
        "cspm_pm_refine": (C.c_int, [vp, C.c_int, pp]),
        "cspm_get_planes": (C.c_int, [vp, C.c_int, dp, dp]),
        "cspm_set_planes": (C.c_int, [vp, C.c_int, dp, dp]),
        "cspm_get_disparity_u8": (C.c_int, [vp, C.c_int, C.c_int, u8p, C.c_size_t]),
        "cspm_get_disparity_f64": (C.c_int, [vp, C.c_int, dp]),
        "cspm_disparity_u8_device": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "cspm_postprocess": (C.c_int, [vp, C.c_int, u8p, u8p, C.c_size_t]),
        "cspm_postprocess_device": (C.c_int, [vp, C.c_int, vp, vp]),
        "cspm_postprocess_f64": (C.c_int, [vp, dp, dp, u8p, u8p]),
        "cspm_postprocess_f64_device": (C.c_int, [vp, vp, vp]),
        "cspm_enable_timing": (C.c_int, [vp, C.c_int]),
        "cspm_reset_timing": (C.c_int, [vp]),
        "cspm_get_timing": (C.c_int, [vp, C.c_int, llp, dp, llp]),
        "cspm_fpm_begin": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "cspm_fpm_candidates": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, pp, ip, ip, ip, dp]),
        "cspm_fpm_commit": (C.c_int, [vp, dp]),
        "cspm_taps_per_view_pass": (C.c_longlong, [vp]),
        "cspm_row_engine_taps_per_view_pass": (C.c_longlong, [vp]),
        "cspm_aggregate_cv_host": (C.c_int, [C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_local_stereo": (C.c_int, [vp, C.c_int]),
        "cspm_rescore_planes": (C.c_int, [vp]),
        "cspm_patchmatch_warm": (C.c_int, [vp, C.c_int, pp]),
        "cspm_upsample_planes": (C.c_int, [vp, vp]),
        "cspm_merge_planes": (C.c_int, [vp, vp]),
        "cspm_merge_planes_host": (C.c_int, [vp, C.c_int, dp, u8p]),
        "cspm_pm_init_keep": (C.c_int, [vp, pp]),
        "cspm_set_pp_speckle": (C.c_int, [vp, C.c_int, C.c_double]),
        "cspm_get_pp_speckle": (C.c_int, [vp, ip, dp]),
        "cspm_filter_speckles_host": (C.c_int, [C.c_int, dp, u8p, C.c_int, C.c_int, C.c_int, C.c_double, u8p, C.POINTER(C.c_int32)]),
        "cspm_median_filter_u8_host": (C.c_int, [C.c_int, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_size_t]),
        "cspm_median_filter_f64_host": (C.c_int, [C.c_int, dp, C.c_int, C.c_int, C.c_int, dp]),
        "cspm_set_pp_median": (C.c_int, [vp, C.c_int]),
        "cspm_get_pp_median": (C.c_int, [vp, ip]),
        "cspm_smooth_default_params": (C.c_int, [mp]),
        "cspm_smooth_disparity_host": (C.c_int, [C.c_int, dp, dp, u8p, C.c_int, C.c_int, mp, C.c_int, dp]),
        "cspm_set_pp_smooth": (C.c_int, [vp, mp]),
        "cspm_get_pp_smooth": (C.c_int, [vp, mp, ip]),
        "cspm_fit_default_params": (C.c_int, [fp]),
        "cspm_fit_planes_host": (C.c_int, [C.c_int, dp, u8p, u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, fp, dp, u8p]),
        "cspm_fit_planes": (C.c_int, [vp, fp, C.c_int]),
        "cspm_seg_default_params": (C.c_int, [qp]),
        "cspm_segment_count": (C.c_int, [C.c_int, C.c_int, C.c_int]),
        "cspm_segment_host": (C.c_int, [C.c_int, u8p, C.c_size_t, C.c_int, C.c_int, qp, i32p, i32p, i32p]),
        "cspm_segment_planes_host": (C.c_int, [C.c_int, dp, u8p, i32p, C.c_int, C.c_int, C.c_int, qp, dp, i32p, dp, u8p]),
        "cspm_segment_planes": (C.c_int, [vp, qp, C.c_int]),
        "cspm_get_segments": (C.c_int, [vp, C.c_int, i32p]),
        "cspm_geom_default_params": (C.c_int, [gp]),
        "cspm_reproject_host": (C.c_int, [C.c_int, kp, gp, C.c_int, dp, u8p, dp, dp, u8p, C.c_size_t, C.c_int, C.c_int, dp, dp, dp, u8p, vp, C.c_size_t, up]),
        "cspm_reproject": (C.c_int, [vp, C.c_int, C.c_int, kp, gp, fp, dp, dp, dp, u8p, vp, C.c_size_t, up]),
        "cspm_reproject_device": (C.c_int, [vp, C.c_int, C.c_int, kp, gp, fp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "cspm_mesh_default_params": (C.c_int, [mshp]),
        "cspm_mesh_host": (C.c_int, [C.c_int, kp, gp, mshp, C.c_int, dp, u8p, dp, dp, u8p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t,
                                     u8p, up, up]),
        "cspm_mesh": (C.c_int, [vp, C.c_int, C.c_int, kp, gp, fp, mshp, vp, C.c_size_t, vp, C.c_size_t, u8p, up, up]),
        "cspm_mesh_device": (C.c_int, [vp, C.c_int, C.c_int, kp, gp, fp, mshp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp]),
        "cspm_synth_default_params": (C.c_int, [sp]),
        "cspm_synthesize_host": (C.c_int, [C.c_int, sp, C.c_double, svp, svp, C.c_int, C.c_int, u8p, C.c_size_t, dp, u8p]),
        "cspm_synthesize": (C.c_int, [vp, C.c_int, sp, C.c_double, u8p, C.c_size_t, dp, u8p]),
        "cspm_synthesize_device": (C.c_int, [vp, C.c_int, sp, C.c_double, vp, C.c_size_t, vp, vp]),
        "cspm_fuse_default_params": (C.c_int, [fup]),
        "cspm_fuse_depth_maps": (C.c_int, [C.c_int, fup, fuv, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, up, up, u8p]),
        "cspm_fuse_begin": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "cspm_fuse_push": (C.c_int, [vp, C.c_int, C.c_int, kp, gp, fp, dp, dp]),
        "cspm_fuse_push_maps": (C.c_int, [vp, dp, dp, u8p, C.c_size_t, C.c_double, C.c_double, C.c_double, dp, dp]),
        "cspm_fuse_view_count": (C.c_int, [vp]),
        "cspm_fuse_run": (C.c_int, [vp, fup, vp, C.c_size_t, up, up, u8p]),
        "cspm_fuse_run_device": (C.c_int, [vp, fup, vp, C.c_size_t, vp, vp, vp]),
        "cspm_fuse_end": (C.c_int, [vp]),
        "cspm_tsdf_default_params": (C.c_int, [tsp]),
        "cspm_tsdf_begin": (C.c_int, [vp, tsp]),
        "cspm_tsdf_clear": (C.c_int, [vp]),
        "cspm_tsdf_integrate": (C.c_int, [vp, C.c_int]),
        "cspm_tsdf_raycast": (C.c_int, [vp, tcp, C.c_int, C.c_int, C.c_double, dp, dp, u8p, C.c_size_t, u8p]),
        "cspm_tsdf_raycast_device": (C.c_int, [vp, tcp, C.c_int, C.c_int, C.c_double, vp, vp, vp, C.c_size_t, vp]),
        "cspm_tsdf_raycast_push": (C.c_int, [vp, tcp, C.c_double]),
        "cspm_tsdf_points": (C.c_int, [vp, vp, C.c_size_t, up]),
        "cspm_tsdf_points_device": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "cspm_tsdf_get_volume": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u8p]),
        "cspm_tsdf_end": (C.c_int, [vp]),
        "cspm_tsdf_mesh": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, up, up]),
        "cspm_tsdf_mesh_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp]),
        "cspm_tsdf_set_volume": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u8p]),
        "cspm_tsdf_mesh_depth_maps": (C.c_int, [C.c_int, tsp, fuv, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, up, up]),
        "cspm_tsdf_depth_maps": (C.c_int, [C.c_int, tsp, fuv, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, up, C.POINTER(C.c_float), C.POINTER(C.c_float), u8p]),
        "cspm_reg_default_params": (C.c_int, [rgpp]),
        "cspm_fuse_register": (C.c_int, [vp, C.c_int, C.c_ulonglong, rgpp, dp, dp, C.c_int, dp, dp, rgip]),
        "cspm_fuse_get_pose": (C.c_int, [vp, C.c_int, dp, dp]),
        "cspm_fuse_set_pose": (C.c_int, [vp, C.c_int, dp, dp]),
        "cspm_register_depth_maps": (C.c_int, [C.c_int, rgpp, fuv, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, dp, dp, rgip]),
        "cspm_carry_default_params": (C.c_int, [cyp]),
        "cspm_carry_relative_pose": (C.c_int, [dp, dp, dp, dp, dp, dp]),
        "cspm_carry_plane_field": (C.c_int, [C.c_int, dp, u8p, kp, C.c_int, C.c_int, C.c_int, kp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, cyp, dp, u8p,
                                             i32p]),
        "cspm_carry_planes": (C.c_int, [vp, vp, kp, kp, dp, dp, cyp, C.c_int]),
        "cspm_rect_default_params": (C.c_int, [rpp]),
        "cspm_rectify_compute": (C.c_int, [rgp, rpp, rcp, kp]),
        "cspm_rectify_host": (C.c_int, [C.c_int, rgp, rcp, C.c_int, u8p, C.c_size_t, u8p, C.c_size_t, dp, u8p]),
        "cspm_set_rectification": (C.c_int, [vp, rgp, rcp]),
        "cspm_get_rect_map": (C.c_int, [vp, C.c_int, dp, u8p]),
        "cspm_set_images_raw": (C.c_int, [vp, u8p, u8p, C.c_size_t]),
        "cspm_set_images_raw_device": (C.c_int, [vp, vp, vp, C.c_size_t]),
    }
    assert sorted(sig) == sorted(SYMBOLS)
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _opt(conv, a):
    """conv(a), or NULL for an optional argument that is not given"""
    return None if a is None else conv(a)


def _dev(a):
    """a device pointer given as an integer; 0 = not requested"""
    return C.c_void_p(a) if a else None


def _check(rc, ctx=None):
    """a failed call raises with the library's message: the context's, or the thread's for an entry that has none"""
    if rc != 0:
        raise CspmError(f"cspm error {rc}: {load_library().cspm_last_error(ctx).decode()}")


def _params(cls, name, what, params, aliases={}):
    """cls as cspm_<name>_default_params fills it, with the given fields replaced; a value becomes its field's C type"""
    p = cls()
    rc = getattr(load_library(), f"cspm_{name}_default_params")(C.byref(p))
    assert rc == 0
    kinds = dict(cls._fields_)
    for k, v in params.items():
        field = aliases.get(k, k)
        if field not in kinds:
            raise TypeError(f"unknown {what} parameter {k!r}")
        setattr(p, field, float(v) if kinds[field] is C.c_double else int(v))
    return p


def _maps(disp, valid=None, maps=(), bgr=None):
    """the host inputs the one-shot entries share, as the library reads them: disp (h, w) f64; valid (h, w) -> 0 / 1 bytes, or None;
    every further f64 map (slopes, confidences) (h, w) or None; bgr (h, w, 3) uint8 or None"""
    d = np.ascontiguousarray(disp, dtype=np.float64)
    assert d.ndim == 2, d.shape
    m = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, dtype=np.uint8)
    assert m is None or m.shape == d.shape, m.shape
    more = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in maps]
    assert all(a is None or a.shape == d.shape for a in more)
    g = None if bgr is None else np.ascontiguousarray(bgr, dtype=np.uint8)
    assert g is None or g.shape == d.shape + (3,), g.shape
    return d, m, more, g


class StereoContext:
    """One cspm_ctx: one stereo pair on one GPU / stream."""

    def __init__(self, device=0):
        self.L = load_library()
        self.p = C.c_void_p()
        rc = self.L.cspm_create(C.byref(self.p), device)
        if rc != 0:
            raise CspmError(f"cspm_create failed ({rc}): {self.L.cspm_last_error(None).decode()}")
        self.w = self.h = 0
        self._rect = None  # (raw_w, raw_h, w, h) of the stored rectification

    def close(self):
        if getattr(self, "p", None) and self.p:
            self.L.cspm_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        _check(rc, self.p)

    # ---- images / cost ----
    def set_images(self, l_bgr, r_bgr):
        l = np.ascontiguousarray(l_bgr, dtype=np.uint8)
        r = np.ascontiguousarray(r_bgr, dtype=np.uint8)
        assert l.ndim == 3 and l.shape[2] == 3 and l.shape == r.shape
        self.h, self.w = l.shape[:2]
        self._chk(self.L.cspm_set_images(self.p, _u8(l), _u8(r), self.w, self.h, self.w * 3))

    def set_images_device(self, d_l_ptr, d_r_ptr, w, h, stride=None):
        self.h, self.w = h, w
        self._chk(self.L.cspm_set_images_device(self.p, C.c_void_p(d_l_ptr), C.c_void_p(d_r_ptr), w, h, stride or w * 3))

    # ---- rectification ----
    def set_rectification(self, rig, rect=None, **params):
        """build and keep both views' sampling maps (cspm_set_rectification).  rig: a Rig (see make_rig) or None to drop the stored
        rectification; rect: a Rectification, or None to derive it from the rig with rectify_compute(rig, **params).  Returns
        (rect, calib): the rectification in use and the cspm_calib of the rectified pair."""
        if rig is None:
            self._chk(self.L.cspm_set_rectification(self.p, None, None))
            self._rect = None
            return None
        calib = None
        if rect is None:
            rect, calib = rectify_compute(rig, **params)
        elif params:
            raise TypeError("give a Rectification or the parameters to derive one, not both")
        self._chk(self.L.cspm_set_rectification(self.p, C.byref(rig), C.byref(rect)))
        self._rect = (rig.raw_w, rig.raw_h, rect.w, rect.h)
        return rect, calib if calib is not None else Calib(rect.f, rect.cx, rect.cy, rect.baseline, 0.0)

    def _raw_dims(self):
        if self._rect is None:
            self._chk(self.L.cspm_set_images_raw(self.p, None, None, 0))  # CSPM_ERR_STATE with the library's message
        return self._rect

    def set_images_raw(self, l_raw, r_raw):
        """a RAW pair of the rig's size, remapped on the device into the level-0 images (cspm_set_images_raw)"""
        l = np.ascontiguousarray(l_raw, dtype=np.uint8)
        r = np.ascontiguousarray(r_raw, dtype=np.uint8)
        rw, rh, w, h = self._raw_dims()
        if l.shape != (rh, rw, 3) or r.shape != (rh, rw, 3):
            raise CspmError(f"cspm error -1: raw images of the rig's size {rw} x {rh} x 3 expected, got {l.shape} and {r.shape}")
        self._chk(self.L.cspm_set_images_raw(self.p, _u8(l), _u8(r), rw * 3))
        self.h, self.w = h, w

    def set_images_raw_device(self, d_l_ptr, d_r_ptr, stride=None):
        rw, rh, w, h = self._raw_dims()
        self._chk(self.L.cspm_set_images_raw_device(self.p, C.c_void_p(d_l_ptr), C.c_void_p(d_r_ptr), stride or rw * 3))
        self.h, self.w = h, w

    def rect_map(self, view):
        """the stored map of one view: (sx, sy) as (h, w) f64 arrays and the valid bytes (h, w) u8 (cspm_get_rect_map)"""
        if self._rect is None:
            self._chk(self.L.cspm_get_rect_map(self.p, int(view), None, None))
        _, _, w, h = self._rect
        xy, valid = np.empty((2, h, w), np.float64), np.empty((h, w), np.uint8)
        self._chk(self.L.cspm_get_rect_map(self.p, int(view), _dp(xy), _u8(valid)))
        return xy[0], xy[1], valid

    def set_stream(self, stream_ptr):
        self._chk(self.L.cspm_set_stream(self.p, C.c_void_p(stream_ptr)))

    def stream_ptr(self):
        """the hipStream_t the context enqueues on, as an integer (torch.cuda.ExternalStream(ptr))"""
        p = C.c_void_p()
        self._chk(self.L.cspm_get_stream(self.p, C.byref(p)))
        return p.value or 0

    def synchronize(self):
        self._chk(self.L.cspm_synchronize(self.p))

    def set_option(self, key, value):
        self._chk(self.L.cspm_set_option(self.p, key, value))

    def get_option(self, key):
        v = C.c_longlong()
        self._chk(self.L.cspm_get_option(self.p, key, C.byref(v)))
        return v.value

    def build_cost_grd(self, max_dis, wnd_size=35, scale_num=0, reg_lambda=0.0, volumes=False, sweep_pairs=None, table_volumes=None):
        """volumes=False: fused on-the-fly GRD cells (default); True: materialised f64 cost volumes.
        sweep_pairs (CSPM_OPT_SWEEP_PAIRS): None = leave the context's setting alone (the library's default, off, or what the
        environment variable CSPM_SWEEP_PAIRS / an earlier set_option chose); False = the raster sweep recomputes its cells from image
        gathers like every other kernel; True = paired-cell volumes for the sweep when they fit the context's budget (an option that
        measured no faster).
        table_volumes (CSPM_OPT_TABLE_VOLUMES): None = leave the context's setting alone (default on; CSPM_TABLE_VOLUMES=0 turns it
        off); True = device-cell volumes (when they fit) from which the row kernels fill their cell tables by LDS-DMA; False = the
        tables are computed."""
        self.set_option(OPT_GRD_VOLUMES, int(volumes))
        if sweep_pairs is not None:
            self.set_option(OPT_SWEEP_PAIRS, int(bool(sweep_pairs)))
        if table_volumes is not None:
            self.set_option(OPT_TABLE_VOLUMES, int(bool(table_volumes)))
        self._chk(self.L.cspm_build_cost_grd(self.p, max_dis, wnd_size, scale_num, reg_lambda))

    def build_cost_cen(self, max_dis, wnd_size=35, scale_num=0, reg_lambda=0.0, volumes=False):
        self.set_option(OPT_GRD_VOLUMES, int(volumes))
        self._chk(self.L.cspm_build_cost_cen(self.p, max_dis, wnd_size, scale_num, reg_lambda))

    def build_cost_cengrd(self, max_dis, wnd_size=35, scale_num=0, reg_lambda=0.0, fused=None):
        """CENGRD: census and GRD blended per cell; OPT_GRD_VOLUMES has no effect on it.
        fused (CSPM_OPT_CENGRD_FUSED): None = leave the context's setting alone (the library's default: materialised f64 volumes);
        True = no volumes, the PatchMatch kernels compute the cells (identical planes and costs); False = volumes."""
        if fused is not None:
            self.set_option(OPT_CENGRD_FUSED, int(bool(fused)))
        self._chk(self.L.cspm_build_cost_cengrd(self.p, max_dis, wnd_size, scale_num, reg_lambda))

    def build_cost_img(self, max_dis, wnd_size=35, scale_num=0, reg_lambda=0.0):
        """GrdPC (scale_num=0) / CSPC: the volume-free plane costs (plane_cost/grd_pc.cc, cspc.cc)"""
        self._chk(self.L.cspm_build_cost_img(self.p, max_dis, wnd_size, scale_num, reg_lambda))

    def begin_cost(self, max_dis, wnd_size=35, scale_num=0, reg_lambda=0.0):
        self._chk(self.L.cspm_begin_cost(self.p, max_dis, wnd_size, scale_num, reg_lambda))

    def upload_cost_slab(self, view, level, d, slab):
        s = np.ascontiguousarray(slab, dtype=np.float64)
        self._chk(self.L.cspm_upload_cost_slab(self.p, view, level, d, _dp(s), s.shape[1]))

    def finish_cost(self):
        self._chk(self.L.cspm_finish_cost(self.p))

    @property
    def levels(self):
        return self.L.cspm_get_levels(self.p)

    def level_dims(self, s):
        w, h, d = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.cspm_get_level_dims(self.p, s, C.byref(w), C.byref(h), C.byref(d)))
        return w.value, h.value, d.value

    def level_image(self, view, s):
        w, h, _ = self.level_dims(s)
        o = np.zeros((h, w, 3), np.uint8)
        self._chk(self.L.cspm_get_level_image(self.p, view, s, _u8(o)))
        return o

    def cost_slab(self, view, s, d):
        w, h, _ = self.level_dims(s)
        o = np.zeros((h, w))
        self._chk(self.L.cspm_get_cost_slab(self.p, view, s, d, _dp(o)))
        return o

    def cost_volume(self, view, s):
        _, _, D = self.level_dims(s)
        return np.stack([self.cost_slab(view, s, d) for d in range(D + 1)])

    def max_cost(self, view, s):
        o = C.c_double()
        self._chk(self.L.cspm_get_max_cost(self.p, view, s, C.byref(o)))
        return o.value

    def scale_weights(self):
        o = np.zeros(MAX_LEVELS)
        self._chk(self.L.cspm_get_scale_weights(self.p, _dp(o)))
        return o[:self.levels].copy()

    # ---- GetPlaneCost ----
    def plane_cost_batch(self, view, xy, norm_param):
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        npar = np.ascontiguousarray(norm_param, dtype=np.float64).reshape(-1, 6)
        assert len(xy) == len(npar)
        out = np.zeros(len(xy))
        self._chk(self.L.cspm_plane_cost_batch(self.p, view, len(xy), xy.ctypes.data_as(C.POINTER(C.c_int)), _dp(npar), _dp(out)))
        return out

    # ---- local stereo ----
    def local_stereo(self, method):
        """cost aggregation (CA_BOX / CA_GF / CA_BF) + cross-scale winner-take-all into both views' plane fields (asynchronous)"""
        self._chk(self.L.cspm_local_stereo(self.p, int(method)))

    # ---- PatchMatch ----
    def params(self, seed=12345, schedule=SCHED_RASTER, rb_rounds=1, rb_neighbours=4, rng_mode=RNG_PER_PIXEL, early_exit=1):
        return PmParams(seed, schedule, rb_rounds, rb_neighbours, rng_mode, early_exit)

    def patchmatch(self, iters=3, **kw):
        p = self.params(**kw)
        self._chk(self.L.cspm_patchmatch(self.p, iters, C.byref(p)))

    def pm_init(self, **kw):
        p = self.params(**kw)
        self._chk(self.L.cspm_pm_init(self.p, C.byref(p)))

    def pm_spatial(self, it, **kw):
        p = self.params(**kw)
        self._chk(self.L.cspm_pm_spatial(self.p, it, C.byref(p)))

    def pm_view(self, it, **kw):
        p = self.params(**kw)
        self._chk(self.L.cspm_pm_view(self.p, it, C.byref(p)))

    def pm_refine(self, it, **kw):
        p = self.params(**kw)
        self._chk(self.L.cspm_pm_refine(self.p, it, C.byref(p)))

    # ---- warm starts ----
    def rescore_planes(self):
        """min_cost of every stored plane under the current cost object (asynchronous); the planes are not changed"""
        self._chk(self.L.cspm_rescore_planes(self.p))

    def patchmatch_warm(self, iters=1, **kw):
        """PatchMatch from the plane field already in the context: re-score (when the field is stale), then iterations 0 .. iters-1"""
        p = self.params(**kw)
        self._chk(self.L.cspm_patchmatch_warm(self.p, iters, C.byref(p)))

    def upsample_planes_from(self, src):
        """this context's plane field from src's, one pyramid level below (src is ((w+1)/2, (h+1)/2)); min_cost stays stale"""
        self._chk(self.L.cspm_upsample_planes(self.p, src.p))

    # ---- candidate fields (include/cspm.h "candidate fields") ----
    def merge_planes_from(self, src):
        """src's plane field offered to both views of this context: a pixel takes src's plane where it costs less (asynchronous)"""
        self._chk(self.L.cspm_merge_planes(self.p, src.p))

    def carry_planes_from(self, src, src_calib, dst_calib, R, t, merge=True, **params):
        """src's plane field carried across the motion X_dst = R X_src + t between the two view-0 cameras into both views of this context
        (cspm_carry_planes; asynchronous).  merge: the carried planes are candidates under merge_planes' rule;
        otherwise they replace the field where there is one.  params: fill."""
        ks, kt, p = calib_struct(src_calib), calib_struct(dst_calib), carry_params(**params)
        R, t = _pose(R, t)
        self._chk(self.L.cspm_carry_planes(self.p, src.p, C.byref(ks), C.byref(kt), _dp(R), _dp(t), C.byref(p), int(bool(merge))))

    def merge_planes(self, view, field, mask=None):
        """field (h, w, 6) offered to one view; mask (h, w), 0 = no candidate, None = every pixel.  Non-finite planes are no candidates."""
        f = np.ascontiguousarray(field, dtype=np.float64)
        assert f.shape == (self.h, self.w, 6), f.shape
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            assert m.shape == (self.h, self.w), m.shape
        self._chk(self.L.cspm_merge_planes_host(self.p, view, _dp(f), _opt(_u8, m)))

    def merge_disparity(self, view, disp, fit=None):
        """a disparity map (h, w) offered as the fronto-parallel planes (0, 0, 1, 0, 0, d); a non-finite d is no candidate.
        fit: a dict of plane-fit parameters ({} = the defaults): the map is offered as the slanted planes fit_planes_host fits to it
        with the view's level-0 image as guide, under the `fitted` mask."""
        if fit is None:
            self.merge_planes(view, disparity_planes(disp))
            return
        guide = self.level_image(view, 0)
        planes, fitted = fit_planes_host(disp, None, guide, max_dis=self.level_dims(0)[2], **dict(fit))
        self.merge_planes(view, planes, fitted)

    def fit_planes(self, merge=False, **params):
        """slanted planes fitted to the stored field's own disparity maps, both views (cspm_fit_planes; asynchronous).  merge=False:
        every pixel's plane is replaced and min_cost is stale (patchmatch_warm re-scores); merge=True: the fitted planes are
        candidates that win only where they cost less.  params: radius, max_diff, min_support, use_guide."""
        p = fit_params(**params)
        self._chk(self.L.cspm_fit_planes(self.p, C.byref(p), int(bool(merge))))

    def segment_planes(self, merge=False, **params):
        """one robustly fitted plane per superpixel of the stored field's own disparity maps, both views (cspm_segment_planes;
        asynchronous).  merge=False: the planes of fitted segments replace the stored ones and min_cost is stale
        (patchmatch_warm re-scores); merge=True: they are candidates that win only where they cost less.  params: step, compactness,
        iters, tau, rounds, min_support."""
        p = seg_params(**params)
        self._chk(self.L.cspm_segment_planes(self.p, C.byref(p), int(bool(merge))))

    def segments(self, view):
        """the (h, w) int32 labels of the last segment_planes call (cspm_get_segments)"""
        labels = np.zeros((self.h, self.w), np.int32)
        self._chk(self.L.cspm_get_segments(self.p, view, _i32(labels)))
        return labels

    def pm_init_keep(self, **kw):
        """the random init as a challenger: a pixel takes its InitRandomPlane plane only where it costs less than the stored one"""
        p = self.params(**kw)
        self._chk(self.L.cspm_pm_init_keep(self.p, C.byref(p)))

    def get_planes(self, view):
        npar = np.zeros((self.h, self.w, 6))
        cost = np.zeros((self.h, self.w))
        self._chk(self.L.cspm_get_planes(self.p, view, _dp(npar), _dp(cost)))
        return npar, cost

    def set_planes(self, view, norm_param, min_cost):
        npar = np.ascontiguousarray(norm_param, dtype=np.float64)
        cost = np.ascontiguousarray(min_cost, dtype=np.float64)
        assert npar.shape == (self.h, self.w, 6) and cost.shape == (self.h, self.w)
        self._chk(self.L.cspm_set_planes(self.p, view, _dp(npar), _dp(cost)))

    def disparity_u8(self, view, dis_scale):
        o = np.zeros((self.h, self.w), np.uint8)
        self._chk(self.L.cspm_get_disparity_u8(self.p, view, dis_scale, _u8(o), self.w))
        return o

    def disparity_f64(self, view):
        o = np.zeros((self.h, self.w))
        self._chk(self.L.cspm_get_disparity_f64(self.p, view, _dp(o)))
        return o

    def disparity_u8_device(self, view, dis_scale, d_out_ptr):
        self._chk(self.L.cspm_disparity_u8_device(self.p, view, dis_scale, C.c_void_p(d_out_ptr)))

    def postprocess(self, dis_scale):
        l = np.zeros((self.h, self.w), np.uint8)
        r = np.zeros((self.h, self.w), np.uint8)
        self._chk(self.L.cspm_postprocess(self.p, dis_scale, _u8(l), _u8(r), self.w))
        return l, r

    def postprocess_device(self, dis_scale, d_l_ptr, d_r_ptr):
        """PlaneToDisp + PostProcessing with device-resident outputs (asynchronous on the context's stream)"""
        self._chk(self.L.cspm_postprocess_device(self.p, dis_scale, C.c_void_p(d_l_ptr), C.c_void_p(d_r_ptr)))

    def postprocess_f64(self, valid=False):
        """sub-pixel PostProcessing: left-right check, fill and weighted median on the unquantised plane
        disparities.  Returns (l, r) f64 maps, or (l, r, l_valid, r_valid) with the u8 left-right consistency masks."""
        l = np.zeros((self.h, self.w))
        r = np.zeros((self.h, self.w))
        if not valid:
            self._chk(self.L.cspm_postprocess_f64(self.p, _dp(l), _dp(r), None, None))
            return l, r
        lv = np.zeros((self.h, self.w), np.uint8)
        rv = np.zeros((self.h, self.w), np.uint8)
        self._chk(self.L.cspm_postprocess_f64(self.p, _dp(l), _dp(r), _u8(lv), _u8(rv)))
        return l, r, lv, rv

    def set_pp_speckle(self, max_size, max_diff=1.0):
        """speckle filter of every post-processing entry: after the left-right check, connected components
        (4-neighbours whose disparities differ by at most max_diff) of at most max_size pixels leave the consistency mask and are
        filled and medianed like any inconsistent pixel.  max_size = 0 (the default) = no filter."""
        self._chk(self.L.cspm_set_pp_speckle(self.p, int(max_size), float(max_diff)))

    def get_pp_speckle(self):
        n, x = C.c_int(), C.c_double()
        self._chk(self.L.cspm_get_pp_speckle(self.p, C.byref(n), C.byref(x)))
        return n.value, x.value

    def set_pp_median(self, r):
        """median filter of every post-processing entry: as the last step, after the weighted median, every
        pixel of both maps becomes the median of its (2r+1)^2 window with the border replicated -- M8 on the 8-bit maps, M64 (NaN taps
        do not vote, the lower median, a tap's own bits) on the f64 maps.  r = 0 (the default) = no filter; at most MEDIAN_MAX_RADIUS."""
        self._chk(self.L.cspm_set_pp_median(self.p, int(r)))

    def get_pp_median(self):
        r = C.c_int()
        self._chk(self.L.cspm_get_pp_median(self.p, C.byref(r)))
        return r.value

    def set_pp_smooth(self, **params):
        """edge-aware global smoothing of the sub-pixel post-processing: as the last step of postprocess_f64 and
        postprocess_f64_device, after the weighted median and the median filter, both maps are smoothed along their level-0 images with
        confidence 1 where the pixel passed the left-right check and fill_conf elsewhere.  params: lam, sigma_color, iterations,
        fill_conf (the rest keep the defaults 100, 20, 3, 0.25); lam=0 (the context's default) = off.  The 8-bit entries are not affected."""
        p = smooth_params(**params)
        self._chk(self.L.cspm_set_pp_smooth(self.p, C.byref(p)))

    def get_pp_smooth(self):
        """the smoothing parameters as a dict (lam, sigma_color, iterations, fill_conf) and on (bool)"""
        p, on = SmoothParams(), C.c_int()
        self._chk(self.L.cspm_get_pp_smooth(self.p, C.byref(p), C.byref(on)))
        return {"lam": p.lambda_, "sigma_color": p.sigma_color, "iterations": p.iterations, "fill_conf": p.fill_conf, "on": bool(on.value)}

    def postprocess_f64_device(self, d_l_ptr, d_r_ptr):
        """the same with device-resident outputs (packed h*w f64 each; asynchronous on the context's stream)"""
        self._chk(self.L.cspm_postprocess_f64_device(self.p, C.c_void_p(d_l_ptr), C.c_void_p(d_r_ptr)))

    # ---- reprojection ----
    def reproject(self, view, calib, source=GEOM_RAW, fit=None, dense=True, cloud=True, cloud_cap=None, **params):
        """metric geometry of one view of the stored plane field (cspm_reproject): calib a Calib or (f, cx, cy, baseline, doffs);
        source GEOM_RAW (the field's own disparities) or GEOM_PP (the sub-pixel post-processed map); fit: None = the field's slopes, a
        dict of plane-fit parameters ({} = the defaults) = slopes fitted to the map; params: z_near, z_far, min_cos, left_frame,
        consistent_only.  Returns a dict: count always; with dense depth (h, w), xyz (3, h, w), normal (3, h, w), keep (h, w) uint8;
        with cloud the Point records of the kept pixels in raster order (at most cloud_cap of them; None = all)."""
        k, g = calib_struct(calib), geom_params(**params)
        f = fit_params(**dict(fit)) if fit is not None else None
        n = self.w * self.h
        out = {}
        if dense:
            out.update(depth=np.zeros((self.h, self.w)), xyz=np.zeros((3, self.h, self.w)), normal=np.zeros((3, self.h, self.w)),
                       keep=np.zeros((self.h, self.w), np.uint8))
        cap = n if cloud_cap is None else int(cloud_cap)
        pts = np.zeros(cap, Point) if cloud else None
        count = C.c_uint(0)
        self._chk(self.L.cspm_reproject(self.p, int(view), int(source), C.byref(k), C.byref(g), _opt(C.byref, f), _opt(_dp, out.get("depth")),
                                        _opt(_dp, out.get("xyz")), _opt(_dp, out.get("normal")), _opt(_u8, out.get("keep")), _opt(_vp, pts),
                                        cap if cloud else 0, C.byref(count)))
        out["count"] = count.value
        if cloud:
            out["cloud"] = pts[:min(count.value, cap)]
        return out

    def reproject_device(self, view, calib, source=GEOM_RAW, fit=None, d_depth=0, d_xyz=0, d_normal=0, d_keep=0, d_cloud=0, cloud_cap=0, d_count=0,
                         **params):
        """the same with device pointers (integers; 0 = not requested) for every output and a device unsigned int for the count;
        asynchronous on the context's stream (cspm_reproject_device)"""
        k, g = calib_struct(calib), geom_params(**params)
        f = fit_params(**dict(fit)) if fit is not None else None
        self._chk(self.L.cspm_reproject_device(self.p, int(view), int(source), C.byref(k), C.byref(g), _opt(C.byref, f), _dev(d_depth), _dev(d_xyz),
                                               _dev(d_normal), _dev(d_keep), _dev(d_cloud), int(cloud_cap), _dev(d_count)))

    # ---- triangle meshes ----
    def mesh(self, view, calib, source=GEOM_RAW, fit=None, max_diff=1.0, all_vertices=0, vertices=True, faces=True, quad=True, vertex_cap=None,
             face_cap=None, **params):
        """a triangle mesh of one view of the stored plane field (cspm_mesh): calib, source, fit and params (z_near, z_far, min_cos,
        left_frame, consistent_only) as for reproject; max_diff and all_vertices are the cspm_mesh_params.  Returns a dict: n_vertices and
        n_faces always; with vertices the Point records (at most vertex_cap of them; None = all), with faces the Face records (at most
        face_cap), with quad the (h, w) uint8 quad bytes.  The mesh is complete only when both counts fit their capacities."""
        k, g, m = calib_struct(calib), geom_params(**params), mesh_params(max_diff=max_diff, all_vertices=all_vertices)
        f = fit_params(**dict(fit)) if fit is not None else None
        vcap = self.w * self.h if vertex_cap is None else int(vertex_cap)
        fcap = 2 * (self.w - 1) * (self.h - 1) if face_cap is None else int(face_cap)
        pts = np.zeros(vcap, Point) if vertices else None
        tri = np.zeros(fcap, Face) if faces else None
        q = np.zeros((self.h, self.w), np.uint8) if quad else None
        nv, nf = C.c_uint(0), C.c_uint(0)
        self._chk(self.L.cspm_mesh(self.p, int(view), int(source), C.byref(k), C.byref(g), _opt(C.byref, f), C.byref(m), _opt(_vp, pts),
                                   vcap if vertices else 0, _opt(_vp, tri), fcap if faces else 0, _opt(_u8, q), C.byref(nv), C.byref(nf)))
        out = {"n_vertices": nv.value, "n_faces": nf.value}
        if vertices:
            out["vertices"] = pts[:min(nv.value, vcap)]
        if faces:
            out["faces"] = tri[:min(nf.value, fcap)]
        if quad:
            out["quad"] = q
        return out

    def mesh_device(self, view, calib, source=GEOM_RAW, fit=None, max_diff=1.0, all_vertices=0, d_vertices=0, vertex_cap=0, d_faces=0, face_cap=0,
                    d_quad=0, d_n_vertices=0, d_n_faces=0, **params):
        """the same with device pointers (integers; 0 = not requested) for every output and device unsigned ints for the two counts;
        asynchronous on the context's stream (cspm_mesh_device)"""
        k, g, m = calib_struct(calib), geom_params(**params), mesh_params(max_diff=max_diff, all_vertices=all_vertices)
        f = fit_params(**dict(fit)) if fit is not None else None
        self._chk(self.L.cspm_mesh_device(self.p, int(view), int(source), C.byref(k), C.byref(g), _opt(C.byref, f), C.byref(m), _dev(d_vertices),
                                          int(vertex_cap), _dev(d_faces), int(face_cap), _dev(d_quad), _dev(d_n_vertices), _dev(d_n_faces)))

    # ---- depth-map fusion ----
    def fuse_begin(self, w, h, max_views):
        """slots for max_views fusion views of w x h, kept until fuse_end whatever happens to the images (cspm_fuse_begin)"""
        self._chk(self.L.cspm_fuse_begin(self.p, int(w), int(h), int(max_views)))
        self._fuse = (int(w), int(h))

    def fuse_push(self, view, calib, R, t, source=GEOM_RAW, fit=None, **params):
        """appends one view of the stored plane field (cspm_fuse_push): view, calib, source, fit and params as for reproject; R (3, 3)
        and t (3,) the camera -> world pose of the pair's view-0 rectified camera"""
        k, g = calib_struct(calib), geom_params(**params)
        f = fit_params(**dict(fit)) if fit is not None else None
        R, t = _pose(R, t)
        self._chk(self.L.cspm_fuse_push(self.p, int(view), int(source), C.byref(k), C.byref(g), _opt(C.byref, f), _dp(R), _dp(t)))

    def fuse_push_maps(self, depth, f, cx, cy, R, t, normal=None, bgr=None):
        """appends one view from host maps (cspm_fuse_push_maps): depth (h, w) f64, normal (3, h, w) f64 or None, bgr (h, w, 3) uint8 or None"""
        w, h = self._fuse
        d, n, img = _fuse_maps(depth, normal, bgr, w, h)
        R, t = _pose(R, t)
        self._chk(self.L.cspm_fuse_push_maps(self.p, _dp(d), _opt(_dp, n), _opt(_u8, img), 3 * w, float(f), float(cx), float(cy), _dp(R), _dp(t)))

    def fuse_view_count(self):
        return self.L.cspm_fuse_view_count(self.p)

    def fuse_run(self, cloud=True, cloud_cap=None, state=True, out=None, **params):
        """F over the views pushed so far (cspm_fuse_run): params max_reproj, max_rel_depth, min_cos, min_views, suppress.  Returns a
        dict: count, view_counts (K,), with cloud the Point records in (view, raster) order (at most cloud_cap; None = all), with state
        the S bytes (K, h, w).  out: a dict with a preallocated cloud_buffer to write into (tests poison it)."""
        w, h = self._fuse
        K = self.fuse_view_count()
        p = fuse_params(**params)
        cap = max(K, 0) * w * h if cloud_cap is None else int(cloud_cap)
        pts = None
        if cloud:
            pts = (out or {}).get("cloud_buffer")
            if pts is None:
                pts = np.zeros(cap, Point)
        S = np.zeros((max(K, 0), h, w), np.uint8) if state else None
        vc = np.zeros(max(K, 1), np.uint32)
        cnt = C.c_uint(0)
        self._chk(self.L.cspm_fuse_run(self.p, C.byref(p), _opt(_vp, pts), cap if cloud else 0, C.byref(cnt), vc.ctypes.data_as(C.POINTER(C.c_uint)),
                                       _opt(_u8, S)))
        res = dict(count=cnt.value, view_counts=vc[:K])
        if cloud:
            res["cloud"] = pts[:min(cnt.value, cap)]
        if state:
            res["state"] = S
        return res

    def fuse_run_device(self, d_cloud=0, cloud_cap=0, d_count=0, d_view_counts=0, d_state=0, **params):
        """the same with device pointers (integers; 0 = not requested); asynchronous on the context's stream (cspm_fuse_run_device)"""
        p = fuse_params(**params)
        self._chk(self.L.cspm_fuse_run_device(self.p, C.byref(p), _dev(d_cloud), int(cloud_cap), _dev(d_count), _dev(d_view_counts), _dev(d_state)))

    def fuse_end(self):
        self._chk(self.L.cspm_fuse_end(self.p))

    # ---- depth-view registration ----
    def fuse_register(self, src, targets, R0=None, t0=None, apply=False, out=None, **params):
        """view `src` registered against the views of `targets` (a bit mask or a sequence of slots) by projective point-to-plane
        Gauss-Newton (cspm_fuse_register).  R0, t0: the start pose (None = the slot's own); apply: the slot takes the result.  params:
        iters, stride, max_dist, huber, min_cos, min_pairs, pivot_rel.  Returns dict(R (3, 3), t (3,), iters (REG_ITER records)).
        out: a dict with preallocated R, t, iters to write into (tests poison them)."""
        p = reg_params(**params)
        R, t, it = _reg_outputs(p, out)
        R0 = None if R0 is None else np.ascontiguousarray(R0, dtype=np.float64).reshape(9)
        t0 = None if t0 is None else np.ascontiguousarray(t0, dtype=np.float64).reshape(3)
        self._chk(self.L.cspm_fuse_register(self.p, int(src), _mask(targets), C.byref(p), _opt(_dp, R0), _opt(_dp, t0), int(bool(apply)), _dp(R), _dp(t),
                                            it.ctypes.data_as(C.POINTER(RegIter))))
        return dict(R=R.reshape(3, 3), t=t, iters=it[:p.iters])

    def fuse_get_pose(self, slot):
        """-> (R (3, 3), t (3,)): the camera -> world pose of a fusion view (cspm_fuse_get_pose)"""
        R, t = np.zeros(9), np.zeros(3)
        self._chk(self.L.cspm_fuse_get_pose(self.p, int(slot), _dp(R), _dp(t)))
        return R.reshape(3, 3), t

    def fuse_set_pose(self, slot, R, t):
        R, t = _pose(R, t)
        self._chk(self.L.cspm_fuse_set_pose(self.p, int(slot), _dp(R), _dp(t)))

    # ---- TSDF fusion ----
    def tsdf_begin(self, origin, voxel, dims, **params):
        """a cleared volume of dims = (nx, ny, nz) voxels of edge `voxel` with the world corner `origin`, kept until tsdf_end
        (cspm_tsdf_begin); params: trunc, max_weight, min_cos, step_rel"""
        p = tsdf_params(origin, voxel, dims, **params)
        self._chk(self.L.cspm_tsdf_begin(self.p, C.byref(p)))
        self._tsdf = (p.nx, p.ny, p.nz)

    def tsdf_clear(self):
        self._chk(self.L.cspm_tsdf_clear(self.p))

    def tsdf_integrate(self, slot):
        """one fusion view into the volume (cspm_tsdf_integrate); asynchronous on the context's stream"""
        self._chk(self.L.cspm_tsdf_integrate(self.p, int(slot)))

    def tsdf_raycast(self, camera, w, h, z_near=0.0, outputs=("depth", "normal", "bgr", "status"), out=None):
        """the volume seen from `camera` (a dict with f, cx, cy, R, t) as w x h maps (cspm_tsdf_raycast): a dict of the requested outputs
        depth (h, w) f64, normal (3, h, w) f64, bgr (h, w, 3) uint8, status (h, w) uint8.  out: preallocated arrays to write into."""
        k = tsdf_camera(camera)
        res = _ray_outputs(int(h), int(w), outputs, out)
        self._chk(self.L.cspm_tsdf_raycast(self.p, C.byref(k), int(w), int(h), float(z_near), _opt(_dp, res.get("depth")), _opt(_dp, res.get("normal")),
                                           _opt(_u8, res.get("bgr")), 3 * int(w), _opt(_u8, res.get("status"))))
        return res

    def tsdf_raycast_device(self, camera, w, h, z_near=0.0, d_depth=0, d_normal=0, d_bgr=0, stride=0, d_status=0):
        """the same with device pointers (integers; 0 = not requested); asynchronous (cspm_tsdf_raycast_device)"""
        k = tsdf_camera(camera)
        self._chk(self.L.cspm_tsdf_raycast_device(self.p, C.byref(k), int(w), int(h), float(z_near), _dev(d_depth), _dev(d_normal), _dev(d_bgr), int(stride),
                                                  _dev(d_status)))

    def tsdf_raycast_push(self, camera, z_near=0.0):
        """a raycast at the fusion views' size into the next fusion slot (cspm_tsdf_raycast_push); asynchronous"""
        k = tsdf_camera(camera)
        self._chk(self.L.cspm_tsdf_raycast_push(self.p, C.byref(k), float(z_near)))

    def tsdf_points(self, cloud=True, cloud_cap=None, out=None):
        """the surface points (cspm_tsdf_points): dict(count, cloud: the Point records in (voxel, axis) order, at most cloud_cap; None = all).
        out: a dict with a preallocated cloud_buffer to write into (tests poison it)."""
        nx, ny, nz = self._tsdf
        cap = 3 * nx * ny * nz if cloud_cap is None else int(cloud_cap)
        pts = None
        if cloud:
            pts = (out or {}).get("cloud_buffer")
            if pts is None:
                pts = np.zeros(cap, Point)
        cnt = C.c_uint(0)
        self._chk(self.L.cspm_tsdf_points(self.p, _opt(_vp, pts), cap if cloud else 0, C.byref(cnt)))
        res = dict(count=cnt.value)
        if cloud:
            res["cloud"] = pts[:min(cnt.value, cap)]
        return res

    def tsdf_points_device(self, d_cloud=0, cloud_cap=0, d_count=0):
        self._chk(self.L.cspm_tsdf_points_device(self.p, _dev(d_cloud), int(cloud_cap), _dev(d_count)))

    def tsdf_volume(self):
        """-> dict(D, W: (nz, ny, nx) float32, C: (nz, ny, nx, 4) uint8 = b, g, r, has) (cspm_tsdf_get_volume)"""
        nx, ny, nz = self._tsdf
        D, W, Cc = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 4), np.uint8)
        fp = C.POINTER(C.c_float)
        self._chk(self.L.cspm_tsdf_get_volume(self.p, D.ctypes.data_as(fp), W.ctypes.data_as(fp), _u8(Cc)))
        return dict(D=D, W=W, C=Cc)

    def tsdf_set_volume(self, D=None, W=None, colour=None):
        """uploads the given planes of the volume as their bytes stand (cspm_tsdf_set_volume): D, W nx*ny*nz float32, colour (.., 4) uint8 =
        b, g, r, has; None leaves a plane as it is"""
        nx, ny, nz = self._tsdf
        nvox = nx * ny * nz
        planes = []
        for a, dtype, size in ((D, np.float32, nvox), (W, np.float32, nvox), (colour, np.uint8, 4 * nvox)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype)
                assert a.size == size, "a plane of the volume has nx*ny*nz elements"
            planes.append(a)
        fp = C.POINTER(C.c_float)
        self._chk(self.L.cspm_tsdf_set_volume(self.p, planes[0].ctypes.data_as(fp) if planes[0] is not None else None,
                                              planes[1].ctypes.data_as(fp) if planes[1] is not None else None, _opt(_u8, planes[2])))

    def tsdf_mesh(self, vertices=True, faces=True, vertex_cap=None, face_cap=None, out=None):
        """the triangle mesh of the volume (cspm_tsdf_mesh): dict(n_vertices, n_faces, vertices: the Point records of
        tsdf_points, at most vertex_cap; faces: the Face records, at most face_cap; None = all).  The mesh is complete only when both
        counts fit.  out: a dict with preallocated vertex_buffer / face_buffer to write into (tests poison them)."""
        nx, ny, nz = self._tsdf
        vcap, fcap = _tsdf_mesh_caps(nx, ny, nz, vertex_cap, face_cap)
        pts, tri = _tsdf_mesh_buffers(vertices, faces, vcap, fcap, out)
        nv, nf = C.c_uint(0), C.c_uint(0)
        self._chk(self.L.cspm_tsdf_mesh(self.p, _opt(_vp, pts), vcap if vertices else 0, _opt(_vp, tri), fcap if faces else 0, C.byref(nv), C.byref(nf)))
        return _tsdf_mesh_result(nv.value, nf.value, pts, tri, vcap, fcap)

    def tsdf_mesh_device(self, d_vertices=0, vertex_cap=0, d_faces=0, face_cap=0, d_n_vertices=0, d_n_faces=0):
        """the same with device pointers (integers; 0 = not requested); asynchronous on the context's stream (cspm_tsdf_mesh_device)"""
        self._chk(self.L.cspm_tsdf_mesh_device(self.p, _dev(d_vertices), int(vertex_cap), _dev(d_faces), int(face_cap), _dev(d_n_vertices),
                                               _dev(d_n_faces)))

    def tsdf_end(self):
        self._chk(self.L.cspm_tsdf_end(self.p))

    # ---- view synthesis ----
    def synthesize(self, t, source=GEOM_RAW, outputs=("bgr", "disp", "mask"), out=None, **params):
        """the scene from the camera at fraction t of the baseline (0 = view 0, 1 = view 1), rendered from the stored plane field and the
        level-0 images (cspm_synthesize): source GEOM_RAW or GEOM_PP; params: views, max_stretch, merge_diff, fill.  outputs: which of
        bgr (h, w, 3) uint8, disp (h, w) f64 (NaN in holes), mask (h, w) uint8 (0 hole, 1 / 2 one view, 3 both, 4 filled) to compute.
        out: a dict of preallocated arrays to write into (bgr may have padded rows).  Returns a dict of the requested arrays."""
        p = synth_params(**params)
        res = _synth_outputs(self.h, self.w, outputs, out)
        b = res.get("bgr")
        self._chk(self.L.cspm_synthesize(self.p, int(source), C.byref(p), float(t), _opt(_u8, b), b.strides[0] if b is not None else 0,
                                         _opt(_dp, res.get("disp")), _opt(_u8, res.get("mask"))))
        return res

    def synthesize_device(self, t, source=GEOM_RAW, d_bgr=0, out_stride=0, d_disp=0, d_mask=0, **params):
        """the same with device pointers (integers; 0 = not requested): d_bgr rows of out_stride bytes (0 = 3 * w), d_disp h*w f64, d_mask
        h*w bytes; asynchronous on the context's stream (cspm_synthesize_device)"""
        p = synth_params(**params)
        self._chk(self.L.cspm_synthesize_device(self.p, int(source), C.byref(p), float(t), _dev(d_bgr), int(out_stride) or 3 * self.w, _dev(d_disp),
                                                _dev(d_mask)))

    # ---- measurement ----
    def enable_timing(self, on=True):
        self._chk(self.L.cspm_enable_timing(self.p, int(on)))

    def reset_timing(self):
        self._chk(self.L.cspm_reset_timing(self.p))

    def timing(self):
        out = {}
        for k, name in enumerate(K_NAMES):
            n, ms, ev = C.c_longlong(), C.c_double(), C.c_longlong()
            self._chk(self.L.cspm_get_timing(self.p, k, C.byref(n), C.byref(ms), C.byref(ev)))
            out[name] = {"launches": n.value, "ms": ms.value, "evals": ev.value}
        return out

    def taps_per_view_pass(self):
        return self.L.cspm_taps_per_view_pass(self.p)

    def row_engine_taps_per_view_pass(self):
        return self.L.cspm_row_engine_taps_per_view_pass(self.p)


def aggregate_cv_host(device, method, guide, vol):
    """CAMethod::aggreCV on host arrays: guide (h, w, 3) f64 used as given, vol (n, h, w) f64; returns the volume with slices 1..
    filtered (slice 0 as it was)"""
    L = load_library()
    g = np.ascontiguousarray(guide, dtype=np.float64)
    v = np.array(vol, dtype=np.float64, order="C", copy=True)
    assert g.ndim == 3 and g.shape[2] == 3 and v.ndim == 3 and v.shape[1:] == g.shape[:2]
    _check(L.cspm_aggregate_cv_host(device, int(method), _dp(g), g.shape[1], g.shape[0], v.shape[0], _dp(v)))
    return v


def filter_speckles(device, disp, valid, max_size, max_diff):
    """the speckle filter alone on a host map: disp (h, w) f64, valid (h, w) or None (every pixel).  Returns
    (valid_out u8, sizes int32): the mask without the components of at most max_size pixels, and every pixel's component size
    (0 outside the mask)."""
    d, m, _, _ = _maps(disp, valid)
    out = np.zeros(d.shape, np.uint8)
    sizes = np.zeros(d.shape, np.int32)
    _check(load_library().cspm_filter_speckles_host(device, _dp(d), _opt(_u8, m), d.shape[1], d.shape[0], int(max_size), float(max_diff), _u8(out),
                                                    _i32(sizes)))
    return out, sizes


def fit_params(**params):
    """struct cspm_fit_params: cspm_fit_default_params with the given fields replaced"""
    return _params(FitParams, "fit", "plane-fit", params)


def fit_planes_host(disp, valid=None, guide=None, max_dis=0, device=0, **params):
    """slanted planes fitted to a host disparity map (cspm_fit_planes_host): disp (h, w) f64, valid (h, w) or
    None (every pixel), guide (h, w, 3) uint8 BGR or None (no guide weights).  Returns ((h, w, 6) planes in the layout of get_planes,
    (h, w) uint8 fitted); a pixel that is masked out or not finite gets six NaNs and fitted = 0."""
    d, m, _, g = _maps(disp, valid, bgr=guide)
    h, w = d.shape
    p = fit_params(**params)
    planes = np.zeros((h, w, 6))
    fitted = np.zeros((h, w), np.uint8)
    _check(load_library().cspm_fit_planes_host(device, _dp(d), _opt(_u8, m), _opt(_u8, g), w * 3, w, h, int(max_dis), C.byref(p), _dp(planes),
                                               _u8(fitted)))
    return planes, fitted


def seg_params(**params):
    """struct cspm_seg_params: cspm_seg_default_params with the given fields replaced"""
    return _params(SegParams, "seg", "segment-plane", params)


def segment_count(w, h, step):
    """K = ceil(w / step) * ceil(h / step) (cspm_segment_count)"""
    k = load_library().cspm_segment_count(int(w), int(h), int(step))
    if k < 0:
        raise CspmError(f"cspm error {k}: bad size or step")
    return k


def segment_host(bgr, device=0, **params):
    """the superpixel segmentation of a host image (cspm_segment_host): bgr (h, w, 3) uint8.  Returns
    (labels (h, w) int32, centres (K, 5) int32 in 1/16 units (cx, cy, cb, cg, cr), counts (K,) int32).  params: step, compactness, iters."""
    L = load_library()
    g = np.ascontiguousarray(bgr, dtype=np.uint8)
    assert g.ndim == 3 and g.shape[2] == 3, g.shape
    h, w = g.shape[:2]
    p = seg_params(**params)
    K = segment_count(w, h, p.step)
    labels = np.zeros((h, w), np.int32)
    centres = np.zeros((K, 5), np.int32)
    counts = np.zeros(K, np.int32)
    _check(L.cspm_segment_host(device, _u8(g), w * 3, w, h, C.byref(p), _i32(labels), _i32(centres), _i32(counts)))
    return labels, centres, counts


def segment_planes_host(disp, valid, labels, max_dis=0, device=0, **params):
    """one robust plane per segment of a host disparity map (cspm_segment_planes_host): disp (h, w) f64, valid
    (h, w) or None (every pixel), labels (h, w) int32 for the grid of `step`.  Returns (seg_planes (K, 3) f64 (a, b, c), inliers (K,)
    int32, planes (h, w, 6) in the layout of get_planes, fitted (h, w) uint8); an unfitted segment has NaNs, 0 inliers, and its pixels six
    NaNs and fitted = 0.  params: step, tau, rounds, min_support."""
    d, m, _, _ = _maps(disp, valid)
    h, w = d.shape
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    assert lab.shape == d.shape, lab.shape
    p = seg_params(**params)
    K = segment_count(w, h, p.step)
    seg = np.zeros((K, 3))
    inl = np.zeros(K, np.int32)
    planes = np.zeros((h, w, 6))
    fitted = np.zeros((h, w), np.uint8)
    _check(load_library().cspm_segment_planes_host(device, _dp(d), _opt(_u8, m), _i32(lab), w, h, int(max_dis), C.byref(p), _dp(seg), _i32(inl),
                                                   _dp(planes), _u8(fitted)))
    return seg, inl, planes, fitted


def calib_struct(calib):
    """a Calib from a Calib or a sequence (f, cx, cy, baseline, doffs)"""
    if isinstance(calib, Calib):
        return calib
    f, cx, cy, baseline, doffs = (float(t) for t in calib)
    return Calib(f, cx, cy, baseline, doffs)


def geom_params(**params):
    """struct cspm_geom_params: cspm_geom_default_params with the given fields replaced"""
    return _params(GeomParams, "geom", "reprojection", params)


def reproject_host(calib, view, disp, valid=None, slope_a=None, slope_b=None, bgr=None, dense=("depth", "xyz", "normal", "keep"), cloud=True,
                   cloud_cap=None, count=True, device=0, out=None, **params):
    """G alone on host maps (cspm_reproject_host): disp (h, w) f64, valid (h, w) or None, slopes (h, w) f64 or None,
    bgr (h, w, 3) uint8 or None.  dense: the dense outputs to compute (normal is dropped without slopes); cloud / cloud_cap / count as
    for StereoContext.reproject.  out: a dict of preallocated arrays to write into instead of fresh ones (tests poison them).
    Returns a dict with the requested arrays, `count` and `cloud`."""
    d, m, (a, b), img = _maps(disp, valid, (slope_a, slope_b), bgr)
    h, w = d.shape
    k, g = calib_struct(calib), geom_params(**params)
    res = dict(out or {})
    shapes = {"depth": (h, w), "xyz": (3, h, w), "normal": (3, h, w), "keep": (h, w)}
    for name in dense:
        if name == "normal" and a is None and (out is None or "normal" not in out):
            continue
        if name not in res:
            res[name] = np.zeros(shapes[name], np.uint8 if name == "keep" else np.float64)
    cap = w * h if cloud_cap is None else int(cloud_cap)
    pts = None
    if cloud:
        pts = res.get("cloud_buffer")
        if pts is None:
            pts = np.zeros(cap, Point)
    cnt = C.c_uint(0)
    ptr = lambda name, f: f(res[name]) if name in res and name in dense else None
    _check(load_library().cspm_reproject_host(device, C.byref(k), C.byref(g), int(view), _dp(d), _opt(_u8, m), _opt(_dp, a), _opt(_dp, b), _opt(_u8, img),
                                              w * 3, w, h, ptr("depth", _dp), ptr("xyz", _dp), ptr("normal", _dp), ptr("keep", _u8), _opt(_vp, pts),
                                              cap if pts is not None else 0, C.byref(cnt) if count else None))
    if count:
        res["count"] = cnt.value
    if pts is not None:
        res["cloud"] = pts[:min(cnt.value, cap)] if count else pts
    return res


def mesh_params(**params):
    """struct cspm_mesh_params: cspm_mesh_default_params with the given fields replaced"""
    return _params(MeshParams, "mesh", "mesh", params)


def mesh_host(calib, view, disp, valid=None, slope_a=None, slope_b=None, bgr=None, max_diff=1.0, all_vertices=0, vertices=True, faces=True, quad=True,
              vertex_cap=None, face_cap=None, counts=True, device=0, out=None, **params):
    """M alone on host maps (cspm_mesh_host): the inputs as for reproject_host; max_diff and all_vertices are the
    cspm_mesh_params, params the reprojection parameters.  out: a dict of preallocated arrays ("vertex_buffer", "face_buffer", "quad")
    to write into instead of fresh ones (tests poison them).  Returns a dict with n_vertices, n_faces (with counts) and the requested
    vertices, faces and quad."""
    d, vm, (a, b), img = _maps(disp, valid, (slope_a, slope_b), bgr)
    h, w = d.shape
    k, g, m = calib_struct(calib), geom_params(**params), mesh_params(max_diff=max_diff, all_vertices=all_vertices)
    res = dict(out or {})
    vcap = w * h if vertex_cap is None else int(vertex_cap)
    fcap = 2 * (w - 1) * (h - 1) if face_cap is None else int(face_cap)
    pts = tri = q = None
    if vertices:
        pts = res.get("vertex_buffer")
        if pts is None:
            pts = np.zeros(vcap, Point)
    if faces:
        tri = res.get("face_buffer")
        if tri is None:
            tri = np.zeros(fcap, Face)
    if quad:
        q = res.get("quad")
        if q is None:
            q = res["quad"] = np.zeros((h, w), np.uint8)
    nv, nf = C.c_uint(0), C.c_uint(0)
    _check(load_library().cspm_mesh_host(device, C.byref(k), C.byref(g), C.byref(m), int(view), _dp(d), _opt(_u8, vm), _opt(_dp, a), _opt(_dp, b),
                                         _opt(_u8, img), w * 3, w, h, _opt(_vp, pts), vcap if pts is not None else 0, _opt(_vp, tri),
                                         fcap if tri is not None else 0, _opt(_u8, q), C.byref(nv) if counts else None, C.byref(nf) if counts else None))
    if counts:
        res["n_vertices"], res["n_faces"] = nv.value, nf.value
    if pts is not None:
        res["vertices"] = pts[:min(nv.value, vcap)] if counts else pts
    if tri is not None:
        res["faces"] = tri[:min(nf.value, fcap)] if counts else tri
    return res


def make_rig(cam0, cam1, R, T, raw_w, raw_h):
    """a Rig from two cameras (Camera, or a sequence fx, fy, cx, cy[, skew, k1, k2, p1, p2, k3]), R (3 x 3, X1 = R X0 + T), T and the raw size"""
    rig = Rig()
    for v, cam in enumerate((cam0, cam1)):
        if not isinstance(cam, Camera):
            vals = [float(x) for x in cam]
            cam = Camera(*(vals + [0.0] * (10 - len(vals))))
        rig.cam[v] = cam
    rig.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
    rig.T[:] = [float(x) for x in np.asarray(T, np.float64).reshape(3)]
    rig.raw_w, rig.raw_h = int(raw_w), int(raw_h)
    return rig


def rect_params(**params):
    """a RectParams from keywords f, cx, cy, w, h over the library's defaults (everything automatic)"""
    return _params(RectParams, "rect", "rectification", params)


def rectify_compute(rig, **params):
    """the rectifying rotations, the common projection and the cspm_calib of the rectified pair (cspm_rectify_compute): pure host logic,
    answers without a GPU.  Returns (Rectification, Calib)."""
    p, rect, calib = rect_params(**params), Rectification(), Calib()
    _check(load_library().cspm_rectify_compute(C.byref(rig), C.byref(p), C.byref(rect), C.byref(calib)))
    return rect, calib


def rectify_host(rig, rect, view, raw=None, outputs=("bgr", "map", "valid"), raw_stride=None, out_stride=None, device=0):
    """R alone on host memory (cspm_rectify_host): raw (raw_h, raw_w, 3) u8, or a 2-D u8 array of padded rows with
    raw_stride = its row length; returns a dict with the requested outputs: bgr (h, w, 3) u8, map (2, h, w) f64 (sx, sy), valid (h, w) u8.
    out_stride: the image is written into rows of that many bytes, returned as bgr_rows (h, out_stride) with the padding at 0xA5."""
    L = load_library()
    w, h = rect.w, rect.h
    res = {}
    if "bgr" in outputs:
        res["bgr_rows"] = np.full((h, out_stride if out_stride is not None else w * 3), 0xA5, np.uint8)
    if "map" in outputs:
        res["map"] = np.empty((2, h, w), np.float64)
    if "valid" in outputs:
        res["valid"] = np.empty((h, w), np.uint8)
    r = np.ascontiguousarray(raw, dtype=np.uint8) if raw is not None else None
    stride = raw_stride if raw_stride is not None else rig.raw_w * 3
    _check(L.cspm_rectify_host(device, C.byref(rig), C.byref(rect), int(view), _opt(_u8, r), stride, _opt(_u8, res.get("bgr_rows")),
                               out_stride if out_stride is not None else w * 3, _opt(_dp, res.get("map")), _opt(_u8, res.get("valid"))))
    if "bgr_rows" in res:
        res["bgr"] = np.ascontiguousarray(res["bgr_rows"][:, :w * 3]).reshape(h, w, 3)
    return res


def fuse_params(**params):
    """struct cspm_fuse_params: cspm_fuse_default_params with the given fields replaced"""
    return _params(FuseParams, "fuse", "fusion", params)


def _pose(R, t):
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    return R, t


def _fuse_maps(depth, normal, bgr, w, h):
    d = np.ascontiguousarray(depth, dtype=np.float64)
    assert d.shape == (h, w), d.shape
    n = None if normal is None else np.ascontiguousarray(normal, dtype=np.float64)
    assert n is None or n.shape == (3, h, w), n.shape
    img = None if bgr is None else np.ascontiguousarray(bgr, dtype=np.uint8)
    assert img is None or img.shape == (h, w, 3), img.shape
    return d, n, img


def fuse_depth_maps(views, w, h, cloud=True, cloud_cap=None, state=True, device=0, out=None, **params):
    """F alone on host maps (cspm_fuse_depth_maps).  views: a sequence of dicts with depth (h, w) f64, f, cx, cy,
    R (3, 3), t (3,) camera -> world, and optionally normal (3, h, w) f64 and bgr (h, w, 3) uint8.  params: max_reproj, max_rel_depth,
    min_cos, min_views, suppress.  Returns what StereoContext.fuse_run returns."""
    K = len(views)
    p = fuse_params(**params)
    arr = (FuseView * max(K, 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, img = _fuse_maps(v["depth"], v.get("normal"), v.get("bgr"), w, h)
        R, t = _pose(v["R"], v["t"])
        keep.append((d, n, img))
        arr[k] = FuseView(_dp(d), _opt(_dp, n), _opt(_u8, img), 3 * w, float(v["f"]), float(v["cx"]), float(v["cy"]), (C.c_double * 9)(*R), (C.c_double * 3)(*t))
    cap = K * w * h if cloud_cap is None else int(cloud_cap)
    pts = None
    if cloud:
        pts = (out or {}).get("cloud_buffer")
        if pts is None:
            pts = np.zeros(cap, Point)
    S = (out or {}).get("state")
    if S is None and state:
        S = np.zeros((K, h, w), np.uint8)
    vc = (out or {}).get("view_counts")
    if vc is None:
        vc = np.zeros(max(K, 1), np.uint32)
    cnt = C.c_uint(0)
    _check(load_library().cspm_fuse_depth_maps(device, C.byref(p), arr, K, w, h, _opt(_vp, pts), cap if cloud else 0, C.byref(cnt),
                                               vc.ctypes.data_as(C.POINTER(C.c_uint)), _opt(_u8, S)))
    del keep
    res = dict(count=cnt.value, view_counts=vc[:K])
    if cloud:
        res["cloud"] = pts[:min(cnt.value, cap)]
    if S is not None:
        res["state"] = S
    return res


def tsdf_params(origin, voxel, dims, **params):
    """struct cspm_tsdf_params: cspm_tsdf_default_params with the volume and the given fields (trunc, max_weight, min_cos, step_rel)"""
    p = _params(TsdfParams, "tsdf", "TSDF", params)
    p.origin = (C.c_double * 3)(*(float(o) for o in origin))
    p.voxel = float(voxel)
    p.nx, p.ny, p.nz = (int(d) for d in dims)
    return p


def tsdf_camera(camera):
    """struct cspm_tsdf_camera from a dict with f, cx, cy, R (3, 3), t (3,)"""
    R, t = _pose(camera["R"], camera["t"])
    return TsdfCamera(float(camera["f"]), float(camera["cx"]), float(camera["cy"]), (C.c_double * 9)(*R), (C.c_double * 3)(*t))


def _ray_outputs(h, w, outputs, out):
    shapes = dict(depth=((h, w), np.float64), normal=((3, h, w), np.float64), bgr=((h, w, 3), np.uint8), status=((h, w), np.uint8))
    res = {}
    for name in outputs:
        shape, dtype = shapes[name]
        a = (out or {}).get(name)
        res[name] = np.zeros(shape, dtype) if a is None else a
        assert res[name].shape == shape and res[name].dtype == dtype and res[name].flags.c_contiguous, name
    return res


def tsdf_depth_maps(views, w, h, origin, voxel, dims, cloud=True, cloud_cap=None, volume=True, device=0, out=None, **params):
    """T alone on host maps (cspm_tsdf_depth_maps): the views (dicts as for fuse_depth_maps) integrated in list order
    into a cleared volume, then its surface points.  Returns dict(count, cloud, D, W, C) as StereoContext.tsdf_points and tsdf_volume
    return them.  out: a dict with preallocated cloud_buffer, D, W, C to write into (tests poison them)."""
    K = len(views)
    p = tsdf_params(origin, voxel, dims, **params)
    arr = (FuseView * max(K, 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, img = _fuse_maps(v["depth"], v.get("normal"), v.get("bgr"), w, h)
        R, t = _pose(v["R"], v["t"])
        keep.append((d, n, img))
        arr[k] = FuseView(_dp(d), _opt(_dp, n), _opt(_u8, img), 3 * w, float(v["f"]), float(v["cx"]), float(v["cy"]), (C.c_double * 9)(*R), (C.c_double * 3)(*t))
    nx, ny, nz = p.nx, p.ny, p.nz
    nvox = max(nx, 0) * max(ny, 0) * max(nz, 0)
    cap = 3 * nvox if cloud_cap is None else int(cloud_cap)
    pts = None
    if cloud:
        pts = (out or {}).get("cloud_buffer")
        if pts is None:
            pts = np.zeros(cap, Point)
    vol = {}
    if volume:
        for name, shape, dtype in (("D", (nz, ny, nx), np.float32), ("W", (nz, ny, nx), np.float32), ("C", (nz, ny, nx, 4), np.uint8)):
            a = (out or {}).get(name)
            vol[name] = np.zeros(tuple(max(s, 0) for s in shape), dtype) if a is None else a
    cnt = C.c_uint(0)
    fp = C.POINTER(C.c_float)
    _check(load_library().cspm_tsdf_depth_maps(device, C.byref(p), arr, K, w, h, _opt(_vp, pts), cap if cloud else 0, C.byref(cnt),
                                               vol["D"].ctypes.data_as(fp) if volume else None, vol["W"].ctypes.data_as(fp) if volume else None,
                                               _u8(vol["C"]) if volume else None))
    del keep
    res = dict(count=cnt.value, **vol)
    if cloud:
        res["cloud"] = pts[:min(cnt.value, cap)]
    return res


def _tsdf_mesh_caps(nx, ny, nz, vertex_cap, face_cap):
    nvox = max(nx, 0) * max(ny, 0) * max(nz, 0)
    cells = max(nx - 1, 0) * max(ny - 1, 0) * max(nz - 1, 0)
    return 3 * nvox if vertex_cap is None else int(vertex_cap), 5 * cells if face_cap is None else int(face_cap)


def _tsdf_mesh_buffers(vertices, faces, vcap, fcap, out):
    pts = tri = None
    if vertices:
        pts = (out or {}).get("vertex_buffer")
        if pts is None:
            pts = np.zeros(vcap, Point)
    if faces:
        tri = (out or {}).get("face_buffer")
        if tri is None:
            tri = np.zeros(fcap, Face)
    return pts, tri


def _tsdf_mesh_result(nv, nf, pts, tri, vcap, fcap):
    res = dict(n_vertices=nv, n_faces=nf)
    if pts is not None:
        res["vertices"] = pts[:min(nv, vcap)]
    if tri is not None:
        res["faces"] = tri[:min(nf, fcap)]
    return res


def tsdf_mesh_depth_maps(views, w, h, origin, voxel, dims, vertices=True, faces=True, vertex_cap=None, face_cap=None, device=0, out=None, **params):
    """MC alone on host maps (cspm_tsdf_mesh_depth_maps): the views (dicts as for fuse_depth_maps) integrated in list
    order into a cleared volume, then its mesh.  Returns what StereoContext.tsdf_mesh returns."""
    K = len(views)
    p = tsdf_params(origin, voxel, dims, **params)
    arr = (FuseView * max(K, 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, img = _fuse_maps(v["depth"], v.get("normal"), v.get("bgr"), w, h)
        R, t = _pose(v["R"], v["t"])
        keep.append((d, n, img))
        arr[k] = FuseView(_dp(d), _opt(_dp, n), _opt(_u8, img), 3 * w, float(v["f"]), float(v["cx"]), float(v["cy"]), (C.c_double * 9)(*R), (C.c_double * 3)(*t))
    vcap, fcap = _tsdf_mesh_caps(p.nx, p.ny, p.nz, vertex_cap, face_cap)
    pts, tri = _tsdf_mesh_buffers(vertices, faces, vcap, fcap, out)
    nv, nf = C.c_uint(0), C.c_uint(0)
    _check(load_library().cspm_tsdf_mesh_depth_maps(device, C.byref(p), arr, K, w, h, _opt(_vp, pts), vcap if vertices else 0, _opt(_vp, tri),
                                                    fcap if faces else 0, C.byref(nv), C.byref(nf)))
    del keep
    return _tsdf_mesh_result(nv.value, nf.value, pts, tri, vcap, fcap)


def reg_params(**params):
    """struct cspm_reg_params: cspm_reg_default_params with the given fields replaced"""
    return _params(RegParams, "reg", "registration", params)


def _mask(targets):
    """a 64-bit view mask from an integer or a sequence of slots"""
    if isinstance(targets, (int, np.integer)):
        return C.c_ulonglong(int(targets))
    return C.c_ulonglong(sum(1 << int(k) for k in set(targets)))


def _reg_outputs(p, out):
    R = (out or {}).get("R")
    t = (out or {}).get("t")
    it = (out or {}).get("iters")
    return (np.zeros(9) if R is None else R, np.zeros(3) if t is None else t, np.zeros(max(p.iters, 1), REG_ITER) if it is None else it)


def register_depth_maps(views, w, h, src, targets, device=0, out=None, **params):
    """R alone on host maps (cspm_register_depth_maps): view `src` of `views` (dicts as for fuse_depth_maps, with
    normals) registered against the views of `targets` (a bit mask or a sequence of indices), starting from its own pose.  Returns what
    StereoContext.fuse_register returns."""
    K = len(views)
    p = reg_params(**params)
    arr = (FuseView * max(K, 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, _ = _fuse_maps(v["depth"], v.get("normal"), None, w, h)
        Rk, tk = _pose(v["R"], v["t"])
        keep.append((d, n))
        arr[k] = FuseView(_dp(d), _opt(_dp, n), None, 0, float(v["f"]), float(v["cx"]), float(v["cy"]), (C.c_double * 9)(*Rk), (C.c_double * 3)(*tk))
    R, t, it = _reg_outputs(p, out)
    _check(load_library().cspm_register_depth_maps(device, C.byref(p), arr, K, w, h, int(src), _mask(targets), _dp(R), _dp(t),
                                                   it.ctypes.data_as(C.POINTER(RegIter))))
    del keep
    return dict(R=R.reshape(3, 3), t=t, iters=it[:p.iters])


def carry_params(**params):
    """struct cspm_carry_params: cspm_carry_default_params with the given fields replaced"""
    return _params(CarryParams, "carry", "carry", params)


def carry_relative_pose(Rs, ts, Rt, tt):
    """two camera -> world poses into the motion X_t = R X_s + t between the cameras (cspm_carry_relative_pose): returns (R (3, 3), t)"""
    Rs, ts = _pose(Rs, ts)
    Rt, tt = _pose(Rt, tt)
    R, t = np.zeros(9), np.zeros(3)
    _check(load_library().cspm_carry_relative_pose(_dp(Rs), _dp(ts), _dp(Rt), _dp(tt), _dp(R), _dp(t)))
    return R.reshape(3, 3), t


def carry_plane_field(planes, src_calib, src_view, dst_calib, dst_view, w_t, h_t, max_dis, R, t, mask=None, device=0, out=None, **params):
    """C alone on host memory (cspm_carry_plane_field): planes (h_s, w_s, 6) in the layout of get_planes (only the
    param part is read), mask (h_s, w_s) or None, the motion X_t = R X_s + t between the two cameras.  out: a dict of preallocated
    arrays to write into instead of fresh ones (tests poison them).  Returns dict(planes (h_t, w_t, 6), state (h_t, w_t) uint8,
    source (h_t, w_t) int32); params: fill."""
    f = np.ascontiguousarray(planes, dtype=np.float64)
    assert f.ndim == 3 and f.shape[2] == 6, f.shape
    h_s, w_s = f.shape[:2]
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert m.shape == (h_s, w_s), m.shape
    ks, kt, p = calib_struct(src_calib), calib_struct(dst_calib), carry_params(**params)
    R, t = _pose(R, t)
    res = dict(out or {})
    shape = (max(int(h_t), 0), max(int(w_t), 0))
    if "planes" not in res:
        res["planes"] = np.zeros(shape + (6,))
    if "state" not in res:
        res["state"] = np.zeros(shape, np.uint8)
    if "source" not in res:
        res["source"] = np.zeros(shape, np.int32)
    _check(load_library().cspm_carry_plane_field(device, _dp(f), _opt(_u8, m), C.byref(ks), int(src_view), w_s, h_s, C.byref(kt), int(dst_view), int(w_t),
                                                 int(h_t), int(max_dis), _dp(R), _dp(t), C.byref(p), _dp(res["planes"]), _u8(res["state"]),
                                                 _i32(res["source"])))
    return res


def synth_params(**params):
    """struct cspm_synth_params: cspm_synth_default_params with the given fields replaced"""
    return _params(SynthParams, "synth", "view-synthesis", params)


def _synth_outputs(h, w, outputs, out):
    res = dict(out or {})
    for name in outputs:
        if name not in ("bgr", "disp", "mask"):
            raise TypeError(f"unknown view-synthesis output {name!r}")
        if name not in res:
            res[name] = np.zeros({"bgr": (h, w, 3), "disp": (h, w), "mask": (h, w)}[name], np.float64 if name == "disp" else np.uint8)
    res = {k: v for k, v in res.items() if k in outputs}
    if "bgr" in res:
        b = res["bgr"]
        assert b.dtype == np.uint8 and b.shape == (h, w, 3) and b.strides[1:] == (3, 1), "bgr: uint8 (h, w, 3) with packed pixels"
    assert "disp" not in res or (res["disp"].dtype == np.float64 and res["disp"].shape == (h, w) and res["disp"].flags.c_contiguous)
    assert "mask" not in res or (res["mask"].dtype == np.uint8 and res["mask"].shape == (h, w) and res["mask"].flags.c_contiguous)
    return res


def synthesize_host(t, disp, bgr, valid=(None, None), slope_a=(None, None), outputs=("bgr", "disp", "mask"), out=None, device=0, **params):
    """N alone on host maps (cspm_synthesize_host).  disp, bgr, valid, slope_a: pairs (view 0, view 1); disp (h, w)
    f64, bgr (h, w, 3) uint8 (rows may be padded), valid (h, w) or None, slope_a (h, w) f64 or None; both entries of a view that `views`
    does not name may be None.  outputs / out / params and the result as for StereoContext.synthesize."""
    L = load_library()
    p = synth_params(**params)
    keep, views, shape = [], [], None
    for v in range(2):
        if disp[v] is None or bgr[v] is None:
            views.append(None)
            continue
        d = np.ascontiguousarray(disp[v], dtype=np.float64)
        assert d.ndim == 2 and (shape is None or d.shape == shape), d.shape
        shape = d.shape
        img = np.asarray(bgr[v])
        if img.dtype != np.uint8 or img.strides[1:] != (3, 1):
            img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == d.shape + (3,), img.shape
        m = None if valid[v] is None else np.ascontiguousarray(np.asarray(valid[v]) != 0, dtype=np.uint8)
        a = None if slope_a[v] is None else np.ascontiguousarray(slope_a[v], dtype=np.float64)
        assert (m is None or m.shape == shape) and (a is None or a.shape == shape)
        keep += [d, img, m, a]
        views.append(SynthView(_dp(d), _opt(_u8, m), _opt(_dp, a), _u8(img), img.strides[0]))
    assert shape is not None, "no source view"
    h, w = shape
    res = _synth_outputs(h, w, outputs, out)
    b = res.get("bgr")
    _check(L.cspm_synthesize_host(device, C.byref(p), float(t), _opt(C.byref, views[0]), _opt(C.byref, views[1]), w, h, _opt(_u8, b),
                                  b.strides[0] if b is not None else 0, _opt(_dp, res.get("disp")), _opt(_u8, res.get("mask"))))
    return res


def smooth_params(**params):
    """struct cspm_smooth_params: cspm_smooth_default_params with the given fields replaced.  `lambda` is a Python keyword: the field
    is given as lam (or as "lambda" through a dict)."""
    return _params(SmoothParams, "smooth", "smoothing", params, {"lam": "lambda_", "lambda": "lambda_"})


def smooth_disparity(device, disp, conf=None, guide=None, max_dis=0, **params):
    """the edge-aware global smoother alone (cspm_smooth_disparity_host) on a host map: disp (h, w) f64 (a
    non-finite pixel is a hole), conf (h, w) f64 in [0, 1] or None (all 1), guide (h, w, 3) uint8 BGR or None (every weight 1);
    params: lam, sigma_color, iterations; max_dis > 0 clamps the smoothed values to [0, max_dis].  Returns a new (h, w) f64 map."""
    p = smooth_params(**params)
    d, _, (c,), g = _maps(disp, None, (conf,), guide)
    out = np.zeros_like(d)
    _check(load_library().cspm_smooth_disparity_host(device, _dp(d), _opt(_dp, c), _opt(_u8, g), d.shape[1], d.shape[0], C.byref(p), int(max_dis),
                                                     _dp(out)))
    return out


def median_filter(device, img, r):
    """the median filter alone on a host image: uint8 (h, w) or (h, w, 1 .. 4) -> M8 per channel, float64 (h, w)
    -> M64.  Returns a new array of the input's shape and dtype."""
    L = load_library()
    a = np.asarray(img)
    if a.dtype == np.uint8:
        assert a.ndim in (2, 3), a.shape
        src = np.ascontiguousarray(a)
        h, w = src.shape[:2]
        cn = src.shape[2] if src.ndim == 3 else 1
        out = np.zeros_like(src)
        rc = L.cspm_median_filter_u8_host(device, _u8(src), w * cn, w, h, cn, int(r), _u8(out), w * cn)
    elif a.dtype == np.float64:
        assert a.ndim == 2, a.shape
        src = np.ascontiguousarray(a)
        out = np.zeros_like(src)
        rc = L.cspm_median_filter_f64_host(device, _dp(src), src.shape[1], src.shape[0], int(r), _dp(out))
    else:
        raise TypeError(f"median_filter takes uint8 or float64 images, not {a.dtype}")
    _check(rc)
    return out


def disparity_planes(disp):
    """(h, w) disparities -> the (h, w, 6) fronto-parallel planes (0, 0, 1, 0, 0, d)"""
    d = np.asarray(disp, dtype=np.float64)
    f = np.zeros(d.shape + (6,))
    f[..., 2] = 1.0
    f[..., 5] = d
    return f


def seeded_patchmatch(ctx, iters, seeds=(), **kw):
    """PatchMatch whose random start field competes with the caller's hypotheses: pm_init, then every seed merged in turn, then
    `iters` iterations (patchmatch_warm: a cold run's streams).  A seed is a StereoContext (its plane field, both views) or a tuple
    (view, field[, mask]) as for merge_planes.  Asynchronous like patchmatch; ctx has its images and cost object."""
    init_kw = {k: kw[k] for k in ("seed", "rng_mode", "early_exit") if k in kw}
    ctx.pm_init(**init_kw)
    for s in seeds:
        if isinstance(s, StereoContext):
            ctx.merge_planes_from(s)
        else:
            ctx.merge_planes(*s)
    ctx.patchmatch_warm(iters, **kw)
    return ctx


def coarse_to_fine(l, r, max_dis, coarse_iters=3, fine_iters=1, cc="GRD", wnd_size=35, scale_num=5, reg_lambda=0.3, volumes=False,
                   device=0, ctx=None, coarse_ctx=None, fused=None, **pm_kw):
    """PatchMatch on the half-size pair, then `fine_iters` warm iterations on the full pair from the upsampled planes.

    The half-size images are the full cost object's level-1 images (pyrDown); the coarse run uses max_dis (max_dis + 1) // 2 and the
    same cost settings.  ctx / coarse_ctx: contexts to reuse (created and, for the coarse one, closed here when None).  Returns the
    full-size context with the warm run enqueued (asynchronous like patchmatch).  fused: passed to build_cost_cengrd (cc="CENGRD" only)."""
    full = ctx if ctx is not None else StereoContext(device)
    coarse = coarse_ctx if coarse_ctx is not None else StereoContext(device)

    def build(c, md):
        if cc == "GRD":
            c.build_cost_grd(md, wnd_size, scale_num, reg_lambda, volumes=volumes)
        elif cc == "CEN":
            c.build_cost_cen(md, wnd_size, scale_num, reg_lambda, volumes=volumes)
        elif cc == "CENGRD":
            c.build_cost_cengrd(md, wnd_size, scale_num, reg_lambda, fused=fused)
        elif cc == "IMG":
            c.build_cost_img(md, wnd_size, scale_num, reg_lambda)
        else:
            raise ValueError(f"unknown cost {cc!r} (GRD, CEN, CENGRD or IMG)")

    try:
        full.set_images(l, r)
        if scale_num < 2:  # a single-scale cost has no level 1: a two-level volume-free cost provides the pyrDown images
            full.build_cost_img(max_dis, wnd_size, 2, 0.0)
            half = [full.level_image(v, 1) for v in range(2)]
            build(full, max_dis)
        else:
            build(full, max_dis)
            half = [full.level_image(v, 1) for v in range(2)]
        coarse.set_images(half[0], half[1])
        build(coarse, (max_dis + 1) // 2)
        coarse.patchmatch(coarse_iters, **pm_kw)
        full.upsample_planes_from(coarse)
        full.patchmatch_warm(fine_iters, **pm_kw)
    finally:
        if coarse_ctx is None:
            coarse.close()
    return full
