"""TSDF fusion on the GPU (include/cspm.h "TSDF fusion") held to tests/tsdf_ref.py bit for bit (NaN positions
included, any NaN payload): cspm_tsdf_depth_maps and the context entries over the case table of tests/tsdf_cases.py -- volume, count,
records, raycasts -- ; the context entries on pushed plane fields against the one-shot entry and the restatement; the host and device
variants; a raycast pushed as a fusion view and registered against; clear, repeated integration, the timing counts, the error returns
with untouched outputs, a real PatchMatch run, and that a context behaves the same with and without a volume."""
import ctypes as C
import math

import numpy as np
import pytest

import fuse_cases as fc
import tsdf_cases as tc
import tsdf_ref as tr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py)"""
    yield


def _same_volume(got, want, what):
    for name in ("D", "W"):
        a, b = np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)
        assert tr.same_bits(a, b), f"{what}: {name} differs in {np.sum(a != b)} voxels"
    a, b = np.asarray(got["C"]).reshape(-1, 4), np.asarray(want["C"]).reshape(-1, 4)
    assert np.array_equal(a, b), f"{what}: the colour differs in {np.sum(np.any(a != b, 1))} voxels"


def _same_points(got, want, what, cap=None):
    assert got["count"] == want["count"], f"{what}: count {got['count']} != {want['count']}"
    if "cloud" in got:
        ref = want["cloud"] if cap is None else want["cloud"][:cap]
        assert len(got["cloud"]) == len(ref), f"{what}: {len(got['cloud'])} records, {len(ref)} expected"
        for name in tr.POINT.names:
            assert tr.same_bits(got["cloud"][name], ref[name]), f"{what}: cloud field {name} differs in {np.sum(got['cloud'][name] != ref[name])} records"


def _same_ray(got, want, what):
    assert np.array_equal(got["status"], want["status"]), f"{what}: status differs in {np.sum(got['status'] != want['status'])} pixels"
    for name in ("depth", "normal"):
        assert tr.same_bits(got[name], want[name]), f"{what}: {name} differs in {np.sum(~((got[name] == want[name]) | (np.isnan(got[name]) & np.isnan(want[name]))))} values"
    assert np.array_equal(got["bgr"], want["bgr"]), f"{what}: the colour differs"


def _push_maps(ctx, v):
    ctx.fuse_push_maps(v["depth"], v["f"], v["cx"], v["cy"], v["R"], v["t"], normal=v.get("normal"), bgr=v.get("bgr"))


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_one_shot_entry_against_the_restatement(case):
    want = case.reference()
    cap = case.capacity()
    poison = np.frombuffer(bytes([0xAB]) * (32 * (cap + 3)), capi.Point).copy()
    got = capi.tsdf_depth_maps(case.views(), case.w, case.h, case.origin, case.voxel, case.dims, cloud_cap=cap, out={"cloud_buffer": poison}, **case.params)
    _same_volume(got, want, case.name)
    _same_points(got, want, case.name, cap)
    assert np.all(poison[min(cap, want["count"]):].view(np.uint8) == 0xAB), "records beyond the capacity or the count were written"


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_context_entries_and_raycasts_against_the_restatement(gpu_ctx, case):
    ctx = gpu_ctx
    want = case.reference()
    views = case.views()
    ctx.fuse_begin(case.w, case.h, len(views))
    try:
        ctx.tsdf_begin(case.origin, case.voxel, case.dims, **case.params)
        try:
            for k, v in enumerate(views):
                _push_maps(ctx, v)
                ctx.tsdf_integrate(k)
            _same_volume(ctx.tsdf_volume(), want, case.name)
            _same_points(ctx.tsdf_points(), want, case.name)
            for i, (cam, ray) in enumerate(zip(case.ray_cameras(), case.raycasts())):
                _same_ray(ctx.tsdf_raycast(cam, case.w, case.h, 0.0 if i % 2 == 0 else 0.25), ray, f"{case.name} ray camera {i}")
        finally:
            ctx.tsdf_end()
    finally:
        ctx.fuse_end()


def test_counts_only_and_capacities():
    case = tc.BY_NAME["33x17x9_130x67_K3_n1_all_c0.0"]
    want = case.reference()
    views = case.views()
    only = capi.tsdf_depth_maps(views, case.w, case.h, case.origin, case.voxel, case.dims, cloud=False, volume=False, **case.params)
    assert only["count"] == want["count"] and "cloud" not in only and "D" not in only
    for cap in (1, 63, 64, 257, want["count"] - 1, want["count"], want["count"] + 100):
        poison = np.frombuffer(bytes([0x5A]) * (32 * cap), capi.Point).copy()
        got = capi.tsdf_depth_maps(views, case.w, case.h, case.origin, case.voxel, case.dims, cloud_cap=cap, volume=False, out={"cloud_buffer": poison},
                                   **case.params)
        _same_points(got, want, f"cap {cap}", cap)
        assert np.all(poison[min(cap, want["count"]):].view(np.uint8) == 0x5A), cap


# ---- the context entries on pushed plane fields -----------------------------------------------------------------------------------------
from test_gpu_fuse import CAL, H, POSES, PUSHES, W, _push_all  # noqa: E402  (the plane fields, poses and pushes of the fusion tests)

VOL = dict(origin=(-2.5, -1.75, 2.8), voxel=0.25, dims=(20, 14, 10))
PARAMS = dict(trunc=0.6, min_cos=0.3)
RAY_CAM = dict(f=58.0, cx=30.5, cy=22.0, R=fc.rot(1.0, -6.0, 4.0), t=np.array([0.2, -0.05, 0.3]))


@pytest.fixture()
def pushed(gpu_ctx):
    gpu_ctx.fuse_begin(W, H, len(PUSHES) + 1)
    try:
        yield gpu_ctx, _push_all(gpu_ctx, PUSHES)
    finally:
        gpu_ctx.enable_timing(False)
        if gpu_ctx.L.cspm_tsdf_end(gpu_ctx.p) not in (0, ERR_STATE):
            raise AssertionError("cspm_tsdf_end failed")
        gpu_ctx.fuse_end()


def test_context_pushes_equal_the_one_shot_entry_and_the_restatement(pushed):
    ctx, views = pushed
    ctx.tsdf_begin(**VOL, **PARAMS)
    for k in range(len(views)):
        ctx.tsdf_integrate(k)
    want = tr.fuse(views, W, H, **VOL, **PARAMS)
    assert 50 < want["count"] and (want["W"] == len(views)).any() and (want["C"][:, 3] == 1).any()
    got = dict(ctx.tsdf_volume(), **ctx.tsdf_points())
    _same_volume(got, want, "context")
    _same_points(got, want, "context")
    one = capi.tsdf_depth_maps(views, W, H, **VOL, **PARAMS)
    _same_volume(one, got, "one-shot")
    _same_points(one, got, "one-shot")
    ray = tr.raycast(want["vol"], RAY_CAM, W, H, 0.5)
    assert (ray["status"] == 1).sum() > 500
    _same_ray(ctx.tsdf_raycast(RAY_CAM, W, H, 0.5), ray, "raycast")


def test_raycast_device_variant_and_outputs_not_asked_for(pushed):
    import torch
    ctx, views = pushed
    ctx.tsdf_begin(**VOL, **PARAMS)
    for k in range(3):
        ctx.tsdf_integrate(k)
    want = ctx.tsdf_raycast(RAY_CAM, W, H, 0.5)
    n, stride = W * H, 3 * W + 5
    depth = torch.full((H, W), 7.0, dtype=torch.float64, device="cuda")
    normal = torch.full((3, H, W), 7.0, dtype=torch.float64, device="cuda")
    bgr = torch.full((H, stride), 0xAB, dtype=torch.uint8, device="cuda")
    status = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.tsdf_raycast_device(RAY_CAM, W, H, 0.5, d_depth=depth.data_ptr(), d_normal=normal.data_ptr(), d_bgr=bgr.data_ptr(), stride=stride, d_status=status.data_ptr())
    ctx.synchronize()
    rows = bgr.cpu().numpy()
    got = dict(depth=depth.cpu().numpy(), normal=normal.cpu().numpy(), bgr=rows[:, :3 * W].reshape(H, W, 3), status=status.cpu().numpy())
    _same_ray(got, want, "device variant")
    assert np.all(rows[:, 3 * W:] == 0xAB), "bytes between the rows were written"
    some = ctx.tsdf_raycast(RAY_CAM, W, H, 0.5, outputs=("depth",))
    assert set(some) == {"depth"} and tr.same_bits(some["depth"], want["depth"])
    # the points' device variant
    want_pts = ctx.tsdf_points()
    cap = want_pts["count"] + 5
    cloud = torch.full((cap, 32), 0xAB, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.tsdf_points_device(d_cloud=cloud.data_ptr(), cloud_cap=cap, d_count=count.data_ptr())
    ctx.synchronize()
    raw = cloud.cpu().numpy()
    got_pts = dict(count=int(count.item()), cloud=raw.view(capi.Point).reshape(-1)[:int(count.item())])
    _same_points(got_pts, want_pts, "points, device variant")
    assert np.all(raw[want_pts["count"]:] == 0xAB)
    L = capi.load_library()
    assert L.cspm_tsdf_points_device(ctx.p, C.c_void_p(cloud.data_ptr() + 8), 4, None) == ERR_ARG
    assert L.cspm_last_error(ctx.p).decode() == "tsdf: the cloud buffer must be 16-byte aligned"
    assert L.cspm_tsdf_points_device(ctx.p, None, 0, C.c_void_p(count.data_ptr() + 2)) == ERR_ARG
    assert L.cspm_last_error(ctx.p).decode() == "tsdf: the count must be 4-byte aligned"
    k = capi.tsdf_camera(RAY_CAM)
    assert L.cspm_tsdf_raycast_device(ctx.p, C.byref(k), W, H, 0.5, C.c_void_p(depth.data_ptr() + 4), None, None, 0, None) == ERR_ARG
    assert L.cspm_last_error(ctx.p).decode() == "tsdf: the depth and normal maps must be 8-byte aligned"


CORNER_VOL = dict(origin=(-1.5, -1.25, 2.5), voxel=0.125, dims=(28, 22, 19))


def _corner_views():
    """the three-plane corner of the registration tests, rendered exactly from three poses; slot 1 stands at register_cases.TRUE"""
    import register_cases as rc
    views = []
    for k, (R, t) in enumerate([(np.eye(3), np.zeros(3)), rc.TRUE, (fc.rot(-1.0, 2.0, -1.5), np.array([-0.2, 0.03, 0.05]))]):
        cam = fc.camera(W, H, k, R, t)
        depth, normal, bgr = fc.render(cam, W, H, rc.CORNER)
        views.append(fc.view(cam, depth, normal, bgr))
    return views


def test_a_pushed_raycast_is_a_view_to_register_against_and_to_fuse(gpu_ctx):
    """frame to model: cspm_tsdf_raycast_push then cspm_fuse_register == cspm_register_depth_maps on the restatement's raycast maps, the
    pose and every iteration record bit for bit; the slot also serves as a source and in cspm_fuse_run"""
    import fuse_ref as fr
    import register_cases as rc
    ctx = gpu_ctx
    views = _corner_views()
    vol = tr.fuse(views, W, H, **CORNER_VOL, trunc=0.4)["vol"]
    ray = tr.raycast(vol, RAY_CAM, W, H, 0.5)
    assert (ray["status"] == 1).sum() > 2000
    model = dict(RAY_CAM, depth=ray["depth"], normal=ray["normal"], bgr=ray["bgr"])
    slot = len(views)
    ctx.fuse_begin(W, H, slot + 1)
    try:
        ctx.tsdf_begin(**CORNER_VOL, trunc=0.4)
        try:
            for k, v in enumerate(views):
                _push_maps(ctx, v)
                ctx.tsdf_integrate(k)
            ctx.tsdf_raycast_push(RAY_CAM, 0.5)
            assert ctx.fuse_view_count() == slot + 1
            R, t = ctx.fuse_get_pose(slot)
            assert np.array_equal(R, RAY_CAM["R"]) and np.array_equal(t, RAY_CAM["t"])
            reg = dict(iters=4, max_dist=0.3, min_pairs=50)
            R0, t0 = rc.START
            start = dict(views[1], R=R0, t=t0)
            want = capi.register_depth_maps([views[0], start, views[2], model], W, H, 1, [slot], **reg)
            got = ctx.fuse_register(1, [slot], R0=R0, t0=t0, **reg)
            assert np.all(want["iters"]["status"] == 0) and want["iters"]["pairs"][0] > 1000
            rot0, tr0 = rc.pose_error(R0, t0)
            rot1, tr1 = rc.pose_error(got["R"], got["t"])
            print("frame to model: pose error", (rot0, tr0), "->", (rot1, tr1))
            assert rot1 < rot0 / 4 and tr1 < tr0 / 4  # the model is a target worth registering against
            assert tr.same_bits(np.ascontiguousarray(got["R"]), np.ascontiguousarray(want["R"])) and tr.same_bits(got["t"], want["t"])
            for name in ("pairs", "cost", "rot2", "trans2", "status"):
                assert tr.same_bits(np.ascontiguousarray(got["iters"][name]), np.ascontiguousarray(want["iters"][name])), name
            back = ctx.fuse_register(slot, [0, 2], **reg)  # the model view as the SOURCE
            want_back = capi.register_depth_maps(views + [model], W, H, slot, [0, 2], **reg)
            assert tr.same_bits(np.ascontiguousarray(back["R"]), np.ascontiguousarray(want_back["R"])) and tr.same_bits(back["t"], want_back["t"])
            fused = ctx.fuse_run(min_views=1)
            ref = fr.fuse(views + [model], W, H, min_views=1)
            assert fused["count"] == ref["count"] and ref["view_counts"][slot] > 0 and np.array_equal(fused["view_counts"], ref["view_counts"])
            for name in fr.POINT.names:
                assert fr.same_bits(fused["cloud"][name], ref["cloud"][name]), name
        finally:
            ctx.tsdf_end()
    finally:
        ctx.fuse_end()


def test_clear_and_integrate_again_and_after_a_points_call(pushed):
    ctx, views = pushed
    ctx.tsdf_begin(**VOL, **PARAMS)
    for k in (0, 1, 2):
        ctx.tsdf_integrate(k)
    first = dict(ctx.tsdf_volume(), **ctx.tsdf_points())
    _same_volume(first, tr.fuse(views[:3], W, H, **VOL, **PARAMS), "first")
    ctx.tsdf_clear()
    cleared = ctx.tsdf_volume()
    assert (cleared["D"] == 1).all() and (cleared["W"] == 0).all() and not cleared["C"].any() and ctx.tsdf_points()["count"] == 0
    for k in (0, 1, 2):
        ctx.tsdf_integrate(k)
    again = dict(ctx.tsdf_volume(), **ctx.tsdf_points())
    _same_volume(again, first, "after a clear")
    _same_points(again, first, "after a clear")
    ctx.tsdf_integrate(4)  # a further view behind a points call
    want = tr.fuse([views[0], views[1], views[2], views[4]], W, H, **VOL, **PARAMS)
    later = dict(ctx.tsdf_volume(), **ctx.tsdf_points())
    _same_volume(later, want, "a further integrate")
    _same_points(later, want, "a further integrate")
    # the volume outlives the fusion views
    ctx.fuse_end()
    ctx.fuse_begin(W, H, 1)
    _same_volume(ctx.tsdf_volume(), want, "behind cspm_fuse_end")
    assert ctx.L.cspm_tsdf_integrate(ctx.p, 0) == ERR_STATE and _msg(ctx) == "tsdf: no such fusion view"


def test_timing_counts(pushed):
    ctx, views = pushed
    ctx.tsdf_begin(**VOL, **PARAMS)
    nvox = int(np.prod(VOL["dims"]))
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_timing()
    ctx.tsdf_integrate(0)
    ctx.tsdf_integrate(1)
    t = ctx.timing()
    assert (t["misc"]["launches"], t["misc"]["evals"]) == (2, 2 * nvox) and t["post"]["launches"] == 0
    ctx.reset_timing()
    ctx.tsdf_raycast(RAY_CAM, 33, 21, 0.5)
    t = ctx.timing()
    assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, 33 * 21)
    ctx.reset_timing()
    ctx.tsdf_points()
    t = ctx.timing()
    assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, nvox)
    ctx.reset_timing()
    ctx.tsdf_raycast_push(RAY_CAM, 0.5)
    t = ctx.timing()
    assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, W * H)


def _msg(ctx):
    return capi.load_library().cspm_last_error(ctx.p if ctx is not None else None).decode()


def test_error_returns_of_the_context_entries():
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    cnt = C.c_uint(0xABABABAB)
    depth = np.full((H, W), 4.0)
    normal = np.zeros((3, H, W))
    normal[2] = -1.0
    eye = dict(f=50.0, cx=30.0, cy=20.0, R=np.eye(3), t=np.zeros(3))
    k = capi.tsdf_camera(eye)
    out = np.full((H, W), 7.0)
    st = np.full((H, W), 9, np.uint8)
    fp = C.POINTER(C.c_float)
    vol = np.full(8, 7.0, np.float32)

    def begin(**over):
        v = dict(VOL, **{n: over.pop(n) for n in ("origin", "voxel", "dims") if n in over})
        p = capi.tsdf_params(v["origin"], v["voxel"], v["dims"], **over)
        return L.cspm_tsdf_begin(ctx.p, C.byref(p))

    def raycast(cam=k, w=W, h=H, z_near=0.0, bgr=None, stride=0):
        return L.cspm_tsdf_raycast(ctx.p, C.byref(cam) if cam is not None else None, w, h, z_near, capi._dp(out), None, capi._u8(bgr) if bgr is not None else None,
                                   stride, capi._u8(st))

    try:
        first = "tsdf: cspm_tsdf_begin first"
        for call in (lambda: L.cspm_tsdf_clear(ctx.p), lambda: L.cspm_tsdf_integrate(ctx.p, 0), raycast, lambda: L.cspm_tsdf_raycast_push(ctx.p, C.byref(k), 0.0),
                     lambda: L.cspm_tsdf_points(ctx.p, None, 0, C.byref(cnt)), lambda: L.cspm_tsdf_points_device(ctx.p, None, 0, None),
                     lambda: L.cspm_tsdf_get_volume(ctx.p, vol.ctypes.data_as(fp), None, None), lambda: L.cspm_tsdf_end(ctx.p)):
            assert call() == ERR_STATE and _msg(ctx) == first
        for over, msg in ((dict(voxel=0.0), "tsdf: the origin must be finite and voxel finite and > 0"), (dict(dims=(4, 0, 4)), "tsdf: nx, ny and nz must be at least 1"),
                          (dict(dims=(2048, 2048, 512)), "tsdf: nx * ny * nz must be below 2^31"), (dict(trunc=-1.0), "tsdf: trunc must be finite and > 0 (0 = 4 * voxel)"),
                          (dict(max_weight=0.0), "tsdf: max_weight must be in [1, 16777216]"), (dict(min_cos=2.0), "tsdf: min_cos must be in [0, 1]"),
                          (dict(step_rel=math.nan), "tsdf: step_rel must be in (0, 1]")):
            assert begin(**over) == ERR_ARG and _msg(ctx) == msg
        assert L.cspm_tsdf_begin(ctx.p, None) == ERR_ARG and _msg(ctx) == "tsdf: no parameters"
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == 0
        assert begin() == 0
        nvox = int(np.prod(VOL["dims"]))
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == 12 * nvox + 4 * (-(-nvox // 256) + 1)  # three planes and the extraction's counts
        assert begin() == ERR_STATE and _msg(ctx) == "tsdf: cspm_tsdf_begin twice without cspm_tsdf_end"
        assert L.cspm_tsdf_integrate(ctx.p, 0) == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin first"
        assert L.cspm_tsdf_raycast_push(ctx.p, C.byref(k), 0.0) == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin first"
        ctx.fuse_begin(W, H, 2)
        for slot in (0, -1, 5):
            assert L.cspm_tsdf_integrate(ctx.p, slot) == ERR_STATE and _msg(ctx) == "tsdf: no such fusion view"
        assert raycast(cam=None) == ERR_ARG and _msg(ctx) == "tsdf: no camera"
        assert raycast(cam=capi.tsdf_camera(dict(eye, f=0.0))) == ERR_ARG and _msg(ctx) == "fusion: f must be positive"
        assert raycast(cam=capi.tsdf_camera(dict(eye, R=np.eye(3) * 1.1))) == ERR_ARG and _msg(ctx) == "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"
        for z in (-0.1, math.nan, math.inf):
            assert raycast(z_near=z) == ERR_ARG and _msg(ctx) == "tsdf: z_near must be finite and >= 0"
        assert raycast(w=0) == ERR_ARG and _msg(ctx) == "fusion: w and h must be at least 1"
        img = np.zeros((H, W, 3), np.uint8)
        assert raycast(bgr=img, stride=3 * W - 1) == ERR_ARG and _msg(ctx) == "tsdf: stride is below 3 * w"
        assert L.cspm_tsdf_raycast_push(ctx.p, C.byref(k), -1.0) == ERR_ARG and _msg(ctx) == "tsdf: z_near must be finite and >= 0"
        assert (out == 7.0).all() and (st == 9).all() and cnt.value == 0xABABABAB and (vol == 7.0).all()  # no failed call wrote its output
        ctx.fuse_push_maps(depth, 50.0, 30.0, 20.0, np.eye(3), np.zeros(3))  # a view without normals
        assert L.cspm_tsdf_raycast_push(ctx.p, C.byref(k), 0.0) == ERR_ARG and _msg(ctx) == "fusion: normals in some views but not all"
        assert L.cspm_tsdf_integrate(ctx.p, 0) == 0
        ctx.fuse_end()
        ctx.fuse_begin(W, H, 1)
        ctx.fuse_push_maps(depth, 50.0, 30.0, 20.0, np.eye(3), np.zeros(3), normal=normal)
        assert L.cspm_tsdf_raycast_push(ctx.p, C.byref(k), 0.0) == ERR_STATE and _msg(ctx) == "fusion: every view slot is taken (max_views of cspm_fuse_begin)"
        assert raycast() == 0 and L.cspm_tsdf_points(ctx.p, None, 0, C.byref(cnt)) == 0 and cnt.value > 0
        assert L.cspm_tsdf_end(ctx.p) == 0 and ctx.get_option(capi.OPT_DEVICE_BYTES) > 0  # the fusion views are still there
        ctx.fuse_end()
        assert ctx.get_option(capi.OPT_DEVICE_BYTES) == 0
        assert begin() == 0
        ctx.synchronize()
    finally:
        ctx.close()  # with the volume still there: cspm_destroy frees it


def test_real_run_both_views(gpu_ctx, mid_pair):
    """the 96 x 64 pipeline pair after one PatchMatch iteration, both views pushed and integrated"""
    ctx = gpu_ctx
    w, h = mid_pair["w"], mid_pair["h"]
    ctx.set_images(mid_pair["l"], mid_pair["r"])
    ctx.build_cost_grd(mid_pair["max_dis"], 9, 3, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(1, seed=5)
    cal = (90.0, 47.5, 31.5, 0.2, 0.0)
    R, t = fc.rot(2.0, -3.0, 1.0), np.array([0.5, -0.25, 1.0])
    ctx.fuse_begin(w, h, 2)
    try:
        views = []
        for v in (0, 1):
            g = ctx.reproject(v, cal, capi.GEOM_PP, cloud=False, consistent_only=1)
            views.append(dict(depth=np.where(g["keep"] != 0, g["depth"], np.nan), normal=g["normal"], bgr=ctx.level_image(v, 0), f=cal[0],
                              cx=cal[1] + v * cal[4], cy=cal[2], R=R, t=t + (R[:, 0] * cal[3] if v else 0.0)))
            ctx.fuse_push(v, cal, R, t, capi.GEOM_PP, consistent_only=1)
        z = np.concatenate([v["depth"][np.isfinite(v["depth"])] for v in views])
        zm = float(np.median(z))
        voxel = zm / 30.0  # 32 voxels span the view's width at the median depth, and the depths from a half to one and a half of it
        centre = R @ np.array([0.0, 0.0, zm]) + t
        vol = dict(origin=tuple(centre - voxel * np.array([16.0, 12.0, 16.0])), voxel=voxel, dims=(32, 24, 32))
        ctx.tsdf_begin(**vol, min_cos=0.2)
        try:
            for k in (0, 1):
                ctx.tsdf_integrate(k)
            want = tr.fuse(views, w, h, **vol, min_cos=0.2)
            print("real run: median depth", zm, "depths 5..95 %", np.percentile(z, [5, 95]), "surface points", want["count"], "exits", want["exits"])
            assert want["count"] > 100 and (want["W"] == 2).any()
            got = dict(ctx.tsdf_volume(), **ctx.tsdf_points())
            _same_volume(got, want, "real run")
            _same_points(got, want, "real run")
            _same_ray(ctx.tsdf_raycast(views[0], w, h, 0.0), tr.raycast(want["vol"], views[0], w, h, 0.0), "real run, raycast at the left pose")
        finally:
            ctx.tsdf_end()
    finally:
        ctx.fuse_end()


def test_a_context_without_integration_computes_the_same(small_pair):
    """the feature unused: planes and maps of a run are byte-identical with and without cspm_tsdf_begin / cspm_tsdf_end around it"""
    res = []
    for tsdf in (False, True):
        ctx = capi.StereoContext(0)
        try:
            if tsdf:
                ctx.tsdf_begin(**VOL)
            ctx.set_images(small_pair["l"], small_pair["r"])
            ctx.build_cost_grd(small_pair["max_dis"], 9, 3, 0.3)
            ctx.patchmatch(2, seed=7)
            planes = [ctx.get_planes(v) for v in (0, 1)]
            maps = ctx.postprocess_f64(valid=True)
            geo = ctx.reproject(0, (60.0, 31.0, 23.0, 0.3, 0.0))
            if tsdf:
                ctx.tsdf_end()
            res.append((planes, maps, geo))
        finally:
            ctx.close()
    (pa, ma, ga), (pb, mb, gb) = res
    for v in (0, 1):
        assert pa[v][0].tobytes() == pb[v][0].tobytes() and pa[v][1].tobytes() == pb[v][1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ma, mb))
    assert ga["depth"].tobytes() == gb["depth"].tobytes() and ga["cloud"].tobytes() == gb["cloud"].tobytes()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _cli_inputs(tmp_path):
    import os
    import pngio
    from crossscalepatchmatch_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, D = 96, 64, 16
    cal = (90.0, 47.5, 31.5, 0.2, 0.0)
    pairs = [synth.make_pair(w, h, D, regions=3, seed=40 + k)[:2] for k in range(3)]
    lines = []
    for k, (l, r) in enumerate(pairs):
        pngio.write_png(str(tmp_path / f"l{k}.png"), l[..., ::-1])
        pngio.write_png(str(tmp_path / f"r{k}.png"), r[..., ::-1])
        lines.append(" ".join(str(tmp_path / n) for n in (f"l{k}.png", f"r{k}.png", f"ld{k}.png", f"rd{k}.png")))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    calib = tmp_path / "calib.txt"
    calib.write_text(f"cam0=[{cal[0]} 0 {cal[1]}; 0 {cal[0]} {cal[2]}; 0 0 1]\ncam1=[{cal[0]} 0 {cal[1] + cal[4]}; 0 {cal[0]} {cal[2]}; 0 0 1]\n"
                     f"doffs={cal[4]}\nbaseline={cal[3]}\nwidth={w}\nheight={h}\nndisp={D}\n")
    golden = os.path.join(root, "tests", "golden", "fuse", "poses.txt")
    poses = np.array([[float(t) for t in ln.split("#")[0].split()] for ln in open(golden) if ln.split("#")[0].strip()]).reshape(3, 3, 4)
    main = os.path.join(root, "crossscalepatchmatch_amd", "cspm_main")
    base = [main, f"--batch_list={tmp_path / 'list.txt'}", f"--calib={calib}", f"--fuse_poses={golden}", "--fuse_source=pp", "--fuse_min_views=1",
            "--geom_min_cos=0.2", f"--max_dis={D}", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--iters=1", "--seed=3", "--in_flight=2",
            "--tsdf_origin=-2,-1.5,1", "--tsdf_dims=40,30,40", "--tsdf_voxel=0.1", "--tsdf_min_cos=0.1"]
    return dict(w=w, h=h, D=D, cal=cal, pairs=pairs, poses=poses, base=base, vol=dict(origin=(-2.0, -1.5, 1.0), voxel=0.1, dims=(40, 30, 40), min_cos=0.1))


def _pair_views(ctx, k, inp, pose, right):
    """pair k run as the command line runs it, and the fusion views of its post-processed field"""
    l, r = inp["pairs"][k]
    cal = inp["cal"]
    ctx.set_images(l, r)
    ctx.build_cost_grd(inp["D"], 35, 5, 0.3)
    ctx.patchmatch(1, seed=3)
    R, t = pose[:, :3], pose[:, 3]
    views = []
    for v in ((0, 1) if right else (0,)):
        g = ctx.reproject(v, cal, capi.GEOM_PP, cloud=False, consistent_only=1, min_cos=0.2)
        views.append(dict(depth=np.where(g["keep"] != 0, g["depth"], np.nan), normal=g["normal"], bgr=ctx.level_image(v, 0), f=cal[0], cx=cal[1] + v * cal[4],
                          cy=cal[2], R=R, t=t + (R[:, 0] * cal[3] if v else 0.0)))
    return views


def _read_ply(path):
    head, _, body = open(path, "rb").read().partition(b"end_header\n")
    return head, np.frombuffer(body, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))


def test_cli_integrates_a_batch_list(gpu_ctx, tmp_path):
    """cspm_main --fuse_poses --fuse_ply --tsdf_ply on three pairs, both views == the C-ABI path on the same files: the PLY's vertex count
    and bytes"""
    import subprocess
    inp = _cli_inputs(tmp_path)
    ply = tmp_path / "model.ply"
    res = subprocess.run(inp["base"] + [f"--fuse_ply={tmp_path / 'fused.ply'}", f"--tsdf_ply={ply}", "--fuse_right=true"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TSDF: 6 views" in res.stdout, res.stdout + res.stderr
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    views = []
    for k in range(3):
        views += _pair_views(ctx, k, inp, inp["poses"][k], True)
    want = capi.tsdf_depth_maps(views, inp["w"], inp["h"], volume=False, **inp["vol"])
    cl = want["cloud"]
    print("command line: surface points", want["count"])
    assert want["count"] > 100
    head, pts = _read_ply(ply)
    assert f"element vertex {want['count']}\n".encode() in head and len(pts) == len(cl)
    assert tr.same_bits(pts["p"], np.stack([cl["x"], cl["y"], cl["z"]], 1))
    nrm = np.stack([cl["nx"], cl["ny"], cl["nz"]], 1)
    nrm[np.isnan(nrm).any(1)] = 0.0
    assert tr.same_bits(pts["n"], nrm)
    np.testing.assert_array_equal(pts["rgb"], np.stack([cl["r"], cl["g"], cl["b"]], 1))


def test_cli_registers_frame_to_model(gpu_ctx, tmp_path):
    """--fuse_register --tsdf_register: the poses written are those of the C-ABI sequence raycast_push, fuse_register, integrate"""
    import subprocess
    inp = _cli_inputs(tmp_path)
    out = tmp_path / "poses_out.txt"
    res = subprocess.run(inp["base"] + [f"--fuse_ply={tmp_path / 'fused.ply'}", f"--tsdf_ply={tmp_path / 'model.ply'}", "--fuse_register=true", "--tsdf_register=true",
                                        f"--fuse_poses_out={out}", "--fuse_reg_iters=3"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Registration, pair 2" in res.stdout and "TSDF: 3 views" in res.stdout, res.stdout + res.stderr
    got = np.array([[float(t) for t in ln.split()] for ln in open(out) if ln.strip()]).reshape(3, 3, 4)
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    views = [_pair_views(ctx, k, inp, inp["poses"][k], False)[0] for k in range(3)]
    w, h = inp["w"], inp["h"]
    ctx.tsdf_begin(**inp["vol"])
    try:
        for i, v in enumerate(views):
            if i > 0:
                ctx.fuse_begin(w, h, 2)
                try:
                    ctx.fuse_push_maps(v["depth"], v["f"], v["cx"], v["cy"], v["R"], v["t"], normal=v["normal"])
                    ctx.tsdf_raycast_push(views[i - 1], 0.0)
                    r = ctx.fuse_register(0, [1], iters=3)
                finally:
                    ctx.fuse_end()
                v["R"], v["t"] = r["R"].copy(), r["t"].copy()
            ctx.fuse_begin(w, h, 1)
            try:
                _push_maps(ctx, v)
                ctx.tsdf_integrate(0)
            finally:
                ctx.fuse_end()
            assert np.array_equal(got[i][:, :3], v["R"]) and np.array_equal(got[i][:, 3], v["t"]), i
    finally:
        ctx.tsdf_end()
    assert np.array_equal(got[0], inp["poses"][0])  # pair 0 keeps its pose
