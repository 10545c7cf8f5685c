"""Depth-map fusion on the GPU (include/cspm.h "depth-map fusion") held to tests/fuse_ref.py bit for bit (NaN
positions included, any NaN payload): cspm_fuse_depth_maps over the case table of tests/fuse_cases.py; the context entries on plane
fields set for several poses (RAW, PP, fit, consistent_only, view 1) against the one-shot entry on the maps cspm_reproject returns and
against the restatement; a real PatchMatch run; repeated runs, the device variant, the error returns, untouched outputs, the timing
count, and that a context behaves the same with and without fusion views."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref as fr
import geom_ref as gr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py)"""
    yield


def _same(got, want, what, cap=None):
    assert got["count"] == want["count"], f"{what}: count {got['count']} != {want['count']}"
    assert np.array_equal(got["view_counts"], want["view_counts"]), f"{what}: view counts {got['view_counts']} != {want['view_counts']}"
    if "state" in got:
        assert np.array_equal(got["state"], want["state"]), f"{what}: S differs in {np.sum(got['state'] != want['state'])} places"
    if "cloud" in got:
        ref = want["cloud"] if cap is None else want["cloud"][:cap]
        assert len(got["cloud"]) == len(ref), f"{what}: {len(got['cloud'])} records, {len(ref)} expected"
        for name in fr.POINT.names:
            assert fr.same_bits(got["cloud"][name], ref[name]), f"{what}: cloud field {name} differs in {np.sum(got['cloud'][name] != ref[name])} records"


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_one_shot_entry_against_the_restatement(case):
    want = case.reference()
    cap = case.capacity()
    poison = np.frombuffer(bytes([0xAB]) * (32 * (cap + 3)), capi.Point).copy()
    got = capi.fuse_depth_maps(case.views(), case.w, case.h, cloud_cap=cap, out={"cloud_buffer": poison}, **case.params)
    _same(got, want, case.name, cap)
    assert np.all(poison[min(cap, want["count"]):].view(np.uint8) == 0xAB), "records beyond the capacity or the count were written"


def test_counts_only_and_capacities():
    case = fc.BY_NAME["130x67_K3_combo0"]
    want = case.reference()
    views = case.views()
    only = capi.fuse_depth_maps(views, case.w, case.h, cloud=False, state=False, **case.params)
    assert only["count"] == want["count"] and np.array_equal(only["view_counts"], want["view_counts"]) and "cloud" not in only
    a = int(want["view_counts"][0])
    for cap in (1, 63, 64, 257, a - 1, a, a + 1, want["count"] + 100):
        poison = np.frombuffer(bytes([0x5A]) * (32 * cap), capi.Point).copy()
        got = capi.fuse_depth_maps(views, case.w, case.h, cloud_cap=cap, state=False, out={"cloud_buffer": poison}, **case.params)
        _same(got, want, f"cap {cap}", cap)
        assert np.all(poison[min(cap, want["count"]):].view(np.uint8) == 0x5A), cap


# ---- the context entries ---------------------------------------------------------------------------------------------------------------
W, H, MAX_DIS = 64, 48, 16
CAL = (60.0, 31.3, 23.8, 0.3, 1.5)  # f, cx, cy, baseline, doffs
POSES = [(np.eye(3), np.zeros(3)), (fc.rot(1.0, -4.0, 3.0), np.array([0.25, 0.03, 0.1])), (fc.rot(-2.0, 5.0, -6.0), np.array([-0.3, -0.05, -0.2]))]
# per push: pose, view, source, fit, geometry parameters
PUSHES = [(0, 0, capi.GEOM_RAW, None, dict()),
          (0, 1, capi.GEOM_RAW, None, dict(min_cos=0.5)),
          (1, 0, capi.GEOM_PP, None, dict(consistent_only=1)),
          (1, 1, capi.GEOM_PP, None, dict(z_near=1.0, z_far=4.4, left_frame=1)),
          (2, 0, capi.GEOM_RAW, dict(radius=2, max_diff=1.5, min_support=6, use_guide=1), dict()),
          (2, 1, capi.GEOM_PP, dict(radius=2), dict(consistent_only=1))]


def _set_pose(ctx, k, rng):
    """the plane fields of both views of a pair whose view-0 camera has pose k, the world plane of fuse_cases seen from there; new images"""
    R, t = POSES[k]
    n, d = fc.PLANE
    m, hh = R.T @ n, d - n @ t  # the plane in the frame of the pair's view-0 camera
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in (0, 1)]
    ctx.set_images(*imgs)
    ctx.build_cost_grd(MAX_DIS, 9, 2, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    for v in (0, 1):
        D, A, Bs = gr.render_plane(CAL, v, W, H, m, hh)
        D = D + (0.75 if v == 0 else 0.0) * ((x > 40) & (y > 30))  # a patch where the two views disagree: the left-right check has work
        planes = np.zeros((H, W, 6))
        ln = np.sqrt(A * A + Bs * Bs + 1.0)
        planes[..., 0], planes[..., 1], planes[..., 2] = -A / ln, -Bs / ln, 1.0 / ln
        planes[..., 3], planes[..., 4], planes[..., 5] = A, Bs, D - A * x - Bs * y
        ctx.set_planes(v, planes, np.zeros((H, W)))


def _view_from_reproject(ctx, k, view, source, fit, params):
    """the fusion view cspm_fuse_push must have stored, rebuilt on the host from what cspm_reproject returns for the same settings"""
    R, t = POSES[k]
    g = ctx.reproject(view, CAL, source, fit=fit, cloud=False, **dict(params, left_frame=0))
    depth = np.where(g["keep"] != 0, g["depth"], np.nan)
    f, cx, cy, B, doffs = CAL
    return dict(depth=depth, normal=g["normal"], bgr=ctx.level_image(view, 0), f=f, cx=cx + view * doffs, cy=cy, R=R,
                t=t + (R[:, 0] * B if view == 1 else 0.0))


def _push_all(ctx, pushes, seed=1):
    rng = np.random.default_rng(seed)
    views, pose = [], None
    for k, view, source, fit, params in pushes:
        if k != pose:
            _set_pose(ctx, k, rng)
            pose = k
        views.append(_view_from_reproject(ctx, k, view, source, fit, params))
        ctx.fuse_push(view, CAL, POSES[k][0], POSES[k][1], source, fit=fit, **params)
    return views


def test_context_pushes_equal_the_one_shot_entry_and_the_restatement(gpu_ctx):
    ctx = gpu_ctx
    ctx.fuse_begin(W, H, len(PUSHES))
    try:
        views = _push_all(ctx, PUSHES)
        assert ctx.fuse_view_count() == len(PUSHES)
        for params in (dict(), dict(min_views=1, min_cos=0.9, suppress=0), dict(min_views=3, max_reproj=1.0)):
            got = ctx.fuse_run(**params)
            want = fr.fuse(views, W, H, **params)
            assert 0 < want["count"] < len(views) * W * H
            _same(got, want, f"context {params}")
            _same(capi.fuse_depth_maps(views, W, H, **params), got, f"one-shot {params}")
    finally:
        ctx.fuse_end()


def test_run_again_and_after_a_further_push(gpu_ctx):
    ctx = gpu_ctx
    ctx.fuse_begin(W, H, 4)
    try:
        views = _push_all(ctx, PUSHES[:3], seed=2)
        first = ctx.fuse_run(min_views=1)
        _same(first, fr.fuse(views, W, H, min_views=1), "first run")
        _same(ctx.fuse_run(min_views=2, suppress=0), fr.fuse(views, W, H, min_views=2, suppress=0), "second run, other parameters")
        _same(ctx.fuse_run(min_views=1), first, "the first parameters again")
        depth = np.full((H, W), 4.0)
        extra = dict(depth=depth, normal=np.broadcast_to(np.array([0.0, 0.0, -1.0])[:, None, None], (3, H, W)).copy(), bgr=None, f=55.0, cx=30.0, cy=20.0,
                     R=fc.rot(ry=3.0), t=np.array([0.1, 0.0, 0.0]))
        ctx.fuse_push_maps(extra["depth"], extra["f"], extra["cx"], extra["cy"], extra["R"], extra["t"], normal=extra["normal"])
        views.append({k: v for k, v in extra.items() if v is not None})
        _same(ctx.fuse_run(min_views=1), fr.fuse(views, W, H, min_views=1), "after a further push")
        _same(ctx.fuse_run(min_views=1), capi.fuse_depth_maps(views, W, H, min_views=1), "a fresh fusion")
    finally:
        ctx.fuse_end()


def test_real_run_both_views(gpu_ctx, mid_pair):
    """the 96 x 64 pipeline pair after one PatchMatch iteration, both views pushed"""
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
        got = ctx.fuse_run(min_views=1)
        want = fr.fuse(views, w, h, min_views=1)
        assert 100 < want["count"] < 2 * w * h
        _same(got, want, "real run")
    finally:
        ctx.fuse_end()


def test_device_variant_equals_host_variant(gpu_ctx):
    import torch
    ctx = gpu_ctx
    ctx.fuse_begin(W, H, 3)
    try:
        _push_all(ctx, PUSHES[:3], seed=3)
        want = ctx.fuse_run(min_views=1)
        K, n = 3, W * H
        cloud = torch.zeros((K * n, 32), dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        vcounts = torch.full((K,), 7, dtype=torch.int32, device="cuda")
        state = torch.full((K, H, W), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.fuse_run_device(d_cloud=cloud.data_ptr(), cloud_cap=K * n, d_count=count.data_ptr(), d_view_counts=vcounts.data_ptr(), d_state=state.data_ptr(),
                            min_views=1)
        ctx.synchronize()
        got = dict(count=int(count.item()), view_counts=vcounts.cpu().numpy().astype(np.uint32), state=state.cpu().numpy())
        got["cloud"] = cloud.cpu().numpy().view(capi.Point).reshape(-1)[:got["count"]]
        _same(got, want, "device variant")
        count.zero_()
        torch.cuda.synchronize()
        ctx.fuse_run_device(d_count=count.data_ptr(), min_views=1)  # the count alone
        ctx.synchronize()
        assert int(count.item()) == want["count"]
        L = capi.load_library()
        assert L.cspm_fuse_run_device(ctx.p, None, C.c_void_p(cloud.data_ptr() + 8), 4, None, None, None) == ERR_ARG
        assert L.cspm_last_error(ctx.p).decode() == "fusion: the cloud buffer must be 16-byte aligned"
        assert L.cspm_fuse_run_device(ctx.p, None, None, 0, C.c_void_p(count.data_ptr() + 2), None, None) == ERR_ARG
        assert L.cspm_last_error(ctx.p).decode() == "fusion: the counts must be 4-byte aligned"
    finally:
        ctx.fuse_end()


def test_timing_count(gpu_ctx):
    ctx = gpu_ctx
    ctx.fuse_begin(W, H, 3)
    try:
        _push_all(ctx, PUSHES[:3], seed=4)
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.reset_timing()
        ctx.fuse_run()
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, 3 * W * H) and t["post"]["launches"] == 0
    finally:
        ctx.enable_timing(False)
        ctx.fuse_end()


def _msg(ctx):
    return capi.load_library().cspm_last_error(ctx.p if ctx is not None else None).decode()


def test_error_returns_of_the_context_entries():
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    eye, zero = np.eye(3).reshape(9), np.zeros(3)
    depth = np.full((H, W), 4.0)
    normal = np.zeros((3, H, W))
    k = capi.calib_struct(CAL)
    cnt = C.c_uint(0xABABABAB)
    dp = capi._dp

    def push_maps(d=depth, nrm=None, bgr=None, stride=0, f=50.0, R=eye, t=zero):
        return L.cspm_fuse_push_maps(ctx.p, dp(d) if d is not None else None, dp(nrm) if nrm is not None else None, capi._u8(bgr) if bgr is not None else None,
                                     stride, f, 30.0, 20.0, dp(R) if R is not None else None, dp(t) if t is not None else None)

    def push(view=0, R=eye, t=zero):
        return L.cspm_fuse_push(ctx.p, view, capi.GEOM_RAW, C.byref(k), None, None, dp(R), dp(t))

    def run(p=None):
        return L.cspm_fuse_run(ctx.p, C.byref(p) if p is not None else None, None, 0, C.byref(cnt), None, None)

    try:
        for call in (push_maps, run, lambda: L.cspm_fuse_end(ctx.p)):
            assert call() == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin first"
        assert L.cspm_fuse_view_count(ctx.p) == -1
        for w, h, mv, msg in ((0, H, 2, "fusion: w and h must be at least 1"), (W, -1, 2, "fusion: w and h must be at least 1"),
                              (65536, 32768, 2, "w * h must be below 2^31: cloud records hold 32-bit pixel indices"),
                              (W, H, 0, "fusion: max_views must be in 1 .. 64"), (W, H, 65, "fusion: max_views must be in 1 .. 64")):
            assert L.cspm_fuse_begin(ctx.p, w, h, mv) == ERR_ARG and _msg(ctx) == msg
        assert L.cspm_fuse_begin(ctx.p, W, H, 2) == 0
        assert L.cspm_fuse_begin(ctx.p, W, H, 2) == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin twice without cspm_fuse_end"
        assert run() == ERR_STATE and _msg(ctx) == "fusion: no view has been pushed"
        assert push_maps(d=None) == ERR_ARG and _msg(ctx) == "fusion: no depth map"
        assert push_maps(f=0.0) == ERR_ARG and _msg(ctx) == "fusion: f must be positive"
        assert push_maps(f=math.inf) == ERR_ARG and _msg(ctx) == "fusion: the camera and its pose must be finite"
        assert push_maps(t=np.array([0.0, math.nan, 0.0])) == ERR_ARG and _msg(ctx) == "fusion: the camera and its pose must be finite"
        assert push_maps(R=None) == ERR_ARG and _msg(ctx) == "fusion: no pose"
        assert push_maps(R=eye * 1.00001) == ERR_ARG and _msg(ctx) == "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"
        assert push_maps(R=eye * (1.0 + 1e-8)) == 0  # within the tolerance
        assert L.cspm_fuse_view_count(ctx.p) == 1
        assert push_maps(nrm=normal) == ERR_ARG and _msg(ctx) == "fusion: normals in some views but not all"
        img = np.zeros((H, W, 3), np.uint8)
        assert push_maps(bgr=img, stride=3 * W - 1) == ERR_ARG and _msg(ctx) == "fusion: bgr_stride is below 3 * w"
        for bad, msg in ((dict(max_reproj=-1.0), "fusion: max_reproj must be >= 0"), (dict(max_reproj=math.nan), "fusion: max_reproj must be >= 0"),
                         (dict(max_rel_depth=-0.5), "fusion: max_rel_depth must be >= 0"), (dict(max_rel_depth=math.nan), "fusion: max_rel_depth must be >= 0"),
                         (dict(min_cos=1.5), "fusion: min_cos must be in [0, 1]"), (dict(min_cos=-0.1), "fusion: min_cos must be in [0, 1]"),
                         (dict(min_views=-1), "fusion: min_views must be in 0 .. 63"), (dict(min_views=64), "fusion: min_views must be in 0 .. 63")):
            assert run(capi.fuse_params(**bad)) == ERR_ARG and _msg(ctx) == msg
        assert cnt.value == 0xABABABAB  # no failed call wrote its output
        assert run() == 0 and cnt.value == 0  # one view, min_views 2
        # the stored-field push: the state errors of the reprojection, then its own
        assert push() == ERR_STATE and _msg(ctx) == "cspm_set_images first"
        ctx.set_images(np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8))
        assert push() == ERR_STATE and _msg(ctx).startswith("no plane field to reproject")
        for v in (0, 1):
            ctx.set_planes(v, capi.disparity_planes(np.full((H, W), 4.0)), np.zeros((H, W)))
        assert push(view=2) == ERR_ARG and _msg(ctx) == "reprojection: view must be 0 or 1"
        assert push(R=eye * 2.0) == ERR_ARG and _msg(ctx) == "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"
        assert push() == ERR_ARG and _msg(ctx) == "fusion: normals in some views but not all"  # the first view came without normals
        assert L.cspm_fuse_end(ctx.p) == 0 and L.cspm_fuse_begin(ctx.p, W + 1, H, 1) == 0
        assert push() == ERR_STATE and _msg(ctx) == "fusion: the context's images are not of the size given to cspm_fuse_begin"
        assert L.cspm_fuse_end(ctx.p) == 0 and L.cspm_fuse_begin(ctx.p, W, H, 1) == 0
        assert push(view=1) == 0
        assert push() == ERR_STATE and push_maps() == ERR_STATE and _msg(ctx) == "fusion: every view slot is taken (max_views of cspm_fuse_begin)"
        assert run(capi.fuse_params(min_views=0)) == 0 and cnt.value == W * H
        ctx.synchronize()
    finally:
        ctx.close()  # with the views still there: cspm_destroy frees them


def test_one_shot_entry_overruns_and_errors():
    """65 views overrun CSPM_FUSE_MAX_VIEWS; every refused call leaves its outputs as they were"""
    case = fc.BY_NAME["7x5_K5_s1v2c0.0"]
    views = case.views()
    out = dict(cloud_buffer=np.frombuffer(bytes([0xAB]) * (32 * 40), capi.Point).copy(), state=np.full((65, 5, 7), 0xAB, np.uint8),
               view_counts=np.full(65, 0xABABABAB, np.uint32))
    for bad, msg in (((views * 13), "fusion: the number of views must be in 1 .. 64"), ([], "fusion: the number of views must be in 1 .. 64"),
                     ([views[0], dict(views[1], f=-1.0)], "fusion: f must be positive"),
                     ([views[0], {k: v for k, v in views[1].items() if k != "normal"}], "fusion: normals in some views but not all")):
        with pytest.raises(capi.CspmError, match=re.escape("cspm error -1: " + msg)):
            capi.fuse_depth_maps(bad, 7, 5, cloud_cap=40, out=out)
        assert all(np.all(a.view(np.uint8) == 0xAB) for a in out.values())
    with pytest.raises(capi.CspmError, match="max_views"):  # a context's slots overrun
        ctx = capi.StereoContext(0)
        try:
            ctx.fuse_begin(7, 5, 2)
            for v in views[:3]:
                ctx.fuse_push_maps(v["depth"], v["f"], v["cx"], v["cy"], v["R"], v["t"], normal=v["normal"], bgr=v["bgr"])
        finally:
            ctx.close()


def test_a_context_without_pushes_computes_the_same(small_pair):
    """the feature unused: planes and maps of a run are byte-identical with and without cspm_fuse_begin / cspm_fuse_end around it"""
    res = []
    for fusion in (False, True):
        ctx = capi.StereoContext(0)
        try:
            if fusion:
                ctx.fuse_begin(small_pair["w"], small_pair["h"], 4)
            ctx.set_images(small_pair["l"], small_pair["r"])
            ctx.build_cost_grd(small_pair["max_dis"], 9, 3, 0.3)
            ctx.patchmatch(2, seed=7)
            planes = [ctx.get_planes(v) for v in (0, 1)]
            maps = ctx.postprocess_f64(valid=True)
            geo = ctx.reproject(0, (60.0, 31.0, 23.0, 0.3, 0.0))
            if fusion:
                assert ctx.get_option(capi.OPT_DEVICE_BYTES) > 0
                ctx.fuse_end()
            res.append((planes, maps, geo))
        finally:
            ctx.close()
    (pa, ma, ga), (pb, mb, gb) = res
    for v in (0, 1):
        assert pa[v][0].tobytes() == pb[v][0].tobytes() and pa[v][1].tobytes() == pb[v][1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ma, mb))
    assert ga["depth"].tobytes() == gb["depth"].tobytes() and ga["cloud"].tobytes() == gb["cloud"].tobytes()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_fuses_a_batch_list(gpu_ctx, tmp_path):
    """cspm_main --batch_list --calib --fuse_poses --fuse_ply on three pairs == the C-ABI path (cspm_fuse_push of both views of every
    pair, cspm_fuse_run) on the same files: the PLY's vertex count and bytes"""
    import pngio
    from crossscalepatchmatch_amd import synth
    w, h, D, iters, seed = 96, 64, 16, 1, 3
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
    golden = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")
    poses = np.array([[float(t) for t in ln.split("#")[0].split()] for ln in open(golden) if ln.split("#")[0].strip()]).reshape(3, 3, 4)
    ply = tmp_path / "fused.ply"
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    res = subprocess.run([main, f"--batch_list={tmp_path / 'list.txt'}", f"--calib={calib}", f"--fuse_poses={golden}", f"--fuse_ply={ply}", "--fuse_right=true",
                          "--fuse_source=pp", "--fuse_min_views=1", "--fuse_max_reproj=3", "--geom_min_cos=0.2", f"--max_dis={D}", "--dis_scale=4",
                          "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", f"--iters={iters}", f"--seed={seed}", "--in_flight=2"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Fusion: 6 views" in res.stdout, res.stdout + res.stderr
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.fuse_begin(w, h, 6)
    try:
        for k, (l, r) in enumerate(pairs):
            ctx.set_images(l, r)
            ctx.build_cost_grd(D, 35, 5, 0.3)
            ctx.patchmatch(iters, seed=seed)
            for v in (0, 1):
                ctx.fuse_push(v, cal, poses[k][:, :3], poses[k][:, 3], capi.GEOM_PP, consistent_only=1, min_cos=0.2)
        want = ctx.fuse_run(min_views=1, max_reproj=3.0)
    finally:
        ctx.fuse_end()
    cl = want["cloud"]
    assert 1000 < len(cl) < 6 * w * h
    head, _, body = open(ply, "rb").read().partition(b"end_header\n")
    assert f"element vertex {want['count']}\n".encode() in head
    rec = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    pts = np.frombuffer(body, rec)
    assert len(pts) == len(cl)
    assert gr.same_bits(pts["p"], np.stack([cl["x"], cl["y"], cl["z"]], 1))
    nrm = np.stack([cl["nx"], cl["ny"], cl["nz"]], 1)
    nrm[np.isnan(nrm).any(1)] = 0.0
    assert gr.same_bits(pts["n"], nrm)
    np.testing.assert_array_equal(pts["rgb"], np.stack([cl["r"], cl["g"], cl["b"]], 1))
