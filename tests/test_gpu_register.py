"""Depth-view registration on the GPU (include/cspm.h "depth-view registration") held to tests/register_ref.py bit
for bit (the pose and every iteration record; NaN positions included, any NaN payload): cspm_register_depth_maps over the case table of
tests/register_cases.py, the convergence cases and the refused ones; cspm_fuse_register on pushed plane fields against the one-shot
entry on the maps cspm_reproject returns; apply, get_pose and set_pose through a following fusion; the error returns, untouched
outputs and the timing count."""
import ctypes as C
import math

import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref as fr
import geom_ref as gr
import register_cases as rc
import register_ref as rr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py)"""
    yield


def _same(got, want, what):
    for name, a, b in (("R", np.asarray(got["R"]).reshape(9), np.asarray(want["R"]).reshape(9)), ("t", np.asarray(got["t"]), np.asarray(want["t"]))):
        assert fr.same_bits(np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)), f"{what}: {name} differs: {a} != {b}"
    assert len(got["iters"]) == len(want["iters"]), what
    assert np.array_equal(got["iters"]["status"], want["iters"]["status"]), f"{what}: status {got['iters']['status']} != {want['iters']['status']}"
    for name in ("pairs", "cost", "rot2", "trans2"):
        a, b = np.ascontiguousarray(got["iters"][name]), np.ascontiguousarray(want["iters"][name])
        assert fr.same_bits(a, b), f"{what}: {name} differs: {a} != {b}"


@pytest.mark.parametrize("case", rc.CASES + rc.EXTRA, ids=repr)
def test_one_shot_entry_against_the_restatement(case):
    want = case.reference()
    got = capi.register_depth_maps(case.views(), case.w, case.h, rc.SRC, case.targets, **case.params)
    _same(got, want, case.name)


def test_the_device_converges_and_refuses_as_the_restatement_does():
    """the figures behind the bit-for-bit comparison, on the device's own result"""
    for case in rc.CONVERGE:
        v = case.views()
        got = capi.register_depth_maps(v, case.w, case.h, rc.SRC, case.targets, **case.params)
        rot0, tr0 = rc.pose_error(v[rc.SRC]["R"], v[rc.SRC]["t"])
        rot1, tr1 = rc.pose_error(got["R"], got["t"])
        assert rot1 <= rot0 / 20.0 and tr1 <= tr0 / 20.0 and np.all(got["iters"]["status"] == 0)
    case = rc.SINGLE_PLANE
    v = case.views()
    got = capi.register_depth_maps(v, case.w, case.h, rc.SRC, case.targets, **case.params)
    assert got["iters"]["status"][0] == 2 and np.array_equal(got["R"], v[rc.SRC]["R"]) and np.array_equal(got["t"], v[rc.SRC]["t"])


# ---- the context entries ---------------------------------------------------------------------------------------------------------------
W, H, MAX_DIS = 64, 48, 16
CAL = (60.0, 31.3, 23.8, 0.3, 1.5)  # f, cx, cy, baseline, doffs
POSES = [(np.eye(3), np.zeros(3)), rc.TRUE, (fc.rot(-2.0, 5.0, -6.0), np.array([-0.3, -0.05, -0.2]))]
# per push: pose, view, source, geometry parameters.  Slot 1 is the source of the registration.
PUSHES = [(0, 0, capi.GEOM_RAW, dict()), (1, 0, capi.GEOM_RAW, dict()), (2, 1, capi.GEOM_PP, dict(consistent_only=1)), (0, 1, capi.GEOM_RAW, dict(min_cos=0.3))]
WORLD = [fc.PLANE, rc.WALL, rc.FLOOR]


def _set_pose(ctx, k, rng):
    """the plane fields of both views of a pair whose view-0 camera has pose k: per pixel the nearest of the three world planes of the
    corner scene (the largest disparity), the field test_gpu_fuse.py sets for one plane; new images"""
    R, t = POSES[k]
    ctx.set_images(*[rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in (0, 1)])
    ctx.build_cost_grd(MAX_DIS, 9, 2, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    for v in (0, 1):
        maps = [gr.render_plane(CAL, v, W, H, R.T @ n, d - n @ t) for n, d in WORLD]
        D = np.stack([m[0] for m in maps])
        win = np.argmax(D, 0)[None]
        D, A, Bs = (np.take_along_axis(np.stack([m[i] for m in maps]), win, 0)[0] for i in range(3))
        planes = np.zeros((H, W, 6))
        ln = np.sqrt(A * A + Bs * Bs + 1.0)
        planes[..., 0], planes[..., 1], planes[..., 2] = -A / ln, -Bs / ln, 1.0 / ln
        planes[..., 3], planes[..., 4], planes[..., 5] = A, Bs, D - A * x - Bs * y
        ctx.set_planes(v, planes, np.zeros((H, W)))


def _view_from_reproject(ctx, k, view, source, params):
    R, t = POSES[k]
    g = ctx.reproject(view, CAL, source, cloud=False, **dict(params, left_frame=0))
    f, cx, cy, B, doffs = CAL
    return dict(depth=np.where(g["keep"] != 0, g["depth"], np.nan), normal=g["normal"], bgr=ctx.level_image(view, 0), f=f, cx=cx + view * doffs, cy=cy,
                R=R, t=t + (R[:, 0] * B if view == 1 else 0.0))


def _push_all(ctx, seed=1):
    rng = np.random.default_rng(seed)
    views, pose = [], None
    for k, view, source, params in PUSHES:
        if k != pose:
            _set_pose(ctx, k, rng)
            pose = k
        views.append(_view_from_reproject(ctx, k, view, source, params))
        ctx.fuse_push(view, CAL, POSES[k][0], POSES[k][1], source, **params)
    return views


@pytest.fixture()
def pushed(gpu_ctx):
    gpu_ctx.fuse_begin(W, H, len(PUSHES))
    try:
        yield gpu_ctx, _push_all(gpu_ctx)
    finally:
        gpu_ctx.enable_timing(False)
        gpu_ctx.fuse_end()


def test_context_entry_equals_the_one_shot_entry_and_the_restatement(pushed):
    ctx, views = pushed
    for targets, params in (([0, 2, 3], dict(iters=3)), ([0], dict(iters=3, stride=2, min_cos=0.9, min_pairs=20)), (0b1100, dict(iters=8, huber=0.0))):
        got = ctx.fuse_register(rc.SRC, targets, R0=rc.START[0], t0=rc.START[1], **params)
        started = [dict(v, R=rc.START[0], t=rc.START[1]) if k == rc.SRC else v for k, v in enumerate(views)]
        mask = capi._mask(targets).value
        want = rr.register(started, W, H, rc.SRC, mask, **dict(rr.DEFAULTS, **params))
        assert want["iters"]["pairs"][0] > 100 and want["iters"]["status"][0] == 0
        _same(got, want, f"context {params}")
        _same(capi.register_depth_maps(started, W, H, rc.SRC, targets, **params), got, f"one-shot {params}")
        R, t = ctx.fuse_get_pose(rc.SRC)
        assert np.array_equal(R, rc.TRUE[0]) and np.array_equal(t, rc.TRUE[1])  # without apply the slot keeps its pose
    own = ctx.fuse_register(rc.SRC, [0], iters=2)  # NULL R0, t0: the slot's own pose
    _same(own, rr.register(views, W, H, rc.SRC, 1, **dict(rr.DEFAULTS, iters=2)), "own pose")
    only_t = ctx.fuse_register(rc.SRC, [0], t0=rc.START[1], iters=2)
    _same(only_t, rr.register(views, W, H, rc.SRC, 1, t0=rc.START[1], **dict(rr.DEFAULTS, iters=2)), "t0 alone")


def test_apply_get_pose_set_pose_and_a_following_fusion(pushed):
    ctx, views = pushed
    before = ctx.fuse_run(min_views=1)
    _fuse_same(before, fr.fuse(views, W, H, min_views=1), "before")
    got = ctx.fuse_register(rc.SRC, [0, 2, 3], R0=rc.START[0], t0=rc.START[1], apply=True)
    R, t = ctx.fuse_get_pose(rc.SRC)
    assert np.array_equal(R, got["R"]) and np.array_equal(t, got["t"])
    assert not np.array_equal(R, rc.TRUE[0]) and rc.pose_error(R, t)[0] < rc.pose_error(*rc.START)[0] / 5.0
    refined = [dict(v, R=got["R"], t=got["t"]) if k == rc.SRC else v for k, v in enumerate(views)]
    _fuse_same(ctx.fuse_run(min_views=1), fr.fuse(refined, W, H, min_views=1), "after apply")
    again = ctx.fuse_register(rc.SRC, [0, 2, 3], iters=1)  # the slot's own pose is now the refined one
    _same(again, rr.register(refined, W, H, rc.SRC, 0b1101, **dict(rr.DEFAULTS, iters=1)), "from the applied pose")
    ctx.fuse_set_pose(rc.SRC, *rc.TRUE)
    R, t = ctx.fuse_get_pose(rc.SRC)
    assert np.array_equal(R, rc.TRUE[0]) and np.array_equal(t, rc.TRUE[1])
    _fuse_same(ctx.fuse_run(min_views=1), before, "after set_pose")
    for k in range(len(PUSHES)):
        R, t = ctx.fuse_get_pose(k)
        assert np.array_equal(R, views[k]["R"]) and np.array_equal(t, views[k]["t"])


def _fuse_same(got, want, what):
    assert got["count"] == want["count"] and np.array_equal(got["view_counts"], want["view_counts"]), what
    assert np.array_equal(got["state"], want["state"]), what
    for name in fr.POINT.names:
        assert fr.same_bits(got["cloud"][name], want["cloud"][name]), f"{what}: cloud field {name}"


def test_timing_count(pushed):
    ctx, _ = pushed
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_timing()
    ctx.fuse_register(rc.SRC, [0, 2, 3], iters=5, stride=3)
    t = ctx.timing()
    assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, 5 * 22 * 16 * 3) and t["post"]["launches"] == 0


def test_scratch_is_allocated_by_the_first_registration(pushed):
    ctx, _ = pushed
    ctx.synchronize()
    before = ctx.get_option(capi.OPT_DEVICE_BYTES)
    ctx.fuse_register(rc.SRC, [0], iters=1, stride=4)
    first = ctx.get_option(capi.OPT_DEVICE_BYTES)
    ctx.fuse_register(rc.SRC, [0, 2], iters=64, stride=1)
    assert first > before and ctx.get_option(capi.OPT_DEVICE_BYTES) == first


def _msg(ctx):
    return capi.load_library().cspm_last_error(ctx.p if ctx is not None else None).decode()


def _poison():
    return dict(R=np.frombuffer(bytes([0xAB]) * 72, np.float64).copy(), t=np.frombuffer(bytes([0xAB]) * 24, np.float64).copy(),
                iters=np.full(40 * 64, 0xAB, np.uint8).view(capi.REG_ITER))  # a view: a copy of padded records drops the padding


def _untouched(out, ref):
    return all(out[k].tobytes() == ref[k].tobytes() for k in ref)


BAD_PARAMS = [(dict(iters=0), "registration: iters must be in 1 .. 64"), (dict(iters=65), "registration: iters must be in 1 .. 64"),
              (dict(stride=0), "registration: stride must be at least 1"), (dict(max_dist=-1.0), "registration: max_dist must be >= 0"),
              (dict(max_dist=math.nan), "registration: max_dist must be >= 0"), (dict(huber=-0.5), "registration: huber must be >= 0"),
              (dict(huber=math.nan), "registration: huber must be >= 0"), (dict(min_cos=1.5), "registration: min_cos must be in [0, 1]"),
              (dict(min_cos=-0.1), "registration: min_cos must be in [0, 1]"), (dict(min_pairs=-1), "registration: min_pairs must be >= 0"),
              (dict(pivot_rel=1.0), "registration: pivot_rel must be in [0, 1)"), (dict(pivot_rel=-1e-9), "registration: pivot_rel must be in [0, 1)")]
BAD_MASK = "registration: the targets must be other views that exist, at least one"


def test_error_returns_leave_the_outputs_untouched():
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    out, ref = _poison(), _poison()
    dp = capi._dp
    eye, zero = np.eye(3).reshape(9), np.zeros(3)

    def reg(src=1, targets=0b01, p=None, R0=None, t0=None, apply=1):
        return L.cspm_fuse_register(ctx.p, src, targets, C.byref(p) if p is not None else None, dp(R0) if R0 is not None else None,
                                    dp(t0) if t0 is not None else None, apply, dp(out["R"]), dp(out["t"]), out["iters"].ctypes.data_as(C.POINTER(capi.RegIter)))

    try:
        assert reg() == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin first"
        assert L.cspm_fuse_get_pose(ctx.p, 0, dp(out["R"]), dp(out["t"])) == ERR_STATE and _msg(ctx) == "fusion: cspm_fuse_begin first"
        assert L.cspm_fuse_set_pose(ctx.p, 0, dp(eye), dp(zero)) == ERR_STATE
        ctx.fuse_begin(7, 5, 3)
        depth, normal = np.full((5, 7), 4.0), np.broadcast_to(np.array([0.0, 0.0, -1.0])[:, None, None], (3, 5, 7)).copy()
        assert reg() == ERR_ARG and _msg(ctx) == "registration: no such source view"  # no view yet
        for k in range(2):
            ctx.fuse_push_maps(depth, 6.0, 3.0, 2.0, eye, zero)
        assert reg() == ERR_STATE and _msg(ctx) == "registration: the views carry no normals"
        ctx.fuse_end()
        ctx.fuse_begin(7, 5, 3)
        for k in range(2):
            ctx.fuse_push_maps(depth, 6.0, 3.0, 2.0, eye, np.array([0.1 * k, 0.0, 0.0]), normal=normal)
        for bad, msg in BAD_PARAMS:
            assert reg(p=capi.reg_params(**bad)) == ERR_ARG and _msg(ctx) == msg, bad
        for src, targets, msg in ((-1, 1, "registration: no such source view"), (2, 1, "registration: no such source view"), (1, 0, BAD_MASK),
                                  (1, 0b10, BAD_MASK), (1, 0b11, BAD_MASK), (1, 0b101, BAD_MASK), (0, 1 << 63, BAD_MASK)):
            assert reg(src, targets) == ERR_ARG and _msg(ctx) == msg, (src, targets)
        assert reg(R0=eye * 1.00001) == ERR_ARG and _msg(ctx) == "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"
        assert reg(t0=np.array([0.0, math.inf, 0.0])) == ERR_ARG and _msg(ctx) == "fusion: the camera and its pose must be finite"
        assert L.cspm_fuse_get_pose(ctx.p, 2, dp(out["R"]), dp(out["t"])) == ERR_ARG and _msg(ctx) == "fusion: no such view"
        assert L.cspm_fuse_set_pose(ctx.p, -1, dp(eye), dp(zero)) == ERR_ARG and _msg(ctx) == "fusion: no such view"
        assert L.cspm_fuse_set_pose(ctx.p, 1, dp(eye * 2.0), dp(zero)) == ERR_ARG and _msg(ctx) == "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"
        assert L.cspm_fuse_set_pose(ctx.p, 1, None, dp(zero)) == ERR_ARG and _msg(ctx) == "fusion: no pose"
        assert _untouched(out, ref)  # no failed call wrote an output
        R, t = ctx.fuse_get_pose(1)
        assert np.array_equal(R, np.eye(3)) and np.array_equal(t, [0.1, 0.0, 0.0])  # nor applied anything
        assert L.cspm_fuse_register(ctx.p, 1, 1, None, None, None, 0, None, None, None) == 0  # every output may be NULL
        assert reg(apply=0) == 0 and not _untouched(out, ref)
        assert np.all(out["iters"]["status"][:8] == 1) and out["iters"][8:].tobytes() == ref["iters"][8:].tobytes()  # 35 samples: too few pairs
        assert L.cspm_reg_default_params(None) == ERR_ARG
    finally:
        ctx.close()


def test_one_shot_entry_errors_leave_the_outputs_untouched():
    case = rc.BY_NAME["7x5_s1_T3_c0.0"]
    views = case.views()
    out, ref = _poison(), _poison()
    for kw, msg in ((dict(src=4), "registration: no such source view"), (dict(targets=0b10), BAD_MASK), (dict(targets=0b10001), BAD_MASK),
                    (dict(iters=65), "registration: iters must be in 1 .. 64")):
        args = dict(src=rc.SRC, targets=case.targets)
        args.update(kw)
        with pytest.raises(capi.CspmError) as e:
            capi.register_depth_maps(views, 7, 5, args.pop("src"), args.pop("targets"), out=out, **args)
        assert str(e.value) == "cspm error -1: " + msg
        assert _untouched(out, ref)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
CLI_W, CLI_H, CLI_D, CLI_ITERS, CLI_SEED = 96, 64, 16, 1, 3
CLI_CAL = (90.0, 47.5, 31.5, 0.2, 0.0)
CLI_REG = dict(iters=4, stride=2, max_dist=2.0, huber=0.1)


def _cli_files(tmp_path):
    """three synthetic pairs as PNG files, the batch list and the calibration file -> (pairs, the flags every run shares)"""
    import os
    import pngio
    from crossscalepatchmatch_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, D, cal = CLI_W, CLI_H, CLI_D, CLI_CAL
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
    flags = [os.path.join(root, "crossscalepatchmatch_amd", "cspm_main"), f"--batch_list={tmp_path / 'list.txt'}", f"--calib={calib}",
             f"--fuse_ply={tmp_path / 'fused.ply'}", "--fuse_register", f"--fuse_poses_out={tmp_path / 'refined.txt'}", "--fuse_register_window=2",
             "--fuse_reg_iters=4", "--fuse_reg_stride=2", "--fuse_reg_max_dist=2", "--fuse_reg_huber=0.1", "--fuse_source=pp", "--fuse_min_views=1",
             "--fuse_max_reproj=3", "--geom_min_cos=0.2", f"--max_dis={D}", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3",
             f"--iters={CLI_ITERS}", f"--seed={CLI_SEED}", "--in_flight=2"]
    return pairs, flags


def _cli_push(ctx, pairs, poses, views):
    """the views the command line collects: every pair matched, its left (and right) view pushed with the pair's start pose"""
    for k, (l, r) in enumerate(pairs):
        ctx.set_images(l, r)
        ctx.build_cost_grd(CLI_D, 35, 5, 0.3)
        ctx.patchmatch(CLI_ITERS, seed=CLI_SEED)
        for v in range(views):
            ctx.fuse_push(v, CLI_CAL, poses[k][0], poses[k][1], capi.GEOM_PP, consistent_only=1, min_cos=0.2)


def _cli_compare(tmp_path, want_poses, want):
    written = np.array([[float(t) for t in ln.split()] for ln in open(tmp_path / "refined.txt")]).reshape(3, 3, 4)
    for k in range(3):
        assert np.array_equal(written[k][:, :3], want_poses[k][0]) and np.array_equal(written[k][:, 3], want_poses[k][1]), k
    cl = want["cloud"]
    head, _, body = open(tmp_path / "fused.ply", "rb").read().partition(b"end_header\n")
    assert f"element vertex {want['count']}\n".encode() in head
    pts = np.frombuffer(body, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))
    assert len(pts) == len(cl) and gr.same_bits(pts["p"], np.stack([cl["x"], cl["y"], cl["z"]], 1))
    return written


def test_cli_registers_a_batch_list(gpu_ctx, tmp_path):
    """cspm_main --batch_list --calib --fuse_poses --fuse_ply --fuse_register --fuse_poses_out on three pairs, starting from perturbed
    poses == the C-ABI path (cspm_fuse_push of every pair's left view with the file's pose, cspm_fuse_register with apply in list order,
    cspm_fuse_run) on the same files: the poses file to the last digit, the PLY's vertex count and positions"""
    import os
    import subprocess
    pairs, flags = _cli_files(tmp_path)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuse", "poses.txt")
    poses = np.array([[float(t) for t in ln.split("#")[0].split()] for ln in open(golden) if ln.split("#")[0].strip()]).reshape(3, 3, 4)
    start = poses.copy()
    for k, (ang, dt) in enumerate((((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.5, -0.4, 0.3), (0.02, -0.01, 0.015)), ((-0.3, 0.6, 0.2), (-0.015, 0.02, 0.01)))):
        start[k, :, :3] = fc.rot(*ang) @ poses[k, :, :3]
        start[k, :, 3] = poses[k, :, 3] + np.array(dt)
    (tmp_path / "start.txt").write_text("\n".join(" ".join(repr(float(x)) for x in p.ravel()) for p in start) + "\n")
    res = subprocess.run(flags + [f"--fuse_poses={tmp_path / 'start.txt'}"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Registration: 3 pairs" in res.stdout and "Fusion: 3 views" in res.stdout, res.stdout + res.stderr
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.fuse_begin(CLI_W, CLI_H, 3)
    try:
        _cli_push(ctx, pairs, [(p[:, :3], p[:, 3]) for p in start], 1)
        taken = 0
        for k in (1, 2):
            got = ctx.fuse_register(k, list(range(max(0, k - 2), k)), apply=True, **CLI_REG)
            taken += int(np.sum(got["iters"]["status"] == 0))
        assert taken > 0, "no step was taken: the comparison would be vacuous"
        want_poses = [ctx.fuse_get_pose(k) for k in range(3)]
        want = ctx.fuse_run(min_views=1, max_reproj=3.0)
    finally:
        ctx.fuse_end()
    written = _cli_compare(tmp_path, want_poses, want)
    assert np.array_equal(written[0], start[0]) and not np.array_equal(written[1], start[1])


def test_cli_registers_without_a_poses_file(gpu_ctx, tmp_path):
    """no --fuse_poses, --fuse_right: view 0 is the identity, pair i starts from pair i - 1's refined pose, a right view follows its left
    view by the baseline == the same chain through cspm_fuse_set_pose and cspm_fuse_register"""
    import subprocess
    pairs, flags = _cli_files(tmp_path)
    res = subprocess.run(flags + ["--fuse_right=true"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Registration: 3 pairs" in res.stdout and "Fusion: 6 views" in res.stdout, res.stdout + res.stderr
    B = CLI_CAL[3]
    ctx = gpu_ctx
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.fuse_begin(CLI_W, CLI_H, 6)
    try:
        _cli_push(ctx, pairs, [(np.eye(3), np.zeros(3))] * 3, 2)
        taken = 0
        for k in (1, 2):
            R, t = ctx.fuse_get_pose(2 * (k - 1))
            got = ctx.fuse_register(2 * k, [2 * j for j in range(max(0, k - 2), k)], R0=R, t0=t, apply=True, **CLI_REG)
            ctx.fuse_set_pose(2 * k + 1, got["R"], got["t"] + got["R"][:, 0] * B)
            taken += int(np.sum(got["iters"]["status"] == 0))
        assert taken > 0, "no step was taken: the comparison would be vacuous"
        want_poses = [ctx.fuse_get_pose(2 * k) for k in range(3)]
        want = ctx.fuse_run(min_views=1, max_reproj=3.0)
    finally:
        ctx.fuse_end()
    written = _cli_compare(tmp_path, want_poses, want)
    assert np.array_equal(written[0], np.hstack([np.eye(3), np.zeros((3, 1))]))
