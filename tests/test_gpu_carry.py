"""The plane-field carry on the GPU (include/cspm.h "plane-field carry") held to tests/carry_ref.py bit for bit:
cspm_carry_plane_field over the case table of tests/carry_cases.py -- records, state bytes and source map, nothing left out --,
cspm_carry_planes between two contexts against the restatement's candidates, tests/seed_ref.py's merge and tests/warm_ref.py's
iterations on the oracle, CSPatchMatch::PatchMatchCarried and cspm_main --carry_poses against the C ABI, the error returns, the timing
counts and the memory the entry keeps."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import carry_cases as cc
import carry_ref as cr
import crossscalepatchmatch_amd as cs
import seed_ref
import warm_ref
from crossscalepatchmatch_amd import capi
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = po.SUM_DEVICE
W, H, D = 96, 64, 16
KW = dict(seed=9, schedule=po.SCHED_RASTER, sum_order=DEV)


def _same_bits(got, want, what):
    """bit for bit, NaNs included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        gb, wb = (x.reshape(-1).view(np.uint8).reshape(x.size, x.itemsize) for x in (got, want))
        bad = np.flatnonzero((gb != wb).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at flat index {bad[0]}: {got.ravel()[bad[0]]!r} != "
                             f"{want.ravel()[bad[0]]!r}")


# ---- a. the one-shot entry over the case table -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cc.CASES, ids=repr)
def test_carry_equals_the_restatement(gpu_ctx, case):
    i, ref = case.inputs(), case.reference()
    got = capi.carry_plane_field(i["field"], i["calib_s"], i["view_s"], i["calib_t"], i["view_t"], i["w_t"], i["h_t"], i["max_dis"], i["R"], i["t"],
                                 mask=i["mask"], fill=i["fill"])
    _same_bits(got["state"], ref["state"], f"{case}: state")
    _same_bits(got["source"], ref["source"], f"{case}: source")
    _same_bits(got["planes"], ref["planes"], f"{case}: records")


def test_optional_outputs_and_the_param_part_alone_is_read(gpu_ctx):
    case = cc.BY_NAME["stretch_64x48_130x67"]
    i, ref = case.inputs(), case.reference()
    field = i["field"].copy()
    field[..., 0:3] = np.nan  # the norm part is not read
    L = cs.load_library()
    ks, kt, p = capi.calib_struct(i["calib_s"]), capi.calib_struct(i["calib_t"]), capi.carry_params(fill=i["fill"])
    R, t = capi._pose(i["R"], i["t"])
    planes = np.zeros((i["h_t"], i["w_t"], 6))
    args = [0, capi._dp(field), None, C.byref(ks), 0, 64, 48, C.byref(kt), 0, i["w_t"], i["h_t"], i["max_dis"], capi._dp(R), capi._dp(t)]
    assert L.cspm_carry_plane_field(*args, C.byref(p), capi._dp(planes), None, None) == 0
    _same_bits(planes, ref["planes"], "records alone")
    state = np.zeros((i["h_t"], i["w_t"]), np.uint8)
    assert L.cspm_carry_plane_field(*args, None, None, capi._u8(state), None) == 0  # NULL parameters: the defaults (fill = 1)
    _same_bits(state, ref["state"], "state alone")


# ---- b. between two contexts -------------------------------------------------------------------------------------------------------

def _lam(sn):
    return 0.3 if sn else 0.0


def _motion(fr):
    return cr.relative_pose(*fr["poses"][0], *fr["poses"][1])


@pytest.fixture(scope="module")
def src_ctx():
    ctx = cs.StereoContext(0)
    yield ctx
    ctx.close()


def _start(src_ctx, gpu_ctx, sn):
    """frame 0 matched in src_ctx, frame 1 set up in gpu_ctx with its random init; -> (frames, source fields, oracle pm, pc of frame 1)"""
    fr = cc.frames(W, H)
    src_ctx.set_images(*fr["pairs"][0])
    src_ctx.build_cost_grd(D, 35, sn, _lam(sn))
    src_ctx.patchmatch(1, seed=5)
    fields = [src_ctx.get_planes(v)[0] for v in (0, 1)]
    gpu_ctx.set_images(*fr["pairs"][1])
    gpu_ctx.build_cost_grd(D, 35, sn, _lam(sn))
    gpu_ctx.pm_init(seed=9)
    pc = po.PlaneCost(*fr["pairs"][1], D, 35, sn, _lam(sn), "GRD")
    pm = po.PatchMatch(*fr["pairs"][1], D, 4)
    pm.init(pc, seed=9, sum_order=DEV)
    return fr, fields, pm, pc


def _assert_state(ctx, pm, what):
    for v in (0, 1):
        npar, cost = ctx.get_planes(v)
        P = pm.planes(v)
        np.testing.assert_array_equal(npar[..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, pm.min_cost(v), err_msg=f"{what}: min_cost, view {v}")


@pytest.mark.parametrize("sn", [0, 3], ids=["ss", "cs3"])
def test_carry_planes_replace_merge_and_chain(src_ctx, gpu_ctx, sn):
    fr, fields, pm, pc = _start(src_ctx, gpu_ctx, sn)
    R, t = _motion(fr)
    cands, masks = cr.carry_fields(fields, fr["calib"], fr["calib"], R, t, W, H, D)
    assert all(0.5 < (m != 0).mean() < 1.0 and (m == 2).any() for m in masks)  # most of the frame is carried, some of it filled, some not
    # merge = 0: the field equals the candidates wherever S != 0 and the old field elsewhere
    old = [gpu_ctx.get_planes(v)[0] for v in (0, 1)]
    gpu_ctx.carry_planes_from(src_ctx, fr["calib"], fr["calib"], R, t, merge=False)
    for v in (0, 1):
        _same_bits(gpu_ctx.get_planes(v)[0], np.where((masks[v] != 0)[..., None], cands[v], old[v]), f"merge = 0, view {v}")
    # merge = 1 on the init field: seed_ref.merge of the restatement's candidates
    gpu_ctx.pm_init(seed=9)
    gpu_ctx.carry_planes_from(src_ctx, fr["calib"], fr["calib"], R, t, merge=True)
    taken = seed_ref.merge(pm, pc, cands, masks, DEV)
    assert 0 < taken < 2 * W * H
    _assert_state(gpu_ctx, pm, "merge = 1")
    # the chain: one warm iteration on top
    gpu_ctx.patchmatch_warm(1, seed=9)
    warm_ref.iterate(pm, pc, 1, **KW)
    _assert_state(gpu_ctx, pm, "init, carry, one warm iteration")


def test_carry_planes_between_sizes_and_after_a_stale_field(src_ctx, gpu_ctx):
    """a 64 x 48 source into the 96 x 64 target with another calibration; merge = 1 on a field that is not consistent re-scores it first"""
    fr = cc.frames(W, H)
    small = cc.frames(64, 48)
    src_ctx.set_images(*small["pairs"][0])
    src_ctx.build_cost_grd(12, 35, 0, 0.0)
    src_ctx.patchmatch(1, seed=5)
    fields = [src_ctx.get_planes(v)[0] for v in (0, 1)]
    gpu_ctx.set_images(*fr["pairs"][1])
    gpu_ctx.build_cost_grd(D, 35, 0, 0.0)
    pc = po.PlaneCost(*fr["pairs"][1], D, 35, 0, 0.0, "GRD")
    pm = po.PatchMatch(*fr["pairs"][1], D, 4)
    pm.init(pc, seed=3, sum_order=DEV)
    stale = [warm_ref.field_of(pm, v) for v in (0, 1)]
    for v in (0, 1):
        gpu_ctx.set_planes(v, stale[v], np.zeros((H, W)))  # the caller's costs: the field is not consistent
    R, t = _motion(fr)
    gpu_ctx.carry_planes_from(src_ctx, small["calib"], fr["calib"], R, t, merge=True, fill=0)
    cands, masks = cr.carry_fields(fields, small["calib"], fr["calib"], R, t, W, H, D, fill=0)
    assert all((m == 0).any() and (m == 1).any() and not (m == 2).any() for m in masks)
    warm_ref.rescore(pm, pc, DEV)
    seed_ref.merge(pm, pc, cands, masks, DEV)
    _assert_state(gpu_ctx, pm, "64x48 -> 96x64, fill = 0, after set_planes")


# ---- c. errors, timing, memory -----------------------------------------------------------------------------------------------------

def test_error_returns(src_ctx):
    fr = cc.frames(W, H)
    L = src_ctx.L
    cal, p = capi.calib_struct(fr["calib"]), capi.carry_params()
    R, t = capi._pose(*_motion(fr))
    src_ctx.set_images(*fr["pairs"][0])
    src_ctx.build_cost_grd(D, 35, 0, 0.0)
    src_ctx.pm_init(seed=1)
    call = lambda dst, src, merge, k=cal, RR=R, tt=t, par=p: L.cspm_carry_planes(dst, src, C.byref(k), C.byref(k), capi._dp(RR), capi._dp(tt), C.byref(par), merge)
    a, b = cs.StereoContext(0), cs.StereoContext(0)
    try:
        assert call(src_ctx.p, src_ctx.p, 1) == -1 and b"two different contexts" in L.cspm_last_error(src_ctx.p)  # CSPM_ERR_ARG = -1, CSPM_ERR_STATE = -3
        assert call(a.p, b.p, 0) == -3 and b"source context has no plane field" in L.cspm_last_error(a.p)
        assert call(a.p, src_ctx.p, 0) == -3 and b"cspm_set_images first" in L.cspm_last_error(a.p)
        a.set_images(*fr["pairs"][1])
        assert call(a.p, src_ctx.p, 1) == -3  # merge without a cost object
        assert call(a.p, src_ctx.p, 0) == -3  # no plane field
        a.set_planes(0, capi.disparity_planes(np.ones((H, W))), np.zeros((H, W)))
        assert call(a.p, src_ctx.p, 0) == -3 and b"max_dis" in L.cspm_last_error(a.p)
        a.build_cost_grd(D, 35, 0, 0.0)
        a.pm_init(seed=2)
        before = [a.get_planes(v) for v in (0, 1)]
        bad_cal = capi.calib_struct((0.0,) + tuple(fr["calib"][1:]))
        assert call(a.p, src_ctx.p, 1, k=bad_cal) == -1 and L.cspm_last_error(a.p) == b"carry: f and baseline must be positive"
        Rbad = R * 1.00001
        assert call(a.p, src_ctx.p, 1, RR=Rbad) == -1 and L.cspm_last_error(a.p) == b"carry: R is not a rotation (max |R R^T - I| > 1e-6)"
        tbad = np.array([0.0, math.nan, 0.0])
        assert call(a.p, src_ctx.p, 1, tt=tbad) == -1 and L.cspm_last_error(a.p) == b"carry: the motion must be finite"
        assert call(a.p, src_ctx.p, 1, par=capi.carry_params(fill=3)) == -1 and L.cspm_last_error(a.p) == b"carry: fill must be 0 or 1"
        assert L.cspm_carry_planes(a.p, src_ctx.p, C.byref(cal), C.byref(cal), None, capi._dp(t), None, 1) == -1
        for v in (0, 1):  # a refused call changed nothing
            for x, y in zip(before[v], a.get_planes(v)):
                np.testing.assert_array_equal(x, y)
        assert L.cspm_carry_planes(a.p, src_ctx.p, C.byref(cal), C.byref(cal), capi._dp(R), capi._dp(t), None, 1) == 0  # NULL parameters: the defaults
        assert call(a.p, src_ctx.p, 0) == 0
        a.synchronize()
    finally:
        a.close()
        b.close()


def test_carry_is_timed_as_misc_and_its_merge_as_init(src_ctx, gpu_ctx):
    fr, _, _, _ = _start(src_ctx, gpu_ctx, 0)
    R, t = _motion(fr)
    n = W * H
    gpu_ctx.synchronize()
    gpu_ctx.enable_timing(True)
    try:
        gpu_ctx.reset_timing()
        gpu_ctx.carry_planes_from(src_ctx, fr["calib"], fr["calib"], R, t, merge=False)  # one bracket per view; the field is stale afterwards
        gpu_ctx.carry_planes_from(src_ctx, fr["calib"], fr["calib"], R, t, merge=True)   # a re-score (one launch, 2n), one bracket and one merge per view
        gpu_ctx.synchronize()
        tm = gpu_ctx.timing()
    finally:
        gpu_ctx.enable_timing(False)
    assert tm["misc"]["launches"] == 4 and tm["misc"]["evals"] == 4 * n
    assert tm["init"]["launches"] == 3 and tm["init"]["evals"] == 4 * n
    assert all(tm[k]["launches"] == 0 for k in ("spatial", "view", "refine", "grd", "post"))


def test_device_bytes_grow_by_the_keys_and_winners_once(src_ctx):
    fr = cc.frames(W, H)
    R, t = _motion(fr)
    src_ctx.set_images(*fr["pairs"][0])
    src_ctx.build_cost_grd(D, 35, 0, 0.0)
    src_ctx.pm_init(seed=1)
    a = cs.StereoContext(0)
    try:
        a.set_images(*cc.frames(77, 41)["pairs"][1])  # an odd number of pixels
        a.build_cost_grd(D, 35, 0, 0.0)
        a.pm_init(seed=2)
        small = cc.frames(77, 41)["calib"]
        b0, s0 = a.get_option(capi.OPT_DEVICE_BYTES), src_ctx.get_option(capi.OPT_DEVICE_BYTES)
        a.carry_planes_from(src_ctx, fr["calib"], small, R, t, merge=False)
        b1 = a.get_option(capi.OPT_DEVICE_BYTES)
        assert b1 - b0 == 12 * 77 * 41
        a.carry_planes_from(src_ctx, fr["calib"], small, R, t, merge=False, fill=0)
        assert a.get_option(capi.OPT_DEVICE_BYTES) == b1 and src_ctx.get_option(capi.OPT_DEVICE_BYTES) == s0  # kept; the source holds nothing new
        a.carry_planes_from(src_ctx, fr["calib"], small, R, t, merge=True)
        b2 = a.get_option(capi.OPT_DEVICE_BYTES)
        assert b2 - b1 == 8 * (6 * 77 * 41 + (77 * 41 + 7) // 8)  # the shared candidate buffer, as any merging entry allocates it
        a.carry_planes_from(src_ctx, fr["calib"], small, R, t, merge=True)
        assert a.get_option(capi.OPT_DEVICE_BYTES) == b2
        a.synchronize()
    finally:
        a.close()


# ---- d. host layer and command line ------------------------------------------------------------------------------------------------

def _c_abi_chain(src_ctx, gpu_ctx, fr, sn, iters0, iters, seed=12345):
    src_ctx.set_images(*fr["pairs"][0])
    src_ctx.build_cost_grd(D, 35, sn, _lam(sn))
    src_ctx.patchmatch(iters0, seed=seed)
    gpu_ctx.set_images(*fr["pairs"][1])
    gpu_ctx.build_cost_grd(D, 35, sn, _lam(sn))
    gpu_ctx.pm_init(seed=seed)
    R, t = capi.carry_relative_pose(*fr["poses"][0], *fr["poses"][1])
    gpu_ctx.carry_planes_from(src_ctx, fr["calib"], fr["calib"], R, t, merge=True)
    gpu_ctx.patchmatch_warm(iters, seed=seed)
    return R, t


def test_host_layer_carried_start_equals_the_c_abi(src_ctx, gpu_ctx, tmp_path):
    """tests/helpers/carry_check.cc: PatchMatch on frame 0, PatchMatchCarried on frame 1"""
    exe = _build_helper("carry_check")
    fr = cc.frames(W, H)
    sn, iters0, iters = 3, 1, 1
    R, t = _c_abi_chain(src_ctx, gpu_ctx, fr, sn, iters0, iters)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([W, H, D, sn, iters0, iters], np.int32).tobytes())
        f.write(np.array(list(fr["calib"]) + list(R.ravel()) + list(t), np.float64).tobytes())
        for pair in fr["pairs"]:
            for img in pair:
                f.write(np.ascontiguousarray(img).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"foreign refused") == 1 and out.stdout.count(b"no run refused") == 1
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = W * H
    assert raw.size == 2 * 7 * n
    for v in (0, 1):
        npar, cost = gpu_ctx.get_planes(v)
        np.testing.assert_array_equal(raw[v * 7 * n:][:6 * n].reshape(H, W, 6), npar, err_msg=f"PatchMatchCarried: planes, view {v}")
        np.testing.assert_array_equal(raw[v * 7 * n + 6 * n:][:n].reshape(H, W), cost, err_msg=f"PatchMatchCarried: min_cost, view {v}")


def test_cli_carry_poses_equals_the_c_abi(src_ctx, gpu_ctx, tmp_path):
    """cspm_main --carry_poses over the two frames (five levels, as the command line builds them): pair 0 is the cold run, pair 1 the
    carried start; --carry_iters=0 leaves the merged field as it is"""
    from PIL import Image
    fr = cc.frames(W, H)
    f, cx, cy, B, doffs = fr["calib"]
    (tmp_path / "calib.txt").write_text(f"cam0=[{f!r} 0 {cx!r}; 0 {f!r} {cy!r}; 0 0 1]\ncam1=[{f!r} 0 {cx + doffs!r}; 0 {f!r} {cy!r}; 0 0 1]\n"
                                        f"doffs={doffs!r}\nbaseline={B!r}\nwidth={W}\nheight={H}\nndisp={D}\n")
    (tmp_path / "poses.txt").write_text("".join(" ".join(f"{x:.17g}" for x in np.concatenate([Rk, tk[:, None]], 1).ravel()) + "\n" for Rk, tk in fr["poses"]))
    lines = []
    for k, pair in enumerate(fr["pairs"]):
        for name, img in zip("lr", pair):
            Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(tmp_path / f"{name}{k}.png")
        lines.append(f"{tmp_path}/l{k}.png {tmp_path}/r{k}.png {tmp_path}/ld{k}.png {tmp_path}/rd{k}.png")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    cli = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    base = [cli, f"--batch_list={tmp_path}/list.txt", f"--calib={tmp_path}/calib.txt", f"--carry_poses={tmp_path}/poses.txt", f"--max_dis={D}",
            "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--iters=1", "--in_flight=3"]
    for carry_iters in (1, 0):
        out = subprocess.run(base + [f"--carry_iters={carry_iters}"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.count("--in_flight does not apply") == 1 and "2 pairs" in out.stdout and "0 failed" in out.stdout
        _c_abi_chain(src_ctx, gpu_ctx, fr, 5, 1, carry_iters)
        for k, ctx in ((0, src_ctx), (1, gpu_ctx)):
            for v, name in enumerate(("ld", "rd")):
                got = np.asarray(Image.open(tmp_path / f"{name}{k}.png").convert("L"))
                np.testing.assert_array_equal(got, ctx.disparity_u8(v, 4), err_msg=f"--carry_iters={carry_iters}: pair {k}, view {v}")
