"""-m gpu: fused CENGRD cells (CSPM_OPT_CENGRD_FUSED, the kSrcCenGrd source of both tap engines) against the CPU restatement
tests/cengrd_ref.py and against volume-sourced builds of the same inputs, bit for bit: option state, cells through
cspm_get_cost_slab, cspm_plane_cost_batch, PatchMatch phase by phase under all three schedules, whole runs with maps and both
post-processings, window sizes 9 and 45, the row engine on both sides of its strip capacity, local stereo and a warm run, cost
switches on one context, the command line and the C++ host class.  tests/test_cengrd_fused_inputs.py checks on the CPU that the
inputs built here cover what they claim.  Every comparison is assert_array_equal."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import cengrd_fused_cases as cases
import cengrd_ref
import diffuse_ref
import pngio
import pp_sub_ref
from conftest import random_planes
from crossscalepatchmatch_amd import capi
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crossscalepatchmatch_amd")
DIS_SCALE = 4
RASTER, REDBLACK, DIFFUSE = po.SCHED_RASTER, po.SCHED_REDBLACK, capi.SCHED_DIFFUSE


@pytest.fixture
def fused_ctx(gpu_ctx):
    """the session's context; CSPM_OPT_CENGRD_FUSED is back at 0 afterwards, so that no later test inherits it"""
    gpu_ctx.set_option(capi.OPT_CENGRD_FUSED, 0)
    yield gpu_ctx
    gpu_ctx.set_option(capi.OPT_CENGRD_FUSED, 0)


@pytest.fixture(scope="module")
def vol_ctx():
    """a second context for volume-sourced builds of the same inputs"""
    import crossscalepatchmatch_amd as cs
    ctx = cs.StereoContext(0)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _pc(name, sn, lam, wnd=35):
    assert sn in cengrd_ref.SCALES[name], "add the level count to cengrd_ref.SCALES: tests/test_cengrd_ref.py checks the branch fractions for it"
    l, r = cengrd_ref.images(name)
    return cengrd_ref.plane_cost(l, r, cengrd_ref.PAIRS[name].D, wnd, sn, lam)


def _build(ctx, name, sn, lam, fused=True, wnd=35):
    l, r = cengrd_ref.images(name)
    ctx.set_images(l, r)
    ctx.build_cost_cengrd(cengrd_ref.PAIRS[name].D, wnd, sn, lam, fused=fused)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == int(fused)
    return _pc(name, sn, lam, wnd)


def _state(ctx):
    return [ctx.get_planes(v) for v in (0, 1)]


def _assert_state(ctx, pm, what):
    got = _state(ctx)
    for v in (0, 1):
        P = pm.planes(v)
        np.testing.assert_array_equal(got[v][0][..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(got[v][0][..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(got[v][1], pm.min_cost(v), err_msg=f"{what}: min_cost, view {v}")


def _assert_same_state(a, b, what):
    for v in (0, 1):
        np.testing.assert_array_equal(a[v][0], b[v][0], err_msg=f"{what}: planes, view {v}")
        np.testing.assert_array_equal(a[v][1], b[v][1], err_msg=f"{what}: min_cost, view {v}")


def _assert_maps(ctx, pm, l, r, D, what):
    """PlaneToDisp, cspm_postprocess_f64 and cspm_postprocess behind a run == the oracle's / the restatement's"""
    pm.plane_to_disp()
    for v in (0, 1):
        np.testing.assert_array_equal(ctx.disparity_u8(v, DIS_SCALE), pm.dis(v), err_msg=f"{what}: 8-bit map, view {v}")
    abc = [ctx.get_planes(v)[0][..., 3:6] for v in (0, 1)]
    want = pp_sub_ref.postprocess_f64(abc[0], abc[1], l, r, D)
    for k, (g, w) in enumerate(zip(ctx.postprocess_f64(valid=True), want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: sub-pixel post-processing, output {k}")
    pm.postprocess()
    lo, ro = ctx.postprocess(DIS_SCALE)
    np.testing.assert_array_equal(lo, pm.dis(0), err_msg=f"{what}: post-processed left map")
    np.testing.assert_array_equal(ro, pm.dis(1), err_msg=f"{what}: post-processed right map")


# ---- 1. state ------------------------------------------------------------------------------------------------------------------------

def test_option_state(fused_ctx):
    ctx = fused_ctx
    l, r = cengrd_ref.images("small")
    ctx.set_images(l, r)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED) == 0
    ctx.build_cost_cengrd(16, 35, 3, 0.3)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 0  # the default
    for key in (capi.OPT_TABLE_VOLUMES, capi.OPT_SWEEP_PAIRS, capi.OPT_SWEEP_PACKED):
        ctx.set_option(key, 1)
    ctx.build_cost_cengrd(16, 35, 3, 0.3, fused=True)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED) == 1
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 1
    for key in (capi.OPT_TABLE_VOLUMES_ACTIVE, capi.OPT_SWEEP_PAIRS_ACTIVE, capi.OPT_SWEEP_PACKED_ACTIVE):
        assert ctx.get_option(key) == 0  # GRD-only accelerators
    ctx.build_cost_cengrd(16, 35, 3, 0.3)  # fused=None leaves the option alone
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 1
    ctx.set_option(capi.OPT_SWEEP_PAIRS, 0)
    ctx.set_option(capi.OPT_SWEEP_PACKED, 0)
    ctx.build_cost_grd(16, 35, 3, 0.3)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 0
    ctx.build_cost_cengrd(16, 35, 3, 0.3, fused=True)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 1
    ctx.build_cost_cengrd(16, 35, 3, 0.3, fused=False)
    assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == 0
    with pytest.raises(capi.CspmError, match=r"cspm error -1"):
        ctx.set_option(capi.OPT_CENGRD_FUSED_ACTIVE, 1)  # read only: CSPM_ERR_ARG


# ---- 2. cells ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sn,lam", [("small", 5, 0.3), ("odd", 3, 0.3), ("ragged_63x65", 0, 0.0), ("ragged_64x63", 0, 0.0),
                                         ("ragged_65x64", 0, 0.0)])
def test_cells_max_cost_and_weights(fused_ctx, name, sn, lam):
    """every slab of every level and view through cspm_get_cost_slab (k_cengrd_volume's d0 / nd range: no volume exists)"""
    pc = _build(fused_ctx, name, sn, lam)
    assert fused_ctx.levels == pc.levels
    np.testing.assert_array_equal(fused_ctx.scale_weights(), pc.scale_wgt())
    for s in range(pc.levels):
        assert fused_ctx.level_dims(s) == pc.dims(s)
        for v in (0, 1):
            np.testing.assert_array_equal(fused_ctx.cost_volume(v, s), pc.volume(v, s), err_msg=f"level {s}, view {v}")
            assert fused_ctx.max_cost(v, s) == pc.max_cost_dev(v, s) == pc.max_cost(v, s)


# ---- 3. cspm_plane_cost_batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sn,lam", [("small", 0, 0.0), ("small", 5, 0.3), ("odd", 3, 0.3)])
def test_plane_cost_batch(fused_ctx, name, sn, lam):
    """conftest.random_planes, then the hand-made planes of cengrd_fused_cases.hand_planes (pad cells of both borders, disparities
    outside [1, D): tests/test_cengrd_fused_inputs.py counts those taps), in the device order"""
    p = cengrd_ref.PAIRS[name]
    pc = _build(fused_ctx, name, sn, lam)
    rng = np.random.default_rng(78)
    for view in (0, 1):
        xy, norm, _, param = random_planes(rng, 600, p.w, p.h, p.D)
        hxy, hnorm, hparam = cases.hand_planes(p.w, p.h, p.D)
        xy, norm, param = np.concatenate([xy, hxy]), np.concatenate([norm, hnorm]), np.concatenate([param, hparam])
        got = fused_ctx.plane_cost_batch(view, xy, np.concatenate([norm, param], 1))
        dev = np.array([pc.cost(xy[i, 0], xy[i, 1], norm[i], param[i], view, po.SUM_DEVICE) for i in range(len(xy))])
        np.testing.assert_array_equal(got, dev, err_msg=f"view {view}")


# ---- 4. PatchMatch phase by phase --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,early_exit", [(RASTER, 1), (RASTER, 0), (REDBLACK, 1), (REDBLACK, 0)])
def test_phase_by_phase(fused_ctx, sched, early_exit):
    name = "small"
    p = cengrd_ref.PAIRS[name]
    pc = _build(fused_ctx, name, 5, 0.3)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    okw = dict(seed=9, schedule=sched, sum_order=po.SUM_DEVICE)
    gkw = dict(seed=9, schedule=sched, early_exit=early_exit)
    pm.init(pc, **okw)
    fused_ctx.pm_init(**gkw)
    _assert_state(fused_ctx, pm, "init")
    for it in range(2):
        for phase in ("spatial", "view", "refine"):
            getattr(pm, phase)(it, pc, **okw)
            getattr(fused_ctx, "pm_" + phase)(it, **gkw)
            _assert_state(fused_ctx, pm, f"iteration {it}, {phase}")


def test_one_diffuse_propagation(fused_ctx):
    """CSPM_SCHED_DIFFUSE, 8 neighbours, one round, after the random init (k_spatial_diffuse: the row engine on snapshot candidates)"""
    name = "small"
    p = cengrd_ref.PAIRS[name]
    pc = _build(fused_ctx, name, 5, 0.3)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    pm.init(pc, seed=9, schedule=RASTER, sum_order=po.SUM_DEVICE)
    fused_ctx.pm_init(seed=9, schedule=DIFFUSE, rb_neighbours=8)
    _assert_state(fused_ctx, pm, "init")
    diffuse_ref.diffuse(pm, pc, 0, 1, 8, po.SUM_DEVICE)
    fused_ctx.pm_spatial(0, seed=9, schedule=DIFFUSE, rb_rounds=1, rb_neighbours=8)
    _assert_state(fused_ctx, pm, "diffuse propagation")


# ---- 5. whole runs with maps -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sn,sched,early_exit", [("crop", 5, RASTER, 1), ("mid", 0, REDBLACK, 1)])
def test_whole_patchmatch_and_maps(fused_ctx, vol_ctx, name, sn, sched, early_exit):
    p = cengrd_ref.PAIRS[name]
    pc = _build(fused_ctx, name, sn, 0.3)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    pm.run(3, pc, False, seed=31, schedule=sched, sum_order=po.SUM_DEVICE, wavefront=True)
    fused_ctx.patchmatch(3, seed=31, schedule=sched, early_exit=early_exit)
    _assert_state(fused_ctx, pm, f"{name}: 3 iterations")
    if name == "crop":  # and the volume-sourced run on a second context: planes and min_cost
        _build(vol_ctx, name, sn, 0.3, fused=False)
        vol_ctx.patchmatch(3, seed=31, schedule=sched, early_exit=early_exit)
        _assert_same_state(_state(fused_ctx), _state(vol_ctx), "fused against volume-sourced")
    _assert_maps(fused_ctx, pm, l, r, p.D, name)


# ---- 6. window sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wnd", [9, 45])
def test_window_sizes(fused_ctx, wnd):
    """9: two groups of seven taps, the second a tail of two; 45 = kMaxWnd: five chain passes, 64 tree rows"""
    name = "small"
    p = cengrd_ref.PAIRS[name]
    pc = _build(fused_ctx, name, 5, 0.3, wnd=wnd)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    okw = dict(seed=5, schedule=RASTER, sum_order=po.SUM_DEVICE)
    pm.init(pc, **okw)
    fused_ctx.pm_init(seed=5)
    _assert_state(fused_ctx, pm, "init")
    pm.refine(0, pc, **okw)
    fused_ctx.pm_refine(0, seed=5)
    _assert_state(fused_ctx, pm, "refine")
    rng = np.random.default_rng(3)
    xy, norm, _, param = random_planes(rng, 100, p.w, p.h, p.D)
    got = fused_ctx.plane_cost_batch(0, xy, np.concatenate([norm, param], 1))  # the chain engine's passes for this window
    dev = np.array([pc.cost(xy[i, 0], xy[i, 1], norm[i], param[i], 0, po.SUM_DEVICE) for i in range(len(xy))])
    np.testing.assert_array_equal(got, dev)


# ---- 7. the row engine on both sides of its strip capacity -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wide_pc(max_dis):
    l, r = cases.wide_images()
    return cengrd_ref.plane_cost(l, r, max_dis, cases.WIDE_WND, 0, 0.0)


@pytest.mark.parametrize("max_dis", [cases.WIDE_GLOBAL_D, cases.WIDE_STAGED_D])
def test_saturated_strip(fused_ctx, max_dis):
    """352x40, window 35, single scale (cengrd_fused_cases.py works the numbers out; tests/test_cengrd_fused_inputs.py asserts them):
    max_dis 300 -- strip_capacity saturates at 384 slots, a full wave needs 398 / 399: its taps read BOTH VIEWS FROM GLOBAL MEMORY;
    max_dis 250 -- capacity 350, a full wave needs 348 / 349: the widest STAGED strips, six staging registers per lane"""
    l, r = cases.wide_images()
    fused_ctx.set_images(l, r)
    fused_ctx.build_cost_cengrd(max_dis, cases.WIDE_WND, 0, 0.0, fused=True)
    pc = _wide_pc(max_dis)
    pm = po.PatchMatch(l, r, max_dis, 1)
    okw = dict(seed=13, schedule=RASTER, sum_order=po.SUM_DEVICE)
    pm.init(pc, **okw)
    fused_ctx.pm_init(seed=13)
    _assert_state(fused_ctx, pm, "init")
    pm.view(0, pc, **okw)
    fused_ctx.pm_view(0, seed=13)
    _assert_state(fused_ctx, pm, "view propagation")
    pm.refine(0, pc, **okw)
    fused_ctx.pm_refine(0, seed=13)
    _assert_state(fused_ctx, pm, "refine")


# ---- 8. local stereo and a warm run --------------------------------------------------------------------------------------------------

def test_local_stereo_and_a_warm_run(fused_ctx, vol_ctx):
    """cspm_local_stereo(BOX) computes its raw cells slab batch by slab batch on a fused cost: the same field as over the volumes,
    and the same one-iteration warm run from it"""
    name = "kinds"
    _build(fused_ctx, name, 3, 0.3)
    _build(vol_ctx, name, 3, 0.3, fused=False)
    for ctx in (fused_ctx, vol_ctx):
        ctx.local_stereo(capi.CA_BOX)
    _assert_same_state(_state(fused_ctx), _state(vol_ctx), "local stereo BOX")
    for ctx in (fused_ctx, vol_ctx):
        ctx.patchmatch_warm(1, seed=3, schedule=RASTER)
    _assert_same_state(_state(fused_ctx), _state(vol_ctx), "warm run from the BOX field")


# ---- 9. cost switches on one context -----------------------------------------------------------------------------------------------

def test_cost_switches_on_one_context():
    """CENGRD volumes -> CENGRD fused -> GRD -> CENGRD fused -> CEN on one context, then a second pair with fused CENGRD on the
    first one's buffers: after each build the planes of cspm_pm_init equal a fresh context's -- nothing stale is read, and the
    option is part of the reuse key"""
    import crossscalepatchmatch_amd as cs
    D = 16
    a, b = cengrd_ref.images("small"), cengrd_ref.images("adversarial")
    assert a[0].shape == b[0].shape
    builds = {"GRD": lambda c: c.build_cost_grd(D, 35, 3, 0.3), "CEN": lambda c: c.build_cost_cen(D, 35, 3, 0.3),
              "CENGRD volumes": lambda c: c.build_cost_cengrd(D, 35, 3, 0.3, fused=False),
              "CENGRD fused": lambda c: c.build_cost_cengrd(D, 35, 3, 0.3, fused=True)}

    def init_state(ctx, l, r, kind):
        ctx.set_images(l, r)
        builds[kind](ctx)
        assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == int(kind == "CENGRD fused")
        ctx.pm_init(seed=4)
        return _state(ctx), ctx.cost_volume(1, 1)

    ctx = cs.StereoContext(0)
    try:
        for step, (kind, (l, r)) in enumerate((("CENGRD volumes", a), ("CENGRD fused", a), ("GRD", a), ("CENGRD fused", a), ("CEN", a),
                                               ("CENGRD fused", a), ("CENGRD fused", b))):
            got, vol = init_state(ctx, l, r, kind)
            fresh = cs.StereoContext(0)
            try:
                want, want_vol = init_state(fresh, l, r, kind)
            finally:
                fresh.close()
            _assert_same_state(got, want, f"step {step}: {kind}")
            np.testing.assert_array_equal(vol, want_vol, err_msg=f"step {step}: {kind}")
    finally:
        ctx.close()


# ---- 10. command line and host class -------------------------------------------------------------------------------------------------

def _cli(args, timeout=300):
    return subprocess.run([os.path.join(PKG, "cspm_main")] + args, capture_output=True, timeout=timeout)


def test_cli(tmp_path):
    """cspm_main --cc_name=CENGRD --cc_fused --use_cs --use_pp writes the PNGs of the run without --cc_fused, alone and as a
    --batch_list of two pairs; --help names the flag"""
    names = ["small", "mid"]
    for k, name in enumerate(names):
        l, r = cengrd_ref.images(name)
        pngio.write_png(str(tmp_path / f"l{k}.png"), l[..., ::-1])
        pngio.write_png(str(tmp_path / f"r{k}.png"), r[..., ::-1])
    flags = ["--max_dis=16", "--dis_scale=4", "--cc_name=CENGRD", "--use_cs=true", "--use_pp=true", "--reg_lambda=0.3", "--seed=777"]
    maps = {}
    for tag, extra in (("vol", []), ("fused", ["--cc_fused"])):
        io = [f"--l_img_file={tmp_path}/l0.png", f"--r_img_file={tmp_path}/r0.png", f"--l_dis_file={tmp_path}/{tag}_l.png",
              f"--r_dis_file={tmp_path}/{tag}_r.png"]
        p = _cli(io + flags + extra)
        assert p.returncode == 0 and b"Total Time:" in p.stdout, p.stdout.decode() + p.stderr.decode()
        lines = [" ".join(str(tmp_path / n) for n in (f"l{k}.png", f"r{k}.png", f"{tag}_bl{k}.png", f"{tag}_br{k}.png")) for k in (0, 1)]
        (tmp_path / f"{tag}_list.txt").write_text("\n".join(lines) + "\n")
        p = _cli([f"--batch_list={tmp_path}/{tag}_list.txt"] + flags + extra)
        assert p.returncode == 0 and b"Batch: 2 pairs" in p.stdout and b"0 failed" in p.stdout, p.stdout.decode() + p.stderr.decode()
        maps[tag] = [pngio.read_png(str(tmp_path / f"{tag}_{n}.png")) for n in ("l", "r", "bl0", "br0", "bl1", "br1")]
    for x, y in zip(maps["fused"], maps["vol"]):
        np.testing.assert_array_equal(x, y)
    assert np.ptp(maps["fused"][0]) > 0
    p = _cli(["--help"])
    assert b"cc_fused" in p.stdout + p.stderr


@pytest.mark.parametrize("sn", [3, 0])
def test_host_layer_class(fused_ctx, tmp_path, sn):
    """tests/helpers/cengrd_fused_check.cc: PreCSPC / PreSSPC over CenGrdCC(-1, true) report CSPM_OPT_CENGRD_FUSED_ACTIVE, agree with
    the volume-sourced object that inherits their context, and give the C ABI's field"""
    exe = _build_helper("cengrd_fused_check")
    name = "small"
    p = cengrd_ref.PAIRS[name]
    l, r = cengrd_ref.images(name)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<5i", p.w, p.h, p.D, sn, 2))
        f.write(l.tobytes())
        f.write(r.tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0 and b"ok" in out.stdout, f"exit {out.returncode}: " + out.stdout.decode() + out.stderr.decode()
    raw = np.fromfile(tmp_path / "out.bin")
    n = p.w * p.h
    assert raw.size == 2 * 7 * n
    _build(fused_ctx, name, sn, 0.3)
    fused_ctx.patchmatch(2, seed=12345, schedule=RASTER)
    for v in (0, 1):
        blk = raw[v * 7 * n:(v + 1) * 7 * n]
        npar, cost = fused_ctx.get_planes(v)
        np.testing.assert_array_equal(blk[:6 * n].reshape(p.h, p.w, 6), npar, err_msg=f"view {v}")
        np.testing.assert_array_equal(blk[6 * n:].reshape(p.h, p.w), cost, err_msg=f"view {v}")
