"""Spatial propagation under CSPM_SCHED_DIFFUSE on the GPU (k_spatial_diffuse, include/cspm.h) held to its CPU restatement
tests/diffuse_ref.py bit for bit: one propagation phase by phase on the shapes where a lane-per-pixel kernel goes wrong (segment
tails, single-row bands, borders), claimed column bands and the early exit off, every cost source, a field with stale costs, whole
cold and warm runs with their maps, determinism, the argument checks and the command line.  Every comparison is assert_array_equal on
the six plane doubles and min_cost of both views, or on whole maps.  tests/test_diffuse_ref.py checks on the CPU that none of the
cases is vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diffuse_ref
import pngio
import pp_sub_ref
import warm_ref
from crossscalepatchmatch_amd import capi, realdata as rd
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crossscalepatchmatch_amd")
DIS_SCALE = diffuse_ref.DIS_SCALE
DIFFUSE = capi.SCHED_DIFFUSE
assert DIFFUSE == diffuse_ref.SCHED_DIFFUSE


def _build(ctx, c, volumes=False):
    """the context gets the case's pair and cost object; returns the oracle's cost object"""
    ctx.set_images(*diffuse_ref.images(c.w, c.h, c.D, c.img))
    if c.cc == "GRD":
        ctx.build_cost_grd(c.D, 35, c.sn, c.lam, volumes=volumes)
    elif c.cc == "CEN":
        ctx.build_cost_cen(c.D, 35, c.sn, c.lam, volumes=volumes)
    elif c.cc == "IMG":
        ctx.build_cost_img(c.D, 35, c.sn, c.lam)
    else:
        ctx.build_cost_cengrd(c.D, 35, c.sn, c.lam)
    return diffuse_ref.case_cost(c)


def _kw(c, **more):
    return dict(seed=c.seed, schedule=DIFFUSE, rb_rounds=c.rounds, rb_neighbours=c.K, **more)


def _assert_state(ctx, state, what):
    """state: [(planes (h, w, 9), min_cost)] per view (diffuse_ref.state_of)"""
    for v in (0, 1):
        npar, cost = ctx.get_planes(v)
        np.testing.assert_array_equal(npar[..., :3], state[v][0][..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], state[v][0][..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, state[v][1], err_msg=f"{what}: min_cost, view {v}")


def _field(state, v):
    return np.concatenate([state[v][0][..., 0:3], state[v][0][..., 6:9]], -1)


def _start(ctx, c, p, own_init):
    """the start state of a propagation: the device's own random init (held to the oracle's), or the oracle's through cspm_set_planes"""
    if own_init:
        ctx.pm_init(**_kw(c))
        _assert_state(ctx, p.start, "random init")
    else:
        for v in (0, 1):
            ctx.set_planes(v, _field(p.start, v), p.start[v][1])


def _assert_maps(ctx, pm, l, r, D, what):
    """PlaneToDisp, cspm_postprocess_f64 and cspm_postprocess behind a run == the oracle's / the restatement's on the same planes"""
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


# ---- a. one propagation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("it", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("name", diffuse_ref.PHASE_CASES)
def test_one_propagation(gpu_ctx, name, it):
    """random init -> one cspm_pm_spatial.  The even iteration starts from the device's own init (a consistent field), the odd one
    from the oracle's init through cspm_set_planes (costs the library does not trust)."""
    c = diffuse_ref.CASES[name]
    p = diffuse_ref.first_propagation(name, it)
    _build(gpu_ctx, c)
    _start(gpu_ctx, c, p, own_init=it == 0)
    gpu_ctx.pm_spatial(it, **_kw(c))
    _assert_state(gpu_ctx, p.end, f"{name}, iteration {it}")


def test_claimed_column_bands_and_no_early_exit():
    """64x21 with the row kernels' items handed out as claimed column bands (CSPM_ROW_CLAIM=1, as test_row_kernels_claimed_column_bands
    forces them) and with the early exit off: every pixel is still evaluated exactly once, and full evaluations accept what the
    thresholded ones accept"""
    import crossscalepatchmatch_amd as cs
    name = "64x21_cs_k8"
    c = diffuse_ref.CASES[name]
    os.environ["CSPM_ROW_CLAIM"] = "1"
    try:
        ctx = cs.StereoContext(0)
    finally:
        del os.environ["CSPM_ROW_CLAIM"]
    try:
        _build(ctx, c)
        for it in (0, 1):
            p = diffuse_ref.first_propagation(name, it)
            for early_exit in (1, 0):
                _start(ctx, c, p, own_init=True)
                ctx.pm_spatial(it, **_kw(c, early_exit=early_exit))
                _assert_state(ctx, p.end, f"claimed bands, iteration {it}, early_exit {early_exit}")
    finally:
        ctx.close()


SOURCES = [("65x33_grd_k8", False), ("65x33_grd_k8", True), ("65x33_cen_k8", False), ("65x33_cen_k8", True), ("65x33_img_k8", False),
           ("65x33_cengrd_k8", False)]


@pytest.mark.parametrize("name,volumes", SOURCES, ids=[f"{n}{'_volumes' if v else ''}" for n, v in SOURCES])
def test_cost_sources(gpu_ctx, name, volumes):
    """fused GRD cells, GRD and census volumes (CSPM_OPT_GRD_VOLUMES), fused census, GrdPC / CSPC (cspm_build_cost_img) and CENGRD"""
    c = diffuse_ref.CASES[name]
    p = diffuse_ref.first_propagation(name, 0)
    _build(gpu_ctx, c, volumes)
    _start(gpu_ctx, c, p, own_init=True)
    gpu_ctx.pm_spatial(0, **_kw(c))
    _assert_state(gpu_ctx, p.end, f"{name}, volumes {volumes}")


def test_stale_costs(gpu_ctx):
    """cspm_set_planes with a block-constant field whose costs came from a CENSUS cost object, then DIFFUSE under GRD: most
    candidates are bitwise the pixel's own plane, and the stored cost is not what GRD gives that plane -- the plain evaluation
    compares every candidate's GRD cost with the stored census cost, as the restatement does"""
    c = diffuse_ref.CASES["65x33_grd_k8"]
    pc = _build(gpu_ctx, c)
    pc_cen = diffuse_ref.case_cost(diffuse_ref.CASES["65x33_cen_k8"])
    l, r = diffuse_ref.images(c.w, c.h, c.D, c.img)
    rng = np.random.default_rng(5)
    fields = []
    for _ in (0, 1):
        n = rng.normal(size=(c.h, c.w, 3))
        n[..., 2] = np.abs(n[..., 2]) + 1.0
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        z = rng.uniform(0.0, c.D, (c.h, c.w))
        f = np.zeros((c.h, c.w, 6))
        for y in range(c.h):
            for x in range(c.w):
                by, bx = y // 4 * 4, x // 4 * 4
                f[y, x, 0:3] = n[by, bx]
                f[y, x, 3:6] = po.plane_param(n[by, bx], [bx, by, z[by, bx]])
        fields.append(f)
    pm = po.PatchMatch(l, r, c.D, DIS_SCALE)
    warm_ref.inject(pm, fields)
    warm_ref.rescore(pm, pc_cen, po.SUM_DEVICE)
    stale = [pm.min_cost(v).copy() for v in (0, 1)]
    for v in (0, 1):
        gpu_ctx.set_planes(v, fields[v], stale[v])
    gpu_ctx.pm_spatial(0, **_kw(c))
    diffuse_ref.diffuse(pm, pc, 0, c.rounds, c.K, po.SUM_DEVICE)
    end = diffuse_ref.state_of(pm)
    _assert_state(gpu_ctx, end, "stale costs")
    for v in (0, 1):
        changed = np.any(_field(end, v) != fields[v], axis=2)
        assert 0 < changed.sum() < c.w * c.h
        # the case a shortcut that trusted the stored costs would get wrong: a pixel whose candidate is bitwise its own plane takes it
        # all the same, at the GRD cost, because the stored (census) cost is not what GRD gives that plane
        assert np.any(~changed & (end[v][1] < stale[v]))


# ---- b. whole runs --------------------------------------------------------------------------------------------------------------

def test_whole_run_and_maps(gpu_ctx):
    """two iterations on 96x64 (K = 8) == diffuse_ref.run, then PlaneToDisp, cspm_postprocess and cspm_postprocess_f64"""
    c = diffuse_ref.CASES["96x64_cs5_k8"]
    pc = _build(gpu_ctx, c)
    l, r = diffuse_ref.images(c.w, c.h, c.D, c.img)
    pm = po.PatchMatch(l, r, c.D, DIS_SCALE)
    gpu_ctx.patchmatch(2, **_kw(c))
    diffuse_ref.run(pm, pc, 2, c.rounds, c.K, seed=c.seed, sum_order=po.SUM_DEVICE)
    _assert_state(gpu_ctx, diffuse_ref.state_of(pm), "two iterations")
    _assert_maps(gpu_ctx, pm, l, r, c.D, "two iterations")


def test_warm_run_from_a_box_field(gpu_ctx):
    """cspm_local_stereo(BOX) -> cspm_patchmatch_warm(1) under DIFFUSE == tests/warm_ref.py with diffuse in place of the sweep"""
    c = diffuse_ref.CASES["96x64_cs5_k8"]._replace(sn=4)  # four levels down to 12x8: BoxCA needs 7 px on the coarsest one
    pc = _build(gpu_ctx, c)
    l, r = diffuse_ref.images(c.w, c.h, c.D, c.img)
    fields = warm_ref.local_stereo_fields(pc, "BOX", c.D, True)
    gpu_ctx.local_stereo(capi.CA_BOX)
    for v in (0, 1):
        np.testing.assert_array_equal(gpu_ctx.get_planes(v)[0], fields[v], err_msg=f"local stereo, view {v}")
    pm = po.PatchMatch(l, r, c.D, DIS_SCALE)
    warm_ref.inject(pm, fields)
    gpu_ctx.patchmatch_warm(1, **_kw(c))
    warm_ref.rescore(pm, pc, po.SUM_DEVICE)
    diffuse_ref.iterate(pm, pc, 1, c.rounds, c.K, seed=c.seed, sum_order=po.SUM_DEVICE)
    end = diffuse_ref.state_of(pm)
    _assert_state(gpu_ctx, end, "warm run")
    assert all(np.any(_field(end, v) != fields[v]) for v in (0, 1))


def test_determinism(gpu_ctx):
    """two runs on one context and one on a fresh context are identical"""
    import crossscalepatchmatch_amd as cs
    c = diffuse_ref.CASES["130x21_cs_k8"]
    out = []
    fresh = cs.StereoContext(0)
    try:
        for ctx in (gpu_ctx, gpu_ctx, fresh):
            _build(ctx, c)
            ctx.patchmatch(2, **_kw(c))
            out.append([ctx.get_planes(v) for v in (0, 1)] + list(ctx.postprocess(DIS_SCALE)))
    finally:
        fresh.close()
    for other in out[1:]:
        for v in (0, 1):
            np.testing.assert_array_equal(out[0][v][0], other[v][0])
            np.testing.assert_array_equal(out[0][v][1], other[v][1])
            np.testing.assert_array_equal(out[0][2 + v], other[2 + v])


# ---- c. arguments and the command line ------------------------------------------------------------------------------------------

def test_argument_checks(gpu_ctx):
    c = diffuse_ref.CASES["63x21_cs_k8"]
    _build(gpu_ctx, c)
    gpu_ctx.pm_init(seed=1)
    for K in (2, 6, 0):
        with pytest.raises(capi.CspmError, match=r"cspm error -1: rb_neighbours must be 4, 8 or 20"):
            gpu_ctx.pm_spatial(0, schedule=DIFFUSE, rb_neighbours=K)
        with pytest.raises(capi.CspmError, match=r"cspm error -1"):
            gpu_ctx.patchmatch(1, schedule=DIFFUSE, rb_neighbours=K)
    for K in (8, 20):
        with pytest.raises(capi.CspmError, match=r"cspm error -1: rb_neighbours must be 2 or 4"):
            gpu_ctx.pm_spatial(0, schedule=capi.SCHED_REDBLACK, rb_neighbours=K)
    with pytest.raises(capi.CspmError, match=r"cspm error -1: rb_rounds"):
        gpu_ctx.pm_spatial(0, schedule=DIFFUSE, rb_neighbours=8, rb_rounds=0)
    with pytest.raises(capi.CspmError, match=r"cspm error -1: bad schedule"):
        gpu_ctx.pm_spatial(0, schedule=3)
    # the foreign-IPlaneCost protocol stays raster-only
    L = gpu_ctx.L
    n = C.c_int()
    cap = 2 * c.w * c.h
    xy, view, plane = np.zeros(2 * cap, np.int32), np.zeros(cap, np.int32), np.zeros(6 * cap)
    ip = C.POINTER(C.c_int)
    assert L.cspm_fpm_begin(gpu_ctx.p, c.w, c.h, c.D) == 0
    par = gpu_ctx.params(schedule=DIFFUSE, rb_neighbours=8)
    rc = L.cspm_fpm_candidates(gpu_ctx.p, 0, 0, 0, C.byref(par), C.byref(n), xy.ctypes.data_as(ip), view.ctypes.data_as(ip),
                               plane.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -1 and b"raster schedule only" in L.cspm_last_error(gpu_ctx.p)


def test_cli_diffuse_20_neighbours(gpu_ctx, tmp_path):
    """cspm_main --schedule=diffuse --neighbours=20 --use_pp on the half-size Motorcycle crop writes the C ABI's maps; without
    --neighbours the command line runs 8"""
    cfg, l, r, _ = rd.load_crop()
    pngio.write_png(str(tmp_path / "l.png"), l[..., ::-1])
    pngio.write_png(str(tmp_path / "r.png"), r[..., ::-1])
    args = [f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png",
            f"--max_dis={cfg['max_dis']}", f"--dis_scale={DIS_SCALE}", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--seed=777",
            "--iters=2", "--use_pp=true", "--quiet=true", "--schedule=diffuse"]
    maps = {}
    for K, extra in ((20, ["--neighbours=20"]), (8, [])):
        p = subprocess.run([os.path.join(PKG, "cspm_main")] + args + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
        gpu_ctx.set_images(l, r)
        gpu_ctx.build_cost_grd(cfg["max_dis"], 35, 5, 0.3)
        gpu_ctx.patchmatch(2, seed=777, schedule=DIFFUSE, rb_neighbours=K)
        want = gpu_ctx.postprocess(DIS_SCALE)
        maps[K] = pngio.read_png(str(tmp_path / "ld.png")), pngio.read_png(str(tmp_path / "rd.png"))
        for a, b in zip(maps[K], want):
            np.testing.assert_array_equal(a, b, err_msg=f"{K} neighbours")
    assert np.any(maps[20][0] != maps[8][0])
    p = subprocess.run([os.path.join(PKG, "cspm_main")] + args + ["--neighbours=6"], capture_output=True, timeout=300)
    assert p.returncode != 0 and b"rb_neighbours must be 4, 8 or 20" in p.stdout + p.stderr
