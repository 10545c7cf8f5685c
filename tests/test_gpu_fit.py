"""Plane fitting on the GPU (include/cspm.h "plane fitting") held to tests/fit_ref.py bit for bit:
cspm_fit_planes_host over shapes around the kernel's 64 x 4 tile, every radius class and every kind of input; cspm_fit_planes with and
without the merge against the restatements of the warm and seeded pipelines; the error returns, the timing counts, the host layer and
cspm_main --fit_radius.  Every comparison is assert_array_equal on the six plane doubles (NaN positions included) and on `fitted`."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import fit_ref
import seed_ref
import test_gpu_seed as tgs
import warm_ref
from crossscalepatchmatch_amd import capi
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

DEV = po.SUM_DEVICE
MAIN = tgs.MAIN  # 80 x 56, D = 16
TILE_W, TILE_H = 64, 4  # kFitTileW, kFitTileH (csrc/cspm_fit.h)
SHAPES = [(1, 1), (7, 5), (63, 5), (65, 17), (130, 67), (TILE_W, TILE_H), (TILE_W - 1, TILE_H - 1), (TILE_W + 1, TILE_H + 1)]


def _check(D, V, I, max_dis, **params):
    got, fitted = capi.fit_planes_host(D, V, I, max_dis=max_dis, **params)
    want, wfit = fit_ref.fit(D, V, I, max_dis, **{**fit_ref.DEFAULTS, **params})
    np.testing.assert_array_equal(fitted, wfit, err_msg=f"fitted {D.shape} {params}")
    np.testing.assert_array_equal(got, want, err_msg=f"planes {D.shape} {params}")
    return got, fitted


def _random_map(w, h, seed, holes=True):
    rng = np.random.default_rng(seed)
    D = np.round(rng.uniform(0, 6, (h, w)) * 4) / 4 + 0.25 * np.arange(w)[None, :] + 0.5 * (np.arange(h)[:, None] % 5)
    V = None
    if holes:
        V = (rng.uniform(size=(h, w)) > 0.15).astype(np.uint8)
        D[rng.uniform(size=(h, w)) > 0.95] = np.nan
    I = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return D, V, I


@pytest.mark.parametrize("r", [1, 2, 5, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_shapes_and_radii(shape, r):
    w, h = shape
    D, V, I = _random_map(w, h, 100 + w + h)
    _check(D, V, I, 40, radius=r, max_diff=1.5, min_support=6, use_guide=1)
    _check(D, None, None, 40, radius=r, max_diff=math.inf, min_support=3, use_guide=0)


@pytest.mark.parametrize("tau", [0.0, 1.5, math.inf])
@pytest.mark.parametrize("guide", [0, 1])
def test_host_entry_inputs(tau, guide):
    w, h = 67, 11
    rng = np.random.default_rng(7)
    D, V, I = _random_map(w, h, 8)
    kw = dict(radius=3, max_diff=tau, min_support=5, use_guide=guide)
    _check(D, V, I, 40, **kw)                                              # random quantised map with holes
    stairs = np.floor(np.arange(w)[None, :] / 3.0) + np.floor(np.arange(h)[:, None] / 2.0)  # integer staircases: local stereo's maps
    _, fitted = _check(stairs, None, I, 64, **kw)
    assert fitted.all()
    bad = D.copy()
    bad[1::4, 2::5] = np.inf
    bad[2::5, 1::7] = -np.inf
    bad[0, 0] = bad[h - 1, w - 1] = np.nan
    checker = (np.indices((h, w)).sum(0) % 2).astype(np.uint8)
    _, fitted = _check(bad, checker, I, 40, **kw)                          # NaN, inf and a checkerboard mask
    assert not fitted[0, 0] and fitted.sum() < h * w // 2 + 1
    dup = np.ascontiguousarray(np.broadcast_to(np.array([17, 200, 3], np.uint8), (h, w, 3)))   # exact duplicates: table entry 0
    _check(D, V, dup, 40, **kw)
    sat = np.where(rng.uniform(size=(h, w, 1)) > 0.5, 255, 0).astype(np.uint8).repeat(3, axis=2)  # 0 / 255: table entries 0 and 765
    _check(D, V, sat, 40, **kw)
    low_high = np.where(np.arange(w)[None, :] < w // 2, -5.0, 50.0) + 0.125 * np.arange(h)[:, None]  # z clamped at both ends
    got, _ = _check(low_high, None, I, 16, **kw)
    z = got[..., 3] * np.arange(w)[None, :] + got[..., 4] * np.arange(h)[:, None] + got[..., 5]
    assert np.abs(z[:, :w // 2 - 4]).max() < 1e-9 and np.abs(z[:, w // 2 + 4:] - 16.0).max() < 1e-9


def test_constant_map_is_fronto_parallel():
    D = np.full((9, 70), 5.0)
    got, fitted = _check(D, None, None, 16, radius=5)
    np.testing.assert_array_equal(got, capi.disparity_planes(D))
    assert fitted.all()


# ---- the context entry --------------------------------------------------------------------------------------------------------------

def _fields(ctx):
    return [ctx.get_planes(v)[0] for v in (0, 1)]


@pytest.mark.parametrize("sn", [0, 3], ids=["ss", "cs3"])
def test_fit_after_local_stereo_then_warm_run(gpu_ctx, sn):
    p = MAIN
    pc = tgs._build(gpu_ctx, p, "grd_fused", sn)
    gpu_ctx.local_stereo(capi.CA_BOX)
    before = _fields(gpu_ctx)
    disp = [gpu_ctx.disparity_f64(v) for v in (0, 1)]
    imgs = [gpu_ctx.level_image(v, 0) for v in (0, 1)]
    params = dict(radius=2, max_diff=1.5, min_support=6, use_guide=1)
    gpu_ctx.fit_planes(merge=False, **params)
    got = _fields(gpu_ctx)
    want, _, masks = fit_ref.fit_fields(before, imgs, p.D, **params)
    for v in (0, 1):
        np.testing.assert_array_equal(got[v], fit_ref.fit(disp[v], None, imgs[v], p.D, **params)[0], err_msg=f"view {v}: fit of disparity_f64")
        np.testing.assert_array_equal(got[v], want[v], err_msg=f"view {v}: fit_fields")
        assert masks[v].all() and np.any(got[v][..., 3:5] != 0)  # slants were found
    gpu_ctx.patchmatch_warm(1, seed=7)
    pm = tgs._pm(p)
    warm_ref.inject(pm, want)
    warm_ref.warm_run(pm, pc, 1, seed=7, schedule=po.SCHED_RASTER, sum_order=DEV)
    tgs._assert_state(gpu_ctx, pm, f"local stereo, fit, one warm iteration ({sn} levels)")


@pytest.mark.parametrize("cost", ["grd_fused", "grd_volumes"])
def test_fit_merge_after_init_equals_the_restatement(gpu_ctx, cost):
    p = MAIN
    pc = tgs._build(gpu_ctx, p, cost, 3)
    gpu_ctx.pm_init(seed=9)
    pm = tgs._pm(p)
    pm.init(pc, seed=9, sum_order=DEV)
    start = _fields(gpu_ctx)
    imgs = [gpu_ctx.level_image(v, 0) for v in (0, 1)]
    params = dict(radius=3, max_diff=2.0, min_support=6, use_guide=1)
    gpu_ctx.fit_planes(merge=True, **params)
    _, cands, masks = fit_ref.fit_fields(start, imgs, p.D, **params)
    taken = seed_ref.merge(pm, pc, cands, masks, DEV)
    assert 0 < taken < 2 * p.w * p.h
    tgs._assert_state(gpu_ctx, pm, f"fit with merge, {cost}")


def test_merge_disparity_with_fit_is_its_host_composition(gpu_ctx):
    p = MAIN
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    d = tgs._seed_map(p)
    d[d < 0] = np.nan
    params = dict(radius=2, max_diff=1.0)
    gpu_ctx.pm_init(seed=4)
    gpu_ctx.merge_disparity(0, d, fit=params)
    got = tgs._state(gpu_ctx)
    planes, fitted = fit_ref.fit(d, None, gpu_ctx.level_image(0, 0), p.D, **{**fit_ref.DEFAULTS, **params})
    gpu_ctx.pm_init(seed=4)
    gpu_ctx.merge_planes(0, planes, fitted)
    tgs._same_state(got, tgs._state(gpu_ctx), "merge_disparity(fit=...) against fit + merge_planes")
    gpu_ctx.pm_init(seed=4)
    gpu_ctx.merge_disparity(0, d)
    assert np.any(got[0][0] != gpu_ctx.get_planes(0)[0])  # the slanted candidates are not the fronto-parallel ones


# ---- errors and timing ----------------------------------------------------------------------------------------------------------------

def test_error_returns(gpu_ctx):
    import crossscalepatchmatch_amd as cs
    p = MAIN
    L = gpu_ctx.L
    l, r = tgs._images(p)
    dp = C.POINTER(C.c_double)
    d = np.zeros((p.h, p.w))
    out = np.zeros((p.h, p.w, 6))
    good = capi.fit_params()
    host = lambda disp, w, h, md, par, o, guide=None, stride=0: L.cspm_fit_planes_host(0, disp, None, guide, stride, w, h, md, par, o, None)
    assert host(None, p.w, p.h, 16, C.byref(good), out.ctypes.data_as(dp)) == -1      # CSPM_ERR_ARG = -1, CSPM_ERR_STATE = -3
    assert host(d.ctypes.data_as(dp), p.w, p.h, 16, C.byref(good), None) == -1
    assert host(d.ctypes.data_as(dp), 0, p.h, 16, C.byref(good), out.ctypes.data_as(dp)) == -1
    assert host(d.ctypes.data_as(dp), p.w, p.h, -1, C.byref(good), out.ctypes.data_as(dp)) == -1
    g = np.ascontiguousarray(l)
    assert host(d.ctypes.data_as(dp), p.w, p.h, 16, C.byref(good), out.ctypes.data_as(dp), g.ctypes.data_as(C.POINTER(C.c_uint8)), p.w * 3 - 1) == -1
    assert host(d.ctypes.data_as(dp), p.w, p.h, 16, None, out.ctypes.data_as(dp)) == 0  # NULL parameters: the defaults
    for bad in (dict(radius=0), dict(radius=18), dict(min_support=2), dict(max_diff=-0.5), dict(max_diff=math.nan)):
        assert host(d.ctypes.data_as(dp), p.w, p.h, 16, C.byref(capi.fit_params(**bad)), out.ctypes.data_as(dp)) == -1, bad
    a = cs.StereoContext(0)
    try:
        assert L.cspm_fit_planes(None, None, 0) == -1
        assert L.cspm_fit_planes(a.p, None, 0) == -3                                   # no images
        a.set_images(l, r)
        assert L.cspm_fit_planes(a.p, None, 0) == -3                                   # no plane field
        a.set_planes(0, capi.disparity_planes(d), d)
        assert L.cspm_fit_planes(a.p, None, 1) == -3                                   # merge without a cost object
        assert L.cspm_fit_planes(a.p, None, 0) == -3                                   # no max_dis known yet
        a.build_cost_grd(p.D, 35, 0, 0.0)
        for bad in (dict(radius=0), dict(radius=18), dict(min_support=2), dict(max_diff=-0.5), dict(max_diff=math.nan)):
            assert L.cspm_fit_planes(a.p, C.byref(capi.fit_params(**bad)), 0) == -1, bad
            assert b"plane fit" in L.cspm_last_error(a.p)
        assert L.cspm_fit_planes(a.p, None, 0) == 0
        assert L.cspm_fit_planes(a.p, None, 1) == 0
        a.synchronize()
    finally:
        a.close()


def test_fit_is_timed_as_misc_and_its_merge_as_init(gpu_ctx):
    p = MAIN
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    n = p.w * p.h
    gpu_ctx.pm_init(seed=9)
    gpu_ctx.synchronize()
    gpu_ctx.enable_timing(True)
    try:
        gpu_ctx.reset_timing()
        gpu_ctx.fit_planes(merge=False, radius=2)  # one bracket per view; the field is stale afterwards
        gpu_ctx.fit_planes(merge=True, radius=2)   # a re-score (one launch, 2n), one bracket and one merge launch per view
        gpu_ctx.synchronize()
        t = gpu_ctx.timing()
    finally:
        gpu_ctx.enable_timing(False)
    assert t["misc"]["launches"] == 4 and t["misc"]["evals"] == 4 * n
    assert t["init"]["launches"] == 3 and t["init"]["evals"] == 4 * n
    assert all(t[k]["launches"] == 0 for k in ("spatial", "view", "refine", "grd", "post"))


# ---- host layer and command line ------------------------------------------------------------------------------------------------------

def test_host_layer_fit_equals_the_c_abi(gpu_ctx, tmp_path):
    """tests/helpers/fit_check.cc: AddCandidateDisparity(map, fit) + PatchMatchSeeded, and LocalStereo + FitPlanes + PatchMatchFrom"""
    exe = _build_helper("fit_check")
    p = MAIN
    l, r = tgs._images(p)
    d = tgs._seed_map(p)
    radius, iters = 2, 1
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([p.w, p.h, p.D, 3, capi.CA_BOX, iters, radius], np.int32).tobytes())
        f.write(np.ascontiguousarray(l).tobytes())
        f.write(np.ascontiguousarray(r).tobytes())
        f.write(np.ascontiguousarray(d).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"foreign refused") == 1
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = p.w * p.h
    assert raw.size == 4 * 7 * n
    runs = [[(raw[(2 * k + v) * 7 * n:][:6 * n].reshape(p.h, p.w, 6), raw[(2 * k + v) * 7 * n + 6 * n:][:n].reshape(p.h, p.w))
             for v in (0, 1)] for k in (0, 1)]
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    planes, fitted = capi.fit_planes_host(d, np.isfinite(d) & (d >= 0), l, max_dis=p.D, radius=radius)
    gpu_ctx.pm_init(seed=12345)
    gpu_ctx.merge_planes(0, planes, fitted)
    gpu_ctx.patchmatch_warm(iters, seed=12345)
    tgs._same_state(runs[0], tgs._state(gpu_ctx), "AddCandidateDisparity(fit) + PatchMatchSeeded")
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.fit_planes(merge=False, radius=radius)
    gpu_ctx.patchmatch_warm(iters, seed=12345)
    tgs._same_state(runs[1], tgs._state(gpu_ctx), "LocalStereo + FitPlanes + PatchMatchFrom")


def test_cli_warm_ca_with_fit_equals_the_c_abi(gpu_ctx, tmp_path):
    """cspm_main --warm_ca=BOX --fit_radius=2 (five levels, as the command line builds them) == local_stereo, fit_planes, one warm iteration"""
    p = MAIN._replace(w=160, h=128, D=24, seed=22)  # five levels down to 10x8: BOX needs 7
    got = tgs._cli(tmp_path, p, "--warm_ca=BOX", "--fit_radius=2")
    gpu_ctx.set_images(*tgs._images(p))
    gpu_ctx.build_cost_grd(p.D, 35, 5, 0.3)
    gpu_ctx.local_stereo(capi.CA_BOX)
    plain = [gpu_ctx.get_planes(v)[0] for v in (0, 1)]
    gpu_ctx.fit_planes(merge=False, radius=2)
    assert np.any(plain[0] != gpu_ctx.get_planes(0)[0])
    gpu_ctx.patchmatch_warm(1, seed=12345)
    for v in (0, 1):
        np.testing.assert_array_equal(got[v], gpu_ctx.disparity_u8(v, tgs.DIS_SCALE), err_msg=f"--warm_ca=BOX --fit_radius=2, view {v}")
