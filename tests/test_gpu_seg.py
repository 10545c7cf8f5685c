"""Superpixel segment planes on the GPU (include/cspm.h "segment planes") held to tests/seg_ref.py bit for bit:
cspm_segment_host over shapes around the assign kernel's 64 x 4 tile, both owner kinds of the update and fit kernels (a wave up to
step 16, a workgroup above), every kind of image; cspm_segment_planes_host over every kind of map, mask, parameter and label map;
cspm_segment_planes with and without the merge against the restatements of the seeded and warm pipelines; cspm_get_segments, the error
returns, the timing counts, the host layer and cspm_main --seg_step.  Every comparison is assert_array_equal."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import seed_ref
import seg_ref
import test_gpu_seed as tgs
import warm_ref
from crossscalepatchmatch_amd import capi
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

DEV = po.SUM_DEVICE
MAIN = tgs.MAIN  # 80 x 56, D = 16
TILE_W, TILE_H = 64, 4  # kSegTileW, kSegTileH (csrc/cspm_seg.h)
STEPS = [4, 5, 16]      # a wave owns a segment up to kSegWaveStep = 16; 64 (below) takes the workgroup-per-segment path


def _shapes(s):
    return [(1, 1), (3, 2), (s, s), (s + 1, s - 1), (65, 17), (130, 67), (TILE_W, TILE_H), (TILE_W - 1, TILE_H - 1), (TILE_W + 1, TILE_H + 1)]


@functools.lru_cache(maxsize=None)
def _images(w, h):
    """the four kinds of image, computed once per shape and never written to"""
    rng = np.random.default_rng(1000 * w + h)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    const = np.ascontiguousarray(np.broadcast_to(np.array([17, 200, 3], np.uint8), (h, w, 3)))  # ties everywhere; empty segments at m = 0
    tone = np.where(np.arange(w)[None, :, None] < max(1, w // 2), np.array([60, 60, 60]), np.array([200, 180, 160]))
    tone = (np.broadcast_to(tone, (h, w, 3)) + rng.integers(-6, 7, (h, w, 3))).astype(np.uint8)
    sat = np.where(rng.uniform(size=(h, w, 3)) > 0.5, 255, 0).astype(np.uint8)
    for a in (noise, const, tone, sat):
        a.setflags(write=False)
    return dict(noise=noise, constant=const, two_tone=tone, saturated=sat)


def _check_segment(img, s, m, T, what):
    labels, centres, counts = capi.segment_host(img, step=s, compactness=m, iters=T)
    wl, wc, wn = seg_ref.segment(img, s, m, T)
    np.testing.assert_array_equal(labels, wl, err_msg=f"labels {what}")
    np.testing.assert_array_equal(counts, wn, err_msg=f"counts {what}")
    np.testing.assert_array_equal(centres, wc, err_msg=f"centres {what}")
    return labels, counts


@pytest.mark.parametrize("s", STEPS)
@pytest.mark.parametrize("idx", range(9))
def test_segmentation_shapes_steps_and_images(idx, s):
    w, h = _shapes(s)[idx]
    for name, img in _images(w, h).items():
        for T in (1, 5):
            for m in (0, 20, 255):
                _check_segment(img, s, m, T, f"{w}x{h} s={s} m={m} T={T} {name}")


def test_segmentation_with_a_workgroup_per_segment():
    w, h, s = 200, 70, 64
    for name, img in _images(w, h).items():
        for T, m in ((1, 0), (5, 20), (5, 255)):
            _check_segment(img, s, m, T, f"{w}x{h} s={s} m={m} T={T} {name}")


def test_constant_image_has_empty_segments_on_the_device_too():
    img = np.full((9, 13, 3), 77, np.uint8)
    _, counts = _check_segment(img, 4, 0, 3, "constant 13x9")
    assert (counts == 0).sum() == 6
    assert capi.segment_count(13, 9, 4) == 12 and capi.segment_count(200, 70, 64) == 8


# ---- the fit ------------------------------------------------------------------------------------------------------------------------

def _random_map(w, h, seed, quantised=True):
    rng = np.random.default_rng(seed)
    D = rng.uniform(0, 6, (h, w))
    if quantised:
        D = np.round(D * 4) / 4
    D = D + 0.25 * np.arange(w)[None, :] + 0.5 * (np.arange(h)[:, None] % 5)
    D[rng.uniform(size=(h, w)) > 0.9] += 9.0          # outliers for the rounds to reject
    D[rng.uniform(size=(h, w)) > 0.97] = np.nan
    D[rng.uniform(size=(h, w)) > 0.98] = np.inf
    D[rng.uniform(size=(h, w)) > 0.98] = -np.inf
    D[rng.uniform(size=(h, w)) > 0.98] = 32768.25      # beyond the node bound
    D[rng.uniform(size=(h, w)) > 0.98] = -32768.0      # on it: a node
    half = rng.uniform(size=(h, w)) > 0.97
    D[half] = (rng.integers(0, 1 << 20, (h, w))[half] + 0.5) / 65536.0  # q falls on a tie: round to even
    return D


def _label_maps(w, h, s, seed):
    """label maps with the 3 x 3 property: the segmentation's own, every pixel in its home cell, and the farthest drift both ways"""
    nx, ny, _ = seg_ref.grid(w, h, s)
    hx, hy = seg_ref.home_cells(w, h, s)
    img = _images(w, h)["noise"]
    own = capi.segment_host(img, step=s)[0]
    np.testing.assert_array_equal(own, seg_ref.segment(img, s, 20, 5)[0])
    home = (hy * nx + hx).astype(np.int32)
    up = (np.minimum(ny - 1, hy + 1) * nx + np.minimum(nx - 1, hx + 1)).astype(np.int32)
    down = (np.maximum(0, hy - 1) * nx + np.maximum(0, hx - 1)).astype(np.int32)
    rng = np.random.default_rng(seed)
    mixed = (np.clip(hy + rng.integers(-1, 2, (h, w)), 0, ny - 1) * nx + np.clip(hx + rng.integers(-1, 2, (h, w)), 0, nx - 1)).astype(np.int32)
    return dict(own=own, home=home, up=up, down=down, mixed=mixed)


def _check_fit(D, V, labels, s, max_dis, what, **params):
    seg, inl, planes, fitted = capi.segment_planes_host(D, V, labels, max_dis=max_dis, step=s, **params)
    p = {**seg_ref.DEFAULTS, **params}
    wseg, winl, wplanes, wfit = seg_ref.fit_segments(D, V, labels, s, max_dis, p["tau"], p["rounds"], p["min_support"])
    np.testing.assert_array_equal(inl, winl, err_msg=f"inliers {what} {params}")
    np.testing.assert_array_equal(seg, wseg, err_msg=f"segment planes {what} {params}")
    np.testing.assert_array_equal(fitted, wfit, err_msg=f"fitted {what} {params}")
    np.testing.assert_array_equal(planes, wplanes, err_msg=f"planes {what} {params}")
    return seg, inl, planes, fitted


@pytest.mark.parametrize("w,h,s", [(w, h, s) for s in STEPS for w, h in ((65, 17), (130, 67))] + [(200, 70, 64)])
def test_fit_label_maps_masks_and_maps(w, h, s):
    checker = (np.indices((h, w)).sum(0) % 2).astype(np.uint8)
    for q in (True, False):
        D = _random_map(w, h, 5 * w + s + q, quantised=q)
        for name, labels in _label_maps(w, h, s, w + s).items():
            _, inl, _, fitted = _check_fit(D, None, labels, s, 40, f"{w}x{h} s={s} {name}")
            _check_fit(D, checker, labels, s, 40, f"{w}x{h} s={s} {name} checkerboard")
            if name == "home" and s >= 5:
                assert inl.max() > 6 and fitted.any()


@pytest.mark.parametrize("rounds", [0, 1, 3, 8])
@pytest.mark.parametrize("tau", [0.0, 1.0, math.inf])
def test_fit_parameters(tau, rounds):
    w, h = 67, 31
    for s in (5, 16):
        D = _random_map(w, h, 31 + s)
        labels = _label_maps(w, h, s, 3)["own"]
        _check_fit(D, None, labels, s, 40, f"s={s}", tau=tau, rounds=rounds, min_support=6)
        _check_fit(D, None, labels, s, 40, f"s={s}", tau=tau, rounds=rounds, min_support=3)
    _, inl, _, fitted = _check_fit(D, None, labels, 16, 40, "min_support above the segment size", tau=tau, rounds=rounds, min_support=9 * 16 * 16 + 1)
    assert not fitted.any() and not inl.any()


def test_fit_known_answers_on_the_device():
    s = 8
    h, w = 8, 16
    labels = np.broadcast_to((np.arange(w) // s)[None, :], (h, w)).astype(np.int32)
    low_high = np.where(np.arange(w)[None, :] < s, -5.0, 50.0) + 0.125 * np.arange(h)[:, None]  # z clamped at both ends
    _, _, planes, fitted = _check_fit(low_high, None, labels, s, 16, "clamp")
    z = planes[..., 3] * np.arange(w)[None, :] + planes[..., 4] * np.arange(h)[:, None] + planes[..., 5]
    assert fitted.all() and np.abs(z[:, :s]).max() < 1e-9 and np.abs(z[:, s:] - 16.0).max() < 1e-9
    V = np.ones((h, w), np.uint8)
    V[:, :s] = 0
    V[3, :s] = 1  # collinear: unfitted, six NaNs; its holes get nothing
    holes = np.full((h, w), 3.0)
    holes[2, 10] = np.nan  # a hole inside the fitted segment receives the plane
    _, inl, planes, fitted = _check_fit(holes, V, labels, s, 16, "collinear and holes")
    assert not fitted[:, :s].any() and np.isnan(planes[:, :s]).all() and fitted[:, s:].all() and inl.tolist() == [0, s * s - 1]
    np.testing.assert_array_equal(planes[2, 10], [0.0, 0.0, 1.0, 0.0, 0.0, 3.0])


def test_labels_outside_the_3x3_cells_are_refused():
    w, h, s = 40, 24, 8
    D = np.zeros((h, w))
    nx, ny, K = seg_ref.grid(w, h, s)
    good = _label_maps(w, h, s, 1)["home"]
    for y, x, k in ((0, 0, 2), (0, 0, 2 * nx), (h - 1, w - 1, 0), (5, 5, -1), (5, 5, K), (12, 20, nx * 1 + 0)):
        bad = good.copy()
        bad[y, x] = k
        assert not seg_ref.labels_obey_3x3(bad, s)
        with pytest.raises(capi.CspmError, match="3 x 3"):
            capi.segment_planes_host(D, None, bad, max_dis=16, step=s)
    capi.segment_planes_host(D, None, good, max_dis=16, step=s)


# ---- the context entry --------------------------------------------------------------------------------------------------------------

def _fields(ctx):
    return [ctx.get_planes(v)[0] for v in (0, 1)]


PARAMS = dict(step=8, compactness=20, iters=3, tau=1.0, rounds=3, min_support=6)
KW = dict(seed=9, schedule=po.SCHED_RASTER, sum_order=DEV)


def test_replace_after_one_iteration_equals_the_restatement(gpu_ctx):
    p = MAIN
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    gpu_ctx.patchmatch(1, seed=9)
    before = _fields(gpu_ctx)
    disp = [gpu_ctx.disparity_f64(v) for v in (0, 1)]
    imgs = [gpu_ctx.level_image(v, 0) for v in (0, 1)]
    gpu_ctx.segment_planes(merge=False, **PARAMS)
    got = _fields(gpu_ctx)
    want, _, masks, labels = seg_ref.segment_planes_fields(before, imgs, p.D, **PARAMS)
    for v in (0, 1):
        np.testing.assert_array_equal(gpu_ctx.segments(v), labels[v], err_msg=f"view {v}: labels")
        _, _, planes, fitted = seg_ref.fit_segments(disp[v], None, labels[v], PARAMS["step"], p.D, PARAMS["tau"], PARAMS["rounds"], PARAMS["min_support"])
        np.testing.assert_array_equal(got[v], np.where(fitted[..., None] != 0, planes, before[v]), err_msg=f"view {v}: fit of disparity_f64")
        np.testing.assert_array_equal(got[v], want[v], err_msg=f"view {v}: segment_planes_fields")
        assert masks[v].any() and np.any(got[v] != before[v])
    gpu_ctx.patchmatch_warm(1, seed=7)  # the stale field is re-scored
    pc = tgs._pc(p, "GRD", 3)
    pm = tgs._pm(p)
    warm_ref.inject(pm, want)
    warm_ref.warm_run(pm, pc, 1, seed=7, schedule=po.SCHED_RASTER, sum_order=DEV)
    tgs._assert_state(gpu_ctx, pm, "one iteration, segment planes, one warm iteration")


def test_merge_after_one_iteration_then_warm_equals_the_restatement(gpu_ctx):
    p = MAIN
    pc = tgs._build(gpu_ctx, p, "grd_fused", 3)
    gpu_ctx.patchmatch(1, seed=9)
    pm = tgs._pm(p)
    pm.run(1, pc, False, **KW)
    tgs._assert_state(gpu_ctx, pm, "one cold iteration")
    start = _fields(gpu_ctx)
    imgs = [gpu_ctx.level_image(v, 0) for v in (0, 1)]
    gpu_ctx.segment_planes(merge=True, **PARAMS)
    _, cands, masks, labels = seg_ref.segment_planes_fields(start, imgs, p.D, **PARAMS)
    taken = seed_ref.merge(pm, pc, cands, masks, DEV)
    assert 0 < taken < 2 * p.w * p.h
    tgs._assert_state(gpu_ctx, pm, "segment planes with merge")
    for v in (0, 1):
        np.testing.assert_array_equal(gpu_ctx.segments(v), labels[v], err_msg=f"view {v}: labels")
    gpu_ctx.patchmatch_warm(1, seed=7)
    warm_ref.warm_run(pm, pc, 1, seed=7, schedule=po.SCHED_RASTER, sum_order=DEV)
    tgs._assert_state(gpu_ctx, pm, "segment planes with merge, one warm iteration")


def test_error_returns(gpu_ctx):
    import crossscalepatchmatch_amd as cs
    p = MAIN
    L = gpu_ctx.L
    l, r = tgs._images(p)
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    n = p.w * p.h
    d = np.zeros((p.h, p.w))
    out = np.zeros((p.h, p.w, 6))
    img = np.ascontiguousarray(l)
    lab = np.zeros((p.h, p.w), np.int32)
    good = capi.seg_params()
    assert (good.step, good.compactness, good.iters, good.tau, good.rounds, good.min_support) == (16, 20, 5, 1.0, 3, 6)
    assert L.cspm_seg_default_params(None) == -1                                       # CSPM_ERR_ARG = -1, CSPM_ERR_STATE = -3
    for w, h, s in ((0, 5, 8), (5, 0, 8), (5, 5, 3), (5, 5, 65)):
        assert L.cspm_segment_count(w, h, s) == -1
    bads = (dict(step=3), dict(step=65), dict(compactness=-1), dict(compactness=256), dict(iters=0), dict(iters=17), dict(rounds=-1), dict(rounds=9),
            dict(min_support=2), dict(tau=-0.5), dict(tau=math.nan))
    seg = lambda im, stride, w, h, par, o: L.cspm_segment_host(0, im, stride, w, h, par, o, None, None)
    assert seg(None, p.w * 3, p.w, p.h, C.byref(good), lab.ctypes.data_as(i32p)) == -1
    assert seg(img.ctypes.data_as(u8p), p.w * 3, p.w, p.h, C.byref(good), None) == -1
    assert seg(img.ctypes.data_as(u8p), p.w * 3 - 1, p.w, p.h, C.byref(good), lab.ctypes.data_as(i32p)) == -1
    assert seg(img.ctypes.data_as(u8p), p.w * 3, 0, p.h, C.byref(good), lab.ctypes.data_as(i32p)) == -1
    assert seg(img.ctypes.data_as(u8p), p.w * 3, p.w, p.h, None, lab.ctypes.data_as(i32p)) == 0  # NULL parameters: the defaults
    np.testing.assert_array_equal(lab, seg_ref.segment(img, **{k: seg_ref.DEFAULTS[k] for k in ("step", "compactness", "iters")})[0])
    fit = lambda disp, labels, w, h, md, par, o: L.cspm_segment_planes_host(0, disp, None, labels, w, h, md, par, None, None, o, None)
    assert fit(None, lab.ctypes.data_as(i32p), p.w, p.h, 16, C.byref(good), out.ctypes.data_as(dp)) == -1
    assert fit(d.ctypes.data_as(dp), None, p.w, p.h, 16, C.byref(good), out.ctypes.data_as(dp)) == -1
    assert fit(d.ctypes.data_as(dp), lab.ctypes.data_as(i32p), p.w, p.h, 16, C.byref(good), None) == -1
    assert fit(d.ctypes.data_as(dp), lab.ctypes.data_as(i32p), 0, p.h, 16, C.byref(good), out.ctypes.data_as(dp)) == -1
    assert fit(d.ctypes.data_as(dp), lab.ctypes.data_as(i32p), p.w, p.h, -1, C.byref(good), out.ctypes.data_as(dp)) == -1
    assert fit(d.ctypes.data_as(dp), lab.ctypes.data_as(i32p), p.w, p.h, 16, None, out.ctypes.data_as(dp)) == 0
    for bad in bads:
        par = capi.seg_params(**bad)
        assert seg(img.ctypes.data_as(u8p), p.w * 3, p.w, p.h, C.byref(par), lab.ctypes.data_as(i32p)) == -1, bad
        assert fit(d.ctypes.data_as(dp), lab.ctypes.data_as(i32p), p.w, p.h, 16, C.byref(par), out.ctypes.data_as(dp)) == -1, bad
    a = cs.StereoContext(0)
    try:
        assert L.cspm_segment_planes(None, None, 0) == -1
        assert L.cspm_get_segments(None, 0, lab.ctypes.data_as(i32p)) == -1
        assert L.cspm_segment_planes(a.p, None, 0) == -3                               # no images
        a.set_images(l, r)
        assert L.cspm_segment_planes(a.p, None, 0) == -3                               # no plane field
        a.set_planes(0, capi.disparity_planes(d), d)
        assert L.cspm_segment_planes(a.p, None, 1) == -3                               # merge without a cost object
        assert L.cspm_segment_planes(a.p, None, 0) == -3                               # no max_dis known yet
        a.build_cost_grd(p.D, 35, 0, 0.0)
        assert L.cspm_get_segments(a.p, 0, lab.ctypes.data_as(i32p)) == -3             # no segmentation yet
        for bad in bads:
            assert L.cspm_segment_planes(a.p, C.byref(capi.seg_params(**bad)), 0) == -1, bad
            assert b"segment planes" in L.cspm_last_error(a.p)
        assert L.cspm_get_segments(a.p, 0, lab.ctypes.data_as(i32p)) == -3
        assert L.cspm_segment_planes(a.p, None, 0) == 0
        assert L.cspm_segment_planes(a.p, C.byref(capi.seg_params(tau=math.inf, step=4)), 1) == 0
        assert L.cspm_get_segments(a.p, 2, lab.ctypes.data_as(i32p)) == -1
        assert L.cspm_get_segments(a.p, 1, None) == -1
        assert L.cspm_get_segments(a.p, 1, lab.ctypes.data_as(i32p)) == 0
        np.testing.assert_array_equal(lab, seg_ref.segment(np.ascontiguousarray(r), 4, 20, 5)[0])
    finally:
        a.close()
    assert n == lab.size


def test_segment_planes_are_timed_as_misc_and_their_merge_as_init(gpu_ctx):
    p = MAIN
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    n = p.w * p.h
    gpu_ctx.pm_init(seed=9)
    gpu_ctx.synchronize()
    gpu_ctx.enable_timing(True)
    try:
        gpu_ctx.reset_timing()
        gpu_ctx.segment_planes(merge=False, step=8)  # one bracket per view; the field is stale afterwards
        gpu_ctx.segment_planes(merge=True, step=8)   # a re-score (one launch, 2n), one bracket and one merge launch per view
        gpu_ctx.synchronize()
        t = gpu_ctx.timing()
    finally:
        gpu_ctx.enable_timing(False)
    assert t["misc"]["launches"] == 4 and t["misc"]["evals"] == 4 * n
    assert t["init"]["launches"] == 3 and t["init"]["evals"] == 4 * n
    assert all(t[k]["launches"] == 0 for k in ("spatial", "view", "refine", "grd", "post"))


# ---- host layer and command line ------------------------------------------------------------------------------------------------------

def test_host_layer_equals_the_c_abi(gpu_ctx, tmp_path):
    """tests/helpers/seg_check.cc: PatchMatchBegin + CSPatchMatch::SegmentPlanes(merge) + PatchMatchFromBegin, and commfunc.h's
    SegmentImage / SegmentPlanes on Mats"""
    exe = _build_helper("seg_check")
    p = MAIN
    l, r = tgs._images(p)
    step, iters, warm = 8, 1, 1
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([p.w, p.h, p.D, 3, iters, step, warm], np.int32).tobytes())
        f.write(np.ascontiguousarray(l).tobytes())
        f.write(np.ascontiguousarray(r).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"foreign refused") == 1
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = p.w * p.h
    K = capi.segment_count(p.w, p.h, step)
    assert raw.size == 2 * 7 * n + n + 6 * n + n + 3 * K
    run = [(raw[v * 7 * n:][:6 * n].reshape(p.h, p.w, 6), raw[v * 7 * n + 6 * n:][:n].reshape(p.h, p.w)) for v in (0, 1)]
    rest = raw[14 * n:]
    tgs._build(gpu_ctx, p, "grd_fused", 3)
    gpu_ctx.patchmatch(iters, seed=12345)
    gpu_ctx.segment_planes(merge=True, step=step)
    gpu_ctx.patchmatch_warm(warm, seed=12345)
    tgs._same_state(run, tgs._state(gpu_ctx), "PatchMatchBegin + SegmentPlanes(merge) + PatchMatchFromBegin")
    labels = capi.segment_host(l, step=step)[0]
    np.testing.assert_array_equal(rest[:n].reshape(p.h, p.w), labels)
    seg, _, planes, fitted = capi.segment_planes_host(gpu_ctx.disparity_f64(0), None, labels, max_dis=p.D, step=step)
    np.testing.assert_array_equal(rest[n:7 * n].reshape(p.h, p.w, 6), planes)
    np.testing.assert_array_equal(rest[7 * n:8 * n].reshape(p.h, p.w), fitted)
    np.testing.assert_array_equal(rest[8 * n:].reshape(K, 3), seg)
    assert fitted.any()


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_seg_step_equals_the_c_abi(gpu_ctx, tmp_path):
    """cspm_main --seg_step=8 --seg_warm_iters=1 (five levels, as the command line builds them) == patchmatch, segment_planes(merge),
    one warm iteration: the 8-bit maps and the PFM maps; a batch list gives the same maps; the flag conflicts are refused"""
    import os
    p = MAIN
    got = tgs._cli(tmp_path, p, "--seg_step=8", "--seg_warm_iters=1", f"--l_disp_pfm={tmp_path}/l.pfm", f"--r_disp_pfm={tmp_path}/r.pfm")
    gpu_ctx.set_images(*tgs._images(p))
    gpu_ctx.build_cost_grd(p.D, 35, 5, 0.3)
    gpu_ctx.patchmatch(1, seed=12345)
    plain = [gpu_ctx.disparity_f64(v) for v in (0, 1)]
    gpu_ctx.segment_planes(merge=True, step=8)
    gpu_ctx.patchmatch_warm(1, seed=12345)
    for v, name in ((0, "l.pfm"), (1, "r.pfm")):
        np.testing.assert_array_equal(got[v], gpu_ctx.disparity_u8(v, tgs.DIS_SCALE), err_msg=f"--seg_step=8, view {v}")
        d = gpu_ctx.disparity_f64(v)
        np.testing.assert_array_equal(_read_pfm(tmp_path / name), d.astype(np.float32), err_msg=f"--seg_step=8 PFM, view {v}")
        assert np.any(d != plain[v])
    cli = os.path.join(tgs.ROOT, "crossscalepatchmatch_amd", "cspm_main")
    base = [cli, f"--max_dis={p.D}", f"--dis_scale={tgs.DIS_SCALE}", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--iters=1", "--quiet=true"]
    with open(tmp_path / "list.txt", "w") as f:
        f.write(f"{tmp_path}/l.png {tmp_path}/r.png {tmp_path}/bl.png {tmp_path}/br.png\n")
    subprocess.check_call(base + ["--seg_step=8", f"--batch_list={tmp_path}/list.txt"], stdout=subprocess.DEVNULL, timeout=300)
    from PIL import Image
    for v, name in ((0, "bl.png"), (1, "br.png")):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / name).convert("L")), got[v], err_msg=f"--batch_list, view {v}")
    files = [f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/xl.png", f"--r_dis_file={tmp_path}/xr.png"]
    for bad in (["--seg_step=8", "--ca_name=BOX"], ["--seg_step=8", "--pc_name=FOREIGN"], ["--seg_step=3"], ["--seg_step=65"], ["--seg_step=8", "--seg_rounds=9"],
                ["--seg_step=8", "--seg_tau=-1"], ["--seg_step=8", "--seg_warm_iters=16"], ["--seg_step=8", "--seg_iters=0"], ["--seg_step=8", "--seg_compactness=256"]):
        out = subprocess.run(base + files + bad, capture_output=True, timeout=120)
        assert out.returncode != 0 and b"--seg_step" in out.stdout, bad
        assert not os.path.exists(tmp_path / "xl.png")
