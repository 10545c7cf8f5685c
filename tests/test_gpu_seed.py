"""Candidate-field merging on the GPU (include/cspm.h "candidate fields") held to tests/seed_ref.py bit for bit:
cspm_merge_planes, cspm_merge_planes_host and cspm_pm_init_keep under every cost source of the row engine, the seeded pipelines
built from them, their error returns and timing, CSPatchMatch::PatchMatchSeeded / PatchMatchKeep and cspm_main --l_seed_pfm /
--seed_ca.  Every comparison with the restatement is assert_array_equal on the six plane doubles and min_cost of both views, the
restatement summing in the device order."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import ca_ref
import cengrd_ref
import seed_ref
import warm_ref
from crossscalepatchmatch_amd import capi
from crossscalepatchmatch_amd.synth import make_pair
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIS_SCALE = 4
DEV = po.SUM_DEVICE
Pair = collections.namedtuple("Pair", "w h D seed")
MAIN = Pair(80, 56, 16, 21)
WAVE = {64: Pair(64, 24, 16, 22), 65: Pair(65, 24, 16, 23)}  # a full wave; a full wave and a one-lane tail
COSTS = ["grd_fused", "grd_volumes", "cen", "cengrd_volumes", "cengrd_fused", "img"]
ORACLE_CC = {"grd_fused": "GRD", "grd_volumes": "GRD", "cen": "CEN", "cengrd_volumes": "CENGRD", "cengrd_fused": "CENGRD", "img": "IMG"}


@functools.lru_cache(maxsize=None)
def _images(p):
    l, r, _, _ = make_pair(p.w, p.h, p.D, regions=3, seed=p.seed)
    return l, r


@functools.lru_cache(maxsize=None)
def _pc(p, cc, sn):
    l, r = _images(p)
    lam = 0.3 if sn else 0.0
    if cc == "CENGRD":
        return cengrd_ref.plane_cost(l, r, p.D, 35, sn, lam)
    return po.PlaneCost(l, r, p.D, 35, sn, lam, cc)


def _build(ctx, p, cost, sn):
    ctx.set_images(*_images(p))
    lam = 0.3 if sn else 0.0
    if cost == "grd_fused":
        ctx.build_cost_grd(p.D, 35, sn, lam)
    elif cost == "grd_volumes":
        ctx.build_cost_grd(p.D, 35, sn, lam, volumes=True)
    elif cost == "cen":
        ctx.build_cost_cen(p.D, 35, sn, lam)
    elif cost in ("cengrd_volumes", "cengrd_fused"):
        ctx.build_cost_cengrd(p.D, 35, sn, lam, fused=cost == "cengrd_fused")
        assert ctx.get_option(capi.OPT_CENGRD_FUSED_ACTIVE) == int(cost == "cengrd_fused")
    else:
        ctx.build_cost_img(p.D, 35, sn, lam)
    return _pc(p, ORACLE_CC[cost], sn)


def _pm(p):
    return po.PatchMatch(*_images(p), p.D, DIS_SCALE)


def _assert_state(got, pm, what):
    """got: a context, or [(norm_param, min_cost)] per view"""
    for v in (0, 1):
        npar, cost = got.get_planes(v) if hasattr(got, "get_planes") else got[v]
        P = pm.planes(v)
        np.testing.assert_array_equal(npar[..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, pm.min_cost(v), err_msg=f"{what}: min_cost, view {v}")


def _same_state(a, b, what):
    for v in (0, 1):
        for x, y, name in zip(a[v], b[v], ("planes", "min_cost")):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}, view {v}")


def _state(ctx):
    return [ctx.get_planes(v) for v in (0, 1)]


@functools.lru_cache(maxsize=None)
def _candidates(p, name):
    """candidate fields and masks per view, by name; computed once and never written to"""
    checker = (np.indices((p.h, p.w)).sum(0) % 2).astype(np.uint8)
    if name == "other_seed":  # the init field of another RNG seed
        pm = _pm(p)
        pm.init(_pc(p, "GRD", 0), seed=4711, sum_order=DEV)  # the planes do not depend on the cost object
        return [warm_ref.field_of(pm, v) for v in (0, 1)], (None, None)
    if name == "box":  # a BOX local-stereo field (of the GRD cells, whatever cost it is offered to)
        sn = 3 if min(p.w, p.h) >= 4 * ca_ref.MIN_SIZE["BOX"] else 0
        return warm_ref.local_stereo_fields(_pc(p, "GRD", sn), "BOX", p.D, sn > 0), (None, None)
    if name == "zero":
        return [ca_ref.planes_of(np.full((p.h, p.w), 0))] * 2, (None, None)
    if name == "top":
        return [ca_ref.planes_of(np.full((p.h, p.w), p.D - 1))] * 2, (None, None)
    if name == "holes":  # NaN and inf entries, a checkerboard mask on one view and its inverse on the other
        rng = np.random.default_rng(p.seed)
        fields = [f.copy() for f in _candidates(p, "other_seed")[0]]
        for f in fields:
            for bad in (np.nan, np.inf, -np.inf):
                ys, xs, ks = rng.integers(0, p.h, 40), rng.integers(0, p.w, 40), rng.integers(0, 6, 40)
                f[ys, xs, ks] = bad
            f[0, 0, 0] = f[p.h - 1, p.w - 1, 5] = np.nan
        return fields, (checker, 1 - checker)
    raise ValueError(name)


def _merge_both(ctx, pm, pc, p, name):
    fields, masks = _candidates(p, name)
    for v in (0, 1):
        ctx.merge_planes(v, fields[v], masks[v])
    return seed_ref.merge(pm, pc, fields, masks, DEV)


# ---- a. the merge, every cost source ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sn", [0, 3], ids=["ss", "cs3"])
@pytest.mark.parametrize("cost", COSTS)
def test_merge_equals_the_restatement(gpu_ctx, cost, sn):
    """cspm_pm_init, then five candidate fields merged one after the other, compared after each"""
    p = MAIN
    pc = _build(gpu_ctx, p, cost, sn)
    pm = _pm(p)
    gpu_ctx.pm_init(seed=9)
    pm.init(pc, seed=9, sum_order=DEV)
    _assert_state(gpu_ctx, pm, "init")
    taken = {}
    for name in ("holes", "top", "zero", "box", "other_seed"):
        taken[name] = _merge_both(gpu_ctx, pm, pc, p, name)
        _assert_state(gpu_ctx, pm, f"{cost} {sn}: merge of {name}")
    assert taken["holes"] > 0 and taken["other_seed"] > 0 and taken["box"] > 0  # candidates did win
    assert _merge_both(gpu_ctx, pm, pc, p, "box") == 0  # a second merge of the same field accepts nothing
    _assert_state(gpu_ctx, pm, "second merge of box")


@pytest.mark.parametrize("sn", [0, 3], ids=["ss", "cs3"])
@pytest.mark.parametrize("w", sorted(WAVE))
def test_merge_full_wave_and_one_lane_tail(gpu_ctx, w, sn):
    p = WAVE[w]
    pc = _build(gpu_ctx, p, "grd_fused", sn)
    pm = _pm(p)
    gpu_ctx.pm_init(seed=9)
    pm.init(pc, seed=9, sum_order=DEV)
    for name in ("holes", "other_seed", "top"):
        _merge_both(gpu_ctx, pm, pc, p, name)
        _assert_state(gpu_ctx, pm, f"width {w}: merge of {name}")
    for v in (0, 1):
        gpu_ctx.set_planes(v, ca_ref.planes_of(np.full((p.h, p.w), 3)), np.zeros((p.h, p.w)))
    warm_ref.inject(pm, [ca_ref.planes_of(np.full((p.h, p.w), 3))] * 2)
    gpu_ctx.pm_init_keep(seed=2)
    warm_ref.rescore(pm, pc, DEV)
    assert seed_ref.init_keep(pm, pc, seed=2, sum_order=DEV) > 0
    _assert_state(gpu_ctx, pm, f"width {w}: keep-init")


# ---- b. context to context --------------------------------------------------------------------------------------------------------

def test_merge_from_a_context_equals_merge_of_its_planes(gpu_ctx):
    import crossscalepatchmatch_amd as cs
    p = MAIN
    pc = _build(gpu_ctx, p, "grd_fused", 3)
    src = cs.StereoContext(0)
    try:
        src.set_images(*_images(p))
        src.build_cost_cen(p.D, 35, 0, 0.0)  # another cost object: only its planes travel
        src.patchmatch(1, seed=33, schedule=capi.SCHED_REDBLACK)
        gpu_ctx.pm_init(seed=9)
        gpu_ctx.merge_planes_from(src)
        got = _state(gpu_ctx)
        fields = [src.get_planes(v)[0] for v in (0, 1)]
    finally:
        src.close()
    gpu_ctx.pm_init(seed=9)
    for v in (0, 1):
        gpu_ctx.merge_planes(v, fields[v])
    _same_state(got, _state(gpu_ctx), "merge_planes_from against merge_planes")
    pm = _pm(p)
    pm.init(pc, seed=9, sum_order=DEV)
    assert seed_ref.merge(pm, pc, fields, (None, None), DEV) > 0
    _assert_state(got, pm, "merge_planes_from")


# ---- c. pipelines -----------------------------------------------------------------------------------------------------------------

SCHEDULES = {"raster": dict(schedule=capi.SCHED_RASTER), "redblack": dict(schedule=capi.SCHED_REDBLACK, rb_rounds=2),
             "diffuse": dict(schedule=capi.SCHED_DIFFUSE, rb_neighbours=8)}


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_all_masked_seeded_run_is_the_cold_run(gpu_ctx, sched):
    p = MAIN
    _build(gpu_ctx, p, "grd_fused", 3)
    kw = dict(seed=17, **SCHEDULES[sched])
    gpu_ctx.patchmatch(2, **kw)
    cold = _state(gpu_ctx)
    zeros = np.zeros((p.h, p.w), np.uint8)
    fields = _candidates(p, "top")[0]
    capi.seeded_patchmatch(gpu_ctx, 2, [(0, fields[0], zeros), (1, fields[1], zeros)], **kw)
    _same_state(_state(gpu_ctx), cold, f"all-masked seeded run, {sched}")


@pytest.mark.parametrize("cost", ["grd_fused", "cengrd_fused"])
def test_seeded_run_equals_the_restatement_with_and_without_early_exit(gpu_ctx, cost):
    p = MAIN
    pc = _build(gpu_ctx, p, cost, 3)
    kw = dict(seed=17, schedule=capi.SCHED_RASTER)
    seeds = [_candidates(p, "box"), _candidates(p, "holes")]
    runs = []
    for early in (1, 0):
        capi.seeded_patchmatch(gpu_ctx, 1, [(v, f[v], m[v]) for f, m in seeds for v in (0, 1)], early_exit=early, **kw)
        runs.append(_state(gpu_ctx))
    _same_state(runs[0], runs[1], "early_exit 1 against 0")
    pm = _pm(p)
    seed_ref.seeded_run(pm, pc, 1, seeds, sum_order=DEV, **kw)
    _assert_state(runs[0], pm, f"seeded run, {cost}")


def test_keep_init(gpu_ctx):
    """after cspm_pm_init with the same params: nothing changes; after a constant field with bogus costs: the restatement, with and
    without the early exit; local stereo + keep-init + one iteration: the restatement's keep_run"""
    p = MAIN
    pc = _build(gpu_ctx, p, "grd_fused", 3)
    gpu_ctx.pm_init(seed=5)
    first = _state(gpu_ctx)
    gpu_ctx.pm_init_keep(seed=5)
    _same_state(_state(gpu_ctx), first, "keep-init after the init it repeats")
    const = ca_ref.planes_of(np.full((p.h, p.w), p.D // 2))
    got = []
    for early in (1, 0):
        for v in (0, 1):
            gpu_ctx.set_planes(v, const, np.full((p.h, p.w), -7.0))  # below every cost: a skipped re-score keeps every pixel
        gpu_ctx.pm_init_keep(seed=6, early_exit=early)
        got.append(_state(gpu_ctx))
    _same_state(got[0], got[1], "keep-init, early_exit 1 against 0")
    pm = _pm(p)
    warm_ref.inject(pm, [const, const])
    warm_ref.rescore(pm, pc, DEV)
    taken = seed_ref.init_keep(pm, pc, seed=6, sum_order=DEV)
    assert 0 < taken < 2 * p.w * p.h
    _assert_state(got[0], pm, "keep-init over a constant field")
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.pm_init_keep(seed=6)
    gpu_ctx.patchmatch_warm(1, seed=6)
    warm_ref.inject(pm, _candidates(p, "box")[0])
    seed_ref.keep_run(pm, pc, 1, seed=6, schedule=po.SCHED_RASTER, sum_order=DEV)
    _assert_state(gpu_ctx, pm, "local stereo, keep-init, one iteration")


def test_merge_rescores_a_field_that_is_not_consistent(gpu_ctx):
    p = MAIN
    pc = _build(gpu_ctx, p, "cen", 3)
    start = _candidates(p, "other_seed")[0]
    for bogus in (-7.0, 1e9):  # trusted, the first keeps every start plane and the second lets every candidate win
        for v in (0, 1):
            gpu_ctx.set_planes(v, start[v], np.full((p.h, p.w), bogus))
        pm = _pm(p)
        warm_ref.inject(pm, start)
        warm_ref.rescore(pm, pc, DEV)
        taken = _merge_both(gpu_ctx, pm, pc, p, "box")
        assert 0 < taken < 2 * p.w * p.h
        _assert_state(gpu_ctx, pm, f"merge over stale costs {bogus}")


# ---- d. errors and timing ---------------------------------------------------------------------------------------------------------

def test_error_returns(gpu_ctx):
    import ctypes as C
    import crossscalepatchmatch_amd as cs
    p = MAIN
    L = gpu_ctx.L
    l, r = _images(p)
    f = np.ascontiguousarray(_candidates(p, "top")[0][0])
    fp = f.ctypes.data_as(C.POINTER(C.c_double))
    a, b = cs.StereoContext(0), cs.StereoContext(0)
    try:
        assert L.cspm_pm_init_keep(a.p, None) == -3                   # no cost object (CSPM_ERR_STATE = -3, CSPM_ERR_ARG = -1)
        assert L.cspm_merge_planes_host(a.p, 0, fp, None) == -3       # no cost object
        assert L.cspm_merge_planes(a.p, a.p) == -1                    # src == dst
        assert L.cspm_merge_planes(a.p, b.p) == -3                    # src has no plane field
        b.set_images(l, r)
        b.build_cost_grd(p.D, 35, 0, 0.0)
        b.pm_init(seed=1)
        assert L.cspm_merge_planes(a.p, b.p) == -3                    # dst has no images
        a.set_images(l, r)
        assert L.cspm_merge_planes(a.p, b.p) == -3                    # dst has no cost object
        a.build_cost_grd(p.D, 35, 0, 0.0)
        assert L.cspm_merge_planes(a.p, b.p) == -3                    # dst has no plane field
        assert L.cspm_merge_planes_host(a.p, 0, fp, None) == -3       # no plane field
        a.pm_init_keep(seed=3)                                        # without a field: cspm_pm_init
        keep = _state(a)
        a.pm_init(seed=3)
        _same_state(keep, _state(a), "keep-init without a field")
        assert L.cspm_merge_planes_host(a.p, 2, fp, None) == -1       # bad view
        assert L.cspm_merge_planes_host(a.p, -1, fp, None) == -1
        assert L.cspm_merge_planes_host(a.p, 0, None, None) == -1     # no candidates
        assert L.cspm_merge_planes(a.p, b.p) == 0
        q = WAVE[64]
        b.set_images(*_images(q))
        b.build_cost_grd(q.D, 35, 0, 0.0)
        b.pm_init(seed=1)
        assert L.cspm_merge_planes(a.p, b.p) == -1                    # another size
        assert b"x" in L.cspm_last_error(a.p)
        a.synchronize()
    finally:
        a.close()
        b.close()


def test_merges_are_timed_as_init_launches(gpu_ctx):
    p = MAIN
    _build(gpu_ctx, p, "grd_fused", 3)
    n = p.w * p.h
    gpu_ctx.pm_init(seed=9)
    gpu_ctx.synchronize()
    gpu_ctx.enable_timing(True)
    try:
        gpu_ctx.reset_timing()
        fields, masks = _candidates(p, "holes")
        gpu_ctx.merge_planes(0, fields[0], masks[0])                 # one launch, one evaluation per pixel that has a candidate
        gpu_ctx.merge_planes(1, _candidates(p, "top")[0][1])         # one launch, n evaluations
        gpu_ctx.pm_init_keep(seed=4)                                 # one launch, 2n evaluations
        gpu_ctx.synchronize()
        t = gpu_ctx.timing()
    finally:
        gpu_ctx.enable_timing(False)
    assert t["init"]["launches"] == 3
    assert t["init"]["evals"] == int(seed_ref.has_candidate(fields[0], masks[0]).sum()) + n + 2 * n
    assert all(t[k]["launches"] == 0 for k in ("spatial", "view", "refine"))
    assert len(t) == 7  # CSPM_K_COUNT is unchanged


# ---- e. host layer and command line -----------------------------------------------------------------------------------------------

def _seed_map(p):
    """a disparity map with holes: the BOX field's disparities, NaN, inf and negative values in places"""
    d = _candidates(p, "box")[0][0][..., 5].copy()
    d[::7, ::5] = np.nan
    d[3::11, 2::9] = np.inf
    d[5::13, 1::6] = -1.0
    return d


def _map_candidates(d):
    return [seed_ref.disparity_planes(d), None], [np.isfinite(d) & (d >= 0), None]


def test_host_layer_seeded_and_keep_equal_the_restatement(tmp_path):
    """tests/helpers/seed_check.cc: AddCandidateDisparity + PatchMatchSeeded, and LocalStereo + PatchMatchKeep on a second cost object
    (the C ABI's default parameters: seed 12345, raster); a foreign IPlaneCost is refused by both"""
    exe = _build_helper("seed_check")
    p = MAIN
    l, r = _images(p)
    d = _seed_map(p)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([p.w, p.h, p.D, 3, capi.CA_BOX, 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(l).tobytes())
        f.write(np.ascontiguousarray(r).tobytes())
        f.write(np.ascontiguousarray(d).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(b"foreign refused") == 2
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = p.w * p.h
    assert raw.size == 4 * 7 * n
    runs = [[(raw[(2 * k + v) * 7 * n:][:6 * n].reshape(p.h, p.w, 6), raw[(2 * k + v) * 7 * n + 6 * n:][:n].reshape(p.h, p.w))
             for v in (0, 1)] for k in (0, 1)]
    pc = _pc(p, "GRD", 3)
    kw = dict(seed=12345, schedule=po.SCHED_RASTER, sum_order=DEV)
    pm = _pm(p)
    seed_ref.seeded_run(pm, pc, 1, [_map_candidates(d)], **kw)
    _assert_state(runs[0], pm, "AddCandidateDisparity + PatchMatchSeeded")
    pm = _pm(p)
    warm_ref.inject(pm, _candidates(p, "box")[0])
    seed_ref.keep_run(pm, pc, 1, **kw)
    _assert_state(runs[1], pm, "LocalStereo + PatchMatchKeep")


def _write_pfm(path, d):
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.0\n" % (d.shape[1], d.shape[0]))
        f.write(np.ascontiguousarray(d[::-1], dtype="<f4").tobytes())


def _cli(tmp_path, p, *extra):
    from PIL import Image
    l, r = _images(p)
    lf, rf = tmp_path / "l.png", tmp_path / "r.png"
    Image.fromarray(np.ascontiguousarray(l[..., ::-1])).save(lf)
    Image.fromarray(np.ascontiguousarray(r[..., ::-1])).save(rf)
    cli = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    subprocess.check_call([cli, f"--l_img_file={lf}", f"--r_img_file={rf}", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png",
                           f"--max_dis={p.D}", f"--dis_scale={DIS_SCALE}", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3",
                           "--iters=1", "--quiet=true"] + list(extra), stdout=subprocess.DEVNULL, timeout=300)
    return [np.asarray(Image.open(tmp_path / name).convert("L")) for name in ("ld.png", "rd.png")]


def test_cli_seed_pfm_and_seed_ca_equal_the_restatement(tmp_path):
    """cspm_main --l_seed_pfm and cspm_main --seed_ca=BOX (five levels, as the command line builds them): the 8-bit maps == the
    restatement's"""
    p = MAIN._replace(w=160, h=128, D=24, seed=22)  # five levels down to 10x8: BOX needs 7
    pc = _pc(p, "GRD", 5)
    kw = dict(seed=12345, schedule=po.SCHED_RASTER, sum_order=DEV)
    box = warm_ref.local_stereo_fields(pc, "BOX", p.D, True)
    d = box[0][..., 5].astype(np.float32).astype(np.float64)  # what a float32 PFM carries
    d[::7, ::5] = np.nan
    d[5::13, 1::6] = -1.0
    _write_pfm(tmp_path / "seed.pfm", d)
    got = _cli(tmp_path, p, f"--l_seed_pfm={tmp_path}/seed.pfm")
    pm = _pm(p)
    seed_ref.seeded_run(pm, pc, 1, [_map_candidates(d)], **kw)
    cold = _pm(p)
    cold.run(1, pc, False, **kw)
    assert np.any(warm_ref.field_of(pm, 0) != warm_ref.field_of(cold, 0))  # the seeds changed the run
    pm.plane_to_disp()
    for v in (0, 1):
        np.testing.assert_array_equal(got[v], pm.dis(v), err_msg=f"--l_seed_pfm, view {v}")
    got = _cli(tmp_path, p, "--seed_ca=BOX")
    pm = _pm(p)
    warm_ref.inject(pm, box)
    seed_ref.keep_run(pm, pc, 1, **kw)
    pm.plane_to_disp()
    for v in (0, 1):
        np.testing.assert_array_equal(got[v], pm.dis(v), err_msg=f"--seed_ca=BOX, view {v}")
