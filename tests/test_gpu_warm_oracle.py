"""Warm-started PatchMatch on the GPU held to the CPU oracle bit for bit: cspm_rescore_planes, the single phases and
cspm_patchmatch_warm from start fields that drive the kernels unlike the random init does (local-stereo fields: all table rows and
exact ties; constant and 2x2-block fields; doubled, out-of-range planes; the previous pair's field), the field_consistent
transitions, capi.coarse_to_fine, CSPatchMatch::PatchMatchFrom and cspm_main --warm_ca.  The expected state is tests/warm_ref.py
(the oracle's phases from an injected field, device summation order); every comparison is assert_array_equal on the six plane
doubles and min_cost of both views.  tests/test_warm_ref.py checks the restatement itself without a GPU."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import ca_ref
import warm_ref
from crossscalepatchmatch_amd import capi, realdata as rd
from crossscalepatchmatch_amd.synth import make_pair
from oracle import pyoracle as po
from test_gpu_warm_start import KINDS, _build_helper, _random_field

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIS_SCALE = 4
RASTER, REDBLACK = po.SCHED_RASTER, po.SCHED_REDBLACK
METHODS = {"box": capi.CA_BOX, "gf": capi.CA_GF}

Pair = collections.namedtuple("Pair", "w h D seed")
Cost = collections.namedtuple("Cost", "cc sn lam src")  # src: the GPU's cell source, ((option, value), ...)
PAIRS = {"small": Pair(64, 48, 16, 11), "mid": Pair(96, 64, 16, 12), "odd": Pair(77, 41, 21, 13),
         "wide": Pair(421, 40, 16, 14),      # wider than a row kernel's 350-column band, not a multiple of 64
         "kinds": Pair(100, 76, 20, 15)}     # three levels down to 25x19: the smallest GF filters (19 px)
KIND_COSTS = {"grd_cs": Cost("GRD", 3, 0.3, ()), "grd_ss": Cost("GRD", 0, 0.0, ()),
              "grd_cs_volumes": Cost("GRD", 3, 0.3, (("volumes", True),)), "grd_ss_no_tables": Cost("GRD", 0, 0.0, (("table_volumes", False),)),
              "cen_cs": Cost("CEN", 3, 0.3, ()), "cen_ss_volumes": Cost("CEN", 0, 0.0, (("volumes", True),)),
              "grdpc": Cost("IMG", 0, 0.0, ()), "cspc": Cost("IMG", 3, 0.3, ())}
assert sorted(KIND_COSTS) == sorted(KINDS)  # the cost kinds of tests/test_gpu_warm_start.py, one oracle cost object each
FIELDS = ["box", "gf", "constant", "constant_top", "constant_zero", "blocks2x2", "random", "previous_pair"]


@functools.lru_cache(maxsize=None)
def _images(p):
    l, r, _, _ = make_pair(p.w, p.h, p.D, regions=3, seed=p.seed)
    return l, r


@functools.lru_cache(maxsize=None)
def _pc(p, cc, sn, lam):
    l, r = _images(p)
    return po.PlaneCost(l, r, p.D, 35, sn, lam, cc)


def _gpu_build(ctx, D, cost, lam=None):
    src = dict(cost.src)
    lam = cost.lam if lam is None else lam
    volumes = src.get("volumes", False)
    if cost.cc == "GRD":
        pairs, tables = src.get("sweep_pairs", False), src.get("table_volumes", True)
        ctx.build_cost_grd(D, 35, cost.sn, lam, volumes=volumes, sweep_pairs=pairs, table_volumes=tables)
        assert ctx.get_option(capi.OPT_SWEEP_PAIRS_ACTIVE) == int(pairs and not volumes)
        assert ctx.get_option(capi.OPT_TABLE_VOLUMES_ACTIVE) == int(tables and not volumes)
    elif cost.cc == "CEN":
        ctx.build_cost_cen(D, 35, cost.sn, lam, volumes=volumes)
    else:
        ctx.build_cost_img(D, 35, cost.sn, lam)


def _feasible(name, p, sn):
    """BoxCA / GFCA filter every level: the coarsest one has to hold the filter (7 / 19 px, ca_ref.MIN_SIZE)"""
    if name not in METHODS:
        return True
    w, h = p.w, p.h
    for _ in range(max(sn, 1) - 1):
        w, h = (w + 1) // 2, (h + 1) // 2
    return min(w, h) >= ca_ref.MIN_SIZE[name.upper()]


def _deepest(name, p):
    """GRD cross-scale, lambda 0.3, with as many of five levels as the start field allows"""
    return Cost("GRD", max(sn for sn in (2, 3, 4, 5) if _feasible(name, p, sn)), 0.3, ())


def _made_field(name, rng, w, h, D):
    if name == "constant":
        return ca_ref.planes_of(np.full((h, w), D // 2))
    if name == "constant_top":
        return ca_ref.planes_of(np.full((h, w), D - 1))
    if name == "constant_zero":
        return ca_ref.planes_of(np.full((h, w), 0))
    if name == "blocks2x2":  # identical planes in 2x2 blocks; the doubled c takes about half of them to or beyond max_dis
        return warm_ref.upsample([_random_field(rng, (w + 1) // 2, (h + 1) // 2, D)], w, h)[0]
    if name == "random":
        return _random_field(rng, w, h, D)
    raise ValueError(name)


def _assert_field(ctx, fields, what):
    for v in (0, 1):
        np.testing.assert_array_equal(ctx.get_planes(v)[0], fields[v], err_msg=f"{what}: start field, view {v}")


def _prepare(ctx, name, p, cost, stale=-7.0):
    """the context gets p's images, the cost object and the start field `name`; returns (pc, pm, fields) with the same field injected
    into a fresh oracle PatchMatch.  Hand-made fields arrive through cspm_set_planes with `stale` as every min_cost; box / gf and
    previous_pair leave the GPU's own field in place, after it was found equal to the CPU's."""
    l, r = _images(p)
    pc = _pc(p, cost.cc, cost.sn, cost.lam)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    if name in METHODS:
        # the volume-free costs (GrdPC / CSPC) have no cells to aggregate: their field comes from the GRD cells of the same pyramid,
        # then the cost object is replaced (which keeps the field and withdraws its costs)
        ls_cost = cost if cost.cc != "IMG" else Cost("GRD", cost.sn, cost.lam, ())
        fields = warm_ref.local_stereo_fields(_pc(p, ls_cost.cc, ls_cost.sn, ls_cost.lam), name.upper(), p.D, cost.sn > 0)
        ctx.set_images(l, r)
        _gpu_build(ctx, p.D, ls_cost)
        ctx.local_stereo(METHODS[name])
        _assert_field(ctx, fields, f"local stereo {name}")  # a difference here is a finding in local stereo, not in the warm run
        if cost.cc == "IMG":
            _gpu_build(ctx, p.D, cost)
    elif name == "previous_pair":
        q = p._replace(seed=p.seed + 100)
        kw = dict(seed=3, schedule=RASTER)
        prev = po.PatchMatch(*_images(q), p.D, DIS_SCALE)
        prev.run(1, _pc(q, cost.cc, cost.sn, cost.lam), False, sum_order=po.SUM_DEVICE, **kw)
        fields = [warm_ref.field_of(prev, v) for v in (0, 1)]
        ctx.set_images(*_images(q))
        _gpu_build(ctx, p.D, cost)
        ctx.patchmatch(1, **kw)
        _assert_field(ctx, fields, "cold run on the previous pair")
        ctx.set_images(l, r)  # same size: the field stays, its costs belong to the previous pair
        _gpu_build(ctx, p.D, cost)
    else:
        rng = np.random.default_rng(p.seed * 1000 + FIELDS.index(name))
        fields = [_made_field(name, rng, p.w, p.h, p.D) for _ in (0, 1)]
        ctx.set_images(l, r)
        _gpu_build(ctx, p.D, cost)
        for v in (0, 1):
            ctx.set_planes(v, fields[v], np.full((p.h, p.w), stale))
    warm_ref.inject(pm, fields)
    return pc, pm, fields


def _assert_state(got, pm, what):
    """got: a context, or [(norm_param, min_cost)] per view"""
    for v in (0, 1):
        npar, cost = got.get_planes(v) if hasattr(got, "get_planes") else got[v]
        P = pm.planes(v)
        np.testing.assert_array_equal(npar[..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, pm.min_cost(v), err_msg=f"{what}: min_cost, view {v}")


def _changed(pm, fields):
    """pixels of both views whose oracle plane differs from fields"""
    return int(sum(np.any(warm_ref.field_of(pm, v) != fields[v], axis=2).sum() for v in (0, 1)))


def _assert_maps(ctx, pm, what):
    """PlaneToDisp and PostProcessing behind the run == the oracle's"""
    pm.plane_to_disp()
    for v in (0, 1):
        np.testing.assert_array_equal(ctx.disparity_u8(v, DIS_SCALE), pm.dis(v), err_msg=f"{what}: 8-bit map, view {v}")
    pm.postprocess()
    lo, ro = ctx.postprocess(DIS_SCALE)
    np.testing.assert_array_equal(lo, pm.dis(0), err_msg=f"{what}: post-processed left map")
    np.testing.assert_array_equal(ro, pm.dis(1), err_msg=f"{what}: post-processed right map")


# ---- a. re-score ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIELDS)
def test_rescore_equals_the_oracle(gpu_ctx, name, kind):
    """k_rescore on a non-init field, every cost kind: garbage costs in, the oracle's plane costs out, the planes untouched"""
    p = PAIRS["kinds"]
    pc, pm, fields = _prepare(gpu_ctx, name, p, KIND_COSTS[kind])
    for v in (0, 1):
        gpu_ctx.set_planes(v, gpu_ctx.get_planes(v)[0], np.full((p.h, p.w), -7.0))
    gpu_ctx.rescore_planes()
    warm_ref.rescore(pm, pc, po.SUM_DEVICE)
    _assert_state(gpu_ctx, pm, f"{name}/{kind}")
    assert _changed(pm, fields) == 0
    assert all(np.all(pm.min_cost(v) != -7.0) for v in (0, 1))  # no garbage cost is left


# ---- b. phase by phase from a warm field ----------------------------------------------------------------------------------------

Cfg = collections.namedtuple("Cfg", "id sched early_exit src sn view_sort launches fold")
CFGS = [Cfg("raster_fused", RASTER, 1, (), 3, 1, 0, 0),
        Cfg("redblack_fused", REDBLACK, 1, (), 3, 1, 0, 0),
        Cfg("raster_computed_tables_noexit_unsorted_launches", RASTER, 0, (("table_volumes", False),), 3, 0, 1, 0),
        Cfg("redblack_volumes_noexit_ss", REDBLACK, 0, (("volumes", True),), 0, 1, 0, 0),
        Cfg("raster_sweep_pairs_2", RASTER, 1, (("sweep_pairs", True),), 2, 1, 0, 0),
        Cfg("raster_volumes_unsorted_2", RASTER, 1, (("volumes", True),), 2, 0, 0, 0),
        Cfg("raster_fold_4", RASTER, 1, (), 4, 1, 0, 1),
        Cfg("raster_fold_5_launches", RASTER, 1, (), 5, 1, 1, 1)]
# a local-stereo field only where the coarsest level holds its filter: such a case is not generated otherwise
PHASE_CASES = [pytest.param(name, cfg, id=f"{name}-{cfg.id}") for cfg in CFGS for name in FIELDS if _feasible(name, PAIRS["small"], cfg.sn)]
assert {c.values[0] for c in PHASE_CASES} == set(FIELDS)


@pytest.mark.parametrize("name,cfg", PHASE_CASES)
def test_phase_by_phase_from_a_warm_field(gpu_ctx, name, cfg):
    """re-score, then spatial / view / refine of iterations 0 and 1, compared after every phase so that a failure names the kernel"""
    p = PAIRS["small"]
    gpu_ctx.set_option(capi.OPT_VIEW_SORT, cfg.view_sort)
    gpu_ctx.set_option(capi.OPT_RASTER_LAUNCHES, cfg.launches)
    gpu_ctx.set_option(capi.OPT_SWEEP_FOLD, cfg.fold)
    pc, pm, fields = _prepare(gpu_ctx, name, p, Cost("GRD", cfg.sn, 0.3 if cfg.sn else 0.0, cfg.src))
    kw = dict(seed=777, schedule=cfg.sched, rb_rounds=2, rb_neighbours=4)
    kw_o = dict(sum_order=po.SUM_DEVICE, **kw)
    kw_g = dict(early_exit=cfg.early_exit, **kw)
    gpu_ctx.rescore_planes()
    warm_ref.rescore(pm, pc, po.SUM_DEVICE)
    _assert_state(gpu_ctx, pm, "re-score")
    for it in (0, 1):
        for phase in ("spatial", "view", "refine"):
            before = [warm_ref.field_of(pm, v) for v in (0, 1)]
            getattr(pm, phase)(it, pc, **kw_o)
            getattr(gpu_ctx, "pm_" + phase)(it, **kw_g)
            _assert_state(gpu_ctx, pm, f"{phase} {it}")
            if it == 0 and phase == "spatial" and name.startswith("constant"):
                assert _changed(pm, before) == 0  # every neighbour carries the pixel's own plane at its own cost: `<` accepts none
            if it == 0 and phase == "view" and name == "box":
                assert _changed(pm, before) > 0
            if phase == "refine":
                assert _changed(pm, fields) > 0


# ---- c. whole warm runs ---------------------------------------------------------------------------------------------------------

def _whole_run(ctx, name, p, cost, iters, **kw):
    # stale costs of -7 lie below every plane cost: a skipped re-score would keep them and, with them, every start plane
    pc, pm, fields = _prepare(ctx, name, p, cost)
    stale = [ctx.get_planes(v)[1] for v in (0, 1)]
    ctx.patchmatch_warm(iters, early_exit=1, **kw)
    warm_ref.warm_run(pm, pc, iters, sum_order=po.SUM_DEVICE, **kw)
    _assert_state(ctx, pm, f"{name} {p} {iters} iterations")
    assert all(np.mean(pm.min_cost(v) != stale[v]) > 0.5 for v in (0, 1))  # (equal by chance where two costs are all max_cost)
    if iters:
        assert _changed(pm, fields) > 0
    else:
        assert _changed(pm, fields) == 0
    _assert_maps(ctx, pm, f"{name} {p} {iters} iterations")


@pytest.mark.parametrize("iters,sched", [(0, RASTER), (1, RASTER), (2, RASTER), (2, REDBLACK)])
@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("pname", ["mid", "odd"])
def test_whole_warm_run(gpu_ctx, pname, name, iters, sched):
    p = PAIRS[pname]
    _whole_run(gpu_ctx, name, p, _deepest(name, p), iters, seed=4242, schedule=sched, rb_rounds=1, rb_neighbours=4)


@pytest.mark.parametrize("iters", [0, 1, 2])
@pytest.mark.parametrize("name", ["box", "constant"])
def test_whole_warm_run_wider_than_a_column_band(gpu_ctx, name, iters):
    p = PAIRS["wide"]
    _whole_run(gpu_ctx, name, p, _deepest(name, p), iters, seed=8, schedule=RASTER)


def test_whole_warm_run_row_shared_rng(gpu_ctx):
    p = PAIRS["mid"]
    _whole_run(gpu_ctx, "random", p, _deepest("random", p), 2, seed=9, schedule=RASTER, rng_mode=po.RNG_ROW_SHARED)


def test_whole_warm_run_two_redblack_rounds_two_neighbours(gpu_ctx):
    p = PAIRS["odd"]
    _whole_run(gpu_ctx, "blocks2x2", p, _deepest("blocks2x2", p), 2, seed=10, schedule=REDBLACK, rb_rounds=2, rb_neighbours=2)


# ---- d. state transitions -------------------------------------------------------------------------------------------------------

GRD3 = Cost("GRD", 3, 0.3, ())
KW = dict(seed=21, schedule=RASTER)
KW_O = dict(sum_order=po.SUM_DEVICE, **KW)


def test_two_warm_runs_in_a_row(gpu_ctx):
    """local_stereo -> patchmatch_warm(1) -> patchmatch_warm(1).  The first run has to re-score: a field wrongly taken for
    consistent would keep local stereo's aggregated costs as min_cost.  The second starts from a consistent field, iteration
    numbers 0 again: it continues from the first run's end state, and a re-score there changes no cost."""
    p = PAIRS["small"]
    pc, pm, fields = _prepare(gpu_ctx, "box", p, GRD3)
    gpu_ctx.patchmatch_warm(1, **KW)
    warm_ref.warm_run(pm, pc, 1, **KW_O)
    _assert_state(gpu_ctx, pm, "first warm run")
    first = [warm_ref.field_of(pm, v) for v in (0, 1)]
    gpu_ctx.patchmatch_warm(1, **KW)
    warm_ref.iterate(pm, pc, 1, **KW_O)
    _assert_state(gpu_ctx, pm, "second warm run")
    assert _changed(pm, first) > 0 and _changed(pm, fields) > 0


def test_warm_run_under_a_new_cost_object(gpu_ctx):
    """patchmatch(1) -> build_cost with another reg_lambda -> patchmatch_warm(1).  A new cost object withdraws the stored costs: a
    skipped re-score would compare lambda 0.1 costs with stored lambda 0.3 costs and report the latter as min_cost."""
    p = PAIRS["small"]
    l, r = _images(p)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    gpu_ctx.set_images(l, r)
    _gpu_build(gpu_ctx, p.D, GRD3)
    gpu_ctx.patchmatch(1, **KW)
    pm.run(1, _pc(p, "GRD", 3, 0.3), False, **KW_O)
    _assert_state(gpu_ctx, pm, "cold run")
    cold = [warm_ref.field_of(pm, v) for v in (0, 1)]
    old_cost = [pm.min_cost(v).copy() for v in (0, 1)]
    _gpu_build(gpu_ctx, p.D, GRD3, lam=0.1)
    gpu_ctx.patchmatch_warm(1, **KW)
    warm_ref.warm_run(pm, _pc(p, "GRD", 3, 0.1), 1, **KW_O)
    _assert_state(gpu_ctx, pm, "warm run under lambda 0.1")
    assert _changed(pm, cold) > 0
    kept = [~np.any(warm_ref.field_of(pm, v) != cold[v], axis=2) for v in (0, 1)]
    assert any(np.any(pm.min_cost(v)[kept[v]] != old_cost[v][kept[v]]) for v in (0, 1))  # a kept plane shows its re-scored cost


def test_upsample_rescore_get_then_warm_run(gpu_ctx):
    """upsample_planes_from -> rescore_planes -> get_planes -> patchmatch_warm(1).  The explicit re-score makes the field
    consistent: the run does not repeat it, and its sweep skips a neighbour whose plane is bitwise the pixel's own -- most
    neighbours in a field of 2x2 blocks.  A field marked consistent without its costs re-scored (the stale -3 here) would keep every
    start plane."""
    import crossscalepatchmatch_amd as cs
    p = PAIRS["odd"]
    l, r = _images(p)
    ws, hs = (p.w + 1) // 2, (p.h + 1) // 2
    rng = np.random.default_rng(17)
    half = [_random_field(rng, ws, hs, (p.D + 1) // 2) for _ in (0, 1)]
    src = cs.StereoContext(0)
    try:
        src.set_images(*make_pair(ws, hs, (p.D + 1) // 2, seed=1)[:2])
        for v in (0, 1):
            src.set_planes(v, half[v], np.zeros((hs, ws)))
        gpu_ctx.set_images(l, r)
        _gpu_build(gpu_ctx, p.D, GRD3)
        for v in (0, 1):  # a field and stale costs to overwrite
            gpu_ctx.set_planes(v, np.zeros((p.h, p.w, 6)), np.full((p.h, p.w), -3.0))
        gpu_ctx.upsample_planes_from(src)
    finally:
        src.close()
    pc = _pc(p, "GRD", 3, 0.3)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    fields = warm_ref.upsample(half, p.w, p.h)
    warm_ref.inject(pm, fields)
    gpu_ctx.rescore_planes()
    warm_ref.rescore(pm, pc, po.SUM_DEVICE)
    _assert_state(gpu_ctx, pm, "upsampled and re-scored")
    gpu_ctx.patchmatch_warm(1, **KW)
    warm_ref.iterate(pm, pc, 1, **KW_O)
    _assert_state(gpu_ctx, pm, "warm run")
    assert _changed(pm, fields) > 0


@pytest.mark.parametrize("stale", [-1.0, 1e9], ids=["too_low", "too_high"])
def test_set_planes_costs_are_never_trusted(gpu_ctx, stale):
    """set_planes with wrong costs -> patchmatch_warm(1).  Trusted costs of -1 would reject every candidate and keep every start
    plane at cost -1; trusted costs of 1e9 would let the sweep's first candidate win at every pixel, whatever the pixel's own plane
    costs.  Both end where the restatement ends."""
    p = PAIRS["small"]
    pc, pm, fields = _prepare(gpu_ctx, "random", p, GRD3, stale=stale)
    gpu_ctx.patchmatch_warm(1, **KW)
    warm_ref.warm_run(pm, pc, 1, **KW_O)
    _assert_state(gpu_ctx, pm, f"stale costs {stale}")
    assert 0 < _changed(pm, fields) < 2 * p.w * p.h  # some start planes lost, some survived


def test_sweep_timeout_retry_equals_the_oracle():
    """The existing hook (CSPM_OPT_SWEEP_TIMEOUT_MS = 0), once, from a box field: the getter repeats the run from the re-scored
    snapshot.  A retry that re-scored nothing and restored nothing would start from the aborted sweep's planes; one that restored the
    field but not the flag would distrust nothing visible -- the planes decide."""
    import crossscalepatchmatch_amd as cs
    p = Pair(128, 96, 24, 21)
    ctx = cs.StereoContext(0)
    try:
        pc, pm, fields = _prepare(ctx, "box", p, GRD3)
        assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 0
        ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 0)
        try:
            ctx.patchmatch_warm(2, seed=9, schedule=RASTER)
            got = [ctx.get_planes(v) for v in (0, 1)]
        finally:
            ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 3000)
        assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 1
        warm_ref.warm_run(pm, pc, 2, seed=9, schedule=RASTER, sum_order=po.SUM_DEVICE)
        _assert_state(got, pm, "repeated warm run")
        assert _changed(pm, fields) > 0
    finally:
        ctx.close()


# ---- e. coarse to fine ----------------------------------------------------------------------------------------------------------

def _levels_allowed(w, h, max_dis):
    """cross-scale levels, five at most, that still see the pair: every level at least 2 px in both directions with a disparity
    range D_s = max_dis >> s of at least 1 (at D_s = 0 every tap is out of range)"""
    n = 0
    while n < 5 and min(w, h) >= 2 and max_dis >= 1:
        n, w, h, max_dis = n + 1, (w + 1) // 2, (h + 1) // 2, max_dis // 2
    return n


def _coarse_to_fine(gpu_ctx, l, r, D, lam, coarse_iters):
    h, w = l.shape[:2]
    sn = _levels_allowed((w + 1) // 2, (h + 1) // 2, (D + 1) // 2)
    capi.coarse_to_fine(l, r, D, coarse_iters, 1, "GRD", 35, sn, lam, ctx=gpu_ctx, **KW)
    pm, _ = warm_ref.coarse_to_fine(l, r, D, coarse_iters, 1, "GRD", 35, sn, lam, dis_scale=DIS_SCALE, **KW_O)
    _assert_state(gpu_ctx, pm, f"coarse to fine, {sn} levels")
    f = warm_ref.field_of(pm, 0)[: h // 2 * 2, : w // 2 * 2]
    assert np.any(f[0::2, 0::2] != f[1::2, 1::2])  # the fine iteration broke up 2x2 blocks of the upsampled field
    _assert_maps(gpu_ctx, pm, "coarse to fine")
    return sn


def test_coarse_to_fine_odd_sized_pair(gpu_ctx):
    p = PAIRS["odd"]  # 77x41, max_dis 21: the half-size pair is 39x21 with max_dis 11
    assert _coarse_to_fine(gpu_ctx, *_images(p), p.D, 0.3, 2) == 4


def test_coarse_to_fine_motorcycle_crop(gpu_ctx):
    cfg, l, r, _ = rd.load_crop()  # 200x128, max_dis 32: the half-size pair is 100x64 with max_dis 16
    assert _coarse_to_fine(gpu_ctx, l, r, cfg["max_dis"], cfg["reg_lambda"], 3) == 5


# ---- f. host layer and command line ---------------------------------------------------------------------------------------------

def test_patchmatch_from_equals_the_oracle(tmp_path):
    """tests/helpers/warm_from_check.cc: LocalStereo + PatchMatchFrom, then SetPlanes of its end field under a second cost object +
    PatchMatchFrom -- each == the restatement (the C ABI's default parameters: seed 12345, raster)"""
    exe = _build_helper("warm_from_check")
    p = Pair(128, 96, 24, 21)
    l, r = _images(p)
    iters = 2
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([p.w, p.h, p.D, 3, capi.CA_BOX, iters], np.int32).tobytes())
        f.write(np.ascontiguousarray(l).tobytes())
        f.write(np.ascontiguousarray(r).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = p.w * p.h
    assert raw.size == 4 * 7 * n
    runs = [[(raw[(2 * k + v) * 7 * n:][:6 * n].reshape(p.h, p.w, 6), raw[(2 * k + v) * 7 * n + 6 * n:][:n].reshape(p.h, p.w))
             for v in (0, 1)] for k in (0, 1)]
    pc = _pc(p, "GRD", 3, 0.3)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    fields = warm_ref.local_stereo_fields(pc, "BOX", p.D, True)
    warm_ref.inject(pm, fields)
    kw = dict(seed=12345, schedule=RASTER, sum_order=po.SUM_DEVICE)
    warm_ref.warm_run(pm, pc, iters, **kw)
    _assert_state(runs[0], pm, "LocalStereo + PatchMatchFrom")
    assert _changed(pm, fields) > 0
    first = [warm_ref.field_of(pm, v) for v in (0, 1)]
    warm_ref.warm_run(pm, pc, iters, **kw)  # SetPlanes carries the planes only: the second matcher re-scores them
    _assert_state(runs[1], pm, "SetPlanes + PatchMatchFrom")
    assert _changed(pm, first) > 0


def test_cli_warm_ca_box_equals_the_oracle(tmp_path):
    """cspm_main --warm_ca=BOX --iters=2 --use_pp=true: its 8-bit maps == the restatement's post-processed maps"""
    from PIL import Image
    p = Pair(160, 128, 24, 22)  # five levels down to 10x8: BOX needs 7
    l, r = _images(p)
    lf, rf = tmp_path / "l.png", tmp_path / "r.png"
    Image.fromarray(np.ascontiguousarray(l[..., ::-1])).save(lf)
    Image.fromarray(np.ascontiguousarray(r[..., ::-1])).save(rf)
    cli = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    subprocess.check_call([cli, f"--l_img_file={lf}", f"--r_img_file={rf}", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png",
                           f"--max_dis={p.D}", f"--dis_scale={DIS_SCALE}", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3",
                           "--use_pp=true", "--iters=2", "--warm_ca=BOX", "--quiet=true"], stdout=subprocess.DEVNULL, timeout=300)
    pc = _pc(p, "GRD", 5, 0.3)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    fields = warm_ref.local_stereo_fields(pc, "BOX", p.D, True)
    warm_ref.inject(pm, fields)
    warm_ref.warm_run(pm, pc, 2, seed=12345, schedule=RASTER, sum_order=po.SUM_DEVICE)
    assert _changed(pm, fields) > 0
    pm.plane_to_disp()
    raw = pm.dis(0)
    pm.postprocess()
    assert np.any(pm.dis(0) != raw)  # post-processing changed pixels
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "ld.png").convert("L")), pm.dis(0))
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "rd.png").convert("L")), pm.dis(1))
