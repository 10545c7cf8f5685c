"""-m gpu: the products of the axes the suite holds to the oracle one at a time.  Every cost source of the tap engines (the ten of
tests/edge_matrix.py: fused, computed-table, volume-sourced, paired and packed GRD, fused and volume-sourced census and CENGRD, GrdPC /
CSPC) under every schedule at degenerate image sizes; under folded sweep workgroups (CSPM_OPT_SWEEP_FOLD) with the persistent sweep,
the per-diagonal launches and the dataflow sweep; with the row kernels' items handed out as claimed column bands (CSPM_ROW_CLAIM) and
the refinement split into several launches (CSPM_REFINE_CHUNK); and on tie-heavy pairs through CENGRD, the snapshot schedule and the
fold.  Every comparison is assert_array_equal against the oracle in the device order: norm, param and min_cost of both views, the
8-bit and f64 disparity maps, and the post-processed maps where a whole run is made.  The one input the reference cannot run -- GrdPC /
CSPC with max_dis > width, where its single wrap-around reads beyond the row -- must be refused with CSPM_ERR_ARG, and runs with
max_dis = width instead.  tests/test_edge_matrix.py checks on the CPU that none of the cases is vacuous."""
import contextlib
import functools
import os

import numpy as np
import pytest

import edge_matrix as em
import pp_sub_ref
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

assert capi.SCHED_DIFFUSE == em.DIFFUSE and capi.SCHED_REDBLACK == em.REDBLACK and capi.SCHED_RASTER == em.RASTER


def _opt(name):
    return getattr(capi, name)


@contextlib.contextmanager
def _built(ctx, src, pair, sn, lam):
    """the pair and the source's cost object on the context, the source's "active" options asserted; every option the source touched
    is back at the library's default afterwards"""
    l, r = em.images(pair)
    try:
        for key, value in src.options.items():
            ctx.set_option(_opt(key), value)
        ctx.set_images(l, r)
        getattr(ctx, src.build)(em.size_of(pair)[2], em.WND, sn, lam, **src.kwargs)
        assert ctx.levels == max(sn, 1)
        for key, value in src.active.items():
            assert ctx.get_option(_opt(key)) == value, f"{src.name}, {em.pair_id(pair)}, levels {sn}: {key}"
        yield
    finally:
        for key, value in src.restore.items():
            ctx.set_option(_opt(key), value)


@contextlib.contextmanager
def _options(ctx, **options):
    """options by their capi names, back at 0 afterwards (the library's default of every option used here)"""
    try:
        for key, value in options.items():
            ctx.set_option(_opt(key), value)
        yield
    finally:
        for key in options:
            ctx.set_option(_opt(key), 0)


def _assert_refused(ctx, src, pair):
    """GrdPC / CSPC with max_dis > width (edge_matrix.refused: the reference's single wrap-around reads beyond the row, grd_pc.cc:153-165,
    cspc.cc:153-166): CSPM_ERR_ARG as include/cspm.h states, with and without a pyramid; the context stays usable"""
    assert src.kind == "IMG" and em.size_of(pair)[2] > em.size_of(pair)[0]
    ctx.set_images(*em.images(pair))
    for sn, lam in em.MODES:
        with pytest.raises(capi.CspmError, match=em.REFUSAL):
            ctx.build_cost_img(em.size_of(pair)[2], em.WND, sn, lam)
    ctx.build_cost_img(em.size_of(pair)[0], em.WND, 0, 0.0)  # max_dis = width is taken
    ctx.pm_init(seed=em.SEED)


def _gkw(sched, K, early_exit=1, seed=em.SEED):
    return dict(seed=seed, schedule=sched, rb_rounds=1, rb_neighbours=K, early_exit=early_exit)


def _assert_state(ctx, state, what):
    """state: [(planes (h, w, 9), min_cost)] per view (edge_matrix.state_of)"""
    for v in (0, 1):
        npar, cost = ctx.get_planes(v)
        np.testing.assert_array_equal(npar[..., :3], state[v][0][..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], state[v][0][..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, state[v][1], err_msg=f"{what}: min_cost, view {v}")


def _field(state, v):
    return np.concatenate([state[v][0][..., 0:3], state[v][0][..., 6:9]], -1)


def _assert_run(ctx, run, what):
    """a whole run: the state, PlaneToDisp's maps, then cspm_postprocess"""
    _assert_state(ctx, run.state, what)
    for v in (0, 1):
        np.testing.assert_array_equal(ctx.disparity_u8(v, em.DIS_SCALE), run.dis[v], err_msg=f"{what}: 8-bit map, view {v}")
        np.testing.assert_array_equal(ctx.disparity_f64(v), run.disp[v], err_msg=f"{what}: disparity, view {v}")
    lo, ro = ctx.postprocess(em.DIS_SCALE)
    np.testing.assert_array_equal(lo, run.post[0], err_msg=f"{what}: post-processed left map")
    np.testing.assert_array_equal(ro, run.post[1], err_msg=f"{what}: post-processed right map")


def _whole_run(ctx, src, pair, sn, lam, sched, K, what, early_exit=1, seed=em.SEED):
    ctx.patchmatch(em.ITERS, **_gkw(sched, K, early_exit, seed))
    run = em.whole_run(pair, src.kind, sn, lam, sched, K, seed)
    _assert_run(ctx, run, what)
    return run


# ---- a. degenerate sizes ---------------------------------------------------------------------------------------------------------

GEOM_CASES = [(g, k) for k in em.KINDS for g in em.geometries_of(k)]


@pytest.mark.parametrize("geom,kind", GEOM_CASES, ids=[f"{em.pair_id(g)}-{k}" for g, k in GEOM_CASES])
def test_every_source_and_schedule_at_degenerate_sizes(gpu_ctx, geom, kind):
    """1x1, single rows and columns, images smaller than the window and than the far offsets of the snapshot schedule, max_dis > width,
    max_dis = 1, pyramids that collapse to 1x1 and to levels without a single disparity: every source of the kind, single scale and five
    levels, raster, red-black and the snapshot schedule, two iterations and the post-processing.  GrdPC / CSPC refuse max_dis > width and
    run the same sizes with max_dis = width instead."""
    fallbacks = gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    for src in em.sources_of(kind):
        if em.refused(geom, kind):
            _assert_refused(gpu_ctx, src, geom)
            continue
        for sn, lam in em.MODES:
            with _built(gpu_ctx, src, geom, sn, lam):
                for sched, K in em.schedules_at(geom):
                    _whole_run(gpu_ctx, src, geom, sn, lam, sched, K, f"{src.name}, levels {sn}, {em.sched_id(sched, K)}")
    assert gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == fallbacks


# ---- b. the folded sweep ---------------------------------------------------------------------------------------------------------

SWEEPS = [("persistent", {}), ("per-diagonal launches", dict(OPT_RASTER_LAUNCHES=1)), ("dataflow", dict(OPT_SWEEP_FLOW=1))]


FOLD_CASES = [(n, p) for n, s in em.SOURCES.items() for p in em.fold_pairs_of(s.kind)]


@pytest.mark.parametrize("name,pair", FOLD_CASES, ids=[f"{n}-{em.pair_id(p)}" for n, p in FOLD_CASES])
def test_folded_sweep_every_source(gpu_ctx, name, pair):
    """CSPM_OPT_SWEEP_FOLD = 1 (what every caller with pairs in flight sets, whatever the cost): workgroups of levels - 1 waves, the
    coarsest level shared between them.  With four and five levels, from the random init both sweep directions, each as the persistent
    sweep, as per-diagonal launches and as the dataflow sweep from the same start; then a whole run.  No sweep may have timed out: the
    planes are the persistent kernels' own.  Three levels with the option on (one pair) do not fold and give the oracle's planes all
    the same.  (One id per source and pair: the oracle's share of an id stays at a few seconds.)"""
    src = em.SOURCES[name]
    if em.refused(pair, src.kind):
        return _assert_refused(gpu_ctx, src, pair)
    fallbacks = gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    levels = em.FOLD_LEVELS + ((em.UNFOLDED_CASE[1],) if pair == em.UNFOLDED_CASE[0] else ())
    with _options(gpu_ctx, OPT_SWEEP_FOLD=1):
        for sn in levels:
            what = f"{name}, {em.pair_id(pair)}, {sn} levels"
            states = em.sweep_phases(pair, src.kind, sn, em.FOLD_LAM)
            with _built(gpu_ctx, src, pair, sn, em.FOLD_LAM):
                gpu_ctx.pm_init(**_gkw(em.RASTER, 4))
                _assert_state(gpu_ctx, states[0], f"{what}: random init")
                for it in (0, 1):
                    start = [gpu_ctx.get_planes(v) for v in (0, 1)]
                    for k, (sweep, options) in enumerate(SWEEPS):
                        if k:
                            for v in (0, 1):
                                gpu_ctx.set_planes(v, *start[v])
                        with _options(gpu_ctx, **options):
                            gpu_ctx.pm_spatial(it, **_gkw(em.RASTER, 4))
                            _assert_state(gpu_ctx, states[it + 1], f"{what}: sweep of iteration {it}, {sweep}")
                _whole_run(gpu_ctx, src, pair, sn, em.FOLD_LAM, em.RASTER, 4, f"{what}: whole run")
    assert gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == fallbacks


# ---- c. the row kernels' hand-out ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=em.ROW_ENV, ids=["%s=%s" % e for e in em.ROW_ENV])
def row_ctx(request):
    """a context created under CSPM_ROW_CLAIM=1 (claimed column bands for every row-engine launch), CSPM_REFINE_CHUNK=1 (one launch per
    halving step of PlaneRefinement) or CSPM_REFINE_CHUNK=3 (launches of 3, 3, ... and a shorter last one)"""
    import crossscalepatchmatch_amd as cs
    key, value = request.param
    os.environ[key] = value
    try:
        ctx = cs.StereoContext(0)
    finally:
        del os.environ[key]
    try:
        yield ctx
    finally:
        ctx.close()


@pytest.mark.parametrize("name", em.ROW_SOURCES)
def test_row_hand_out_every_source(gpu_ctx, row_ctx, name):
    """one source of each element layout (12-byte GRD pixels, f64 volumes, 16-byte census elements, census elements with their gradient
    array, GrdPC / CSPC pixels) through k_init, k_view_eval, k_refine and k_spatial_diffuse with the items handed out the other way:
    whole runs with five levels under raster and the snapshot schedule at 1x1 .. 129x3, and one single-scale raster run"""
    src = em.SOURCES[name]
    cases = [(pair, 5, 0.3, sched, K) for pair in em.row_pairs_of(src.kind) for sched, K in em.ROW_SCHEDULES] + [(em.ROW_SINGLE_SCALE_PAIR, 0, 0.0, em.RASTER, 4)]
    for pair, sn, lam, sched, K in cases:
        if em.refused(pair, src.kind):
            _assert_refused(row_ctx, src, pair)
            continue
        with _built(row_ctx, src, pair, sn, lam):
            _whole_run(row_ctx, src, pair, sn, lam, sched, K, f"{name}, {em.pair_id(pair)}, levels {sn}, {em.sched_id(sched, K)}")
    assert row_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 0


# ---- d. ties ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _post_f64(pair, kind, sched, K):
    """tests/pp_sub_ref.py on the oracle's planes of the run"""
    sn, lam = em.TIE_MODE
    run = em.whole_run(pair, kind, sn, lam, sched, K, em.TIE_SEED)
    l, r = em.images(pair)
    return pp_sub_ref.postprocess_f64(run.state[0][0][..., 6:9], run.state[1][0][..., 6:9], l, r, em.size_of(pair)[2])


@pytest.mark.parametrize("early_exit", [1, 0])
@pytest.mark.parametrize("name,sched,K,fold", em.TIE_CASES, ids=[f"{n}-{em.sched_id(s, K)}{'-fold' if f else ''}" for n, s, K, f in em.TIE_CASES])
def test_ties_through_the_newer_paths(gpu_ctx, name, sched, K, fold, early_exit):
    """all-black, all-white and saturated stripes: candidate planes tie exactly and the strict `<` rules decide everything -- through
    CENGRD in both forms, through the snapshot schedule and through folded sweep workgroups, early exit on and off; two iterations,
    cspm_postprocess and cspm_postprocess_f64"""
    src = em.SOURCES[name]
    sn, lam = em.TIE_MODE
    fallbacks = gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    with _options(gpu_ctx, OPT_SWEEP_FOLD=fold):
        for pair in em.TIE_PAIRS:
            what = f"{pair}, {name}, {em.sched_id(sched, K)}, fold {fold}, early_exit {early_exit}"
            with _built(gpu_ctx, src, pair, sn, lam):
                _whole_run(gpu_ctx, src, pair, sn, lam, sched, K, what, early_exit, em.TIE_SEED)
                want = _post_f64(pair, src.kind, sched, K)
                for k, (g, w) in enumerate(zip(gpu_ctx.postprocess_f64(valid=True), want)):
                    np.testing.assert_array_equal(g, w, err_msg=f"{what}: sub-pixel post-processing, output {k}")
    assert gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == fallbacks
