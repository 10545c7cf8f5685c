"""-m gpu: the chain engine's sweep on plane fields BUILT to take every leaf of its path decisions (tests/chain_path_ref.py: the all-valid
decision of chain_passes<SRC, 2> and chain_passes<SRC, 1>, plain loop, per level and candidate pair; sweep_candidates' same01 / own0 /
own1 leaves and the three-way dispatch behind them; tests/test_chain_path_ref.py holds the table non-vacuous on the CPU), against the CPU
oracle bit for bit.  cspm_set_planes (trust 0), or cspm_set_planes + cspm_rescore_planes (trust 1), then ONE cspm_pm_spatial in either
direction, each from the freshly set field: the planes of both views are compared as 64-bit patterns (a -0.0 is not a +0.0), the stored
costs as doubles, with PatchMatch.spatial(it, pc, sum_order=SUM_DEVICE).  Every case under the fused GRD cost and all three raster
schedules (the persistent sweep, the dataflow sweep, one launch per anti-diagonal), folded and unfolded workgroups on the five-level
geometries, one workgroup per row band (CSPM_OPT_SWEEP_GRID = 8) on one case of each kind; the probe field of the five-level geometry
under every other sweep source; and at a sample of probes cspm_plane_cost_batch -- the pipelined loop -- on both candidates: the stored
cost is the smaller result, the stored plane that candidate, slot 0 on a tie.  assert_array_equal only; no sweep may fall back.  A
mismatch names the first pixel, its candidates, its sweep leaf and the path of every level."""
import contextlib

import numpy as np
import pytest

import chain_cases as cc
import chain_path_ref as cp
import edge_matrix as em
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

SWEEPS = [("persistent", {}), ("dataflow", dict(OPT_SWEEP_FLOW=1)), ("per-diagonal launches", dict(OPT_RASTER_LAUNCHES=1))]
OTHER_SOURCES = [n for n in em.SOURCES if n not in ("grd_fused", "grd_computed")]  # grd_computed differs in the row engine only
assert set(OTHER_SOURCES) == {"grd_volumes", "grd_pairs", "grd_packed", "cen_fused", "cen_volumes", "cengrd_volumes", "cengrd_fused", "img"}
KW = dict(seed=1, schedule=capi.SCHED_RASTER)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@contextlib.contextmanager
def _options(ctx, **options):
    """options by their capi names, back afterwards at the values they had before"""
    before = {key: ctx.get_option(getattr(capi, key)) for key in options}
    try:
        for key, value in options.items():
            ctx.set_option(getattr(capi, key), value)
        yield
    finally:
        for key, value in before.items():
            ctx.set_option(getattr(capi, key), value)


@contextlib.contextmanager
def _built(ctx, name, src):
    """the case's pair and the source's cost object on the context, the source's "active" options asserted; every option the source
    touched is back at the library's default afterwards (as tests/test_gpu_edge_matrix.py does)"""
    c = cp.BY_NAME[name]
    g = c.geom
    try:
        for key, value in src.options.items():
            ctx.set_option(getattr(capi, key), value)
        ctx.set_images(*cc.images(name))
        getattr(ctx, src.build)(g.max_dis, g.wnd, g.scale_num, c.lam, **src.kwargs)
        assert ctx.levels == max(g.scale_num, 1)
        for key, value in src.active.items():
            assert ctx.get_option(getattr(capi, key)) == value, f"{src.name}: {key}"
        yield
    finally:
        for key, value in src.restore.items():
            ctx.set_option(getattr(capi, key), value)


def _set_start(ctx, name, trust):
    """trust 0: cspm_set_planes with the case's costs (a block field: the oracle's re-score).  trust 1: garbage costs, then
    cspm_rescore_planes, which must store the same costs and sets Pm::trust_cost"""
    st = cc.start(name)
    for v in (0, 1):
        ctx.set_planes(v, st[v][0], np.full(st[v][1].shape, -7.0) if trust else st[v][1])
    if trust:
        ctx.rescore_planes()


def _explain(name, kind, it, trust, v, x, y, got, gcost):
    c = cp.BY_NAME[name]
    F = cc.start(name)[v][0]
    want = cc.swept(name, kind, it)
    leaf, c0, c1, same_bits = cp.sweep_leaves(F, cc.field_of(want, v), cc.INC[it], trust)
    lf = int(leaf[y, x])
    cands = {"eval0 && eval1": [c0[y, x], c1[y, x]], "eval0": [c0[y, x]], "eval1": [c1[y, x]], "none": []}[cp.DISPATCH[lf]]
    paths = cp.level_paths(c.geom, x, y, cands) if cands else []
    wins = [w._asdict() for w in cp.level_windows(c.geom, x, y)]
    return (f"first differing pixel (x {x}, y {y}) of view {v}: device plane {got[y, x].tolist()} cost {gcost[y, x]!r}, oracle plane "
            f"{cc.field_of(want, v)[y, x].tolist()} cost {want[v][1][y, x]!r}; own plane {F[y, x].tolist()}; candidate 0 {c0[y, x].tolist()}, "
            f"candidate 1 {c1[y, x].tolist()} (bitwise equal: {bool(same_bits[y, x])}); sweep leaf {cp.leaf_name(lf)}; level paths {paths}; windows {wins}")


def _assert_swept(ctx, name, kind, it, trust, what):
    want = cc.swept(name, kind, it)
    for v in (0, 1):
        got, gcost = ctx.get_planes(v)
        wf, wcost = cc.field_of(want, v), want[v][1]
        bad = np.argwhere(np.any(_bits(got) != _bits(wf), -1) | ~(gcost == wcost))
        msg = f"{what}, view {v}"
        if len(bad):
            y, x = (int(t) for t in bad[0])
            msg += f": {len(bad)} pixels differ; " + _explain(name, kind, it, trust, v, x, y, got, gcost)
        np.testing.assert_array_equal(_bits(got), _bits(wf), err_msg=msg)
        np.testing.assert_array_equal(gcost, wcost, err_msg=msg)


def _sweeps(ctx, name, kind, what, sweeps=SWEEPS):
    """every schedule, both directions, trust 1 and 0 (probe fields: 0), folded and unfolded where the case asks for it"""
    c = cp.BY_NAME[name]
    for fold in ((0, 1) if c.fold else (0,)):
        with _options(ctx, OPT_SWEEP_FOLD=fold):
            for sweep, options in sweeps:
                with _options(ctx, **options):
                    for it in (0, 1):
                        for trust in ((1, 0) if c.kind == "block" else (0,)):
                            _set_start(ctx, name, trust)
                            if trust:  # cspm_rescore_planes stored the costs the trust-0 run is handed
                                for v in (0, 1):
                                    np.testing.assert_array_equal(ctx.get_planes(v)[1], cc.start(name)[v][1], err_msg=f"{what}: re-score, view {v}")
                            ctx.pm_spatial(it, **KW)
                            _assert_swept(ctx, name, kind, it, trust, f"{what}, {sweep}, fold {fold}, direction {cc.INC[it]:+d}, trust {trust}")


def _cross_check(ctx, name, what):
    """the plain loop against the pipelined one on the same built planes: after a sweep, at a sample of probes of every leaf,
    cspm_plane_cost_batch on both candidates -- the stored cost is the smaller, the stored plane that candidate, slot 0 on a tie"""
    c = cp.BY_NAME[name]
    for it in (0, 1):
        _set_start(ctx, name, 0)
        ctx.pm_spatial(it, **KW)
        for v in (0, 1):
            F, cost = cc.start(name)[v]
            T = cp.probe_tags(c.geom, F, cc.INC[it])[0]
            _, c0, c1, _ = cp.sweep_leaves(F, F, cc.INC[it], False)
            pick = np.zeros(cost.shape, bool)
            for m in T.values():  # up to six probes of every leaf, spread over the leaf's pixels
                idx = np.flatnonzero(m)
                pick.flat[idx[np.linspace(0, len(idx) - 1, min(6, len(idx))).astype(int)] if len(idx) else idx] = True
            ys, xs = np.nonzero(pick)
            xy = np.stack([xs, ys], 1).astype(np.int32)
            k0 = ctx.plane_cost_batch(v, xy, c0[ys, xs])
            k1 = ctx.plane_cost_batch(v, xy, c1[ys, xs])
            second = k1 < k0
            got, gcost = ctx.get_planes(v)
            np.testing.assert_array_equal(gcost[ys, xs], np.where(second, k1, k0), err_msg=f"{what}: stored cost vs plane_cost_batch, view {v}, direction {cc.INC[it]:+d}")
            np.testing.assert_array_equal(_bits(got[ys, xs]), _bits(np.where(second[:, None], c1[ys, xs], c0[ys, xs])),
                                          err_msg=f"{what}: stored plane vs the cheaper candidate, view {v}, direction {cc.INC[it]:+d}")
            assert len(xy) >= len(T) and second.any() and (~second).any()


@pytest.mark.parametrize("name", [c.name for c in cp.CASES])
def test_fused_grd_sweep_of_a_built_field_equals_the_oracle(gpu_ctx, name):
    fallbacks = gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    with _built(gpu_ctx, name, em.SOURCES["grd_fused"]):
        _sweeps(gpu_ctx, name, "GRD", f"{name}, fused GRD")
        if cp.BY_NAME[name].kind == "probe":
            _cross_check(gpu_ctx, name, name)
    assert gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == fallbacks


@pytest.mark.parametrize("source", OTHER_SOURCES)
def test_every_other_sweep_source_on_the_probe_field(gpu_ctx, source):
    """volume-sourced, paired (kSrcVol2) and packed GRD, fused and volume-sourced census and CENGRD take the all-valid path like the fused
    GRD cells; GrdPC / CSPC never does -- the control"""
    src = em.SOURCES[source]
    name = cp.SOURCE_CASE
    fallbacks = gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    with _built(gpu_ctx, name, src):
        _sweeps(gpu_ctx, name, src.kind, f"{name}, {source}")
        _cross_check(gpu_ctx, name, f"{name}, {source}")
    assert gpu_ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == fallbacks


@pytest.mark.parametrize("name", cp.GRID_CASES)
def test_one_workgroup_per_row_band(_gpu_ctx_session, name):
    """CSPM_OPT_SWEEP_GRID = 8 on a context of the test's own: a workgroup's consecutive items are a pixel and its direct successor"""
    ctx = capi.StereoContext(0)
    try:
        ctx.set_option(capi.OPT_SWEEP_GRID, 8)
        with _built(ctx, name, em.SOURCES["grd_fused"]):
            _sweeps(ctx, name, "GRD", f"{name}, one workgroup per band", SWEEPS[:2])
        assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 0
    finally:
        ctx.close()
