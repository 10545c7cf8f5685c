"""CPU only: the case table tests/edge_matrix.py is not vacuous.  On the oracle alone, for every case tests/test_gpu_edge_matrix.py
uses: every kind builds and runs with finite costs and the level count the fold condition needs; each phase of the first iteration
changes the planes of a twentieth of the pixels or more wherever an image is large enough for planes to differ in cost; the tie-heavy
pairs do tie; the refinement has more halving steps than a chunk.  The oracle states computed here are the ones the GPU module
compares with (functools.lru_cache in tests/edge_matrix.py)."""
import numpy as np
import pytest

import edge_matrix as em
from oracle import pyoracle as po

MOVED = 0.05  # of view 0's pixels, per phase
TIED = 0.20   # of view 0's pixels


def _finite(run, what):
    for v in (0, 1):
        assert np.all(np.isfinite(run.state[v][1])), f"{what}: min_cost, view {v}"
        assert np.all(np.isfinite(run.state[v][0])), f"{what}: planes, view {v}"
        assert np.all(np.isfinite(run.disp[v])), f"{what}: disparity, view {v}"


GEOM_CASES = [(g, k) for k in em.KINDS for g in em.geometries_of(k)]
GEOM_IDS = [f"{em.pair_id(g)}-{k}" for g, k in GEOM_CASES]


@pytest.mark.parametrize("geom,kind", GEOM_CASES, ids=GEOM_IDS)
def test_every_kind_runs_at_every_geometry(geom, kind):
    """test a's cases: both level counts under every schedule; five levels are five levels even at 1x1, so `levels >= 4` holds.
    GrdPC / CSPC with max_dis > width is no case: the reference reads out of range there (edge_matrix.refused)"""
    w, h, D = geom
    if em.refused(geom, kind):
        assert kind == "IMG" and D > w and geom in [(1, 1, 2), (1, 7, 3), (20, 20, 25), (65, 2, 70)]
        return
    for sn, lam in em.MODES:
        pc = em.plane_cost(geom, kind, sn, lam)
        assert pc.levels == max(sn, 1)
        assert pc.dims(0) == (w, h, D)
        for sched, K in em.schedules_at(geom):
            _finite(em.whole_run(geom, kind, sn, lam, sched, K), f"{em.pair_id(geom)} {kind} levels {sn} {em.sched_id(sched, K)}")


MOVING_CASES = [(g, k) for g, k in GEOM_CASES if g not in em.THIN and not em.refused(g, k)]


@pytest.mark.parametrize("geom,kind", MOVING_CASES, ids=[f"{em.pair_id(g)}-{k}" for g, k in MOVING_CASES])
def test_phases_change_pixels(geom, kind):
    """after the random init each of the first spatial propagation, view propagation and refinement changes >= 5 % of view 0's planes,
    under every schedule test a runs there (tests c and d run a subset of them)"""
    for sched, K in em.schedules_at(geom):
        states = em.first_iteration(geom, kind, 5, 0.3, sched, K)
        for k, phase in enumerate(("spatial", "view", "refine")):
            f = em.changed_fraction(states[k], states[k + 1])
            assert f >= MOVED, f"{em.pair_id(geom)} {kind} {em.sched_id(sched, K)}: {phase} changed {f:.3f} of view 0"


def test_no_test_runs_thin_geometries_only():
    """1x1, 2x1, 1x7 and 3x3 are launch-shape cases: every list that holds one also holds geometries where planes move"""
    assert len([c for c in MOVING_CASES if c[1] == "IMG"]) == 8 and len(MOVING_CASES) == 32  # GrdPC / CSPC: two refused, two added
    assert len([c for c in FOLD_CASES if c[1] == "IMG"]) == 6 and len(FOLD_CASES) == 24
    assert [p for p in em.row_pairs_of("IMG") if not em.refused(p, "IMG")] == [(9, 2, 4), (37, 3, 6), (129, 3, 8), (65, 2, 65)]
    for pairs in (em.GEOMETRIES, em.ROW_PAIRS):
        assert any(p in em.THIN for p in pairs) and sum(p in em.MOVING for p in pairs) >= 4
    assert not any(p in em.THIN for p in em.FOLD_PAIRS)
    assert em.ROW_SINGLE_SCALE_PAIR in em.MOVING and em.UNFOLDED_CASE[0] in em.MOVING


FOLD_CASES = [(p, k) for k in em.KINDS for p in em.fold_pairs_of(k) if not em.refused(p, k)]


@pytest.mark.parametrize("pair,kind", FOLD_CASES, ids=[f"{em.pair_id(p)}-{k}" for p, k in FOLD_CASES])
def test_fold_cases(pair, kind):
    """test b's cases: four and five levels fold (levels >= 4), three do not; the forward sweep after the random init and the backward
    sweep after it each change >= 5 % of view 0's planes"""
    for sn in em.FOLD_LEVELS:
        assert em.plane_cost(pair, kind, sn, em.FOLD_LAM).levels == sn >= 4
        states = em.sweep_phases(pair, kind, sn, em.FOLD_LAM)
        for it, sweep in enumerate(("forward", "backward")):
            f = em.changed_fraction(states[it], states[it + 1])
            assert f >= MOVED, f"{em.pair_id(pair)} {kind} levels {sn}: the {sweep} sweep changed {f:.3f} of view 0"
        _finite(em.whole_run(pair, kind, sn, em.FOLD_LAM, em.RASTER), f"{em.pair_id(pair)} {kind} levels {sn}")
    if pair == em.UNFOLDED_CASE[0]:
        sn = em.UNFOLDED_CASE[1]
        assert em.plane_cost(pair, kind, sn, em.FOLD_LAM).levels == sn < 4
        states = em.sweep_phases(pair, kind, sn, em.FOLD_LAM)
        assert em.changed_fraction(states[0], states[1]) >= MOVED


def test_row_hand_out_cases():
    """test c's cases: every source exists, every pair runs under test a's schedules (checked above), and the refinement has more
    halving steps than CSPM_REFINE_CHUNK = 3 puts into one launch, so both chunk sizes split it"""
    assert sorted(em.SOURCES[s].kind for s in em.ROW_SOURCES) == ["CEN", "CENGRD", "GRD", "GRD", "IMG"]
    for pair in em.row_pairs_of("IMG"):
        assert pair in em.geometries_of("IMG")
        assert all(sk in em.schedules_at(pair) for sk in em.ROW_SCHEDULES)
        assert po.lib().csor_refine_steps(pair[2]) > 3
    assert sorted(e for e, _ in em.ROW_ENV) == ["CSPM_REFINE_CHUNK", "CSPM_REFINE_CHUNK", "CSPM_ROW_CLAIM"]


@pytest.mark.parametrize("kind", em.KINDS)
@pytest.mark.parametrize("pair", em.TIE_PAIRS)
def test_ties_exist(pair, kind):
    """after two raster iterations with five levels >= 20 % of view 0's pixels share their min_cost with another pixel, bit for bit: the
    sweep has spread planes over pixels that cost them alike, and every later candidate there meets a stored cost it can only equal.
    (Red-black and the snapshot schedule spread a plane over fewer pixels per iteration: 4-10 % on black and white after the same two
    iterations, IMG 94 % and more.  Test d runs them on the same pairs; the bound is the raster run's.)"""
    sn, lam = em.TIE_MODE
    run = em.whole_run(pair, kind, sn, lam, em.RASTER, 4, em.TIE_SEED)
    f = em.tied_fraction(run.state[0][1])
    assert f >= TIED, f"{pair} {kind}: {f:.3f} of view 0's pixels tie"
    for name, sched, K, _ in em.TIE_CASES:
        if em.SOURCES[name].kind == kind:
            _finite(em.whole_run(pair, kind, sn, lam, sched, K, em.TIE_SEED), f"{pair} {kind} {em.sched_id(sched, K)}")


def test_table_is_complete():
    """the ten sources, each under the fold; the newer paths of test d"""
    assert list(em.SOURCES) == ["grd_fused", "grd_computed", "grd_volumes", "grd_pairs", "grd_packed", "cen_fused", "cen_volumes",
                                "cengrd_volumes", "cengrd_fused", "img"]
    assert sorted(em.KINDS) == sorted({s.kind for s in em.SOURCES.values()})
    assert len(em.sources_of("GRD")) == 5
    assert all(name in em.SOURCES for name, _, _, _ in em.TIE_CASES)
    for s in em.SOURCES.values():  # every option a source sets or passes is restored afterwards
        touched = set(s.options) | {dict(volumes="OPT_GRD_VOLUMES", sweep_pairs="OPT_SWEEP_PAIRS", table_volumes="OPT_TABLE_VOLUMES",
                                         fused="OPT_CENGRD_FUSED")[k] for k in s.kwargs}
        assert touched == set(s.restore), s.name
