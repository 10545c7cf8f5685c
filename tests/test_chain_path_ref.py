"""CPU: the case table of tests/chain_path_ref.py is not vacuous.  With the restatement and the oracle only (tests/chain_cases.py): every
leaf the emitter / probe fields are built for is taken by at least 4 probes per view and sweep direction, every two-candidate leaf is won
by either slot at 2 or more of them (the oracle's costs decide), every own-plane shortcut of the block fields is taken at 4 or more pixels
per view and direction (the oracle's field before and after the sweep decides), every built candidate keeps its window corners 2^-30 away
from the all-valid thresholds, the border leaf (level 0 general, every coarse level all-valid) is built where it can be, emitters and the sweep's first pixel keep their planes, and the geometries have the window shapes they
were chosen for.  These are conditions on the INPUTS of tests/test_gpu_chain_paths.py; each test prints its counts (pytest -s)."""
import numpy as np
import pytest

import chain_cases as cc
import chain_path_ref as cp

MIN_PIXELS, MIN_WINS = 4, 2
PROBE_CASES = [c.name for c in cp.CASES if c.kind == "probe"]
BLOCK_CASES = [c.name for c in cp.CASES if c.kind == "block"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _probe_counts(name, kind, it, v):
    """{tag: (pixels, won by slot 0, won by slot 1)} of view v swept in the direction of iteration `it`, the oracle's costs of `kind`"""
    c = cp.BY_NAME[name]
    F = cc.start(name)[v][0]
    F2 = cc.field_of(cc.swept(name, kind, it), v)
    T, guard, _ = cp.probe_tags(c.geom, F, cc.INC[it])
    _, c0, c1, _ = cp.sweep_leaves(F, F, cc.INC[it], False)
    won0 = np.all(_bits(F2) == _bits(c0), -1)
    won1 = np.all(_bits(F2) == _bits(c1), -1) & ~won0
    return {k: (int(m.sum()), int((m & won0).sum()), int((m & won1).sum())) for k, m in T.items()}, guard


@pytest.mark.parametrize("name", PROBE_CASES)
def test_probe_fields_take_every_leaf_and_either_slot_wins(name):
    c = cp.BY_NAME[name]
    g = c.geom
    for it in (0, 1):
        want = cc.swept(name, "GRD", it)
        for v in (0, 1):
            counts, guard = _probe_counts(name, "GRD", it, v)
            print(f"\n{name}, view {v}, direction {cc.INC[it]:+d}: guard distance 2^{np.log2(guard):.1f}")
            for k, (n, w0, w1) in counts.items():
                print(f"  {k:58s} {n:5d} pixels, slot 0 wins {w0:4d}, slot 1 wins {w1:4d}")
            assert guard >= cp.GUARD
            for k, (n, w0, w1) in counts.items():
                assert n >= MIN_PIXELS, f"{name}, view {v}, direction {cc.INC[it]}: {k}: {n} probes"
                if k.startswith("pair:"):
                    assert w0 >= MIN_WINS and w1 >= MIN_WINS, f"{name}, view {v}, direction {cc.INC[it]}: {k}: slot 0 wins {w0}, slot 1 wins {w1}"
            # the oracle's result: emitters (and with them the sweep's first pixel) keep plane and cost, every probe accepted
            F, cost = cc.start(name)[v]
            F2, cost2 = cc.field_of(want, v), want[v][1]
            em = cost == cp.EMITTER_COST
            assert np.array_equal(_bits(F2)[em], _bits(F)[em]) and np.all(cost2[em] == cp.EMITTER_COST)
            first = (0, 0) if cc.INC[it] > 0 else (g.h - 1, g.w - 1)
            assert em[first]
            assert np.all(cost2[~em] < cp.PROBE_COST) and np.all(cost2[~em] >= 0.0)
            _, c0, c1, _ = cp.sweep_leaves(F, F, cc.INC[it], False)
            taken = np.all(_bits(F2) == _bits(c0), -1) | np.all(_bits(F2) == _bits(c1), -1)
            assert np.all(taken[~em])


@pytest.mark.parametrize("kind", [k for k in cc.KINDS if k != "GRD"])
def test_probe_field_under_the_other_costs(kind):
    """the case the other cost sources take: under CEN, CENGRD and GrdPC / CSPC costs the emitters stay (the costs are >= 0), every probe
    accepts, and either slot wins every two-candidate leaf"""
    name = cp.SOURCE_CASE
    for it in (0, 1):
        want = cc.swept(name, kind, it)
        for v in (0, 1):
            F, cost = cc.start(name)[v]
            em = cost == cp.EMITTER_COST
            assert np.array_equal(_bits(cc.field_of(want, v))[em], _bits(F)[em]) and np.all(want[v][1][em] == cp.EMITTER_COST)
            assert np.all(want[v][1][~em] < cp.PROBE_COST) and np.all(want[v][1][~em] >= 0.0)
            counts, _ = _probe_counts(name, kind, it, v)
            print(f"\n{name} under {kind}, view {v}, direction {cc.INC[it]:+d}")
            for k, (n, w0, w1) in counts.items():
                print(f"  {k:58s} {n:5d} pixels, slot 0 wins {w0:4d}, slot 1 wins {w1:4d}")
                if k.startswith("pair:"):
                    assert w0 >= MIN_WINS and w1 >= MIN_WINS, f"{kind}, view {v}, direction {cc.INC[it]}: {k}: slot 0 wins {w0}, slot 1 wins {w1}"


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_fields_take_every_shortcut(name):
    c = cp.BY_NAME[name]
    g = c.geom
    xx, yy = np.meshgrid(np.arange(g.w), np.arange(g.h))
    for v in (0, 1):
        F = cc.start(name)[v][0]
        # piecewise constant, every piece at least two pixels wide and high: each pixel has an equal neighbour in its row and in its column
        eq_x = np.all(_bits(F)[:, 1:] == _bits(F)[:, :-1], -1)
        eq_y = np.all(_bits(F)[1:] == _bits(F)[:-1], -1)
        assert np.all(np.pad(eq_x, ((0, 0), (1, 0))) | np.pad(eq_x, ((0, 0), (0, 1))))
        assert np.all(np.pad(eq_y, ((1, 0), (0, 0))) | np.pad(eq_y, ((0, 1), (0, 0))))
    for it in (0, 1):
        want = cc.swept(name, "GRD", it)
        for v in (0, 1):
            F, cost = cc.start(name)[v]
            F2 = cc.field_of(want, v)
            leaf, c0, c1, _ = cp.sweep_leaves(F, F2, cc.INC[it], True)
            counts = {cp.LEAVES[k]: int((leaf == k).sum()) for k in range(len(cp.LEAVES))}
            changed = int(np.any(_bits(F) != _bits(F2), -1).sum())
            print(f"\n{name}, view {v}, direction {cc.INC[it]:+d}, trust 1: {counts}; {changed} pixels change their plane")
            off = cp.sweep_leaves(F, F2, cc.INC[it], False)[0]
            print(f"  trust 0: { {cp.LEAVES[k]: int((off == k).sum()) for k in range(len(cp.LEAVES))} }")
            for k in cp.SHORTCUT_LEAVES:
                assert counts[cp.LEAVES[k]] >= MIN_PIXELS, f"{name}, view {v}, direction {cc.INC[it]}: {cp.LEAVES[k]}"
                assert not np.any(off == k)
            assert counts["pair"] >= MIN_PIXELS and counts["same01"] >= MIN_PIXELS and changed >= MIN_PIXELS
            # a shortcut pixel kept its plane and cost or took the candidate that was evaluated; the guard distance of every candidate
            for cand in (c0, c1):
                assert min(float(l.guard.min()) for l in cp.classify(g, xx.ravel(), yy.ravel(), cand.reshape(-1, 6))) >= cp.GUARD
            none = np.isin(leaf, [cp.OWN01, cp.ROW_OWN, cp.COL_OWN, cp.CORNER])
            assert np.array_equal(_bits(F2)[none], _bits(F)[none]) and np.array_equal(want[v][1][none], cost[none])


def test_the_geometries_have_the_windows_they_were_chosen_for():
    def windows(g, level):
        return [cp.level_windows(g, x, y)[level] for y in range(g.h) for x in range(g.w)]

    per_level = [windows(cp.G5, s) for s in range(5)]
    assert {w.passes for ws in per_level for w in ws} == {1, 2, 3, 4}
    assert all(w.nrows <= w.H < 35 for s in (1, 2, 3, 4) for w in per_level[s])            # levels shorter than the window
    assert any(w.r_lo > 0 and w.nrows < 35 - w.r_lo for w in per_level[1])                  # rows clipped at both ends
    assert any(w.r_lo > 0 for w in per_level[0]) and any(w.r_lo == 0 and w.nrows < 35 for w in per_level[0])
    last = per_level[4][0]
    assert (last.W, last.H, last.D, last.passes, last.has_valid) == (3, 3, 1, 1, False)     # folded: one pass for three sharing waves
    assert [w.D for w in cp.level_windows(cp.G3, 0, 0)] == [16, 8, 4]
    ss = windows(cp.GSS, 0)
    assert {w.passes for w in ss} == {2, 3, 4}                                               # four waves: clipped windows leave some idle
    assert {w.passes for w in windows(cp.G45T, 0)} >= {3, 5} and cp.G45T.w < cp.K_ROW_MOD * windows(cp.G45T, 0)[0].nsteps
    assert all(w.nrows <= 12 and w.passes <= 2 and w.nsteps == 7 for s in (0, 1) for w in windows(cp.G45, s))
    w9 = cp.level_windows(cp.G9, 20, 15)[0]
    assert (w9.nsteps, w9.x1 - w9.x0 + 1, w9.passes) == (2, 14, 1)                           # the corner test covers five masked columns
    assert cp.GWIDE.max_dis > cp.GWIDE.w and [w.D for w in cp.level_windows(cp.GWIDE, 0, 0)] == [40, 20, 10, 5, 2]
    for c in cp.CASES:  # the sweep's first pixel in either direction is an emitter
        assert (c.geom.w - 1 + c.geom.h - 1) % 2 == 0


def test_the_border_leaf_is_built_where_max_dis_halves_into_every_level():
    """level 0 general, every coarse level all-valid: a y-sloped plane at the odd row 1, where the fine window reaches one row above its
    centre and the coarse one, centred on row 0, none"""
    assert [c.name for c in cp.CASES if c.kind == "probe" and cp.border_leaf_built(c.geom)] == ["probe_5lv", "probe_3lv", "probe_w45", "probe_w9"]
    for g in (cp.G5, cp.G3, cp.G45, cp.G9):
        for spec in cp.border_planes(g)[0]:
            L = cp.classify(g, [20], [1], cp.make_plane(spec, 20, 1))
            assert not L[0].ok[0] and L[0].qmax[0] > L[0].D and all(l.ok[0] for l in L[1:] if l.has_valid)
            even = cp.classify(g, [20], [2], cp.make_plane(spec, 20, 1))  # an even row: the coarse centre is the fine one, level 1 fails too
            assert not even[0].ok[0] and not even[1].ok[0]
        for spec in cp.border_planes(g)[1]:
            assert all(l.ok[0] for l in cp.classify(g, [20], [1], cp.make_plane(spec, 20, 1)) if l.has_valid)


def test_leaf_restatement_on_a_hand_made_field():
    """sweep_leaves on a 3 x 3 field whose leaves can be read off: planes by number, 0 the own plane of every pixel"""
    def P(k):
        return np.array([0.0, 0.0, 1.0, -0.0, -0.0, float(k)])

    F = np.stack([np.stack([P(0)] * 3)] * 3)
    F2 = F.copy()
    F2[0, 1], F2[1, 0], F2[1, 1], F2[0, 2], F2[1, 2] = P(1), P(1), P(2), P(0), P(3)
    leaf, c0, c1, bits = cp.sweep_leaves(F, F2, 1, True)
    names = [[cp.LEAVES[k] for k in row] for row in leaf]
    assert names[0] == ["corner", "row/own", "row/eval"]       # (1,0): left final plane 0 = own; (2,0): left final plane 1
    assert names[1] == ["col/own", "same01", "own1"]           # (1,1): left 1, up 1; (2,1): left 2, up 0 = own
    assert names[2] == ["col/eval", "own0", "own0"]            # (1,2): left 0 = own, up 2; (2,2): left 0 = own, up 3
    assert cp.sweep_leaves(F, F, 1, True)[0][1, 1] == cp.OWN01 and cp.sweep_leaves(F, F, 1, False)[0][1, 1] == cp.SAME01
    assert cp.sweep_leaves(F, F2, 1, False)[0][1, 2] == cp.PAIR and cp.sweep_leaves(F, F2, 1, False)[0][0, 1] == cp.ROW_EVAL
    Z = F.copy()
    Z[0, 1] = [-0.0, -0.0, 1.0, 0.0, 0.0, 0.0]
    leaf, _, _, bits = cp.sweep_leaves(F, Z, 1, False)
    assert leaf[1, 1] == cp.SAME01 and not bits[1, 1] and bits[2, 2]
    back = cp.sweep_leaves(F, F2, -1, True)[0]
    assert back[2, 2] == cp.CORNER and back[2, 1] == cp.ROW_OWN and back[1, 2] == cp.COL_OWN
