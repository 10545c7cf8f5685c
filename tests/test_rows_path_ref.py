"""tests/rows_path_ref.py -- the row engine's path decision restated -- held to the device: the leaves its sweep finds reachable are
all taken by the constructed CASES, no other leaf occurs, and the restated histogram of every case equals the counters an MI355X
recorded (tests/golden/row_paths.json, written by tools/row_paths.py from the statistics build) per (case, source, view, level, leaf).
The record carries the sha256 of the cspm_rows.h it was taken from: a change to that file makes this test fail until the tool has
run again, so the coverage claim does not outlive a change to the decision.  No GPU needed."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import rows_path_ref as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_paths.json")
ROWS_H = os.path.join(ROOT, "crossscalepatchmatch_amd", "csrc", "cspm_rows.h")


def _union():
    """{leaf: [(case, source, view, level, y, x0)]} over CASES"""
    seen = collections.defaultdict(list)
    for case in rp.CASES:
        for source in ("tables", "computed"):
            for v, s, y, x0, p in rp.case_passes(case, source):
                seen[p.leaf].append((case.name, source, v, s, y, x0))
    return seen


def test_lds_budget_and_thresholds():
    """the figures DESIGN.md section 5.1 quotes, derived here: window 35, max_dis 128, a level-0 interior wave of 64 centres"""
    assert rp.strip_capacity(128, 17) == 228 and rp.own_capacity(17) == 100 and rp.strip_capacity(320, 17) == 384
    assert rp.wave_lds_bytes(228, 100) == 2 * (228 * 16 + 100 * 12) == 9696

    def leaf(max_dis, nd, cvol=True, level=0, wnd=35, edge=False):
        cmin = 0 if edge else 1024
        return rp.decide(max_dis, wnd, max_dis >> level, 4096, 40, 0, cmin, cmin + (64 >> level) - 1, cvol, lambda: ([True], [1], [nd])).leaf

    R, T, P = rp.RANGE_DMA, rp.TBUF2, rp.PADDED
    assert [leaf(128, nd) for nd in (4, 5, 6, 8, 9, 11, 12)] == [R | T | P, R | T, R | P, R | P, R, R, rp.GEN_MANY]
    assert [leaf(32, nd) for nd in (2, 3, 4, 5, 6, 7, 8)] == [R | T | P, R | T, R | P, R | P, R, R, rp.GEN_MANY]
    assert leaf(128, 2, edge=True) == rp.GEN_MANY | rp.EDGE          # a 35-wide window leaves a level-0 border wave no room for the weight table
    assert leaf(128, 2, wnd=9, edge=True) == R | T | rp.WTAB | rp.EDGE  # a 9-wide one does
    assert leaf(320, 2) == rp.UNSTAGED                                # beyond the strip
    assert leaf(320, 2, level=1) == R | T | P


def test_the_quoted_threshold_table():
    """lds_room and, for a level-0 interior wave of 64 centres, the first nd of every leaf, DMA-filled and computed"""
    room = {(d, w): rp.wave_lds_bytes(rp.strip_capacity(d, w // 2), rp.own_capacity(w // 2)) - 64 for d in (32, 128) for w in (35, 9)}
    assert room == {(32, 35): 6560, (128, 35): 9632, (32, 9): 5120, (128, 9): 8192}

    def firsts(max_dis, wnd, cvol, edge=False):
        out, prev = [], None
        for nd in range(2, max_dis + 1):
            cmin = 0 if edge else 1024
            leaf = rp.decide(max_dis, wnd, max_dis, 4096, 40, 0, cmin, cmin + 63, cvol, lambda: ([True], [1], [nd])).leaf & ~rp.EDGE
            if leaf != prev:
                out.append((nd, leaf))
                prev = leaf
        return out

    R, C, T, P, G, W = rp.RANGE_DMA, rp.RANGE_COMP, rp.TBUF2, rp.PADDED, rp.GEN_MANY, rp.WTAB
    assert firsts(32, 35, True) == [(2, R | T | P), (3, R | T), (4, R | P), (6, R), (8, G)]
    assert firsts(128, 35, True) == [(2, R | T | P), (5, R | T), (6, R | P), (9, R), (12, G)]
    assert firsts(32, 9, True) == [(2, R | T | P), (3, R | T), (4, R | P), (6, R), (8, G)]
    assert firsts(128, 9, True) == [(2, R | T | P), (5, R | T), (7, R | P), (10, R), (14, G)]
    assert firsts(32, 35, False) == [(2, C | P), (4, C), (5, G)] and firsts(128, 35, False) == [(2, C | P), (7, C), (9, G)]
    assert firsts(32, 9, False) == [(2, C | P), (4, C), (5, G)] and firsts(128, 9, False) == [(2, C | P), (8, C), (10, G)]
    # border waves: no room for the weight table under a 35-wide window, range tables with it under a 9-wide one
    assert firsts(32, 35, True, True) == [(2, G)] and firsts(128, 35, True, True) == [(2, G)]
    assert firsts(128, 9, True, True) == [(2, R | T | W), (3, R | P | W), (4, R | W), (5, G)]


def _lanes_of(case_name, view):
    case = next(c for c in rp.CASES if c.name == case_name)
    return case, rp.launch_lanes(case.geom, rp.case_fields(case)[view])


@pytest.mark.parametrize("name,view,x0", rp.STRADDLE_WAVES)
def test_one_straddling_lane_keeps_a_wave_off_the_cluster_table(name, view, x0):
    """the cluster cut's ballot at its edge: an interior level-0 wave whose range test passes in all 64 lanes and whose two clusters would
    fit a table, but for ONE lane whose interval straddles the cut -- it takes general taps; with that lane on a surface, the cluster table"""
    case, lanes = _lanes_of(name, view)
    g = case.geom
    waves = [t for t in lanes if t[0] == 0 and t[2] == x0]
    assert len(waves) == g.h
    for s, y, _, (W, H, D), cmin, cmax, safe, fl, fh, _ in waves:
        assert all(safe) and cmin - g.wnd // 2 >= 0 and cmax + g.wnd // 2 < W
        f_lo, f_hi = min(fl), max(fh)
        cut = (f_lo + f_hi + 1) // 2
        straddling = [i for i in range(64) if not (fh[i] < cut or fl[i] >= cut)]
        assert len(straddling) == 1, (y, straddling)
        got = rp.decide(g.max_dis, g.wnd, D, W, H, view, cmin, cmax, True, lambda: (safe, fl, fh))
        assert got.leaf == rp.GEN_MANY, (y, rp.leaf_name(got.leaf))
        i = straddling[0]
        fl2, fh2 = list(fl), list(fh)
        fl2[i], fh2[i] = fl[0], fh[0]
        alt = rp.decide(g.max_dis, g.wnd, D, W, H, view, cmin, cmax, True, lambda: (safe, fl2, fh2))
        assert alt.leaf & 7 == rp.CLUSTER_DMA and alt.nd < f_hi - f_lo + 1, (y, rp.leaf_name(alt.leaf))


def test_unsafe_corner_fields_leave_the_range_at_one_corner_only():
    case = next(c for c in rp.CASES if c.name == "unsafe_corners")
    g = case.geom
    half = g.wnd // 2
    for view, x0 in rp.ONE_CORNER_WAVES:
        waves = [t for t in rp.launch_lanes(g, rp.case_fields(case)[view]) if t[0] == 0 and t[2] == x0 and half <= t[1] < g.h - half]
        assert waves
        for _, y, _, _, _, _, safe, _, _, nbad in waves:
            assert nbad == [1] * 64 and not any(safe), (view, x0, y)
    # and the two other kinds of lane that fail the test: |nz| < kDoubleEps, a huge slope (one lane in four each)
    for view, x0 in ((0, 192), (1, 128), (1, 0), (0, 256)):
        for t in rp.launch_lanes(g, rp.case_fields(case)[view]):
            if t[0] == 0 and t[2] == x0:
                assert sum(not ok for ok in t[6]) == 16, (view, x0, t[1])


def test_widths_below_145_have_no_interior_level0_wave():
    flat = np.zeros((36, 144, 6))
    flat[..., 2], flat[..., 5] = 1.0, 7.5
    for w in (64, 77, 96, 100, 144):
        g = rp.Geom(w, 36, 32, 35, 1)
        assert all(p.leaf & rp.EDGE for s, _, _, p in rp.launch_leaves(g, True, 0, flat[:, :w]))
    assert any(not p.leaf & rp.EDGE for s, _, _, p in rp.launch_leaves(rp.Geom(145, 36, 32, 35, 1), True, 0, np.repeat(flat, 2, 1)[:, :145]))


def test_cases_take_every_reachable_leaf_and_no_other():
    reachable, seen = rp.sweep(), _union()
    missing = sorted(set(reachable) - set(seen))
    assert not missing, "no case takes: " + ", ".join(f"{rp.leaf_name(l)} (e.g. {sorted(reachable[l].items())[0]})" for l in missing)
    extra = sorted(set(seen) - set(reachable))
    assert not extra, "taken but listed unreachable: " + ", ".join(f"{rp.leaf_name(l)} by {seen[l][0]}" for l in extra)
    # interior and border waves each: `edge` is part of the leaf, and the sweep reaches both kinds of every table leaf but those
    # whose weights an interior wave never takes from the table
    for kind in range(8):
        assert {bool(l & rp.EDGE) for l in seen if l & 7 == kind} == {False, True}, rp.KINDS[kind]


def test_restated_histograms_equal_the_device_record():
    with open(GOLDEN) as f:
        gold = json.load(f)
    with open(ROWS_H, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    assert gold["cspm_rows_h_sha256"] == sha, (
        "crossscalepatchmatch_amd/csrc/cspm_rows.h changed since tests/golden/row_paths.json was recorded: build libcspm_rowstats.so and run "
        "tools/row_paths.py on the GPU again (and update tests/rows_path_ref.py if the decision changed)")
    want = {f"{c.name}/{src}" for c in rp.CASES for src in ("tables", "computed")}
    assert set(gold["cases"]) == want
    reachable = rp.sweep()
    for key in sorted(want):
        name, source = key.split("/")
        case = next(c for c in rp.CASES if c.name == name)
        assert rp.case_histogram(case, source) == gold["cases"][key], key
        for k in gold["cases"][key]:
            assert int(k.split("/")[2]) in reachable, f"{key}: the device counted the unreachable leaf {rp.leaf_name(int(k.split('/')[2]))}"


def test_volume_source_runs_no_decision():
    assert all(rp.case_passes(next(c for c in rp.CASES if c.name == n), "volumes") == [] for n in rp.VOLUME_CASES)
