"""The row engine on plane fields BUILT to take every reachable leaf of its path decision (tests/rows_path_ref.py CASES; which leaf which
wave takes is restated there and held to the device's counters by tests/test_rows_path_ref.py), against the CPU oracle bit for bit:
k_rescore on every case under DMA-filled tables, computed tables and (nd = 2, cluster and single-scale fields) cost volumes, the chain
engine on a sample of the same pixels, and k_refine / k_view_eval after the re-score with the early exit on and off.  Every comparison is
assert_array_equal; nothing here takes a tolerance.  The product library only."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import ca_ref
import rows_path_ref as rp
import warm_ref
from crossscalepatchmatch_amd import capi
from crossscalepatchmatch_amd.synth import make_pair
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

DIS_SCALE = 4
BY_NAME = {c.name: c for c in rp.CASES}
RESCORE = [(c.name, src) for c in rp.CASES for src in rp.SOURCES if src != "volumes" or c.name in rp.VOLUME_CASES]
GT = rp.Case("ground_truth", rp.G32, 40, None, True)  # the pair's own disparities: low stored costs, candidates die in mid-level inside table rows
PHASES = [c for c in rp.CASES if c.phases] + [GT]
ALL = dict(BY_NAME, ground_truth=GT)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_paths.json")


@functools.lru_cache(maxsize=None)
def _pair_of(name):
    case = ALL[name]
    g = case.geom
    return make_pair(g.w, g.h, g.max_dis, regions=3, seed=case.seed)


def _pair(case):
    return _pair_of(case.name)


def _lam(case):
    return 0.3 if case.geom.scale_num else 0.0


def _pc(case):
    return _pc_of(case.name)


@functools.lru_cache(maxsize=None)
def _pc_of(name):
    case = ALL[name]
    g = case.geom
    l, r, _, _ = _pair(case)
    return po.PlaneCost(l, r, g.max_dis, g.wnd, g.scale_num, _lam(case), "GRD")


def _fields(case):
    if case is GT:
        _, _, gl, gr = _pair(case)
        return [ca_ref.planes_of(np.nan_to_num(d, nan=1.0)) for d in (gl, gr)]
    return rp.case_fields(case)


def _rescored(case):
    """(planes, min_cost) per view of the oracle's re-score of the case's field, computed once and left unchanged"""
    return _rescored_of(case.name)


@functools.lru_cache(maxsize=None)
def _rescored_of(name):
    case = ALL[name]
    l, r, _, _ = _pair(case)
    pm = po.PatchMatch(l, r, case.geom.max_dis, DIS_SCALE)
    warm_ref.inject(pm, _fields(case))
    warm_ref.rescore(pm, _pc(case), po.SUM_DEVICE)
    out = [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]
    for a, b in out:
        a.setflags(write=False)
        b.setflags(write=False)
    return out


def _assert_state(ctx, want, what):
    """want: (planes (h, w, 9), min_cost) per view, the oracle's"""
    for v in (0, 1):
        npar, cost = ctx.get_planes(v)
        P, c = want[v]
        np.testing.assert_array_equal(npar[..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(npar[..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(cost, c, err_msg=f"{what}: min_cost, view {v}")


def _start(ctx, case, source):
    g = case.geom
    l, r, _, _ = _pair(case)
    ctx.set_images(l, r)
    ctx.build_cost_grd(g.max_dis, g.wnd, g.scale_num, _lam(case), volumes=source == "volumes", table_volumes=source == "tables")
    assert ctx.get_option(capi.OPT_TABLE_VOLUMES_ACTIVE) == int(source == "tables")
    fields = _fields(case)
    for v in (0, 1):
        ctx.set_planes(v, fields[v], np.full((g.h, g.w), -7.0))  # garbage costs
    return fields


@pytest.mark.parametrize("name,source", RESCORE, ids=[f"{n}-{s}" for n, s in RESCORE])
def test_rescore_of_a_built_field_equals_the_oracle(gpu_ctx, name, source):
    case = BY_NAME[name]
    g = case.geom
    fields = _start(gpu_ctx, case, source)
    gpu_ctx.rescore_planes()
    want = _rescored(case)
    rng = np.random.default_rng(case.seed)
    for v in (0, 1):
        npar, cost = gpu_ctx.get_planes(v)
        np.testing.assert_array_equal(npar, fields[v], err_msg=f"{name}/{source}: the planes changed, view {v}")
        bad = np.argwhere(cost != want[v][1])
        if len(bad):  # name the waves and the leaves the restatement gives them
            y, x = (int(t) for t in bad[0])
            leaves = [(s, rp.leaf_name(p.leaf), p.why) for s, yy, x0, p in rp.launch_leaves(g, source == "tables", v, fields[v])
                      if yy == y and x0 == x // 64 * 64] if source != "volumes" else []
            lanes = sorted({int(b[1]) % 64 for b in bad if b[0] == y and b[1] // 64 == x // 64})
            pytest.fail(f"{name}/{source} view {v}: {len(bad)} costs differ from the oracle, first at (x {x}, y {y}): device {cost[y, x]!r}, "
                        f"oracle {want[v][1][y, x]!r}; wave x0 {x // 64 * 64} lanes {lanes}; its level passes {leaves}")
        # the chain engine on a sample of the same pixels and planes: both engines agree on the same fields
        xy = np.stack([rng.integers(0, g.w, 48), rng.integers(0, g.h, 48)], 1).astype(np.int32)
        xy[:4] = [[0, 0], [g.w - 1, 0], [0, g.h - 1], [g.w - 1, g.h - 1]]
        got = gpu_ctx.plane_cost_batch(v, xy, fields[v][xy[:, 1], xy[:, 0]])
        np.testing.assert_array_equal(got, want[v][1][xy[:, 1], xy[:, 0]], err_msg=f"{name}/{source}: chain engine, view {v}")


@pytest.mark.parametrize("case", PHASES, ids=[c.name for c in PHASES])
def test_refine_and_view_after_the_rescore_equal_the_oracle(gpu_ctx, case):
    """k_refine and k_view_eval start from low, exact stored costs: candidates are rejected in mid-level, inside table rows.  With the
    early exit on and off the device gives the oracle's planes and costs, and the same as each other."""
    l, r, _, _ = _pair(case)
    pc = _pc(case)
    pm = po.PatchMatch(l, r, case.geom.max_dis, DIS_SCALE)
    warm_ref.inject(pm, _fields(case))
    for v in (0, 1):
        pm.min_cost(v)[...] = _rescored(case)[v][1]
    kw = dict(seed=777, schedule=po.SCHED_RASTER)
    pm.refine(0, pc, sum_order=po.SUM_DEVICE, **kw)
    after_refine = [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]
    pm.view(0, pc, sum_order=po.SUM_DEVICE, **kw)
    after_view = [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]
    states = []
    for early_exit in (1, 0):
        _start(gpu_ctx, case, "tables")
        gpu_ctx.rescore_planes()
        gpu_ctx.pm_refine(0, early_exit=early_exit, **kw)
        _assert_state(gpu_ctx, after_refine, f"refine, early_exit {early_exit}")
        gpu_ctx.pm_view(0, early_exit=early_exit, **kw)
        _assert_state(gpu_ctx, after_view, f"view, early_exit {early_exit}")
        states.append([gpu_ctx.get_planes(v) for v in (0, 1)])
    for v in (0, 1):
        np.testing.assert_array_equal(states[0][v][0], states[1][v][0], err_msg=f"early exit on / off: planes, view {v}")
        np.testing.assert_array_equal(states[0][v][1], states[1][v][1], err_msg=f"early exit on / off: costs, view {v}")
    assert any(np.any(after_refine[v][1] != _rescored(case)[v][1]) for v in (0, 1))  # the refinement accepted something


@pytest.mark.parametrize("name", [c.name for c in rp.CASES])
def test_costs_of_the_counted_launches_are_the_oracles(name):
    """the statistics build whose counters tests/golden/row_paths.json records is not the product: the record carries the sha256 of the costs
    that build stored on every case, and the oracle's costs hash to the same (tools/ does not load the oracle, this test does)"""
    with open(GOLDEN) as f:
        gold = json.load(f)["min_cost_sha256"]
    want = _rescored(BY_NAME[name])
    for v in (0, 1):
        for source in ("tables", "computed"):
            assert hashlib.sha256(np.ascontiguousarray(want[v][1]).tobytes()).hexdigest() == gold[f"{name}/{source}/{v}"], f"{name}/{source} view {v}"
