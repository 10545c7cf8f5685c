"""The item loop of the persistent raster sweep (cspm_chain.h k_spatial_sweep) with FEW workgroups: on a test-size image the library's grid
(at least 256 workgroups) hands every workgroup a handful of unrelated pixels, so consecutive turns of a workgroup's loop are never a pixel
and its direct successor -- the case in which whatever the loop carries from one turn into the next (the item number, the predecessors'
planes, the pixel's own plane and cost loaded before the wait, the level terms) can go wrong.  CSPM_OPT_SWEEP_GRID caps the grid: 8 = one
workgroup per row band, every pair of consecutive, dependent items; 9 and 37 = uneven shares of the bands; 0 = the library's grid.

Per case, for every grid and for five-wave and folded workgroups: planes and stored costs of three iterations (both sweep directions; the
third sweep takes the own0 / own1 / same01 shortcuts) equal, bit for bit, those of the same run with one launch per anti-diagonal
(CSPM_OPT_RASTER_LAUNCHES = 1) and, on the 80 x 56 cases, those of the oracle in device order; no sweep fell back.  Every case runs on a
context of its own, so the hook cannot leak.  Sizes: 80 x 56 D = 16 with five levels (folded: levels == waves + 1), three levels and single
scale; 70 x 1, 1 x 40 and 9 x 9 (no y- or x-predecessors at all; row bands without rows)."""
import functools

import numpy as np
import pytest

from crossscalepatchmatch_amd import capi, synth
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ITERS, SEED, WND = 3, 4711, 35
# name: (w, h, max_dis, scale_num, reg_lambda, compared with the oracle)
CASES = {
    "80x56_5lv": (80, 56, 16, 5, 0.3, True),
    "80x56_3lv": (80, 56, 16, 3, 0.3, True),
    "80x56_ss": (80, 56, 16, 0, 0.0, True),
    "70x1": (70, 1, 8, 5, 0.3, False),
    "1x40": (1, 40, 4, 5, 0.3, False),
    "9x9": (9, 9, 4, 5, 0.3, False),
}
GRIDS = (0, 8, 9, 37)


@functools.lru_cache(maxsize=None)
def _pair(name):
    w, h, D = CASES[name][:3]
    l, r = synth.make_pair(w, h, D, regions=3, seed=100 * w + h)[:2]
    return l, r


def _run(name, fold, grid, launches):
    """planes and costs of both views after ITERS iterations on a fresh context, and its count of sweep fall-backs"""
    w, h, D, scale_num, lam, _ = CASES[name]
    l, r = _pair(name)
    ctx = capi.StereoContext(0)
    try:
        ctx.set_option(capi.OPT_SWEEP_FOLD, fold)
        ctx.set_option(capi.OPT_SWEEP_GRID, grid)
        ctx.set_option(capi.OPT_RASTER_LAUNCHES, launches)
        ctx.set_images(l, r)
        ctx.build_cost_grd(D, WND, scale_num, lam)
        ctx.patchmatch(ITERS, seed=SEED, schedule=capi.SCHED_RASTER)
        state = [ctx.get_planes(v) for v in (0, 1)]
        return state, ctx.get_option(capi.OPT_SWEEP_FALLBACKS)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _per_diagonal(name, fold):
    """the same run with one launch per anti-diagonal: computed once per case and workgroup shape, never written to"""
    state, fallbacks = _run(name, fold, 0, 1)
    assert fallbacks == 0
    for npar, cost in state:
        npar.setflags(write=False)
        cost.setflags(write=False)
    return state


@functools.lru_cache(maxsize=None)
def _oracle(name):
    w, h, D, scale_num, lam, _ = CASES[name]
    l, r = _pair(name)
    pc = po.PlaneCost(l, r, D, WND, scale_num, lam)
    pm = po.PatchMatch(l, r, D, 4)
    pm.run(ITERS, pc, False, seed=SEED, schedule=po.SCHED_RASTER, sum_order=po.SUM_DEVICE)
    return [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]


@pytest.mark.parametrize("fold", [0, 1], ids=["five_waves", "folded"])
@pytest.mark.parametrize("grid", GRIDS, ids=["grid%d" % g for g in GRIDS])
@pytest.mark.parametrize("name", list(CASES))
def test_few_workgroups_walk_dependent_items(_gpu_ctx_session, name, grid, fold):
    state, fallbacks = _run(name, fold, grid, 0)
    assert fallbacks == 0, "a persistent sweep timed out and was repeated per diagonal"
    want = _per_diagonal(name, fold)
    for v in (0, 1):
        np.testing.assert_array_equal(state[v][0], want[v][0], err_msg=f"planes vs per-diagonal launches, view {v}")
        np.testing.assert_array_equal(state[v][1], want[v][1], err_msg=f"stored costs vs per-diagonal launches, view {v}")
    if CASES[name][5]:
        ref = _oracle(name)
        for v in (0, 1):
            P, cost = ref[v]
            np.testing.assert_array_equal(state[v][0][..., :3], P[..., 0:3], err_msg=f"norm vs oracle, view {v}")
            np.testing.assert_array_equal(state[v][0][..., 3:], P[..., 6:9], err_msg=f"param vs oracle, view {v}")
            np.testing.assert_array_equal(state[v][1], cost, err_msg=f"stored costs vs oracle, view {v}")
