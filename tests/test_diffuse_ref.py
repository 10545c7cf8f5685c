"""The CPU restatement of CSPM_SCHED_DIFFUSE (tests/diffuse_ref.py) checked without a GPU: its offset tables against include/cspm.h,
its serial loop against a second, vectorised formulation, and every pair and setting of tests/test_gpu_diffuse.py against the
conditions that keep the GPU comparisons from being vacuous."""
import os
import re

import numpy as np
import pytest

import diffuse_ref
import warm_ref
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_offsets():
    """CSPM_DIFFUSE_OFFSETS_<K> of include/cspm.h, each expanded where it names a shorter list"""
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read().replace("\\\n", " ")
    raw = {int(m.group(1)): m.group(2) for m in re.finditer(r"^#define\s+CSPM_DIFFUSE_OFFSETS_(\d+)\s+(.*)$", hdr, re.M)}
    out = {}
    for K in sorted(raw):
        txt = re.sub(r"CSPM_DIFFUSE_OFFSETS_(\d+)", lambda m: ", ".join("{%d, %d}" % o for o in out[int(m.group(1))]), raw[K])
        out[K] = [(int(a), int(b)) for a, b in re.findall(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*\}", txt)]
    return out


def test_offset_tables_equal_the_header():
    hdr = _header_offsets()
    assert sorted(hdr) == [4, 8, 20] and hdr == diffuse_ref.OFFSETS
    for K, offs in hdr.items():
        assert len(offs) == K == len(set(offs))
    assert hdr[4] == [(-1, 0), (0, -1), (1, 0), (0, 1)]
    assert hdr[8] == hdr[4] + [(-5, 0), (0, -5), (5, 0), (0, 5)]
    assert hdr[20] == hdr[4] + [(-3, 0), (0, -3), (3, 0), (0, 3), (-5, 0), (0, -5), (5, 0), (0, 5),
                                (-1, -2), (1, -2), (2, -1), (2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1)]
    assert re.search(r"^#define\s+CSPM_SCHED_DIFFUSE\s+2\b", open(os.path.join(ROOT, "include", "cspm.h")).read(), re.M)
    assert diffuse_ref.SCHED_DIFFUSE == 2


def _hand_made_field(rng, w, h, D):
    """2x3 blocks of one plane each (bitwise equal neighbours: exact ties for the strict `<`), a third of them out of range"""
    n = rng.normal(size=(h, w, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.5
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    z = rng.uniform(-0.5 * D, 1.5 * D, (h, w))
    f = np.zeros((h, w, 6))
    for y in range(h):
        for x in range(w):
            by, bx = y // 2 * 2, x // 3 * 3
            f[y, x, 0:3] = n[by, bx]
            f[y, x, 3:6] = po.plane_param(n[by, bx], [bx, by, z[by, bx]])
    return f


@pytest.mark.parametrize("K,rounds", [(4, 1), (8, 2), (20, 1)])
@pytest.mark.parametrize("it", [0, 1])
@pytest.mark.parametrize("stale", [False, True], ids=["rescored", "stale_costs"])
def test_serial_loop_equals_the_vectorised_formulation(K, rounds, it, stale):
    w, h, D = 9, 7, 4
    l, r = diffuse_ref.images(21, 15, D, 5)  # a small synthetic pair, cut to 9x7
    l, r = np.ascontiguousarray(l[4:4 + h, 6:6 + w]), np.ascontiguousarray(r[4:4 + h, 6:6 + w])
    pc = po.PlaneCost(l, r, D, 35, 2, 0.3)
    rng = np.random.default_rng(1000 * K + 10 * rounds + it)
    fields = [_hand_made_field(rng, w, h, D) for _ in (0, 1)]
    pms = [po.PatchMatch(l, r, D, 4) for _ in (0, 1)]
    for pm in pms:
        warm_ref.inject(pm, fields)
        if stale:  # costs that belong to no plane: some far too low (the pixel keeps its plane), some far too high
            for v in (0, 1):
                pm.min_cost(v)[...] = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) % 3 == 0, -1.0, 1e9)
        else:
            warm_ref.rescore(pm, pc, po.SUM_DEVICE)
    before = diffuse_ref.state_of(pms[0])
    diffuse_ref.diffuse(pms[0], pc, it, rounds, K, po.SUM_DEVICE)
    diffuse_ref.diffuse_vectorised(pms[1], pc, it, rounds, K, po.SUM_DEVICE)
    a, b = diffuse_ref.state_of(pms[0]), diffuse_ref.state_of(pms[1])
    for v in (0, 1):
        np.testing.assert_array_equal(a[v][0], b[v][0], err_msg=f"planes, view {v}")
        np.testing.assert_array_equal(a[v][1], b[v][1], err_msg=f"min_cost, view {v}")
        changed = np.any(a[v][0] != before[v][0], axis=2)
        assert 0 < changed.sum() < w * h
        assert np.all(a[v][1] <= before[v][1])
        if stale:  # no plane costs less than -1
            assert not np.any(changed[before[v][1] == -1.0]) and np.all(a[v][1][before[v][1] == -1.0] == -1.0)
        # an adopted plane is a snapshot neighbour's, taken whole: the point stays the neighbour's
        assert np.any(a[v][0][changed][:, 3] != np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))[changed])


@pytest.mark.parametrize("it", [0, 1])
@pytest.mark.parametrize("name", sorted(diffuse_ref.CASES))
def test_gpu_cases_are_not_vacuous(name, it):
    """the first propagation after the random init, on the restatement alone: a quarter of each view's pixels or more adopt a plane,
    every offset index is the last one accepted by some pixel of each view, and every offset index points outside the image from some
    pixel of each view"""
    c = diffuse_ref.CASES[name]
    p = diffuse_ref.first_propagation(name, it)
    inc = 1 if it % 2 == 0 else -1
    ys, xs = np.mgrid[0:c.h, 0:c.w]
    for v in (0, 1):
        a = p.adopted[v]
        assert np.mean(a >= 0) >= 0.25, (name, v, np.mean(a >= 0))
        hist = np.bincount(a[a >= 0], minlength=c.K)
        assert hist.min() >= 1, (name, v, hist)
        changed = np.any(p.end[v][0] != p.start[v][0], axis=2)
        assert np.all(changed <= (a >= 0))
        for k, (ox, oy) in enumerate(diffuse_ref.OFFSETS[c.K]):
            outside = (xs + inc * ox < 0) | (xs + inc * ox >= c.w) | (ys + inc * oy < 0) | (ys + inc * oy >= c.h)
            assert outside.any(), (name, k)
