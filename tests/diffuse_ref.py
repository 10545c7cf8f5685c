"""CPU restatement of spatial propagation under CSPM_SCHED_DIFFUSE (include/cspm.h): every pixel tries the
planes of K fixed near and far neighbours, read from a snapshot of the field taken when the round starts.  It works on the objects of
the CPU oracle (oracle/pyoracle.py) only and never loads the GPU library; tests/test_gpu_diffuse.py holds the HIP kernel to it bit
for bit, tests/test_diffuse_ref.py checks the restatement itself without a GPU.

The specification, literally: a round copies both views' planes into S; then every pixel (x, y) of every view v, independently of
every other pixel, starts from m = its stored min_cost and walks k = 0 .. K-1: (ox, oy) = inc * O_k (inc = +1 for even iterations,
-1 for odd ones); a neighbour outside the image is no candidate; otherwise the candidate is S[v][y+oy][x+ox] taken whole and where
its cost at (x, y) is < m the pixel's plane and min_cost become the candidate and that cost."""
import collections
import functools

import numpy as np

from crossscalepatchmatch_amd import synth
from oracle import pyoracle as po

SCHED_DIFFUSE = 2  # CSPM_SCHED_DIFFUSE

_NEAR = [(-1, 0), (0, -1), (1, 0), (0, 1)]  # the order of the red-black kernel's four neighbours
_R3 = [(-3, 0), (0, -3), (3, 0), (0, 3)]
_R5 = [(-5, 0), (0, -5), (5, 0), (0, 5)]
_KNIGHT = [(-1, -2), (1, -2), (2, -1), (2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1)]
OFFSETS = {4: _NEAR, 8: _NEAR + _R5, 20: _NEAR + _R3 + _R5 + _KNIGHT}  # O_0 .. O_{K-1} as (ox, oy); K = 20: Gipuma's pattern


def diffuse(pm, pc, it, rounds=1, neighbours=8, sum_order=po.SUM_DEVICE, adopted=None):
    """one SpatialPropagation of iteration `it` on the oracle PatchMatch pm under the oracle PlaneCost pc.
    adopted: optional list of two (h, w) int arrays that receive, per view, the index k of the last candidate each pixel accepted
    in this propagation (-1: it kept its plane through every round)."""
    inc = 1 if it % 2 == 0 else -1
    offs = [(inc * ox, inc * oy) for ox, oy in OFFSETS[neighbours]]
    if adopted is not None:
        for a in adopted:
            a[...] = -1
    for _ in range(rounds):
        snap = [pm.planes(v).copy() for v in (0, 1)]
        for v in (0, 1):
            P, cost, S = pm.planes(v), pm.min_cost(v), snap[v]
            for y in range(pm.h):
                for x in range(pm.w):
                    m = cost[y, x]
                    for k, (ox, oy) in enumerate(offs):
                        xn, yn = x + ox, y + oy
                        if xn < 0 or xn >= pm.w or yn < 0 or yn >= pm.h:
                            continue
                        cand = S[yn, xn]
                        c = pc.cost(x, y, cand[0:3], cand[6:9], v, sum_order)
                        if c < m:
                            P[y, x, :] = cand  # norm, point and param of the neighbour: the Plane as a whole
                            cost[y, x] = c
                            m = c
                            if adopted is not None:
                                adopted[v][y, x] = k


def diffuse_vectorised(pm, pc, it, rounds=1, neighbours=8, sum_order=po.SUM_DEVICE):
    """the same propagation in a second formulation: the costs of ALL candidates of a round are evaluated from the snapshot first
    (no candidate depends on an acceptance), then every pixel applies the strict `<` over k in order with array operations"""
    inc = 1 if it % 2 == 0 else -1
    offs = [(inc * ox, inc * oy) for ox, oy in OFFSETS[neighbours]]
    h, w = pm.h, pm.w
    ys, xs = np.mgrid[0:h, 0:w]
    for _ in range(rounds):
        snap = [pm.planes(v).copy() for v in (0, 1)]
        for v in (0, 1):
            S = snap[v]
            table = np.full((len(offs), h, w), np.inf)
            for k, (ox, oy) in enumerate(offs):
                for y in range(max(0, -oy), min(h, h - oy)):
                    for x in range(max(0, -ox), min(w, w - ox)):
                        table[k, y, x] = pc.cost(x, y, S[y + oy, x + ox, 0:3], S[y + oy, x + ox, 6:9], v, sum_order)
            m = pm.min_cost(v).copy()
            best = np.full((h, w), -1)
            for k in range(len(offs)):  # +inf (no candidate) is never < m
                take = table[k] < m
                m = np.where(take, table[k], m)
                best = np.where(take, k, best)
            P = pm.planes(v)
            for k, (ox, oy) in enumerate(offs):
                sel = best == k
                P[sel] = S[ys[sel] + oy, xs[sel] + ox]
            pm.min_cost(v)[...] = m


def run(pm, pc, iters, rounds=1, neighbours=8, **opts):
    """cspm_patchmatch under CSPM_SCHED_DIFFUSE: the random init, then per iteration diffuse, view propagation, refinement
    (opts as for PatchMatch.run: seed, sum_order, rng_mode)"""
    pm.init(pc, **opts)
    iterate(pm, pc, iters, rounds, neighbours, **opts)


def iterate(pm, pc, iters, rounds=1, neighbours=8, **opts):
    """iterations 0 .. iters-1 from the state that is there (a warm run after its re-score)"""
    for it in range(iters):
        diffuse(pm, pc, it, rounds, neighbours, opts.get("sum_order", po.SUM_SERIAL))
        pm.view(it, pc, **opts)
        pm.refine(it, pc, **opts)


# ---- the pairs and settings of tests/test_gpu_diffuse.py ------------------------------------------------------------------------
# tests/test_diffuse_ref.py checks on the CPU that the first propagation after the random init of every one of them adopts planes at
# a quarter of the pixels or more, through every offset index, and meets the image border with every offset index.
# cc: GRD | CEN | IMG (GrdPC / CSPC) | CENGRD (tests/cengrd_ref.py); sn: pyramid levels, 0 = single scale; K, rounds: rb_neighbours,
# rb_rounds; img / seed: the seeds of the synthetic pair and of the random init
Case = collections.namedtuple("Case", "w h D img cc sn lam K rounds seed")
CASES = {
    "65x33_ss_k20": Case(65, 33, 12, 31, "GRD", 0, 0.0, 20, 1, 101),
    "63x21_cs_k8": Case(63, 21, 12, 32, "GRD", 3, 0.3, 8, 1, 102),
    "64x21_cs_k8": Case(64, 21, 12, 33, "GRD", 3, 0.3, 8, 1, 103),
    "130x21_cs_k8": Case(130, 21, 12, 34, "GRD", 3, 0.3, 8, 1, 104),  # three segments, the last of 2 lanes
    # most far neighbours outside the image; 63 pixels for 20 offset indices: the seeds were searched for (about 1 in 300 init seeds
    # lets every index be some pixel's last acceptance in both views and both directions)
    "9x7_ss_k20": Case(9, 7, 4, 37, "GRD", 0, 0.0, 20, 1, 89),
    "96x64_cs5_k4_r2": Case(96, 64, 16, 12, "GRD", 5, 0.3, 4, 2, 106),
    "96x64_cs5_k8_r2": Case(96, 64, 16, 12, "GRD", 5, 0.3, 8, 2, 107),
    "96x64_cs5_k8": Case(96, 64, 16, 12, "GRD", 5, 0.3, 8, 1, 108),   # the whole run
    "65x33_grd_k8": Case(65, 33, 12, 31, "GRD", 3, 0.3, 8, 1, 109),    # the cost sources: fused and volume-sourced GRD, ...
    "65x33_cen_k8": Case(65, 33, 12, 31, "CEN", 3, 0.3, 8, 1, 110),
    "65x33_img_k8": Case(65, 33, 12, 31, "IMG", 3, 0.3, 8, 1, 111),
    "65x33_cengrd_k8": Case(65, 33, 12, 31, "CENGRD", 3, 0.3, 8, 1, 112),
}
PHASE_CASES = ["65x33_ss_k20", "63x21_cs_k8", "64x21_cs_k8", "130x21_cs_k8", "9x7_ss_k20", "96x64_cs5_k4_r2", "96x64_cs5_k8_r2"]
DIS_SCALE = 4


@functools.lru_cache(maxsize=None)
def images(w, h, D, seed):
    l, r, _, _ = synth.make_pair(w, h, D, regions=3, seed=seed)
    return l, r


@functools.lru_cache(maxsize=None)
def plane_cost(w, h, D, img, cc, sn, lam):
    l, r = images(w, h, D, img)
    if cc == "CENGRD":
        import cengrd_ref
        return cengrd_ref.plane_cost(l, r, D, 35, sn, lam)
    return po.PlaneCost(l, r, D, 35, sn, lam, cc)


def case_cost(c):
    return plane_cost(c.w, c.h, c.D, c.img, c.cc, c.sn, c.lam)


def state_of(pm):
    """[(planes (h, w, 9), min_cost (h, w))] per view, copies"""
    return [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]


Propagation = collections.namedtuple("Propagation", "start end adopted")


@functools.lru_cache(maxsize=None)
def first_propagation(name, it):
    """the random init of CASES[name], then one propagation of iteration `it`: the oracle's state before and after it and, per view,
    the offset index every pixel ended with (-1: it kept its plane).  Computed once per session; callers must not write into it."""
    c = CASES[name]
    pc = case_cost(c)
    pm = po.PatchMatch(*images(c.w, c.h, c.D, c.img), c.D, DIS_SCALE)
    pm.init(pc, seed=c.seed, sum_order=po.SUM_DEVICE)
    start = state_of(pm)
    adopted = [np.zeros((c.h, c.w), np.int64) for _ in (0, 1)]
    diffuse(pm, pc, it, c.rounds, c.K, po.SUM_DEVICE, adopted)
    return Propagation(start, state_of(pm), adopted)
