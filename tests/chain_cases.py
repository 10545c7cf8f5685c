"""The CPU oracle's side of tests/chain_path_ref.py's case table: the synthetic pair of every case, the oracle's cost object per cost
kind, the start state (a block field's start costs are the oracle's re-score of it) and the state after ONE raster sweep in either
direction from that start, each computed once per session.  CPU only: the oracle (oracle/pyoracle.py), tests/cengrd_ref.py,
tests/warm_ref.py and the synthetic pairs, never the GPU library.  Callers must not write into what the cached functions return."""
import functools

import numpy as np

import cengrd_ref
import chain_path_ref as cp
import warm_ref
from crossscalepatchmatch_amd import synth
from oracle import pyoracle as po

DIS_SCALE = 4
KINDS = ("GRD", "CEN", "CENGRD", "IMG")
INC = {0: 1, 1: -1}  # the sweep direction of iteration `it`


@functools.lru_cache(maxsize=None)
def images(name):
    return _pair(name)[:2]


@functools.lru_cache(maxsize=None)
def _pair(name):
    c = cp.BY_NAME[name]
    g = c.geom
    return synth.make_pair(g.w, g.h, g.max_dis, regions=3, seed=c.seed)


@functools.lru_cache(maxsize=None)
def plane_cost(name, kind="GRD"):
    c = cp.BY_NAME[name]
    g = c.geom
    l, r = images(name)
    if kind == "CENGRD":
        return cengrd_ref.plane_cost(l, r, g.max_dis, g.wnd, g.scale_num, c.lam)
    return po.PlaneCost(l, r, g.max_dis, g.wnd, g.scale_num, c.lam, kind)


def _frozen(state):
    for a, b in state:
        a.setflags(write=False)
        b.setflags(write=False)
    return state


def _patchmatch(name):
    l, r = images(name)
    return po.PatchMatch(l, r, cp.BY_NAME[name].geom.max_dis, DIS_SCALE)


@functools.lru_cache(maxsize=None)
def start(name):
    """[(field (h, w, 6), stored cost (h, w))] per view: what cspm_set_planes gets.  Probe fields: the built costs (-1 / 1e300).  Block
    fields: the oracle's re-score under the fused GRD cost in the device order -- the costs cspm_rescore_planes must store."""
    c = cp.BY_NAME[name]
    fields = cp.case_fields(c, _pair(name)[2:])
    if c.kind == "probe":
        return _frozen([(f.copy(), cost.copy()) for f, cost in fields])
    pm = _patchmatch(name)
    warm_ref.inject(pm, [f for f, _ in fields])
    warm_ref.rescore(pm, plane_cost(name, "GRD"), po.SUM_DEVICE)
    return _frozen([(fields[v][0].copy(), pm.min_cost(v).copy()) for v in (0, 1)])


@functools.lru_cache(maxsize=None)
def swept(name, kind, it):
    """[(planes (h, w, 9), min_cost (h, w))] per view after PatchMatch.spatial(it) from start(name) under the cost of `kind`"""
    g = cp.BY_NAME[name].geom
    pm = _patchmatch(name)
    st = start(name)
    warm_ref.inject(pm, [f for f, _ in st])
    for v in (0, 1):
        pm.min_cost(v)[...] = st[v][1]
    pm.spatial(it, plane_cost(name, kind), sum_order=po.SUM_DEVICE, schedule=po.SCHED_RASTER, wavefront=min(g.w, g.h) >= 16)
    return _frozen([(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)])


def field_of(state, v):
    return np.concatenate([state[v][0][..., 0:3], state[v][0][..., 6:9]], -1)
