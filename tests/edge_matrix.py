"""The case table of tests/test_gpu_edge_matrix.py: every cost source of the tap engines crossed with every way the host hands the
work out (folded sweep workgroups, per-diagonal launches, dataflow claims, claimed column bands, refinement steps per launch), at
degenerate image sizes and on tie-heavy pairs -- and the CPU oracle's state for every case, computed once per session.

CPU only: it imports the oracle (oracle/pyoracle.py), the restatements tests/cengrd_ref.py and tests/diffuse_ref.py and the synthetic
pairs, never the GPU library.  Options are named by the attribute they have in crossscalepatchmatch_amd/capi.py, as strings; the GPU
module resolves them.  tests/test_edge_matrix.py checks on the CPU that none of the cases listed here is vacuous.

Callers must not write into what the cached functions return."""
import collections
import functools

import numpy as np

import cengrd_ref
import diffuse_ref
from crossscalepatchmatch_amd import synth
from oracle import pyoracle as po

WND = 35
DIS_SCALE = 2
SEED = 3        # the random init of every case but the tie-heavy ones (TIE_SEED)
ITERS = 2
RASTER, REDBLACK, DIFFUSE = po.SCHED_RASTER, po.SCHED_REDBLACK, diffuse_ref.SCHED_DIFFUSE
MODES = ((0, 0.0), (5, 0.3))  # (scale_num, reg_lambda): single scale, five levels
KINDS = ("GRD", "CEN", "CENGRD", "IMG")

# ---- sources ---------------------------------------------------------------------------------------------------------------------
# build: the StereoContext method; kwargs: its keyword arguments; options: set before the build; active: what get_option must report
# after it; restore: the library defaults of every option the build touched, set again in a `finally`
Source = collections.namedtuple("Source", "name kind build kwargs options active restore")


def _src(name, kind, build, kwargs=(), options=(), active=(), restore=()):
    return Source(name, kind, build, dict(kwargs), dict(options), dict(active), dict(restore))


SOURCES = collections.OrderedDict((s.name, s) for s in (
    _src("grd_fused", "GRD", "build_cost_grd"),
    _src("grd_computed", "GRD", "build_cost_grd", dict(table_volumes=False), active=dict(OPT_TABLE_VOLUMES_ACTIVE=0), restore=dict(OPT_TABLE_VOLUMES=1)),
    _src("grd_volumes", "GRD", "build_cost_grd", dict(volumes=True), restore=dict(OPT_GRD_VOLUMES=0)),
    _src("grd_pairs", "GRD", "build_cost_grd", dict(sweep_pairs=True), active=dict(OPT_SWEEP_PAIRS_ACTIVE=1), restore=dict(OPT_SWEEP_PAIRS=0)),
    _src("grd_packed", "GRD", "build_cost_grd", options=dict(OPT_SWEEP_PACKED=1), active=dict(OPT_SWEEP_PACKED_ACTIVE=1, OPT_SWEEP_PACKED_BAD=0),
         restore=dict(OPT_SWEEP_PACKED=0)),
    _src("cen_fused", "CEN", "build_cost_cen"),
    _src("cen_volumes", "CEN", "build_cost_cen", dict(volumes=True), restore=dict(OPT_GRD_VOLUMES=0)),
    _src("cengrd_volumes", "CENGRD", "build_cost_cengrd", dict(fused=False), active=dict(OPT_CENGRD_FUSED_ACTIVE=0), restore=dict(OPT_CENGRD_FUSED=0)),
    _src("cengrd_fused", "CENGRD", "build_cost_cengrd", dict(fused=True), active=dict(OPT_CENGRD_FUSED_ACTIVE=1), restore=dict(OPT_CENGRD_FUSED=0)),
    _src("img", "IMG", "build_cost_img"),
))
assert len(SOURCES) == 10


def sources_of(kind):
    return [s for s in SOURCES.values() if s.kind == kind]


# ---- pairs -----------------------------------------------------------------------------------------------------------------------
# a pair is a hashable key: (w, h, max_dis) -- synth.make_pair(w, h, D, regions=3, seed=100 * w + h); "odd" -- conftest.py's odd_pair;
# "black" / "white" / "stripes" -- the tie-heavy pairs
GEOMETRIES = [(1, 1, 2), (2, 1, 2), (1, 7, 3), (3, 3, 1),
              (9, 2, 4), (5, 40, 4), (37, 3, 6), (20, 20, 25),
              (64, 1, 5), (65, 2, 70), (63, 5, 8), (129, 3, 8)]
# launch-shape and memory-safety cases: GRD, CEN and CENGRD cost every plane alike there.  Never the only cases of a test
THIN = [(1, 1, 2), (2, 1, 2), (1, 7, 3), (3, 3, 1)]
MOVING = [g for g in GEOMETRIES if g not in THIN]
assert len(MOVING) == 8 and all(w * h >= 18 for w, h, _ in MOVING)
# GrdPC / CSPC where the reference cannot run the geometry above it (refused() below): the same images' sizes with max_dis = width
IMG_EXTRA = [(20, 20, 20), (65, 2, 65)]
ODD = "odd"
ODD_SIZE = (77, 41, 21)
TIE_PAIRS = ("black", "white", "stripes")
TIE_SIZE = (80, 24, 12)


@functools.lru_cache(maxsize=None)
def images(pair):
    if pair == ODD:
        w, h, D = ODD_SIZE
        l, r = synth.make_pair(w, h, D, regions=3, seed=13)[:2]
    elif pair in TIE_PAIRS:
        w, h, D = TIE_SIZE
        l, r = synth.make_adversarial(pair, w, h, D, seed=5)
    else:
        w, h, D = pair
        l, r = synth.make_pair(w, h, D, regions=3, seed=100 * w + h)[:2]
    assert l.shape == r.shape == (h, w, 3)
    return l, r


def size_of(pair):
    return ODD_SIZE if pair == ODD else TIE_SIZE if pair in TIE_PAIRS else pair


def pair_id(pair):
    return pair if isinstance(pair, str) else "%dx%dx%d" % pair


REFUSAL = r"cspm error -1: cspm_build_cost_img: max_dis must not exceed the image width"


def refused(pair, kind):
    """GrdPC / CSPC with max_dis > width: HandleBorder (the reference's commfunc.h:129-145) wraps a column once, a tap at
    q_x + q_disp >= 2 * width then reads beyond the other view's row (grd_pc.cc:153-165, cspc.cc:153-166; oracle/cspm_oracle.c tap()
    likewise).  There is nothing to compare with: cspm_build_cost_img returns CSPM_ERR_ARG (include/cspm.h), the oracle is not run."""
    w, _, D = size_of(pair)
    return kind == "IMG" and D > w


def geometries_of(kind):
    return GEOMETRIES + (IMG_EXTRA if kind == "IMG" else [])


def fold_pairs_of(kind):
    return FOLD_PAIRS + (IMG_EXTRA if kind == "IMG" else [])


def row_pairs_of(kind):
    return ROW_PAIRS + (IMG_EXTRA[1:] if kind == "IMG" else [])


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plane_cost(pair, kind, sn, lam):
    """the oracle's cost object of one kind; the five GRD sources share it"""
    assert not refused(pair, kind), "the oracle would index out of range"
    l, r = images(pair)
    D = size_of(pair)[2]
    if kind == "CENGRD":
        return cengrd_ref.plane_cost(l, r, D, WND, sn, lam)
    return po.PlaneCost(l, r, D, WND, sn, lam, kind)


def _patchmatch(pair):
    l, r = images(pair)
    return po.PatchMatch(l, r, size_of(pair)[2], DIS_SCALE)


def state_of(pm):
    """[(planes (h, w, 9), min_cost (h, w))] per view, copies"""
    return [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]


def _okw(sched, K, seed=SEED):
    return dict(seed=seed, schedule=sched, sum_order=po.SUM_DEVICE, rb_rounds=1, rb_neighbours=K)


def _spatial(pm, pc, it, sched, K):
    if sched == DIFFUSE:
        diffuse_ref.diffuse(pm, pc, it, 1, K, po.SUM_DEVICE)
    else:
        pm.spatial(it, pc, **_okw(sched, K))


# state: after the iterations; dis / disp: PlaneToDisp's 8-bit and f64 maps of both views; post: the post-processed 8-bit maps
Run = collections.namedtuple("Run", "state dis disp post")


@functools.lru_cache(maxsize=None)
def whole_run(pair, kind, sn, lam, sched, K=4, seed=SEED, iters=ITERS):
    """the random init and `iters` iterations under one schedule (K: rb_neighbours), then the maps and the post-processing"""
    pc = plane_cost(pair, kind, sn, lam)
    pm = _patchmatch(pair)
    if sched == DIFFUSE:
        diffuse_ref.run(pm, pc, iters, 1, K, seed=seed, sum_order=po.SUM_DEVICE)
        pm.plane_to_disp()
    else:
        # thin images walk the reference's serial double loop: anti-diagonals of one to five pixels give the parallel walk nothing
        pm.run(iters, pc, False, wavefront=min(pm.w, pm.h) >= 16, **_okw(sched, K, seed))
    state = state_of(pm)
    dis = [pm.dis(v) for v in (0, 1)]
    disp = [pm.disp_f64(v) for v in (0, 1)]
    pm.postprocess()
    return Run(state, dis, disp, [pm.dis(v) for v in (0, 1)])


@functools.lru_cache(maxsize=None)
def sweep_phases(pair, kind, sn, lam):
    """the states after the random init, the raster sweep of iteration 0 (forwards) and that of iteration 1 (backwards)"""
    pc = plane_cost(pair, kind, sn, lam)
    pm = _patchmatch(pair)
    pm.init(pc, **_okw(RASTER, 4))
    out = [state_of(pm)]
    for it in (0, 1):
        pm.spatial(it, pc, **_okw(RASTER, 4))
        out.append(state_of(pm))
    return out


@functools.lru_cache(maxsize=None)
def first_iteration(pair, kind, sn, lam, sched, K=4):
    """the states after the random init and after each of the first spatial propagation, view propagation and refinement"""
    pc = plane_cost(pair, kind, sn, lam)
    pm = _patchmatch(pair)
    pm.init(pc, **_okw(RASTER, 4))
    out = [state_of(pm)]
    _spatial(pm, pc, 0, sched, K)
    out.append(state_of(pm))
    pm.view(0, pc, **_okw(RASTER, 4))
    out.append(state_of(pm))
    pm.refine(0, pc, **_okw(RASTER, 4))
    out.append(state_of(pm))
    return out


def changed_fraction(before, after, view=0):
    """fraction of a view's pixels whose plane (norm or param) differs between two states"""
    a, b = before[view][0], after[view][0]
    return float(np.mean(np.any(a[..., 0:3] != b[..., 0:3], axis=2) | np.any(a[..., 6:9] != b[..., 6:9], axis=2)))


def tied_fraction(min_cost):
    """fraction of pixels whose min_cost another pixel also holds exactly"""
    _, inverse, counts = np.unique(min_cost.ravel(), return_inverse=True, return_counts=True)
    return float(np.mean(counts[inverse] > 1))


# ---- the cases of tests/test_gpu_edge_matrix.py ----------------------------------------------------------------------------------

def schedules_at(geom):
    """(schedule, rb_neighbours) of test a; K = 20 where most of its offsets leave the image"""
    out = [(RASTER, 4), (REDBLACK, 4), (DIFFUSE, 8)]
    if geom[:2] in ((9, 2), (1, 7)):
        out.append((DIFFUSE, 20))
    return out


# b. the folded sweep
FOLD_PAIRS = [(9, 2, 4), (37, 3, 6), (20, 20, 25), (65, 2, 70), (129, 3, 8), ODD]
FOLD_LEVELS = (4, 5)
FOLD_LAM = 0.3
UNFOLDED_CASE = ((37, 3, 6), 3)  # three levels with the option on: sweep_folded() is false

# c. the row kernels' hand-out
ROW_ENV = [("CSPM_ROW_CLAIM", "1"), ("CSPM_REFINE_CHUNK", "1"), ("CSPM_REFINE_CHUNK", "3")]
ROW_SOURCES = ["grd_fused", "grd_volumes", "cen_fused", "cengrd_fused", "img"]  # one of each element layout
ROW_PAIRS = [(1, 1, 2), (9, 2, 4), (37, 3, 6), (65, 2, 70), (129, 3, 8)]
ROW_SCHEDULES = [(RASTER, 4), (DIFFUSE, 8)]
ROW_SINGLE_SCALE_PAIR = (37, 3, 6)

# d. ties: (source, schedule, rb_neighbours, CSPM_OPT_SWEEP_FOLD)
TIE_CASES = [("cengrd_volumes", RASTER, 4, 0), ("cengrd_volumes", REDBLACK, 4, 0), ("cengrd_fused", RASTER, 4, 0), ("cengrd_fused", REDBLACK, 4, 0),
             ("grd_fused", DIFFUSE, 8, 0), ("cen_fused", DIFFUSE, 8, 0), ("cengrd_fused", DIFFUSE, 8, 0),
             ("cen_fused", RASTER, 4, 1), ("img", RASTER, 4, 1), ("cengrd_fused", RASTER, 4, 1)]
TIE_MODE = (5, 0.3)
# the init seed of the tie cases: with SEED the stripes pair under census ends a raster run with 18 % of view 0's pixels sharing a
# min_cost, below what tests/test_edge_matrix.py asks for; with this one every kind stays above it on every pair
TIE_SEED = 7


def sched_id(sched, K):
    return {RASTER: "raster", REDBLACK: "redblack", DIFFUSE: "diffuse%d" % K}[sched]
