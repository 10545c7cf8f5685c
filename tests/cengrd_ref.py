"""CPU restatement of the CENGRD matching cost (include/cspm.h):

    cell = fma(KAPPA, min(H, TAU_CEN), G)        KAPPA = 2^-4, TAU_CEN = 32

G = the GRD cell the device reads (the oracle's volume_dev of a GRD cost), H = the census cell (the oracle's volume of a CEN cost).
KAPPA is a power of two and min(H, TAU_CEN) an integer <= 32, so KAPPA * min(H, TAU_CEN) is exact and the fma is the plain sum
G + KAPPA * min(H, TAU_CEN), rounded once: numpy's arithmetic gives the same bits.

plane_cost() writes the cells into an oracle cost object (its volume and volume_dev arrays, then refresh_max_cost(), as
tests/test_gpu_cost.py does for a foreign CCMethod's volumes), so the oracle's PatchMatch, its device summation order and its
post-processing run on CENGRD unchanged.  tests/test_gpu_cengrd.py holds the HIP entries to it bit for bit; tests/test_cengrd_ref.py
holds it to hand-derived cells and to tests/pyref.py.  It never imports the GPU package's library."""
import collections
import functools

import numpy as np

from crossscalepatchmatch_amd import realdata, synth
from oracle import pyoracle as po

KAPPA = 0.0625
TAU_CEN = 32.0

# the pairs of tests/test_gpu_cengrd.py: tests/test_cengrd_ref.py checks on the CPU that each of them exercises both branches of the min
Pair = collections.namedtuple("Pair", "kind w h D seed")
PAIRS = {"small": Pair("synth", 64, 48, 16, 11), "mid": Pair("synth", 96, 64, 16, 12), "odd": Pair("synth", 77, 41, 21, 13),
         "kinds": Pair("synth", 100, 76, 20, 15),  # three levels down to 25x19: the smallest GF filter (19 px)
         "ragged_63x65": Pair("synth", 63, 65, 12, 21), "ragged_64x63": Pair("synth", 64, 63, 12, 22), "ragged_65x64": Pair("synth", 65, 64, 12, 23),
         "adversarial": Pair("half_flat", 64, 48, 16, 5),
         "small_swapped": Pair("swapped", 64, 48, 16, 11),  # "small" with the two views exchanged (the batch driver's second pair)
         "crop": Pair("crop", 200, 128, 32, 0)}  # the committed half-size Motorcycle crop
# the level counts (scale_num; 0 = single scale) tests/test_gpu_cengrd.py builds each pair with: its _build() refuses any other, and
# tests/test_cengrd_ref.py asserts the branch fractions for exactly these
SCALES = {"small": (0, 3, 5), "mid": (0, 3, 5), "odd": (0, 3), "kinds": (3,), "ragged_63x65": (0, 3), "ragged_64x63": (0, 3),
          "ragged_65x64": (0, 3), "adversarial": (0, 3), "small_swapped": (3,), "crop": (5,)}
assert sorted(SCALES) == sorted(PAIRS)


@functools.lru_cache(maxsize=None)
def images(name):
    p = PAIRS[name]
    if p.kind == "synth":
        l, r, _, _ = synth.make_pair(p.w, p.h, p.D, regions=3, seed=p.seed)
    elif p.kind == "swapped":
        r, l, _, _ = synth.make_pair(p.w, p.h, p.D, regions=3, seed=p.seed)
    elif p.kind == "crop":
        cfg, l, r, _ = realdata.load_crop()
        assert (cfg["w"], cfg["h"], cfg["max_dis"]) == (p.w, p.h, p.D)
    else:
        l, r = synth.make_adversarial(p.kind, p.w, p.h, p.D, seed=p.seed)
    assert l.shape == (p.h, p.w, 3)
    return l, r


def combine(G, H):
    """the cells from GRD device cells and census cells of one level and view"""
    return np.asarray(G, dtype=np.float64) + KAPPA * np.minimum(np.asarray(H, dtype=np.float64), TAU_CEN)


def cells_from(grd_pc, cen_pc):
    """[view][level] cells from two cost objects with volume_dev / volume accessors (the oracle's, or adapters around tests/pyref.py)"""
    return [[combine(grd_pc.volume_dev(v, s), cen_pc.volume(v, s)) for s in range(grd_pc.levels)] for v in (0, 1)]


def inject(pc, cells):
    """cells[view][level] -> the oracle cost object's volume and volume_dev arrays; both summation orders then read exactly these"""
    for v in (0, 1):
        for s in range(pc.levels):
            assert pc.volume(v, s).shape == cells[v][s].shape
            pc.volume(v, s)[...] = cells[v][s]
            pc.volume_dev(v, s)[...] = cells[v][s]
    pc.refresh_max_cost()
    return pc


def plane_cost(l, r, max_dis, wnd=35, scale_num=0, lam=0.0, cells=None):
    """an oracle PlaneCost (PreSSPC / PreCSPC) whose volumes hold the CENGRD cells; `cells` replaces the oracle-built ones"""
    pc = po.PlaneCost(l, r, max_dis, wnd, scale_num, lam, "GRD")
    if cells is None:
        cells = cells_from(pc, po.PlaneCost(l, r, max_dis, wnd, scale_num, lam, "CEN"))
    return inject(pc, cells)


class PyrefVolumes:
    """tests/pyref.py's independent volumes behind the accessors cells_from() uses"""

    def __init__(self, l, r, max_dis, scale_num, cc):
        import pyref
        self.pc = pyref.PlaneCost(l, r, max_dis, 35, scale_num, 0.0, cc, dev=True)
        self.levels = len(self.pc.dims)

    def volume(self, v, s):
        return self.pc.vol[v][s]

    def volume_dev(self, v, s):
        return self.pc.vol_dev[v][s]


def branch_fractions(l, r, max_dis, scale_num):
    """[(view, level, fraction of cells with H < TAU_CEN, fraction with H >= TAU_CEN)]"""
    cen = po.PlaneCost(l, r, max_dis, 35, scale_num, 0.0, "CEN")
    out = []
    for v in (0, 1):
        for s in range(cen.levels):
            H = cen.volume(v, s)
            out.append((v, s, float(np.mean(H < TAU_CEN)), float(np.mean(H >= TAU_CEN))))
    return out
