"""-m "not gpu": the CPU restatement of the CENGRD cost (tests/cengrd_ref.py) against cells derived by hand, against tests/pyref.py's
independent volumes, and the check that every pair tests/test_gpu_cengrd.py uses exercises both branches of min(H, TAU_CEN)."""
from fractions import Fraction

import numpy as np
import pytest

import cengrd_ref
from oracle import pyoracle as po


def _tiny_pair():
    """9x9 gray-valued pair.  With a 9x9 image the wrap-around 9x9 census window of ANY pixel covers every other pixel exactly once, so
    a pixel's code has one bit per other pixel that is darker than it.
    left : rows 0-2 and columns 0-4 of row 3 are 50 (32 pixels), pixel (4, 6) is 200, the other 48 pixels are 250
    right: 100 everywhere (every code is zero, every gradient is zero)"""
    l = np.full((9, 9), 250, np.uint8)
    l[0:3, :] = 50
    l[3, 0:5] = 50
    l[6, 4] = 200
    r = np.full((9, 9), 100, np.uint8)
    return np.repeat(l[..., None], 3, 2), np.repeat(r[..., None], 3, 2)


def test_hand_derived_cells():
    l, r = _tiny_pair()
    pc = cengrd_ref.plane_cost(l, r, 4)
    L, R = pc.volume(0, 0), pc.volume(1, 0)
    assert L.shape == (5, 9, 9)
    np.testing.assert_array_equal(pc.volume_dev(0, 0), L)
    # every colour difference here is >= 50 per channel (or 97 against the border's 3): the colour term is ALPHA * TAU_CLR = 1.0
    clr = 0.1 * 10.0
    assert clr == 1.0
    # d = 0, pixels whose row neighbours are equal (own gradient 0, the other view's gradient 0): G = fma(0.9, 0, 1.0) = 1.0
    #   (4, 6) = 200: darker pixels = the 32 fifties           H = 32 exactly -> 1.0 + 2^-4 * 32 = 3.0
    #   (4, 1) = 50 : nothing is darker                        H = 0          -> 1.0
    #   (4, 7) = 250: the 32 fifties and the 200               H = 33 -> 32   -> 3.0
    assert L[0, 6, 4] == 3.0
    assert L[0, 1, 4] == 1.0
    assert L[0, 7, 4] == 3.0
    cen_pc = po.PlaneCost(l, r, 4, 35, 0, 0.0, "CEN")
    cen = cen_pc.volume(0, 0)
    assert (cen[0, 6, 4], cen[0, 1, 4], cen[0, 7, 4]) == (32.0, 0.0, 33.0)
    # borders: the other view is outside, G comes from the constant-3 branch -- gradient difference |0 - 3| truncated to TAU_GRD = 2,
    # G = fma(1 - ALPHA, 2, 1.0) rounded once -- and H = 80 -> 32
    g_border = float(Fraction(1 - 0.1) * 2 + Fraction(clr))
    assert L[2, 7, 1] == g_border + 2.0          # left view, x - d = -1
    assert R[2, 7, 8] == g_border + 2.0          # right view, x + d = 10 >= 9
    assert 4.79 < g_border + 2.0 < 4.81
    # max_cost is the maximum over the volume
    assert pc.max_cost(0, 0) == L.max() and pc.max_cost_dev(1, 0) == R.max()
    assert L.min() >= 0.0 and R.min() >= 0.0


@pytest.mark.parametrize("scale_num", [0, 2])
def test_restatement_from_independent_volumes(scale_num):
    """the cells built from tests/pyref.py's GRD (device form, exact rational fma) and census volumes == the ones built from the oracle"""
    from crossscalepatchmatch_amd import synth
    l, r, _, _ = synth.make_pair(26, 18, 6, regions=2, seed=4)
    grd, cen = po.PlaneCost(l, r, 6, 35, scale_num, 0.0, "GRD"), po.PlaneCost(l, r, 6, 35, scale_num, 0.0, "CEN")
    want = cengrd_ref.cells_from(grd, cen)
    got = cengrd_ref.cells_from(cengrd_ref.PyrefVolumes(l, r, 6, scale_num, "GRD"), cengrd_ref.PyrefVolumes(l, r, 6, scale_num, "CEN"))
    pc = cengrd_ref.plane_cost(l, r, 6, 35, scale_num, 0.0)
    for v in (0, 1):
        assert len(got[v]) == len(want[v]) == pc.levels
        for s in range(pc.levels):
            np.testing.assert_array_equal(got[v][s], want[v][s])
            np.testing.assert_array_equal(pc.volume(v, s), want[v][s])
            np.testing.assert_array_equal(pc.volume_dev(v, s), want[v][s])
            assert pc.max_cost(v, s) == pc.max_cost_dev(v, s) == want[v][s].max()
    # the fma of the definition, in exact rational arithmetic, on a sample of cells: the plain sum has the same bits
    import pyref
    g, h = grd.volume_dev(0, 0).ravel(), cen.volume(0, 0).ravel()  # views of the two cost objects' memory: they stay alive above
    for i in range(0, g.size, 7):
        assert pyref.fma(cengrd_ref.KAPPA, min(h[i], cengrd_ref.TAU_CEN), g[i]) == want[0][0].ravel()[i]


@pytest.mark.parametrize("name", sorted(cengrd_ref.PAIRS))
def test_gpu_pairs_exercise_both_branches(name):
    """on every level and in both views at least 1 % of the cells have H < TAU_CEN and at least 1 % have H >= TAU_CEN, for every level
    count the GPU tests build the pair with (cengrd_ref.SCALES, which their _build() enforces)"""
    p = cengrd_ref.PAIRS[name]
    l, r = cengrd_ref.images(name)
    for scale_num in cengrd_ref.SCALES[name]:
        for v, s, below, at_or_above in cengrd_ref.branch_fractions(l, r, p.D, scale_num):
            assert below >= 0.01 and at_or_above >= 0.01, (name, scale_num, v, s, below, at_or_above)


def test_constants_agree_with_the_header():
    """KAPPA and TAU_CEN are restated here on purpose (the restatement does not read the product); the header's #defines and the
    binding's copy must say the same"""
    import os
    import re
    from crossscalepatchmatch_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cspm.h")).read()
    defs = {m.group(1): float(m.group(2)) for m in re.finditer(r"^#define\s+(CSPM_CENGRD_[A-Z]+)\s+([0-9.]+)", hdr, re.M)}
    assert defs == {"CSPM_CENGRD_KAPPA": cengrd_ref.KAPPA, "CSPM_CENGRD_TAU": cengrd_ref.TAU_CEN}
    assert (capi.CENGRD_KAPPA, capi.CENGRD_TAU) == (cengrd_ref.KAPPA, cengrd_ref.TAU_CEN)
