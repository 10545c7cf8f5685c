"""-m "not gpu": the CPU restatement of the sub-pixel PostProcessing (tests/pp_sub_ref.py) against answers
derived by hand, against a scalar loop, and against the oracle's 8-bit PostProcessing in the case where the two must coincide."""
import ctypes as C
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

import pp_sub_ref as ps
from crossscalepatchmatch_amd import capi, synth
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = math.exp(-76.5)  # the smallest weight: |colour difference| = 765
FAR = 1000.0         # a disparity whose left-right target lies outside every image here


def _row(w, left=None, right=None, h=1):
    """h x w all-black pair (every weight is 1); fields: FAR in the left view and 0 in the right one (both inconsistent) except the
    listed columns: left = {x: (a, c)}, right = {x: c}, the same on every row"""
    abc_l, abc_r = ps.fronto_field(np.full((h, w), FAR)), ps.fronto_field(np.zeros((h, w)))
    for x, (a, c) in (left or {}).items():
        abc_l[:, x] = (a, 0.0, c)
    for x, c in (right or {}).items():
        abc_r[:, x, 2] = c
    img = np.zeros((h, w, 3), np.uint8)
    return abc_l, abc_r, img, img


# ---- the median of one pixel -------------------------------------------------------------------------------------------------
def test_tie_takes_the_smaller_value():
    # sum_wgt = 2, median_wgt = 1; the walk reaches exactly 1 at the smaller value and `>=` stops there
    assert ps.weighted_median_pixel(np.array([2.0, 1.0]), np.array([1.0, 1.0])) == 1.0
    assert ps.weighted_median_pixel(np.array([1.0, 2.0]), np.array([1.0, 1.0])) == 1.0


def test_answer_follows_the_f64_sums_not_exact_arithmetic():
    """values 1, 2, 3 with weights 1, exp(-76.5), 1.  In f64 sum_wgt = (1 + e) + 1 = 2 exactly (e is absorbed), median_wgt = 1, and the
    walk stops at value 1 (1 >= 1).  Exact arithmetic has median_wgt = 1 + e/2 > 1 and would go on to value 2."""
    for order in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        v, w = np.array([1.0, 2.0, 3.0])[order], np.array([1.0, E, 1.0])[order]
        assert ps.weighted_median_pixel(v, w) == 1.0
    # the same absorption inside one bin: value 1 collects (1 + e) = 1, value 2 collects 1: a tie, the smaller value
    assert ps.weighted_median_pixel(np.array([1.0, 2.0, 1.0]), np.array([1.0, 1.0, E])) == 1.0
    # and a walk that only tiny weights start: e, then e + 1 = 1 >= 1 stops at the middle value
    assert ps.weighted_median_pixel(np.array([1.0, 2.0, 3.0]), np.array([E, 1.0, 1.0])) == 2.0


def test_no_contribution_keeps_the_fill():
    assert ps.weighted_median_pixel(np.array([]), np.array([])) is None


def _scalar_median(vals, wgts):
    """the specification word for word, in Python floats"""
    sum_wgt = 0.0
    for w in wgts:
        sum_wgt += w
    bins = {}
    for v, w in zip(vals, wgts):
        bins[v] = bins.get(v, 0.0) + w
    median_wgt = sum_wgt / 2.0
    run = 0.0
    for u in sorted(bins):
        run += bins[u]
        if run >= median_wgt:
            return u if median_wgt > 0.0 else None
    return None


def test_vectorised_sums_are_the_serial_chains():
    """np.cumsum / np.add.at must add one by one in the stated order: compared with the scalar loop on windows of generic weights,
    where any other association shows up in the last bits of sum_wgt and moves the median of a tie-rich window"""
    rng = np.random.default_rng(5)
    moved = 0
    for trial in range(300):
        n = int(rng.integers(1, 1226))
        wgts = ps.LUT[rng.integers(0, 766 if trial % 2 else 40, n)]
        vals = rng.choice(rng.uniform(0.1, 60.0, int(rng.integers(1, 6 if trial % 3 else n + 1))), n)
        assert ps.weighted_median_pixel(vals, wgts) == _scalar_median(list(vals), list(wgts))
        serial = 0.0
        for w in wgts:
            serial += float(w)
        assert np.cumsum(wgts)[-1] == serial
        moved += serial != float(np.sum(wgts))
    assert moved > 0  # the pairwise sum differs somewhere: the comparison above can tell the two apart


# ---- whole maps ----------------------------------------------------------------------------------------------------------------
def test_nothing_consistent_keeps_the_raw_map_unclamped():
    abc_l, abc_r, il, ir = _row(9, h=3)
    abc_l[..., 2] = 3.7      # every target holds 0 in the other view: |3.7 - 0| > 0.5
    abc_l[1, 4, 2] = FAR     # a target outside the image
    abc_r[..., 2] = 0.0      # d == 0 is never consistent
    l, r, lv, rv = ps.postprocess_f64(abc_l, abc_r, il, ir, max_dis=2)
    assert not lv.any() and not rv.any()
    assert np.array_equal(l, ps.plane_disp(abc_l)) and l[0, 0] == 3.7 and l[1, 4] == FAR  # no side found: not filled, not clamped (D = 2)
    assert np.array_equal(r, np.zeros((3, 9)))


def test_zero_disparity_is_inconsistent_even_when_it_matches():
    # left 0.3 rounds to 0 and meets right 0.0 within half a pixel: left consistent; right 0.0 meets 0.3 too but fails `d > 0`
    abc_l, abc_r, il, ir = _row(3, left={1: (0.0, 0.3)}, right={1: 0.0})
    l, r, lv, rv = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert lv.tolist() == [[0, 1, 0]] and rv.tolist() == [[0, 0, 0]]
    assert l.tolist() == [[0.3, 0.3, 0.3]]  # the one consistent value reaches both neighbours through the median
    assert r.tolist() == [[0.0, 0.0, 0.0]]


def test_one_sided_fill_clamps_a_steep_plane_at_both_ends():
    """w = 40, one consistent left pixel at x = 20 on the plane d = 10 x - 199 (d(20) = 1, target column 19).  Columns within 17 of it
    take the median of its single value; beyond the window the one-sided fill stays: 10 x - 199 clamped to [0, D = 3]."""
    abc_l, abc_r, il, ir = _row(40, left={20: (10.0, -199.0)}, right={19: 1.0})
    l, r, lv, rv = ps.postprocess_f64(abc_l, abc_r, il, ir, max_dis=3)
    assert lv[0].nonzero()[0].tolist() == [20]
    want = np.full(40, 1.0)
    want[:3] = 0.0     # x = 0..2: only a right neighbour, plane value -199, -189, -179
    want[38:] = 3.0    # x = 38, 39: only a left neighbour, plane value 181, 191
    assert l[0].tolist() == want.tolist()
    # the right view: x = 19 (1.0 -> column 20 holds 1.0) is consistent, everything else fills from its fronto-parallel plane
    assert rv[0].nonzero()[0].tolist() == [19] and r[0].tolist() == [1.0] * 40


def test_two_sided_fill_takes_the_left_plane_unless_the_right_one_is_smaller():
    """consistent left pixels at x = 5 (fronto 2.0) and x = 55 (d = 0.5 x - 25.5, d(55) = 2.0).  x = 30 is 25 columns from both: no
    median.  dl = 2.0, dr = 0.5*30 - 25.5 = -10.5: dl <= dr fails, the right plane wins and is clamped to 0.  With the right plane
    made fronto 2.0 as well dl <= dr holds with equality and the left one is taken."""
    abc_l, abc_r, il, ir = _row(60, left={5: (0.0, 2.0), 55: (0.5, -25.5)}, right={3: 2.0, 53: 2.0})
    l, _, lv, _ = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert lv[0].nonzero()[0].tolist() == [5, 55]
    assert l[0, 30] == 0.0 and l[0, 23] == 0.0 and l[0, 37] == 0.0   # 23 = 5 + 18, 37 = 55 - 18: the first columns outside both windows
    assert l[0, 22] == 2.0 and l[0, 38] == 2.0                          # inside a window: the median of the one value in it
    abc_l[0, 55] = (0.0, 0.0, 2.25)                                     # rounds to 2: still consistent with right[53] = 2.0
    l, _, lv, _ = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert lv[0].nonzero()[0].tolist() == [5, 55] and l[0, 30] == 2.0   # dl = 2.0 <= dr = 2.25: the left one


def test_median_of_unit_weights_on_a_slanted_row():
    """all-black 1 x 6 pair.  Left: x = 0 holds 5.0 (target outside), x = 1..5 the plane 1 + 0.25 x = 1.25 .. 2.25 with targets
    0, 0, 1, 2, 3 (1.5 rounds to the even 2); right 1.4, 1.75, 2.0, 2.25 meets them within 0.5.  x = 0 is filled with 1 + 0.25*0 = 1.0
    and then takes the median of 1.25, 1.5, 1.75, 2.0, 2.25 (sum 5, half 2.5: the third value).  Right x = 4, 5 hold 0: filled with
    2.25 from x = 3, then the median of 1.4, 1.75, 2.0, 2.25 (sum 4, half 2: reached exactly at the second value)."""
    left = {x: (0.25, 1.0) for x in range(1, 6)}
    left[0] = (0.0, 5.0)
    abc_l, abc_r, il, ir = _row(6, left=left, right={0: 1.4, 1: 1.75, 2: 2.0, 3: 2.25})
    l, r, lv, rv = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert lv.tolist() == [[0, 1, 1, 1, 1, 1]] and rv.tolist() == [[1, 1, 1, 1, 0, 0]]
    assert l.tolist() == [[1.75, 1.25, 1.5, 1.75, 2.0, 2.25]]
    assert r.tolist() == [[1.4, 1.75, 2.0, 2.25, 1.75, 1.75]]


def test_colour_weights_decide_the_median():
    """1 x 5, left x = 2 inconsistent with colour (10, 0, 0); consistent neighbours x = 0, 1 hold 1.0 and x = 3, 4 hold 2.0.  Colours make
    the weights exp(-1), exp(-1) on the left and 1, exp(-0.3) on the right: sum = 2.4766.., half = 1.2383..; the walk has
    2 exp(-1) = 0.7358 after value 1.0 and passes the half at 2.0."""
    abc_l, abc_r, il, ir = _row(5, left={0: (0.0, 1.0), 1: (0.0, 1.0), 3: (0.0, 2.0), 4: (0.0, 2.0)}, right={0: 1.0, 1: 2.0, 2: 2.0})
    il = il.copy()
    il[0, :, 0] = [0, 20, 10, 10, 13]
    l, _, lv, _ = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert lv.tolist() == [[0, 1, 0, 1, 1]]   # x = 0: target -1 lies outside
    assert l[0, 2] == 2.0
    il[0, :, 0] = [0, 10, 10, 40, 40]          # now the left neighbour weighs 1 and the right ones exp(-3) each
    l, _, _, _ = ps.postprocess_f64(abc_l, abc_r, il, ir, 16)
    assert l[0, 2] == 1.0


# ---- reduction to the reference ------------------------------------------------------------------------------------------------
def _integer_fields(kind, h, w, top, rng):
    if kind == "random":
        return [rng.integers(0, top + 1, (h, w)) for _ in (0, 1)]
    if kind == "few":  # a handful of values per pixel: many inconsistent pixels whose windows hold few bins with many entries each
        return [rng.choice(rng.integers(0, top + 1, 3), (h, w)) for _ in (0, 1)]
    out = []
    for _ in (0, 1):   # piecewise constant: rectangles of one disparity
        by, bx = max(h // 4, 1), max(w // 6, 1)
        cells = rng.integers(1, top + 1, (-(-h // by), -(-w // bx)))
        out.append(np.repeat(np.repeat(cells, by, 0), bx, 1)[:h, :w])
    out[1] = np.where(rng.random((h, w)) < 0.8, out[0], out[1])  # mostly the same surface in both views: large consistent regions
    return out


def _images(kind, w, h, D, seed):
    if kind == "noise":
        l, r, _, _ = synth.make_pair(w, h, D, regions=3, seed=seed)
        return l, r
    return synth.make_adversarial(kind, w, h, D, seed=seed)


@pytest.mark.parametrize("dis_scale,D", [(1, 16), (1, 255), (2, 127)])
@pytest.mark.parametrize("images", ["noise", "blocks", "black"])
@pytest.mark.parametrize("field", ["random", "few", "piecewise"])
def test_integer_fronto_parallel_fields_reduce_to_the_reference(images, field, dis_scale, D):
    """fronto-parallel planes of integer disparity in [0, min(D, 255)]: every expression of DESIGN.md section 12 is then the
    reference's own, so the f64 maps equal its 8-bit maps (divided by dis_scale) at EVERY pixel of both views"""
    w, h = 61, 44
    rng = np.random.default_rng(zlib.crc32(repr((images, field, dis_scale, D)).encode()))
    l, r = _images(images, w, h, min(D, 40), 3)
    disp = _integer_fields(field, h, w, min(D, 255 // dis_scale), rng)
    pm = po.PatchMatch(l, r, D, dis_scale)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    for v in (0, 1):
        pl = pm.planes(v)  # live view: norm, point, param
        pl[...] = 0.0
        pl[..., 2] = 1.0
        pl[..., 3], pl[..., 4], pl[..., 5] = xs, ys, disp[v]
        pl[..., 8] = disp[v]
    pm.plane_to_disp()
    for v in (0, 1):
        assert np.array_equal(pm.dis(v), disp[v] * dis_scale)
    pm.postprocess()
    got = ps.postprocess_f64(ps.fronto_field(disp[0]), ps.fronto_field(disp[1]), l, r, D)
    for v in (0, 1):
        assert got[2 + v].sum() < h * w, "no inconsistent pixel: the case checks nothing"
        assert np.array_equal(got[v] * dis_scale, pm.dis(v).astype(np.float64)), f"view {v}: {np.sum(got[v] * dis_scale != pm.dis(v))} pixels differ"


# ---- the public surface ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    L = capi.load_library()
    for name in ("cspm_postprocess_f64", "cspm_postprocess_f64_device"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert L.cspm_postprocess_f64.argtypes is not None and len(L.cspm_postprocess_f64.argtypes) == 5
    assert callable(capi.StereoContext.postprocess_f64) and callable(capi.StereoContext.postprocess_f64_device)
    assert L.cspm_postprocess_f64(None, None, None, None, None) == -1  # CSPM_ERR_ARG without a context: host logic, no device needed


def test_cli_refuses_pp_pfm_without_use_pp(tmp_path):
    exe = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(exe), "build the host layer: python -c 'import __graft_entry__ as g; g.build()'"
    p = subprocess.run([exe, "--pp_pfm", f"--l_img_file={tmp_path}/none.png", f"--r_img_file={tmp_path}/none.png", "--max_dis=16", "--dis_scale=4",
                        "--cc_name=GRD", f"--l_disp_pfm={tmp_path}/l.pfm"], capture_output=True, timeout=120)
    assert p.returncode != 0
    assert b"--pp_pfm" in p.stdout and b"--use_pp" in p.stdout
    assert not os.path.exists(tmp_path / "l.pfm")
