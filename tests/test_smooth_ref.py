"""-m "not gpu": the CPU restatement of the edge-aware global smoother (tests/smooth_ref.py): its two forms
against each other bit for bit, one pass against numpy.linalg.solve on the dense system, the properties the specification promises
(constants stay, lambda = 0 and C = 0 are the identity, outputs stay within the confident nodes' range, edges stop the diffusion,
holes are filled), lines of length 1, the clamp, the argument errors the bindings report without a device, and header against bindings.

The two tolerance bounds are 100 x the largest deviation measured once on the CPU with these very inputs:
1.1e-14 against the dense solve (rows of 9 and 33 pixels, values below 50, lambda = 100, sigma = 20) and 3.6e-14 on the constant map
(17 x 33, value 37.25, T = 3).  A transcription slip is of order 1e-1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import smooth_ref as sr
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_BOUND = 100 * 1.1e-14
CONST_BOUND = 100 * 3.6e-14
PALETTE = sr.PALETTE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def palette_guide(rng, h, w):
    return PALETTE[rng.integers(0, 4, (h, w))]


def holed_map(rng, h, w, frac=0.05):
    d = rng.random((h, w)) * 40.0 + 2.0
    bad = rng.random((h, w)) < frac
    d[bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    return d


def test_the_two_restatements_agree_bit_for_bit():
    for (w, h), T in (((1, 1), 1), ((1, 7), 3), ((7, 1), 3), ((3, 9), 1), ((13, 6), 3), ((21, 17), 2)):
        rng = np.random.default_rng([w, h, T])
        d = holed_map(rng, h, w, 0.15)
        g = palette_guide(rng, h, w)
        conf = rng.random((h, w)) * (rng.random((h, w)) > 0.3)
        for guide in (None, g):
            for c in (None, conf):
                for max_dis in (0, 30):
                    a = sr.smooth_py(d, c, guide, 100.0, 20.0, T, max_dis)
                    b = sr.smooth(d, c, guide, 100.0, 20.0, T, max_dis)
                    assert np.array_equal(_bits(a), _bits(b)), (w, h, T, guide is not None, c is not None, max_dis)


def _dense_deviation(n, seed, lam=100.0, sigma=20.0, h=6):
    rng = np.random.default_rng([n, seed])
    D = rng.random((h, n)) * 50.0
    wh, _ = sr.weights(palette_guide(rng, h, n), sigma, (h, n))
    _, N, M = sr.init(D, rng.random((h, n)))
    un, um = sr.horizontal_pass(N, M, wh, lam)
    worst = 0.0
    for y in range(h):
        A = np.zeros((n, n))
        for i in range(n):
            a = -(lam * wh[y, i - 1]) if i > 0 else 0.0
            cc = -(lam * wh[y, i]) if i < n - 1 else 0.0
            A[i, i] = (1.0 - a) - cc
            if i > 0:
                A[i, i - 1] = a
            if i < n - 1:
                A[i, i + 1] = cc
        worst = max(worst, np.abs(np.linalg.solve(A, N[y]) - un[y]).max(), np.abs(np.linalg.solve(A, M[y]) - um[y]).max())
    return worst


def test_one_horizontal_pass_solves_the_dense_system():
    worst = max(_dense_deviation(n, seed) for n in (9, 33) for seed in range(8))
    print(f"largest deviation from numpy.linalg.solve: {worst:.3g}")
    assert worst <= DENSE_BOUND


def test_a_constant_map_stays_constant():
    worst = 0.0
    for seed in range(4):
        rng = np.random.default_rng(seed)
        out = sr.smooth(np.full((33, 17), 37.25), None, rng.integers(0, 256, (33, 17, 3)).astype(np.uint8), 100.0, 20.0, 3)
        worst = max(worst, float(np.abs(out - 37.25).max()))
    print(f"largest deviation from the constant: {worst:.3g}")
    assert worst <= CONST_BOUND


@pytest.mark.parametrize("T", [1, 3])
def test_lambda_zero_with_full_confidence_is_the_identity(T):
    rng = np.random.default_rng(T)
    d = rng.random((12, 19)) * 60.0 - 5.0
    g = palette_guide(rng, 12, 19)
    for guide in (None, g):
        assert np.array_equal(_bits(sr.smooth(d, None, guide, 0.0, 20.0, T)), _bits(d))
        assert np.array_equal(_bits(sr.smooth_py(d, None, guide, 0.0, 20.0, T)), _bits(d))


def test_zero_confidence_everywhere_is_the_identity():
    rng = np.random.default_rng(2)
    d = holed_map(rng, 11, 14, 0.2)
    d[3, 4] = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    out = sr.smooth(d, np.zeros_like(d), palette_guide(rng, 11, 14), 100.0, 20.0, 3, 30)
    assert np.array_equal(_bits(out), _bits(d))


def test_quotients_stay_within_the_confident_nodes_range():
    for (w, h) in ((7, 5), (33, 20), (130, 67)):
        rng = np.random.default_rng([w, h])
        d = holed_map(rng, h, w, 0.15)
        conf = rng.random((h, w)) * (rng.random((h, w)) > 0.33)
        out, q = sr.smooth(d, conf, palette_guide(rng, h, w), 100.0, 20.0, 3, with_quotient_mask=True)
        sure = np.isfinite(d) & (conf > 0)
        assert sure.any() and q.any() and (~np.isfinite(d)).any()
        lo, hi = d[sure].min(), d[sure].max()
        assert (out[q] >= lo - 1e-9).all() and (out[q] <= hi + 1e-9).all(), (w, h)
        assert np.array_equal(_bits(out[~q]), _bits(d[~q]))


def test_a_guide_edge_stops_the_diffusion_across_a_band_without_confidence():
    h, w = 12, 20
    d = np.where(np.arange(w)[None, :] < w // 2, 10.0, 50.0) * np.ones((h, 1))
    g = np.zeros((h, w, 3), np.uint8)
    g[:, w // 2:] = 255
    conf = np.ones((h, w))
    conf[:, w // 2 - 3:w // 2 + 3] = 0.0
    noisy = d.copy()
    noisy[:, w // 2 - 3:w // 2 + 3] = 99.0  # what the band holds does not matter: its confidence is 0
    out = sr.smooth(noisy, conf, g, 100.0, 20.0, 3)
    assert np.abs(out - d).max() <= 1e-6
    assert np.abs(sr.smooth(noisy, conf, None, 100.0, 20.0, 3) - d).max() > 1.0  # without the guide the two sides mix


def test_non_nodes_are_filled_when_a_confident_pixel_is_in_reach():
    rng = np.random.default_rng(5)
    d = rng.random((9, 13)) * 20.0 + 5.0
    d[4, :] = np.nan
    d[:, 6] = np.inf
    out = sr.smooth(d, None, None, 100.0, 20.0, 3)
    assert np.isfinite(out).all() and out.min() >= 5.0 - 1e-9 and out.max() <= 25.0 + 1e-9
    alone = np.full((3, 4), np.nan)
    assert np.array_equal(_bits(sr.smooth(alone, None, None)), _bits(alone))  # no confident pixel anywhere: nothing in reach


def test_lines_of_length_one_and_the_clamp():
    one = np.array([[7.5]])
    assert sr.smooth(one, None, None)[0, 0] == 7.5 and sr.smooth_py(one, np.array([[0.5]]), None)[0, 0] == 7.5
    un, um = sr.solve_line_py([3.0], [1.0], [], 100.0)
    assert (un, um) == ([3.0], [1.0])
    col = np.array([[1.0], [2.0], [4.0]])
    row = np.ascontiguousarray(col.T)
    assert np.array_equal(_bits(sr.smooth(col, None, None, 100.0, 20.0, 1).T), _bits(sr.smooth(row, None, None, 100.0, 20.0, 1)))
    d = np.array([[-5.0, -4.0, 90.0, 95.0]])
    g = np.zeros((1, 4, 3), np.uint8)
    g[0, 2:] = 255
    free, clamped = sr.smooth(d, None, g), sr.smooth(d, None, g, max_dis=64)
    assert free[0, 0] < 0 and free[0, 3] > 64
    assert np.array_equal(clamped, np.array([[0.0, 0.0, 64.0, 64.0]]))
    holes = np.array([[np.nan, -3.0]])
    out = sr.smooth(holes, np.array([[1.0, 0.0]]), None, max_dis=64)
    assert np.array_equal(_bits(out), _bits(holes))  # D's own bits are not clamped


def test_the_schedule():
    assert sr.lambdas(100.0, 1) == [((1.5 * 1.0) / 3.0) * 100.0]
    lam = sr.lambdas(100.0, 3)
    assert lam == [((1.5 * 16.0) / 63.0) * 100.0, ((1.5 * 4.0) / 63.0) * 100.0, ((1.5 * 1.0) / 63.0) * 100.0]
    assert sr.lut(20.0)[0] == 1.0 and len(sr.lut(20.0)) == 766


# ---- the bindings, where no device is needed ---------------------------------------------------------------------------------------
def test_argument_errors_are_reported_before_a_device_is_opened():
    L = capi.load_library()
    p = capi.SmoothParams()
    assert L.cspm_smooth_default_params(C.byref(p)) == 0 and L.cspm_smooth_default_params(None) == -1
    assert (p.lambda_, p.sigma_color, p.iterations, p.fill_conf) == (100.0, 20.0, 3, 0.25)
    d, o = np.ones((4, 5)), np.zeros((4, 5))
    g = np.zeros((4, 5, 3), np.uint8)
    f = L.cspm_smooth_disparity_host
    dev = 1 << 20  # no such device: an argument error must come first (-1), a valid call fails later with another code

    def call(disp=d, conf=None, out=o, w=5, h=4, max_dis=0, **kw):
        q = capi.smooth_params(**kw)
        return f(dev, capi._dp(disp) if disp is not None else None, capi._dp(conf) if conf is not None else None, capi._u8(g), w, h, C.byref(q),
                 max_dis, capi._dp(out) if out is not None else None)

    assert call() not in (0, -1)
    for bad in (dict(lam=-1.0), dict(lam=np.nan), dict(lam=np.inf), dict(sigma_color=0.0), dict(sigma_color=-2.0), dict(sigma_color=np.inf),
                dict(sigma_color=np.nan), dict(iterations=0), dict(iterations=9), dict(iterations=-1)):
        assert call(**bad) == -1, bad
    assert call(fill_conf=7.0) not in (0, -1)  # ignored by the host entry
    for conf in (np.full((4, 5), 1.5), np.full((4, 5), -0.1), np.full((4, 5), np.nan)):
        assert call(conf=conf) == -1
    assert b"confidence" in L.cspm_last_error(None)
    assert call(disp=None) == -1 and call(out=None) == -1 and call(out=d) == -1 and call(w=0) == -1 and call(h=0) == -1 and call(max_dis=-1) == -1
    assert L.cspm_set_pp_smooth(None, C.byref(p)) == -1 and L.cspm_get_pp_smooth(None, C.byref(p), None) == -1
    with pytest.raises(TypeError):
        capi.smooth_params(radius=3)


def test_header_and_bindings_agree():
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read()
    m = re.search(r"typedef struct cspm_smooth_params \{(.*?)\} cspm_smooth_params;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(double|int)\s+(\w+);", body)]
    assert fields == [("double", "lambda"), ("double", "sigma_color"), ("int", "iterations"), ("double", "fill_conf")]
    ctypes_of = {"double": C.c_double, "int": C.c_int}
    assert [(ctypes_of[t], n.rstrip("_")) for t, n in fields] == [(t, n.rstrip("_")) for n, t in capi.SmoothParams._fields_]
    for name in ("cspm_smooth_default_params", "cspm_smooth_disparity_host", "cspm_set_pp_smooth", "cspm_get_pp_smooth"):
        assert name in capi.SYMBOLS and re.search(r"\bint " + name + r"\(", hdr), name
    L = capi.load_library()
    assert len(L.cspm_smooth_disparity_host.argtypes) == 9 and len(L.cspm_get_pp_smooth.argtypes) == 3
    assert sr.DEFAULTS == dict(lam=100.0, sigma_color=20.0, iterations=3, fill_conf=0.25)
