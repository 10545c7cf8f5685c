"""-m "not gpu": the CPU restatement of the median filter (tests/median_ref.py) against the recorded outputs of
the reference's own filter (tests/golden/refmedian_*.npz), against the reference compiled live where its checkout and gcc are
present, against scipy, and on hand cases of M8 and M64."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest

import median_ref as mr

CASE_IDS = [mr.case_name(*c) for c in mr.all_cases()]


def _record(case):
    z = np.load(mr.golden_path(mr.case_name(*case)))
    w, h, r, cn, memsize, _ = case
    assert (int(z["r"]), int(z["cn"]), int(z["memsize"])) == (r, cn, memsize)
    assert z["src"].shape == ((h, w) if cn == 1 else (h, w, cn)) and np.array_equal(z["src"], mr.case_input(*case))
    return z["src"], z["out"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", mr.all_cases(), ids=CASE_IDS)
def test_restatement_equals_the_recorded_reference_output(case):
    src, out = _record(case)
    got = mr.median_u8(src, case[2])
    assert got.dtype == np.uint8 and np.array_equal(got, out), f"{int((got != out).sum())} of {out.size} bytes differ"


def test_the_records_are_small():
    total = sum(os.path.getsize(mr.golden_path(n)) for n in CASE_IDS)
    assert total < 300 * 1000, total


@pytest.fixture(scope="module")
def live_filter():
    """the reference's filter compiled here (tests/golden/make_refmedian.py), or a skip where its checkout or gcc is missing"""
    spec = importlib.util.spec_from_file_location("make_refmedian", os.path.join(mr.GOLDEN, "make_refmedian.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with tempfile.TemporaryDirectory() as tmp:
        fn = gen.load_reference_filter(tmp)
        if fn is None:
            pytest.skip("no reference checkout or no gcc: the recorded outputs stand alone")
        yield lambda img, r, cn, memsize: gen.run_reference(fn, img, r, cn, memsize)


def test_live_reference_reproduces_every_record(live_filter):
    for case in mr.all_cases():
        src, out = _record(case)
        got = live_filter(src, case[2], case[3], case[4])
        assert np.array_equal(got, out), mr.case_name(*case)


def test_scipy_agrees_with_m8():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for (w, h), r in (((1, 1), 7), ((3, 9), 2), ((70, 33), 1), ((70, 33), 2), ((41, 29), 3), ((37, 20), 7)):
        img = (3 * rng.integers(0, 6, (h, w)) + 100).astype(np.uint8)
        want = ndimage.median_filter(img, size=2 * r + 1, mode="nearest")
        assert np.array_equal(mr.median_u8(img, r), want), (w, h, r)
    img = rng.integers(0, 256, (20, 31, 3)).astype(np.uint8)
    want = ndimage.median_filter(img, size=(5, 5, 1), mode="nearest")
    assert np.array_equal(mr.median_u8(img, 2), want)


# ---- M8 by hand --------------------------------------------------------------------------------------------------------------------
def test_m8_constant_impulse_and_step_edge():
    for r in (1, 2, 7):
        assert (mr.median_u8(np.full((9, 11), 37, np.uint8), r) == 37).all()
    img = np.full((9, 11), 40, np.uint8)
    img[4, 5] = 255
    img[0, 0] = 0  # a corner impulse: the replicated border gives it (r+1)^2 of the (2r+1)^2 taps, below the median rank
    for r in (1, 2, 3):
        assert (mr.median_u8(img, r) == 40).all()
    step = np.zeros((9, 12), np.uint8)
    step[:, 6:] = 200
    for r in (1, 2, 3):
        assert np.array_equal(mr.median_u8(step, r), step)
        assert np.array_equal(mr.median_u8(np.ascontiguousarray(step.T), r), step.T)


def test_m8_window_larger_than_the_image():
    one = np.array([[91]], np.uint8)
    assert np.array_equal(mr.median_u8(one, 7), one)
    img = np.arange(27, dtype=np.uint8).reshape(9, 3) * 7   # 3 x 9 (w x h) with r = 2: every window leaves the image on both sides
    got = mr.median_u8(img, 2)
    for y in range(9):
        for x in range(3):
            taps = sorted(int(img[min(max(y + j, 0), 8), min(max(x + i, 0), 2)]) for j in range(-2, 3) for i in range(-2, 3))
            assert got[y, x] == taps[12]
    # by hand, corner (0, 0): rows 0 0 0 1 2 x columns 0 0 0 1 2 of 3y + x -> 0 x9, 1 x3, 2 x3, ...: rank 12 is a 2
    assert got[0, 0] == 2 * 7 and got[8, 2] == 24 * 7


def test_m8_channels_are_independent():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (12, 17, 4)).astype(np.uint8)
    got = mr.median_u8(img, 2)
    for c in range(4):
        assert np.array_equal(got[..., c], mr.median_u8(np.ascontiguousarray(img[..., c]), 2))


# ---- M64 by hand -------------------------------------------------------------------------------------------------------------------
def test_m64_nan_taps_do_not_vote_and_an_even_count_gives_the_lower_median():
    d = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, np.nan]])
    got = mr.median_f64(d, 1)
    assert got[1, 1] == 4.0                    # 8 votes 1 .. 8: rank 7 // 2 = 3 -> 4.0, not 4.5 and not 5.0
    # corner (0, 0): clamped taps 1 1 2 1 1 2 4 4 5, nine votes, rank 4 -> 2
    assert got[0, 0] == 2.0
    # (1, 2): taps 2 3 3 5 6 6 8 NaN NaN: seven votes, rank 3 -> 5
    assert got[1, 2] == 5.0
    assert np.isnan(got[2, 2]) and not np.isnan(got[:2]).any() and not np.isnan(got[2, :2]).any()


def test_m64_nan_centre_keeps_its_bits():
    d = np.full((5, 5), 2.5)
    payload = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF], np.uint64).view(np.float64)
    d[1, 1], d[2, 3], d[4, 4] = payload
    got = mr.median_f64(d, 2)
    assert np.array_equal(_bits(got)[[1, 2, 4], [1, 3, 4]], payload.view(np.uint64))
    mask = np.isnan(d)
    assert (got[~mask] == 2.5).all()
    alone = np.full((3, 3), np.nan)
    assert np.array_equal(_bits(mr.median_f64(alone, 1)), _bits(alone))  # no vote anywhere: every centre is a NaN and stays


def test_m64_signed_zeros_and_infinities():
    d = np.array([[-0.0, 0.0, -0.0]])
    got = mr.median_f64(d, 1)  # 1 x 3: each window is three rows of the same three clamped taps
    # x = 0: taps (-0 -0 +0) x 3 -> rank 4 of [-0 x6, +0 x3] = -0; x = 1: (-0 +0 -0) x 3 -> -0; x = 2: (+0 -0 -0) x 3 -> -0
    assert np.array_equal(_bits(got), _bits(np.array([[-0.0, -0.0, -0.0]])))
    d = np.array([[0.0, -0.0, 0.0]])
    assert np.array_equal(_bits(mr.median_f64(d, 1)), _bits(np.array([[0.0, 0.0, 0.0]])))
    inf = np.inf
    d = np.array([[-inf, -1e308, inf, inf, 1e308]])
    got = mr.median_f64(d, 1)
    assert np.array_equal(got, np.array([[-inf, -1e308, inf, inf, 1e308]]))
    d = np.array([[-inf, inf, -inf, 3.0, -inf]])
    assert np.array_equal(mr.median_f64(d, 1), np.array([[-inf, -inf, 3.0, -inf, -inf]]))
    keys = mr.f64_key(np.array([-inf, -1.0, -0.0, 0.0, 5e-324, 1.0, inf]))
    assert (np.diff(keys.astype(object)) > 0).all()
    assert np.array_equal(_bits(mr.f64_unkey(keys)), _bits(np.array([-inf, -1.0, -0.0, 0.0, 5e-324, 1.0, inf])))


def test_m64_of_integer_data_equals_m8():
    rng = np.random.default_rng(11)
    for (w, h), r in (((1, 1), 3), ((3, 9), 2), ((33, 21), 1), ((33, 21), 2), ((33, 21), 7)):
        img = (3 * rng.integers(0, 6, (h, w)) + 100).astype(np.uint8)
        assert np.array_equal(mr.median_f64(img.astype(np.float64), r), mr.median_u8(img, r).astype(np.float64))
