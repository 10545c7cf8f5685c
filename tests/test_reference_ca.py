"""The reference's OWN cost-aggregation filters next to tests/ca_ref.py.

ca_filter/GuidedFilter.cpp (CumSum, BoxFilter, GuidedFilter), BilateralFilter.cpp, BoxCA.cpp, GFCA.cpp and BFCA.cpp are compiled
UNMODIFIED against the test-only stand-in for <opencv2/opencv.hpp> (tests/helpers/refcheck/: Mat::ones, split, multiply and the
elementwise Mat operators, each one IEEE f64 operation per element) and driven by tests/helpers/cacheck_main.cc through CAMethod*.
THIS PINS NOTHING -- a build against a stand-in is not a reference build (DESIGN.md sections 2 and 10; in particular cv::divide of
OpenCV 2.4 may not be the plain quotient) -- but it is the one available check that ca_ref.py, the definition every GPU aggregation
test uses, TRANSCRIBES the reference's filters without a slip: band limits, CumSum's starting value, the cofactors of FAST_INV,
channel order, eps as a promoted float, sig_sp = wndSZ / 2.0f, the 0.333333333 factor, the wrap-around border.

What that binary computed on every case below is recorded under tests/golden/refca_<case>.npz (inputs and outputs,
tests/golden/make_refca.py).  Three legs, as in tests/test_reference_loops.py: the record is of exactly the inputs built here; where
build() could compile the binary (oracle/build_ref.py -> oracle/_ref/cacheck) it is run and must reproduce the record bit for bit;
ca_ref equals the record -- bit for bit for CumSum, BoxFilter, BOX and GF (only + - * /, no contraction on either side), and within
rtol 1e-12 for BF: the exponent is built from identical IEEE operations, so only exp differs (about an ulp between glibc and
numpy), every term is positive, the centre weight is exactly 1, and accumulating 1225 terms costs at most 1225 x 1.1e-16 in the
numerator and in the denominator, about 3e-13 together.  The largest BF difference seen is printed (run with -s) and kept in
DESIGN.md section 10.  tests/test_gpu_ca_reference.py holds the HIP kernels to the same records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ca_ref
from crossscalepatchmatch_amd import synth
from oracle import build_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
METHOD_CODE = {"BOX": 0, "GF": 1, "BF": 2, "CUMSUM1": 11, "CUMSUM2": 12}  # tests/helpers/cacheck_main.cc; BoxFilter(r): 100 + r

# name, operation, (w, h, n), what the slabs hold
PRIMITIVES = [
    ("cumsum1", "CUMSUM1", (9, 11, 2), "signed+big"),
    ("cumsum2", "CUMSUM2", (9, 11, 2), "signed+big"),
    ("boxfilter_r3_7x7", "BOXFILTER3", (7, 7, 2), "signed+big"),      # 2r+1
    ("boxfilter_r3_8x8", "BOXFILTER3", (8, 8, 2), "signed+big"),      # 2r+2: the middle band is one row / column
    ("boxfilter_r3_23x12", "BOXFILTER3", (23, 12, 2), "signed+big"),
    ("boxfilter_r9_19x19", "BOXFILTER9", (19, 19, 2), "signed+big"),
    ("boxfilter_r9_20x20", "BOXFILTER9", (20, 20, 2), "signed+big"),
    ("boxfilter_r9_31x24", "BOXFILTER9", (31, 24, 2), "signed+big"),
]
# name, method, (w, h, n), guide, slabs.  n counts slice 0, which aggreCV leaves alone: n = 1 filters nothing
AGGRE = [
    ("box_7x7", "BOX", (7, 7, 3), "none", "signed"),
    ("box_7x30", "BOX", (7, 30, 2), "none", "signed"),
    ("box_30x7", "BOX", (30, 7, 2), "none", "signed"),
    ("box_45x33", "BOX", (45, 33, 3), "none", "signed"),
    ("box_n1", "BOX", (9, 8, 1), "none", "signed"),
    ("gf_19x19", "GF", (19, 19, 3), "random", "signed"),
    ("gf_19x45", "GF", (19, 45, 2), "random", "signed"),
    ("gf_45x19", "GF", (45, 19, 2), "random", "signed"),
    ("gf_45x33", "GF", (45, 33, 3), "random", "signed"),
    ("gf_n1", "GF", (19, 19, 1), "random", "signed"),
    # DET near eps^3 = 1e-12: the variances are rounding noise or exactly 0 over large areas, so every rounding shows
    ("gf_const_guide", "GF", (24, 21, 2), "const", "signed"),
    ("gf_black_guide", "GF", (21, 23, 2), "black", "signed"),
    ("gf_blocks_guide", "GF", (45, 33, 3), "blocks", "signed"),
    ("gf_twin_channels", "GF", (30, 22, 2), "twin", "signed"),
    ("bf_17x20", "BF", (17, 20, 3), "random", "positive"),  # 35 = 2 * 17 + 1: each window wraps over the image twice along x
    ("bf_20x17", "BF", (20, 17, 2), "random", "positive"),  # ... and along y
    ("bf_45x33", "BF", (45, 33, 2), "random", "positive"),
    ("bf_dup_colours", "BF", (24, 19, 3), "dup", "positive"),
    ("bf_n1", "BF", (17, 17, 1), "random", "positive"),
]
CASES = [c + ("none",) for c in PRIMITIVES] + [(name, method, dims, slabs, guide) for name, method, dims, guide, slabs in AGGRE]
_SEED = {c[0]: 9000 + i for i, c in enumerate(CASES)}


def golden_path(name):
    return os.path.join(GOLDEN, f"refca_{name}.npz")


def method_code(op):
    return 100 + int(op[len("BOXFILTER"):]) if op.startswith("BOXFILTER") else METHOD_CODE[op]


def case_inputs(name, dims, slabs, guide="none"):
    """(guide (h, w, 3), stack (n, h, w)) of one case: what its record was made from"""
    w, h, n = dims
    rng = np.random.default_rng(_SEED[name])
    if guide == "none":
        g = np.zeros((h, w, 3))
    elif guide == "random":
        g = rng.random((h, w, 3))
    elif guide == "const":
        g = np.broadcast_to(np.array([0.3, 0.55, 0.8]), (h, w, 3)).copy()
    elif guide in ("black", "blocks"):  # an 8-bit image times (double)(1.0f/255.0f), large flat areas
        g = ca_ref.guide_from_bgr(synth.make_adversarial(guide, w, h, 8, seed=3)[0])
    elif guide == "twin":
        g = rng.random((h, w, 3))
        g[:, :, 1] = g[:, :, 0]
    elif guide == "dup":  # four levels per channel: many pixels of exactly the same colour, clrDis == 0 away from the centre
        g = ca_ref.guide_from_bgr((rng.integers(0, 4, (h, w, 3)) * 80).astype(np.uint8))
    else:
        raise ValueError(guide)
    if slabs == "positive":  # strictly positive, so a relative bound means something
        vol = rng.uniform(0.5, 10.0, (n, h, w))
    elif slabs == "signed":
        vol = rng.normal(0.0, 5.0, (n, h, w))
    elif slabs == "signed+big":  # the last slab: magnitudes 1e16 and 1 of mixed sign, so the order of summation shows
        vol = rng.normal(0.0, 5.0, (n, h, w))
        vol[-1] = rng.choice([1e16, -1e16, 1.0, -1.0, 3.0], (h, w))
    else:
        raise ValueError(slabs)
    return np.ascontiguousarray(g), np.ascontiguousarray(vol)


def run_reference(exe, tmp_path, op, guide, vol):
    """oracle/_ref/cacheck on one case: the stack as the reference's code leaves it"""
    n, h, w = vol.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", w, h, n, method_code(op)))
        f.write(np.ascontiguousarray(guide, np.float64).tobytes())
        f.write(np.ascontiguousarray(vol, np.float64).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.DEVNULL, timeout=900)
    return np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(n, h, w)


def ca_ref_output(op, guide, vol):
    if op == "CUMSUM1":
        return np.stack([ca_ref.cumsum(s, 1) for s in vol])
    if op == "CUMSUM2":
        return np.stack([ca_ref.cumsum(s, 2) for s in vol])
    if op.startswith("BOXFILTER"):
        return np.stack([ca_ref.box_filter(s, int(op[len("BOXFILTER"):])) for s in vol])
    return ca_ref.aggre_cv(op, guide, vol)


def load_record(name):
    with np.load(golden_path(name)) as g:
        return g["guide"], g["vol"], g["out"]


def max_rel_diff(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("name,op,dims,slabs,guide", CASES, ids=[c[0] for c in CASES])
def test_reference_filters_equal_ca_ref(tmp_path, name, op, dims, slabs, guide):
    w, h, n = dims
    g, vol = case_inputs(name, dims, slabs, guide)
    rec_g, rec_vol, rec_out = load_record(name)
    # the record is of exactly these inputs
    np.testing.assert_array_equal(rec_g, g, err_msg=f"{name}: recorded guide (tests/golden/make_refca.py)")
    np.testing.assert_array_equal(rec_vol, vol, err_msg=f"{name}: recorded stack (tests/golden/make_refca.py)")
    assert rec_out.shape == (n, h, w) and np.all(np.isfinite(rec_out))
    if op in ("BOX", "GF", "BF"):
        np.testing.assert_array_equal(rec_out[0], vol[0], err_msg=f"{name}: aggreCV leaves slice 0")
        for d in range(1, n):
            assert not np.array_equal(rec_out[d], vol[d]), f"{name}: slice {d} came back unfiltered"
    # the reference's filters themselves, where build() could compile them: they reproduce the record
    failed = build_ref.failure(build_ref.CACHECK)
    if failed is not None:
        pytest.fail("oracle/_ref/cacheck did not build:\n" + failed)
    if os.path.exists(build_ref.CACHECK):
        live = run_reference(build_ref.CACHECK, tmp_path, op, g, vol)
        np.testing.assert_array_equal(live, rec_out, err_msg=f"{name}: the reference binary against its record")
    # tests/ca_ref.py
    got = ca_ref_output(op, g, vol)
    if op == "BF":
        if n > 1:
            print(f"{name}: ca_ref vs record, largest relative difference {max_rel_diff(got[1:], rec_out[1:]):.3e}")
        np.testing.assert_allclose(got, rec_out, rtol=1e-12, atol=0, err_msg=f"{name}: ca_ref.bilateral_filter against the reference's")
    else:
        np.testing.assert_array_equal(got, rec_out, err_msg=f"{name}: tests/ca_ref.py against the reference's own code")
