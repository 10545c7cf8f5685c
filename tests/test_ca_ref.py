"""-m "not gpu": the numpy restatement of cost aggregation (tests/ca_ref.py) against direct definitions, and the command line's
--ca_name checks, which happen before any device is opened."""
import os
import subprocess

import numpy as np
import pytest

import ca_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _direct_box(im, r):
    H, W = im.shape
    out = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            out[y, x] = im[max(0, y - r):min(H, y + r + 1), max(0, x - r):min(W, x + r + 1)].sum()
    return out


@pytest.mark.parametrize("r", [3, 9])
@pytest.mark.parametrize("extra", [(0, 0), (0, 5), (4, 0), (13, 22)])
def test_box_filter_is_the_clipped_window_sum(r, extra):
    H, W = 2 * r + 1 + extra[0], 2 * r + 1 + extra[1]
    im = np.random.default_rng(r * 100 + H + W).random((H, W))
    np.testing.assert_allclose(ca_ref.box_filter(im, r), _direct_box(im, r), rtol=1e-9, atol=0)


def test_cumsum_is_serial():
    a = np.array([[1e16, 1.0], [1.0, -1e16], [-1e16, 1.0]])
    np.testing.assert_array_equal(ca_ref.cumsum(a, 1)[-1], [(1e16 + 1.0) + -1e16, (1.0 + -1e16) + 1.0])
    np.testing.assert_array_equal(ca_ref.cumsum(a, 2)[:, -1], [1e16 + 1.0, 1.0 + -1e16, -1e16 + 1.0])


@pytest.mark.parametrize("shape", [(19, 19), (24, 31)])
def test_guided_and_bilateral_filters_keep_a_constant(shape):
    g = np.random.default_rng(3).random(shape + (3,))
    p = np.full(shape, 2.5)
    np.testing.assert_allclose(ca_ref.guided_filter(g, p), p, rtol=1e-12)
    np.testing.assert_allclose(ca_ref.bilateral_filter(g, p), p, rtol=1e-12)


def test_aggre_cv_leaves_slice_0():
    rng = np.random.default_rng(4)
    g, v = rng.random((20, 20, 3)), rng.random((4, 20, 20))
    for m in ("BOX", "GF", "BF"):
        out = ca_ref.aggre_cv(m, g, v)
        np.testing.assert_array_equal(out[0], v[0])
        assert not np.array_equal(out[1], v[1])


def test_wta_takes_the_first_minimum():
    costs = np.array([[[3.0, 1.0]], [[2.0, 1.0]], [[2.0, 0.5]], [[5.0, 0.5]]])  # d = 1 .. 4, two pixels
    d, c = ca_ref.wta(costs)
    np.testing.assert_array_equal(d, [[2, 3]])
    np.testing.assert_array_equal(c, [[2.0, 0.5]])


def test_impossible_disparities_cost_the_level_max():
    """a coarse level contributes M where d halved is below 1 or at / beyond its range (pre_cs_pc.cc:168-170)"""
    agg0 = np.stack([np.full((2, 2), float(k)) for k in range(5)])  # D_0 = 4
    agg1 = np.stack([np.full((1, 1), 10.0 * k) for k in range(3)])  # D_1 = 2
    m = [ca_ref.level_max(agg0), ca_ref.level_max(agg1)]
    costs = ca_ref.local_costs([agg0, agg1], m, [1.0, 0.5], True, 4, 2, 2)
    # d = 1: q1 = 0.5 -> f = 0 -> M1 = 20;  d = 2, 3: f = 1 -> interpolation;  level 0 always interpolates (f = d)
    np.testing.assert_array_equal(costs[:, 0, 0], [1.0 + 0.5 * 20.0, 2.0 + 0.5 * 10.0, 3.0 + 0.5 * (0.5 * 10.0 + 0.5 * 20.0)])
    assert ca_ref.level_max(np.full((1, 2, 2), -5.0)) == -1.0  # max_cost_ starts at -1.0


def _cli():
    exe = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crossscalepatchmatch_amd", "host")], stdout=subprocess.DEVNULL)
    return exe


@pytest.mark.parametrize("flags,needle", [(["--ca_name=NL"], "--ca_name must be BOX, GF or BF (got NL)"),
                                          (["--ca_name=GF", "--pc_name=IMG"], "--ca_name aggregates cost volumes; --pc_name=IMG")])
def test_cli_rejects_bad_ca_flags_before_the_device(flags, needle, tmp_path):
    p = subprocess.run([_cli(), f"--l_img_file={tmp_path}/none.png", f"--r_img_file={tmp_path}/none.png", "--max_dis=16", "--dis_scale=4",
                        "--cc_name=GRD"] + flags, capture_output=True, timeout=120)
    assert p.returncode != 0
    out = (p.stdout + p.stderr).decode()
    assert needle in out, out
    assert "no HIP device" not in out and "Load Image" not in out, out
