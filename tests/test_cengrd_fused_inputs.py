"""No GPU: conditions on the inputs of tests/test_gpu_cengrd_fused.py, so that a green GPU test cannot be green for lack of coverage.
The wide pair exercises both branches of the CENGRD min on both sides of the row engine's strip limit (the condition
tests/test_cengrd_ref.py puts on every other pair), the two max_dis values really fall on the two sides of that limit, and the
hand-made planes of the cspm_plane_cost_batch test reach the pad columns and leave the disparity range in both views."""
import numpy as np
import pytest

import cengrd_fused_cases as cases
import cengrd_ref


@pytest.mark.parametrize("max_dis", [cases.WIDE_STAGED_D, cases.WIDE_GLOBAL_D])
def test_wide_pair_exercises_both_branches_of_the_min(max_dis):
    l, r = cases.wide_images()
    for v, s, below, at_or_above in cengrd_ref.branch_fractions(l, r, max_dis, 0):
        assert below >= 0.01 and at_or_above >= 0.01, (max_dis, v, s, below, at_or_above)


def test_wide_pair_is_on_both_sides_of_the_strip_limit():
    half = cases.WIDE_WND // 2
    for view in (0, 1):
        assert cases.full_wave_strip(cases.WIDE_STAGED_D, half, view) <= cases.strip_capacity(cases.WIDE_STAGED_D, half) < cases.K_STRIP_SLOTS
        assert cases.strip_capacity(cases.WIDE_STAGED_D, half) > 5 * 64  # the sixth staging register of a lane is in use
        assert cases.strip_capacity(cases.WIDE_GLOBAL_D, half) == cases.K_STRIP_SLOTS < cases.full_wave_strip(cases.WIDE_GLOBAL_D, half, view)
    assert cases.WIDE_W >= 2 * 64  # full waves exist


@pytest.mark.parametrize("name", ["small", "odd"])
def test_hand_made_planes_hit_what_they_claim(name):
    p = cengrd_ref.PAIRS[name]
    xy, norm, param = cases.hand_planes(p.w, p.h, p.D)
    assert np.all(np.isfinite(param))
    n0 = cases.tap_counts(xy, param, p.w, p.h, p.D, 0)
    n1 = cases.tap_counts(xy, param, p.w, p.h, p.D, 1)
    assert n0["pad_left"] > 0 and n1["pad_right"] > 0  # the other view's pad cells: H = 80, the border branch of G
    for n in (n0, n1):
        assert n["out_of_range"] > 0  # the max_cost branch
        assert n["own_left"] > 0 and n["own_right"] > 0  # the window itself beyond either border: masked taps
