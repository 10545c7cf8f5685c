"""-m "not gpu": the registration's case table (tests/register_cases.py) is not vacuous and the restatement (tests/register_ref.py) does
what DESIGN.md section 26 says: every exit of the pair loop and every status occur, the reduction tree is a sum, the loop converges on
the corner scene and refuses the single plane."""
import numpy as np
import pytest

import register_cases as rc
import register_ref as rr


def test_every_exit_and_every_status_occur():
    exits = dict.fromkeys(rr.EXITS, 0)
    status = set()
    for case in rc.CASES + rc.EXTRA:
        ref = case.reference()
        for k, v in ref["exits"].items():
            exits[k] += v
        status |= set(ref["iters"]["status"].tolist())
    assert all(v > 0 for v in exits.values()), exits
    assert status == {0, 1, 2, 3}


def test_every_shape_of_the_table_associates_something_somewhere():
    """the blocks the shapes were chosen for exist: one block exactly, a second block with one sample, 258 partials"""
    blocks = {(w, h, s): -(-(-(-w // s) * -(-h // s)) // rr.BLOCK) for w, h, s in rc.SHAPES}
    assert blocks[(64, 4, 1)] == 1 and blocks[(257, 1, 1)] == 2 and blocks[(300, 220, 1)] == 258 and blocks[(130, 67, 3)] == 4
    assert any(c.reference()["iters"]["pairs"][0] > 0 for c in rc.CASES if (c.w, c.h) == (300, 220))


def test_the_tree_is_a_sum():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 66000):
        acc = rng.uniform(-1.0, 2.0, (n, rr.SUMS))
        got, want = rr.reduce_samples(acc), acc.sum(0)
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(acc).sum(0))
    case = rc.BY_NAME["300x220_s1_T3_c0.0"]
    v = case.views()
    acc = rr.sample_sums(v, case.w, case.h, rc.SRC, case.targets, v[rc.SRC]["R"], v[rc.SRC]["t"], 1, 0.5, 0.05, 0.0)
    got, want = rr.reduce_samples(acc), acc.sum(0)
    assert got[28] == want[28] == case.reference()["iters"]["pairs"][0]
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(acc).sum(0))


def test_cayley_is_a_rotation():
    for om in ([0.0, 0.0, 0.0], [0.03, -0.02, 0.01], [1.0, -2.0, 0.5]):
        E = rr.cayley(np.array(om))
        assert np.abs(E @ E.T - np.eye(3)).max() < 1e-15 and np.linalg.det(E) > 0.0
    assert np.array_equal(rr.cayley(np.zeros(3)), np.eye(3))
    E = rr.cayley(np.array([0.0, 0.0, 0.02]))  # a small rotation about z by 0.02 rad, to second order
    assert abs(np.arctan2(E[1, 0], E[0, 0]) - 0.02) < 1e-6


@pytest.mark.parametrize("case", rc.CONVERGE, ids=repr)
def test_convergence_condition(case):
    """with the default parameters both errors end at no more than 1/20 of their start"""
    assert case.params == rr.DEFAULTS or case.params == dict(rr.DEFAULTS, stride=2)
    v = case.views()
    rot0, tr0 = rc.pose_error(v[rc.SRC]["R"], v[rc.SRC]["t"])
    assert abs(rot0 - 2.07) < 0.01 and abs(tr0 - 0.0707) < 0.001
    ref = case.reference()
    rot1, tr1 = rc.pose_error(ref["R"], ref["t"])
    assert np.all(ref["iters"]["status"] == 0) and len(ref["iters"]) == 8
    assert rot1 <= rot0 / 20.0 and tr1 <= tr0 / 20.0, (rot0, rot1, tr0, tr1)
    assert ref["iters"]["cost"][-1] < ref["iters"]["cost"][0]
    assert np.abs(ref["R"] @ ref["R"].T - np.eye(3)).max() < 1e-12  # eight Cayley steps later still a rotation


def test_single_plane_is_refused():
    case = rc.SINGLE_PLANE
    ref = case.reference()
    v = case.views()
    assert ref["iters"]["status"][0] == 2 and ref["iters"]["pairs"][0] >= case.params["min_pairs"]
    assert np.all(ref["iters"]["status"] == 2) and np.all(ref["iters"]["rot2"] == 0.0) and np.all(ref["iters"]["trans2"] == 0.0)
    assert np.array_equal(ref["R"], v[rc.SRC]["R"]) and np.array_equal(ref["t"], v[rc.SRC]["t"])


def test_too_few_pairs_and_a_non_finite_step_leave_the_pose():
    for case, status in ((rc.BY_NAME["257x1_s1_T1_c0.0"], 1), (rc.NONFINITE, 3)):
        ref, v = case.reference(), case.views()
        assert np.all(ref["iters"]["status"] == status)
        assert np.array_equal(ref["R"], v[rc.SRC]["R"]) and np.array_equal(ref["t"], v[rc.SRC]["t"])
    assert rc.NONFINITE.reference()["iters"]["pairs"][0] > 0


def test_argument_rules():
    v = rc.CONVERGE[0].views()
    assert rr.check_args(v, 1, 0b01)
    for bad in (dict(src=2), dict(targets=0), dict(targets=0b10), dict(targets=0b101), dict(iters=0), dict(iters=65), dict(stride=0),
                dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(huber=-0.1), dict(min_cos=1.5), dict(pivot_rel=1.0), dict(min_pairs=-1)):
        args = dict(src=1, targets=0b01)
        args.update(bad)
        assert not rr.check_args(v, **args), bad
