"""The plane-fit restatement tests/fit_ref.py itself (include/cspm.h "plane fitting"), without a GPU: against an
independent least-squares solve, on exact planes, on the behavioural cases of the specification; and the header and command-line
surface of the feature."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The restatement solves the 3x3 normal equations by cofactors, numpy.linalg.lstsq the sqrt(w)-scaled rows by SVD: the two differ by
# rounding scaled by the conditioning of the window only -- and guide weights exp(-k/10) of random colours span thirty decades, so a
# window that passes the 1e-6 collinearity condition can still be conditioned like 1e6, worst at the smallest radius.  Largest
# |difference| of (a, b, c0) measured once on the maps below (x86-64, numpy 2.x), per radius; the bound is 100 times that.  A
# transcription slip (a swapped cofactor, a sign) is of the order of the solution itself, 1e-1.
LSTSQ_MEASURED = {1: 4.24e-9, 2: 4.91e-10, 5: 4.32e-11}
# Exact planes with dyadic slopes: every e is exact, the sums carry the rounding of the weights' products only (weights are 1.0 here, so
# the sums are exact integers and dyadic fractions) -- measured largest |a - a_true|, |b - b_true|: 0.0 (23x19, r in {1, 2, 5}); bounded
# at 100 ulp of the largest slope all the same, since a division by det need not be exact on other shapes.
PLANE_BOUND = 100 * np.finfo(np.float64).eps * 0.5


def _random_case(seed, w=23, h=19):
    rng = np.random.default_rng(seed)
    D = np.round(rng.uniform(0, 12, (h, w)) * 8) / 8  # quantised to 1/8
    D += 0.25 * np.arange(w)[None, :] - 0.125 * np.arange(h)[:, None]
    V = (rng.uniform(size=(h, w)) > 0.1).astype(np.uint8)
    D[rng.integers(0, h, 6), rng.integers(0, w, 6)] = np.nan
    I = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    I[:, : w // 2] //= 16  # a half with many near-duplicate colours
    return D, V, I


def _lstsq_pixel(D, V, I, x, y, r, tau, guided):
    node = fit_ref.nodes(D, V)
    rows, rhs = [], []
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            qx, qy = x + i, y + j
            if not (0 <= qx < D.shape[1] and 0 <= qy < D.shape[0]) or not node[qy, qx]:
                continue
            e = D[qy, qx] - D[y, x]
            if not abs(e) <= tau:
                continue
            wq = math.exp(-np.abs(I[qy, qx].astype(int) - I[y, x].astype(int)).sum() / 10.0) if guided else 1.0
            s = math.sqrt(wq)
            rows.append([s * i, s * j, s])
            rhs.append(s * e)
    return np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0], len(rows)


@pytest.mark.parametrize("r", [1, 2, 5])
def test_restatement_equals_an_independent_least_squares_solve(r):
    worst = 0.0
    checked = 0
    for seed, guided, tau in ((1, 1, 1.5), (2, 0, math.inf), (3, 1, 3.0)):
        D, V, I = _random_case(seed)
        a, b, c0, n, degenerate, node = fit_ref.solve(D, V, I, radius=r, max_diff=tau, min_support=6, use_guide=guided)
        for y in range(D.shape[0]):
            for x in range(D.shape[1]):
                if not node[y, x] or degenerate[y, x]:
                    continue
                sol, rows = _lstsq_pixel(D, V, I, x, y, r, tau, guided)
                assert rows == n[y, x]
                worst = max(worst, np.abs(sol - (a[y, x], b[y, x], c0[y, x])).max())
                checked += 1
    print(f"radius {r}: largest |restatement - lstsq| = {worst:.3e} over {checked} pixels")
    assert checked > 300
    assert worst <= 100 * LSTSQ_MEASURED[r]


def test_vectorised_restatement_equals_the_per_pixel_specification():
    for seed, params in ((1, dict(radius=2, max_diff=1.5, min_support=6, use_guide=1)), (2, dict(radius=5, max_diff=math.inf, min_support=3, use_guide=0)),
                         (3, dict(radius=1, max_diff=0.0, min_support=3, use_guide=1))):
        D, V, I = _random_case(seed, 13, 11)
        planes, fitted = fit_ref.fit(D, V, I, max_dis=10, **params)
        for y in range(D.shape[0]):
            for x in range(D.shape[1]):
                want, f = fit_ref.fit_pixel(D, V, I, x, y, 10, **params)
                assert f == fitted[y, x]
                np.testing.assert_array_equal(planes[y, x], np.array(want), err_msg=f"seed {seed} pixel {x},{y}")


@pytest.mark.parametrize("r", [1, 2, 5])
def test_exact_planes_are_recovered(r):
    w, h = 23, 19
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    worst = 0.0
    for sa in (0.0, 0.125, -0.125, 0.5, -0.5):
        for sb in (0.0, 0.125, -0.125, 0.5, -0.5):
            D = sa * xs + sb * ys + 20.0
            a, b, c0, n, degenerate, node = fit_ref.solve(D, None, None, radius=r, max_diff=math.inf, min_support=3, use_guide=0)
            assert node.all() and not degenerate.any()  # every border pixel, corners included, has a non-collinear window
            inner = (slice(r, h - r), slice(r, w - r))
            worst = max(worst, np.abs(a[inner] - sa).max(), np.abs(b[inner] - sb).max())
            planes, fitted = fit_ref.fit(D, None, None, max_dis=64, radius=r, max_diff=math.inf, min_support=3, use_guide=0)
            assert fitted.all()
            np.testing.assert_allclose(planes[inner][..., 3], sa, rtol=0, atol=4 * PLANE_BOUND)  # the stored a, b come back from the normal
            np.testing.assert_allclose(planes[inner][..., 4], sb, rtol=0, atol=4 * PLANE_BOUND)
    print(f"radius {r}: largest slope error on exact planes = {worst:.3e}")
    assert worst <= PLANE_BOUND


def test_constant_map_gives_fronto_parallel_planes():
    D = np.full((9, 12), 7.0)
    I = np.random.default_rng(0).integers(0, 256, (9, 12, 3), dtype=np.uint8)
    for guide in (None, I):
        planes, fitted = fit_ref.fit(D, None, guide, max_dis=16, radius=2)
        want = np.zeros((9, 12, 6))
        want[..., 2] = 1.0
        want[..., 5] = 7.0
        np.testing.assert_array_equal(planes, want)
        assert fitted.all()


def test_single_node_and_a_line_of_nodes_are_degenerate():
    V = np.zeros((9, 9), np.uint8)
    V[4, 4] = 1
    D = np.arange(81, dtype=np.float64).reshape(9, 9)
    _, _, _, n, degenerate, node = fit_ref.solve(D, V, None, radius=3, max_diff=math.inf, min_support=3, use_guide=0)
    assert node.sum() == 1 and n[4, 4] == 1 and degenerate[4, 4]
    planes, fitted = fit_ref.fit(D, V, None, max_dis=100, radius=3, max_diff=math.inf, min_support=3, use_guide=0)
    np.testing.assert_array_equal(planes[4, 4], [0, 0, 1, 0, 0, D[4, 4]])
    assert fitted.sum() == 1
    for line in (np.s_[4, :], np.s_[:, 2]):  # one pixel wide, horizontal and vertical: collinear, det = 0
        V = np.zeros((9, 9), np.uint8)
        V[line] = 1
        _, _, _, n, degenerate, node = fit_ref.solve(D, V, None, radius=3, max_diff=math.inf, min_support=3, use_guide=0)
        assert (n[node] >= 4).all() and degenerate[node].all()
        planes, _ = fit_ref.fit(D, V, None, max_dis=100, radius=3, max_diff=math.inf, min_support=3, use_guide=0)
        np.testing.assert_array_equal(planes[node][:, :5], np.broadcast_to([0, 0, 1, 0, 0], (9, 5)))
        np.testing.assert_array_equal(planes[node][:, 5], D[node])


def test_non_nodes_are_nan_and_not_fitted():
    D, V, I = _random_case(5)
    D[3, 3] = np.inf
    D[4, 4] = -np.inf
    planes, fitted = fit_ref.fit(D, V, I, max_dis=16)
    node = np.isfinite(D) & (V != 0)
    assert not node.all()
    assert np.isnan(planes[~node]).all() and np.isfinite(planes[node]).all()
    np.testing.assert_array_equal(fitted, node.astype(np.uint8))
    assert not fitted[3, 3] and not fitted[4, 4]


def test_a_step_edge_below_the_threshold_fits_each_side_alone():
    w, h = 20, 11
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    left = 0.25 * xs + 0.125 * ys + 3.0
    right = -0.125 * xs + 0.5 * ys + 30.0  # at least 20 above the left side everywhere: the step
    D = np.where(xs < 10, left, right)
    params = dict(radius=3, max_diff=4.0, min_support=3, use_guide=0)
    both, fitted = fit_ref.fit(D, None, None, max_dis=64, **params)
    for side, keep in ((left, xs < 10), (right, xs >= 10)):
        V = np.broadcast_to(keep, (h, w)).astype(np.uint8)
        alone, _ = fit_ref.fit(D, V, None, max_dis=64, **params)
        np.testing.assert_array_equal(both[V != 0], alone[V != 0])
    assert fitted.all()
    assert np.abs(both[:, :10, 3] - 0.25).max() < 1e-12 and np.abs(both[:, 10:, 3] + 0.125).max() < 1e-12


def test_z_is_clamped_to_the_disparity_range():
    D = np.array([[-3.0, 2.0, 40.0]] * 3)
    planes, _ = fit_ref.fit(D, None, None, max_dis=16, radius=1, max_diff=0.0, min_support=3)  # every window is one value: degenerate
    np.testing.assert_array_equal(planes[..., 5], [[0.0, 2.0, 16.0]] * 3)


def test_header_declares_the_fit_entries():
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("cspm_fit_default_params", "cspm_fit_planes_host", "cspm_fit_planes"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    m = re.search(r"typedef struct cspm_fit_params \{(.*?)\} cspm_fit_params;", code, re.S)
    assert m
    fields = re.findall(r"\b(int|double)\s+(\w+);", m.group(1))
    assert fields == [("int", "radius"), ("double", "max_diff"), ("int", "min_support"), ("int", "use_guide")]
    from crossscalepatchmatch_amd import capi
    assert [f[0] for f in capi.FitParams._fields_] == [f[1] for f in fields]
    p = capi.fit_params()  # pure host logic: answers without a device
    assert (p.radius, p.max_diff, p.min_support, p.use_guide) == (5, 1.5, 6, 1)
    assert fit_ref.DEFAULTS == dict(radius=5, max_diff=1.5, min_support=6, use_guide=1)


def test_fit_entries_refuse_bad_parameters_before_touching_a_device():
    import ctypes as C
    from crossscalepatchmatch_amd import capi
    L = capi.load_library()
    d = np.zeros((4, 4))
    out = np.zeros((4, 4, 6))
    dp = C.POINTER(C.c_double)
    for bad in (dict(radius=0), dict(radius=18), dict(min_support=2), dict(max_diff=-1.0), dict(max_diff=math.nan)):
        p = capi.fit_params(**bad)
        rc = L.cspm_fit_planes_host(0, d.ctypes.data_as(dp), None, None, 0, 4, 4, 16, C.byref(p), out.ctypes.data_as(dp), None)
        assert rc == -1, bad  # CSPM_ERR_ARG
        assert b"plane fit" in L.cspm_last_error(None)
    assert L.cspm_fit_default_params(None) == -1


def test_cli_fit_flags_and_their_conflicts(tmp_path):
    exe = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(exe), "build the host layer: python -c 'import __graft_entry__ as g; g.build()'"
    common = [exe, f"--l_img_file={tmp_path}/none.png", f"--r_img_file={tmp_path}/none.png", "--max_dis=16", "--dis_scale=4", "--cc_name=GRD"]
    p = subprocess.run(common + ["--fit_radius=2"], capture_output=True, timeout=120)  # nothing to fit
    assert p.returncode != 0 and b"--fit_radius fits planes" in p.stdout and b"--warm_ca" in p.stdout
    p = subprocess.run(common + ["--fit_radius=18", "--warm_ca=BOX"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--fit_radius must be 1 .. 17" in p.stdout
    p = subprocess.run(common + ["--fit_radius=2", "--fit_max_diff=-1", "--warm_ca=BOX"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--fit_max_diff >= 0" in p.stdout
    p = subprocess.run(common + ["--fit_merge", "--warm_ca=BOX"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--fit_merge needs --fit_radius" in p.stdout
    for ok in (["--warm_ca=BOX"], ["--seed_ca=BOX"], ["--ca_name=BOX"], [f"--l_seed_pfm={tmp_path}/none.pfm"]):
        p = subprocess.run(common + ["--fit_radius=2", "--fit_merge"] + ok, capture_output=True, timeout=120)  # accepted: fails later, at the images
        assert p.returncode != 0 and b"--fit_" not in p.stdout and b"can not open image" in p.stdout, ok
