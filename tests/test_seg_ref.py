"""-m "not gpu": known answers for tests/seg_ref.py, the CPU restatement of the superpixel segment planes (include/cspm.h "segment
planes").  tests/test_gpu_seg.py holds the HIP entries to that restatement bit for bit; this file holds the
restatement to what the specification must give on inputs whose answer is known."""
import math

import numpy as np
import pytest

import seg_ref


def two_tone(w=70, h=40, edge=37, seed=3):
    rng = np.random.default_rng(seed)
    img = np.where(np.arange(w)[None, :, None] < edge, np.array([60, 60, 60]), np.array([200, 180, 160]))
    img = np.broadcast_to(img, (h, w, 3)) + rng.integers(-6, 7, (h, w, 3))
    return img.astype(np.uint8)


@pytest.mark.parametrize("m", [10, 20, 40])
@pytest.mark.parametrize("s", [4, 5, 8, 16])
def test_no_segment_straddles_the_edge_of_a_two_tone_image(s, m):
    edge = 37
    img = two_tone(edge=edge)
    labels, _, counts = seg_ref.segment(img, s, m, 5)
    left, right = set(labels[:, :edge].ravel().tolist()), set(labels[:, edge:].ravel().tolist())
    assert not (left & right), sorted(left & right)
    assert counts.min() > 0  # every segment is non-empty


@pytest.mark.parametrize("s,m,T", [(4, 0, 1), (5, 20, 5), (16, 255, 2), (7, 20, 3)])
def test_labels_stay_in_the_3x3_cells_and_counts_sum_to_the_image(s, m, T):
    rng = np.random.default_rng(s)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    labels, centres, counts = seg_ref.segment(img, s, m, T)
    assert seg_ref.labels_obey_3x3(labels, s)
    assert counts.sum() == 37 * 53
    np.testing.assert_array_equal(counts, np.bincount(labels.ravel(), minlength=counts.size))
    assert centres.shape == (seg_ref.grid(53, 37, s)[2], 5)
    assert centres[:, 0].min() >= 0 and centres[:, 0].max() <= 16 * 52 and centres[:, 2:].max() <= 16 * 255


def test_constant_image_without_compactness_has_empty_segments_that_keep_their_centres():
    """m = 0 and one colour: every Dist is 0, the first candidate wins, so the segments of the last row and column of cells that are
    nobody's first candidate stay empty: 6 of the 12 at 13 x 9, s = 4."""
    img = np.full((9, 13, 3), 77, np.uint8)
    s = 4
    nx, ny, K = seg_ref.grid(13, 9, s)
    assert (nx, ny, K) == (4, 3, 12)
    labels, centres, counts = seg_ref.segment(img, s, 0, 3)
    assert (counts == 0).sum() == 6
    for k in np.flatnonzero(counts == 0):
        gx, gy = k % nx, k // nx
        want = [16 * min(12, gx * s + s // 2), 16 * min(8, gy * s + s // 2), 16 * 77, 16 * 77, 16 * 77]
        assert centres[k].tolist() == want
    assert seg_ref.labels_obey_3x3(labels, s)


def test_update_rounds_the_mean_half_up():
    img = np.zeros((4, 4, 3), np.uint8)
    img[0, 0] = (1, 0, 0)  # B sum 16 over 16 members: mean 1 exactly; x mean 16 * 1.5 = 24
    _, centres, counts = seg_ref.segment(img, 4, 0, 1)
    assert counts.tolist() == [16] and centres[0].tolist() == [24, 24, 1, 0, 0]
    img[0, 1] = (1, 0, 0)
    img[0, 2] = (1, 0, 0)  # B sum 48 = 3 * 16 over 16: 3 exactly
    img[3, 3] = (0, 0, 1)  # R sum 16 -> 1
    _, centres, _ = seg_ref.segment(img, 4, 0, 1)
    assert centres[0].tolist() == [24, 24, 3, 0, 1]
    img5 = np.zeros((1, 3, 3), np.uint8)
    img5[0, 0, 1] = 1  # G sum 16 over 3: (32 + 3) // 6 = 5 (5.33 rounded)
    _, centres, _ = seg_ref.segment(img5, 4, 0, 1)
    assert centres[0].tolist() == [16, 0, 0, 5, 0]


# ---- the fit --------------------------------------------------------------------------------------------------------------------------

def _window_case(s, frac, seed):
    """a 3s x 3s image whose centre segment owns every pixel: the plane 0.25 u + 0.125 v + 7 with `frac` of the nodes displaced"""
    w = h = 3 * s
    nx = 3
    k = 1 * nx + 1
    labels = np.full((h, w), k, np.int32)
    u = np.arange(w)[None, :] - s
    v = np.arange(h)[:, None] - s
    D = 0.25 * u + 0.125 * v + 7.0
    rng = np.random.default_rng(seed)
    bad = np.zeros(h * w, bool)
    bad[rng.choice(h * w, int(frac * h * w), replace=False)] = True  # at most `frac` of the nodes
    bad = bad.reshape(h, w)
    D = np.where(bad, D + rng.choice([-10.0, 10.0, 6.5], (h, w)), D)
    return D, labels, k, bad


@pytest.mark.parametrize("frac", [0.05, 0.2])
@pytest.mark.parametrize("s", [4, 5, 16])
def test_outliers_are_rejected_and_the_plane_recovered(s, frac):
    D, labels, k, bad = _window_case(s, frac, 10 * s + int(100 * frac))
    seg, inl, planes, fitted = seg_ref.fit_segments(D, None, labels, s, 64, **{kk: seg_ref.DEFAULTS[kk] for kk in ("tau", "rounds", "min_support")})
    a, b, c = seg[k]
    assert abs(a - 0.25) < 1e-9 and abs(b - 0.125) < 1e-9 and abs(c - (7.0 - 0.25 * s - 0.125 * s)) < 1e-9
    assert inl[k] == (~bad).sum()
    assert fitted.all() and np.isnan(seg[np.arange(9) != k]).all() and not inl[np.arange(9) != k].any()
    h, w = D.shape
    z = planes[..., 3] * np.arange(w)[None, :] + planes[..., 4] * np.arange(h)[:, None] + planes[..., 5]
    np.testing.assert_allclose(z, 0.25 * (np.arange(w)[None, :] - s) + 0.125 * (np.arange(h)[:, None] - s) + 7.0, atol=1e-9)


def test_rounds_0_is_plain_least_squares():
    s = 8
    rng = np.random.default_rng(5)
    h, w = 2 * s, 3 * s
    labels = np.broadcast_to((np.arange(w) // s)[None, :] + 3 * (np.arange(h) // s)[:, None], (h, w)).astype(np.int32)
    D = np.round(rng.uniform(0, 20, (h, w)) * 16) / 16
    seg, inl, _, fitted = seg_ref.fit_segments(D, None, labels, s, 64, tau=1.0, rounds=0, min_support=6)
    assert fitted.all() and (inl == s * s).all()
    for k in range(6):
        ys, xs = np.nonzero(labels == k)
        A = np.stack([xs, ys, np.ones_like(xs)], axis=1).astype(np.float64)
        want = np.linalg.lstsq(A, D[ys, xs], rcond=None)[0]
        np.testing.assert_allclose(seg[k], want, atol=1e-9)


def test_collinear_and_under_supported_segments_are_unfitted():
    s = 4
    h, w = 4, 12
    labels = np.broadcast_to((np.arange(w) // s)[None, :], (h, w)).astype(np.int32)
    D = np.full((h, w), 3.0)
    V = np.ones((h, w), np.uint8)
    V[:, 0:4] = 0
    V[1, 0:4] = 1                        # segment 0: four collinear nodes
    V[:, 4:8] = 0
    V[0, 4] = V[2, 5] = V[3, 7] = V[1, 6] = 1  # segment 1: four nodes in general position, below min_support 6
    seg, inl, planes, fitted = seg_ref.fit_segments(D, V, labels, s, 16, tau=1.0, rounds=3, min_support=6)
    assert np.isnan(seg[0]).all() and np.isnan(seg[1]).all() and inl[:2].tolist() == [0, 0]
    assert not fitted[:, :8].any() and np.isnan(planes[:, :8]).all()
    assert fitted[:, 8:].all() and inl[2] == 16
    np.testing.assert_array_equal(seg[2], [0.0, 0.0, 3.0])
    seg, inl, _, fitted = seg_ref.fit_segments(D, V, labels, s, 16, tau=1.0, rounds=3, min_support=3)
    assert np.isnan(seg[0]).all() and inl[1] == 4 and fitted[:, 4:8].all()  # collinear stays unfitted; four nodes now suffice


def test_holes_receive_the_plane_and_non_nodes_are_ignored():
    s = 5
    h = w = 5
    labels = np.zeros((h, w), np.int32)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    D = 0.5 * u - 0.25 * v + 4.0
    D[2, 2] = np.nan
    D[0, 3] = np.inf
    D[4, 1] = 40000.0  # beyond 32768: not a node
    V = np.ones((h, w), np.uint8)
    V[1, 1] = 0
    D[1, 1] = -7.0     # masked out: ignored
    seg, inl, planes, fitted = seg_ref.fit_segments(D, V, labels, s, 64, tau=1.0, rounds=3, min_support=6)
    assert inl[0] == 25 - 4 and fitted.all()
    np.testing.assert_allclose(seg[0], [0.5, -0.25, 4.0], atol=1e-12)
    z = planes[..., 3] * u + planes[..., 4] * v + planes[..., 5]
    np.testing.assert_allclose(z, 0.5 * u - 0.25 * v + 4.0, atol=1e-9)


def test_z_is_clamped_at_both_ends():
    s = 8
    h, w = 8, 16
    labels = np.broadcast_to((np.arange(w) // s)[None, :], (h, w)).astype(np.int32)
    D = np.where(np.arange(w)[None, :] < s, -5.0, 50.0) + 0.125 * np.arange(h)[:, None]
    _, _, planes, fitted = seg_ref.fit_segments(D, None, labels, s, 16, tau=1.0, rounds=3, min_support=6)
    assert fitted.all()
    z = planes[..., 3] * np.arange(w)[None, :] + planes[..., 4] * np.arange(h)[:, None] + planes[..., 5]
    assert np.abs(z[:, :s]).max() < 1e-9 and np.abs(z[:, s:] - 16.0).max() < 1e-9
    assert np.abs(planes[..., 4] - 0.125).max() < 1e-9  # the slope survives the clamp: only the anchor moves


def test_infinite_tau_keeps_every_node_and_a_degenerate_later_round_keeps_the_previous_plane():
    D, labels, k, bad = _window_case(5, 0.2, 77)
    plain = seg_ref.fit_segments(D, None, labels, 5, 64, tau=1.0, rounds=0, min_support=6)
    every = seg_ref.fit_segments(D, None, labels, 5, 64, tau=math.inf, rounds=3, min_support=6)
    assert every[1][k] == D.size
    np.testing.assert_array_equal(every[0], plain[0])  # the same nodes every round: the same sums, the same plane
    # tau = 0 keeps only nodes that lie on the contaminated round-0 plane exactly: none here, so round 1 is degenerate
    with np.errstate(invalid="ignore"):
        a, b, c = plain[0][k]
        res = D - ((a * (np.arange(15)[None, :] - 5) + b * (np.arange(15)[:, None] - 5)) + ((c + a * 5) + b * 5))
    assert (res == 0).sum() < 6
    zero = seg_ref.fit_segments(D, None, labels, 5, 64, tau=0.0, rounds=1, min_support=6)
    np.testing.assert_array_equal(zero[0], plain[0])
    assert zero[1][k] == D.size and zero[3].all()


def test_labels_obey_3x3():
    assert seg_ref.labels_obey_3x3(np.full((15, 15), 4, np.int32), 5)       # the middle segment may own the whole 3 x 3 window
    assert not seg_ref.labels_obey_3x3(np.full((15, 15), 9, np.int32), 5)   # no such segment
    assert not seg_ref.labels_obey_3x3(np.zeros((15, 15), np.int32), 5)     # segment 0 claimed by pixels two cells away


def test_fields_wrapper_replaces_only_fitted_pixels():
    rng = np.random.default_rng(1)
    h, w = 12, 20
    d = np.round(rng.uniform(0, 8, (h, w)) * 8) / 8
    f = np.zeros((h, w, 6))
    f[..., 2] = 1.0
    f[..., 5] = d
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out, cands, masks, labs = seg_ref.segment_planes_fields([f, f], [img, img], 8, step=4, min_support=17)  # above a 16-pixel cell: only segments that grew are fitted
    for v in (0, 1):
        np.testing.assert_array_equal(out[v][masks[v] == 0], f[masks[v] == 0])
        np.testing.assert_array_equal(out[v][masks[v] != 0], cands[v][masks[v] != 0])
        assert np.isnan(cands[v][masks[v] == 0]).all()
        np.testing.assert_array_equal(labs[v], seg_ref.segment(img, 4, 20, 5)[0])
