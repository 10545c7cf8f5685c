"""-m "not gpu": properties of the fusion restatement tests/fuse_ref.py on exactly rendered scenes, and the
condition that the case table tests/fuse_cases.py is not vacuous: every case that is not labelled degenerate holds a pixel in every
state and leaves the specification's loop by every exit its inputs can reach."""
import numpy as np
import pytest

import fuse_cases as fc
import fuse_ref as fr

W, H = 130, 67
N_PLANE, D_PLANE = fc.PLANE


def _plane_views(K, **kw):
    return list(fc.scene("plane", W, H, K, 3, True, "all", True, False)), kw


def _valid(v):
    return np.isfinite(v["depth"]) & (v["depth"] > 0.0)


@pytest.mark.parametrize("K,params", [(2, dict(min_views=1)), (3, dict(min_views=2)), (5, dict(min_views=2, suppress=0))])
def test_plane_points_lie_on_the_plane(K, params):
    """a mean of exact points of one plane lies on it up to f64 rounding: |n.P - d| <= 1e-9 |d| (the bound of the issue; the largest
    residual observed here was 4.5e-16 |d|, so the bound is not tight and was not widened)"""
    views, _ = _plane_views(K)
    r = fr.fuse(views, W, H, **params)
    assert r["count"] > 1000
    res = np.abs(r["points64"] @ N_PLANE - D_PLANE)
    print("largest residual / |d|:", res.max() / D_PLANE)
    assert res.max() <= 1e-9 * abs(D_PLANE)
    # the records are the float casts of those means
    got = np.stack([r["cloud"][n] for n in ("x", "y", "z")], -1)
    assert np.array_equal(got, r["points64"].astype(np.float32))


def test_plane_normals_are_the_planes_normal():
    """the summed world normals of one plane, normalised, are the plane's normal facing the cameras, to float32 resolution"""
    views, _ = _plane_views(3)
    r = fr.fuse(views, W, H, min_views=1)
    n = np.stack([r["cloud"][k] for k in ("nx", "ny", "nz")], -1).astype(np.float64)
    assert len(n) > 1000 and np.abs(n + N_PLANE).max() <= 1e-6  # the cameras look along +z: the facing normal is -n


@pytest.mark.parametrize("K", [2, 3, 5])
def test_identical_views(K):
    """K copies of one view: with suppression the cloud is exactly view 0's kept pixels, without it K times that"""
    views = list(fc.scene("identical", W, H, K, 4, True, "all", True, False))
    valid = _valid(views[0])
    on = fr.fuse(views, W, H, min_views=K - 1, suppress=1)
    assert on["count"] == valid.sum() and list(on["view_counts"]) == [valid.sum()] + [0] * (K - 1)
    assert np.array_equal(on["cloud"]["pixel"], np.flatnonzero(valid.ravel()))
    assert np.all(on["state"][1:][:, valid] == fr.S_SUPPRESSED) and np.all(on["state"][0][valid] == (K - 1) | fr.S_KEPT)
    off = fr.fuse(views, W, H, min_views=K - 1, suppress=0)
    assert off["count"] == K * valid.sum()
    for k in range(K):
        part = off["cloud"][k * valid.sum():(k + 1) * valid.sum()]
        assert fr.same_cloud(part, on["cloud"])


def test_wrong_depth_blob_is_removed_by_a_third_view():
    views = list(fc.scene("blob", W, H, 3, 5, True, "all", True, False))
    blob = np.zeros((H, W), bool)
    blob[H // 4:H // 2, W // 4:W // 2] = True
    strict = fr.fuse(views, W, H, min_views=2, suppress=0)
    lax = fr.fuse(views, W, H, min_views=0, suppress=0)

    def from_view_1(r):
        a = int(r["view_counts"][0])
        return r["cloud"]["pixel"][a:a + int(r["view_counts"][1])]

    assert not blob.ravel()[from_view_1(strict)].any()
    assert blob.ravel()[from_view_1(lax)].sum() == blob.sum()
    # and nothing that is emitted is off the plane by more than the depth tolerance allows
    assert np.abs(strict["points64"] @ N_PLANE - D_PLANE).max() <= 0.01 * D_PLANE
    assert np.abs(lax["points64"] @ N_PLANE - D_PLANE).max() > 0.1 * D_PLANE


def test_occluded_surface_seen_by_no_other_view_is_not_kept():
    """pixels of the back plane that view 0 sees and view 1 does not (the front rectangle is in the way, or they project outside its
    image) have no consistent view: with min_views = 1 they are evaluated and not kept"""
    views = list(fc.scene("occlusion", W, H, 2, 6, True, "all", True, False))
    v0, v1 = views
    depth = v0["depth"]
    x = np.arange(W)[None, :] + np.zeros((H, 1))
    y = np.arange(H)[:, None] + np.zeros((1, W))
    P = np.stack(fr._world(fr._cam(v0), x, y, depth))            # view 0 is the identity pose: world = camera
    back = depth > 3.0                                            # the front rectangle is at z = 2.5, the plane about 4
    s = (2.5 - v1["t"][2]) / (P[2] - v1["t"][2])                  # where the ray from camera 1 to P crosses z = 2.5
    X = v1["t"][:, None, None] + s[None] * (P - v1["t"][:, None, None])
    g = 4 * 2.5 / v1["f"]  # four pixels of view 1 at the rectangle's distance: view 1 samples a rounded pixel and 2 pixels are tolerated
    hidden = (s > 0) & (s < 1) & (X[0] >= -0.6 + g) & (X[0] <= 0.2 - g) & (X[1] >= -1.0 + g) & (X[1] <= 1.0 - g)
    Q = fr._to_cam(fr._cam(v1), list(P))
    pu, pv = fr._proj(fr._cam(v1), Q)
    outside = (pu < -0.5) | (pu > W - 0.5) | (pv < -0.5) | (pv > H - 0.5)
    unseen = back & (hidden | outside)
    assert unseen.sum() > 50
    r = fr.fuse(views, W, H, min_views=1)
    assert np.all(r["state"][0][unseen] == 0)  # evaluated, c = 0, not kept
    assert (r["state"][0][back & ~unseen] & fr.S_KEPT).any()


def test_one_view():
    views = list(fc.scene("spoiled", W, H, 1, 7, True, "all", True, False))
    valid = _valid(views[0])
    r = fr.fuse(views, W, H, min_views=0)
    assert r["count"] == valid.sum() and np.array_equal(r["cloud"]["pixel"], np.flatnonzero(valid.ravel()))
    x = np.arange(W)[None, :] + np.zeros((H, 1))
    y = np.arange(H)[:, None] + np.zeros((1, W))
    with np.errstate(all="ignore"):
        P = np.stack(fr._world(fr._cam(views[0]), x, y, views[0]["depth"]))[:, valid]
    for i, n in enumerate(("x", "y", "z")):
        assert np.array_equal(r["cloud"][n], P[i].astype(np.float32))  # den = 1: the point itself
    assert np.array_equal(np.stack([r["cloud"][n] for n in ("b", "g", "r")], -1), views[0]["bgr"][valid])
    none = fr.fuse(views, W, H, min_views=1)
    assert none["count"] == 0 and np.all(none["state"][0][valid] == 0)


def test_permuting_the_other_views_leaves_view_0s_states():
    views = list(fc.scene("spoiled", W, H, 5, 8, True, "all", True, True))
    a = fr.fuse(views, W, H, suppress=0, min_cos=0.9)
    perm = [views[0], views[3], views[1], views[4], views[2]]
    b = fr.fuse(perm, W, H, suppress=0, min_cos=0.9)
    assert np.array_equal(a["state"][0], b["state"][0]) and (a["state"][0] & fr.S_KEPT).any()


def test_argument_rules():
    views = list(fc.scene("plane", 7, 5, 2, 9, True, "all", True, False))
    assert fr.check_args(views)
    assert not fr.check_args(views, min_views=64) and not fr.check_args(views, min_cos=1.5) and not fr.check_args(views, max_reproj=-1.0)
    assert not fr.check_args([dict(views[0], R=views[0]["R"] * 1.001), views[1]])
    assert not fr.check_args([dict(views[0], f=0.0), views[1]])
    assert not fr.check_args([views[0], {k: v for k, v in views[1].items() if k != "normal"}])
    assert not fr.check_args([]) and not fr.check_args(views * 33)


# ---- the case table is not vacuous -------------------------------------------------------------------------------------------------
def test_table_covers_the_settings():
    cs = fc.CASES
    assert {c.K for c in cs} >= {1, 2, 3, 5, 64}
    assert {(c.w, c.h) for c in cs} >= {(1, 1), (7, 5), (63, 3), (64, 4), (65, 5), (257, 1), (130, 67), (512, 513)}
    assert {c.params["suppress"] for c in cs} == {0, 1} and {c.params["min_views"] for c in cs} >= {0, 1, 2}
    assert {c.params["min_cos"] for c in cs} == {0.0, 0.9} and {c.scene_args[5] for c in cs} == {True, False}
    assert {c.scene_args[6] for c in cs} == {"all", "none", "some"} and {c.cap for c in cs} == {"exact", "zero", "short"}
    assert sum(not c.degenerate for c in cs) >= 20


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case_is_not_vacuous(case):
    assert fr.check_args(case.views(), **case.params)
    r = case.reference()
    if case.degenerate:
        return
    S = r["state"]
    valid = np.stack([_valid(v) for v in case.views()])
    assert (~valid).any(), "no invalid pixel"
    if case.params["suppress"]:
        assert (S == fr.S_SUPPRESSED).any(), "no suppressed pixel"
    if case.params["min_views"] >= 1:  # with min_views = 0 every evaluated pixel is kept: c >= 0
        assert (valid & ((S & 0xC0) == 0)).any(), "no pixel that was evaluated and not kept"
    assert (((S & fr.S_KEPT) != 0) & ((S & 0x3F) >= 1)).any(), "no kept pixel with a consistent view"
    for e in case.reachable_exits():
        assert r["exits"][e] > 0, f"no loop iteration left by {e}"
    assert 0 < r["count"] < case.K * case.w * case.h
