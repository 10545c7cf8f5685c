"""CPU, seconds: the specification T checked on its numpy restatement tests/tsdf_ref.py alone -- what the device
is then held to bit for bit (test_gpu_tsdf.py) -- and that the case table tests/tsdf_cases.py is not vacuous.

The largest residuals seen (printed by every run, recorded in DESIGN.md section 28):
  cameras facing the plane: D 0, raycast depth 0 over 61224 hits, surface points 0 (bound 1e-9 relative; the geometry is dyadic)
  slanted plane, rotated cameras: 0.0035 over 30961 hits against a bound of 0.2097 (0.0097 between 4-adjacent pixels plus one voxel of 0.2)
  a view's own raycast: 0.0033 against one voxel of 0.2
  permuted views: 6.0e-8 against 2 K 2^-25 = 1.8e-7"""
import itertools

import numpy as np
import pytest

import fuse_cases as fc
import tsdf_cases as tc
import tsdf_ref as tr

# ---- cameras facing the plane -------------------------------------------------------------------------------------------------------------
# The plane z = 4 seen by cameras whose optical axis is its normal.  D is stored as f32, so the geometry is dyadic: voxel 1/4, centres
# at odd multiples of 1/8, trunc 1, translations by multiples of 1/8 -- then (d_plane - z)/trunc and every running mean of it are exact in
# f32 and section 25's bound of 1e-9 relative is a statement about the arithmetic, not about the storage format.
FRONT = (np.array([0.0, 0.0, 1.0]), 4.0, None)
F_DIMS, F_VOXEL, F_ORIGIN, F_TRUNC = (24, 16, 12), 0.25, (-3.0, -2.0, 2.5), 1.0
F_W, F_H = 130, 67
F_POSES = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.375, -0.125, 0.5])), (fc.rot(rz=15.0), np.array([-0.25, 0.125, -0.25])),
           (fc.rot(rz=-9.0), np.array([0.0, 0.0, 0.125]))]


def _front_views():
    views = []
    for k, (R, t) in enumerate(F_POSES):
        cam = fc.camera(F_W, F_H, k, R, t)
        depth, normal, bgr = fc.render(cam, F_W, F_H, [FRONT])
        views.append(fc.view(cam, depth, normal, bgr))
    return views


@pytest.fixture(scope="module")
def front():
    views = _front_views()
    return views, tr.fuse(views, F_W, F_H, F_ORIGIN, F_VOXEL, F_DIMS, trunc=F_TRUNC)


def test_facing_cameras_every_known_voxel_holds_the_plane_distance(front):
    _, res = front
    _, _, k = tr._indices(res["vol"])
    z = F_ORIGIN[2] + (k + 0.5) * F_VOXEL
    want = np.minimum((4.0 - z) / F_TRUNC, 1.0)
    known = res["W"] > 0
    assert known.sum() > 1000 and (want[known] < 0).any() and (want[known] == 1.0).any()
    resid = np.abs(res["D"][known].astype(np.float64) - want[known]) / np.maximum(np.abs(want[known]), 1.0)
    print("facing cameras: largest relative residual of D", resid.max())
    assert resid.max() <= 1e-9
    assert not (known & (want < -1.0)).any()  # nothing behind the band is ever written


def test_facing_cameras_raycast_depth_is_the_ray_plane_depth(front):
    views, res = front
    worst, hits = 0.0, 0
    for step_rel in (0.5, 1.0):
        vol = dict(res["vol"], step=np.float64(step_rel) * res["vol"]["trunc"])
        for v in views:
            ray = tr.raycast(vol, v, F_W, F_H, 0.0)
            hit = ray["status"] == 1
            want = 4.0 - v["t"][2]  # the depth along the optical axis of every point of the plane
            worst = max(worst, float(np.max(np.abs(ray["depth"][hit] - want) / want)))
            hits += int(hit.sum())
            nrm = ray["normal"][:, hit]
            nrm = nrm[:, np.isfinite(nrm[2])]  # NaN where the hit point's own cell has an unseen corner (the rim of the seen part)
            assert nrm.shape[1] > hit.sum() // 2 and np.allclose(nrm, np.array([0.0, 0.0, -1.0])[:, None], atol=1e-9)  # towards the camera
    print("facing cameras: largest relative residual of a raycast depth", worst, "over", hits, "hits")
    assert hits > 10000 and worst <= 1e-9


def test_facing_cameras_surface_points_lie_on_the_plane(front):
    _, res = front
    assert res["count"] > 100
    resid = np.abs(res["points64"][:, 2] - 4.0) / 4.0
    print("facing cameras: largest relative residual of a surface point", resid.max())
    assert resid.max() <= 1e-9
    assert np.all(res["cloud"]["pixel"] < np.prod(F_DIMS))
    inner = ~np.isnan(res["cloud"]["nz"])
    assert inner.any() and np.allclose(res["cloud"]["nz"][inner], -1.0)


# ---- the slanted plane, rotated cameras ---------------------------------------------------------------------------------------------------
S_DIMS, S_VOXEL, S_ORIGIN = (33, 17, 9), 0.2, (-3.3, -1.7, 3.0)
S_W, S_H = 130, 67
S_POSES = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.3, 0.05, 0.5])), (fc.rot(3.0, -8.0, 15.0), np.array([0.4, -0.1, 0.0])),
           (fc.rot(-2.0, 15.0, -6.0), np.array([-0.8, 0.05, 0.2]))]


def _slanted_views():
    views = []
    for k, (R, t) in enumerate(S_POSES):
        cam = fc.camera(S_W, S_H, k, R, t)
        depth, normal, bgr = fc.render(cam, S_W, S_H, [(fc.PLANE[0], fc.PLANE[1], None)])
        views.append(fc.view(cam, depth, normal, bgr))
    return views


def _adjacent_difference(depth):
    """the largest depth difference between 4-adjacent valid pixels"""
    with np.errstate(invalid="ignore"):
        return float(max(np.nanmax(np.abs(np.diff(depth, axis=0))), np.nanmax(np.abs(np.diff(depth, axis=1)))))


def test_slanted_plane_raycast_depth_within_the_nearest_pixel_bound():
    """a voxel takes the depth of the NEAREST pixel, so its sdf is off by at most the depth difference between adjacent pixels; the
    interpolant adds at most a voxel"""
    views = _slanted_views()
    res = tr.fuse(views, S_W, S_H, S_ORIGIN, S_VOXEL, S_DIMS, trunc=0.5)
    bound = max(_adjacent_difference(v["depth"]) for v in views) + S_VOXEL
    worst, hits = 0.0, 0
    for v in views:
        ray = tr.raycast(res["vol"], v, S_W, S_H, 0.0)
        hit = (ray["status"] == 1) & np.isfinite(v["depth"])
        worst = max(worst, float(np.max(np.abs(ray["depth"][hit] - v["depth"][hit]))))
        hits += int(hit.sum())
    print("slanted plane: largest raycast depth error", worst, "bound", bound, "over", hits, "hits")
    assert hits > 10000 and worst <= bound


def test_a_views_own_raycast_reproduces_its_depth_within_one_voxel():
    for v in _slanted_views():
        vol = tr.new_volume(S_ORIGIN, S_VOXEL, S_DIMS, trunc=0.5)
        tr.integrate(vol, v, S_W, S_H)
        ray = tr.raycast(vol, v, S_W, S_H, 0.0)
        hit = (ray["status"] == 1) & np.isfinite(v["depth"])
        err = float(np.max(np.abs(ray["depth"][hit] - v["depth"][hit])))
        print("own raycast: largest depth error", err, "over", int(hit.sum()), "hits")
        assert hit.sum() > 1000 and err <= S_VOXEL


# ---- other properties ---------------------------------------------------------------------------------------------------------------------
def test_identical_views_give_the_volume_of_one_view():
    """the mean of K copies of d: (D*Wo + d)/Wn lies within a quarter of an f32 ulp of D = (float)d, so it rounds to D again"""
    case = tc.BY_NAME["33x17x9_130x67_K3_identical"]
    views = case.views()
    one = tr.fuse(views[:1], case.w, case.h, case.origin, case.voxel, case.dims, **case.params)
    three = case.reference()
    assert one["D"].tobytes() == three["D"].tobytes()
    assert np.array_equal(three["W"], 3.0 * one["W"]) and np.array_equal(one["C"], three["C"])
    assert one["count"] == three["count"] and tr.same_bits(one["cloud"]["x"], three["cloud"]["x"])


def test_the_weight_saturates():
    case = tc.BY_NAME["33x17x9_130x67_K3_identical"]
    views = case.views()
    vol = tr.new_volume(case.origin, case.voxel, case.dims, **dict(case.params, max_weight=2.0))
    seen = []
    for v in views + views:
        tr.integrate(vol, v, case.w, case.h)
        seen.append(vol["W"].copy())
    assert seen[0].max() == 1.0 and all(np.array_equal(s, seen[1]) for s in seen[2:]) and set(np.unique(seen[1])) == {0.0, 2.0}
    sat = tc.BY_NAME["33x17x9_130x67_K3_saturated"].reference()
    assert sat["W"].max() == 2.0 and (sat["W"] == 1.0).any()


def test_permuting_the_views_moves_D_by_f32_rounding_only():
    """Without saturation D is the mean of the views' d whatever the order.  Every step rounds |D| <= 1 to f32, an error of at most 2^-25
    (0 for D = 1) that later steps only scale down: K 2^-25 per order, twice that between two orders (the f64 operations add 1e-15)."""
    case = tc.BY_NAME["33x17x9_130x67_K3_n1_all_c0.0"]
    views = case.views()
    base = case.reference()
    bound = 2 * len(views) * 2.0 ** -25 + 1e-12
    worst = 0.0
    for perm in itertools.permutations(range(len(views))):
        res = tr.fuse([views[k] for k in perm], case.w, case.h, case.origin, case.voxel, case.dims, **case.params)
        assert np.array_equal(res["W"], base["W"])
        worst = max(worst, float(np.max(np.abs(res["D"].astype(np.float64) - base["D"].astype(np.float64)))))
    print("permuted views: largest difference of D", worst, "bound", bound)
    assert 0.0 < worst <= bound


def test_parameter_rules():
    ok = dict(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(4, 4, 4))
    assert tr.check_params(**ok)
    for bad in (dict(voxel=0.0), dict(voxel=np.nan), dict(dims=(0, 4, 4)), dict(dims=(2048, 2048, 512)), dict(trunc=-1.0), dict(max_weight=0.5),
                dict(max_weight=2.0 ** 25), dict(min_cos=1.5), dict(step_rel=0.0), dict(step_rel=1.5), dict(origin=(0.0, np.inf, 0.0))):
        assert not tr.check_params(**dict(ok, **bad)), bad
    vol = tr.new_volume(ok["origin"], 0.1, (4, 4, 4))
    assert vol["trunc"] == np.float64(4.0) * np.float64(0.1) and (vol["D"] == 1).all() and (vol["W"] == 0).all() and not vol["C"].any()


# ---- the case table is not vacuous --------------------------------------------------------------------------------------------------------
LIVE = [c for c in tc.CASES if not c.degenerate]


def test_the_table_covers_the_sizes_and_the_crosses():
    assert {c.dims for c in tc.CASES} == {(1, 1, 1), (3, 2, 2), (64, 4, 3), (65, 5, 2), (257, 1, 2), (33, 17, 9), (96, 96, 64)}
    assert {(c.w, c.h) for c in tc.CASES} == {(1, 1), (7, 5), (65, 5), (130, 67)}
    assert {c.K for c in tc.CASES} == {1, 2, 3, 5} and {c.K for c in LIVE} == {2, 3, 5}
    assert {c.scene_args[5] for c in LIVE} == {True, False} and {c.scene_args[6] for c in LIVE} == {"all", "none", "some"}
    assert {c.params["min_cos"] for c in LIVE} == {0.0, 0.5} and {c.params["step_rel"] for c in LIVE} == {0.5, 1.0}
    assert {c.cap for c in LIVE} == {"exact", "zero", "short"} and {c.kind for c in LIVE} == {"plane", "occlusion", "blob"}
    assert any(c.params["max_weight"] == 2.0 and c.K == 3 for c in LIVE) and any(c.params["trunc"] == 0.0 for c in LIVE)
    assert len(LIVE) >= 10
    big = tc.BY_NAME["96x96x64_130x67_K2"]
    assert -(-np.prod(big.dims) // 256) > 2 * 1024  # the scan's one workgroup takes 1024 counts per pass


@pytest.mark.parametrize("case", LIVE, ids=repr)
def test_integration_is_not_vacuous(case):
    res = case.reference()
    for name in case.reachable_exits():
        assert res["exits"][name] > 0, name
    D, W = res["D"], res["W"]
    known = W > 0
    assert (~known).any(), "no unseen voxel"
    assert (known & (D == 1.0)).any(), "no clamped voxel"
    assert (known & (D > 0.0) & (D < 1.0)).any() and (known & (D < 0.0)).any(), "the band lacks a sign"
    assert W.max() == min(case.K, case.params["max_weight"])
    if case.scene_args[6] != "none":
        assert res["exits"]["painted"] > 0 and (res["C"][:, 3] == 1).any() and (known & (res["C"][:, 3] == 0)).any()
    else:
        assert not res["C"].any()


@pytest.mark.parametrize("case", LIVE, ids=repr)
def test_raycast_is_not_vacuous(case):
    rays = case.raycasts()
    status = np.concatenate([r["status"].ravel() for r in rays])
    assert set(np.unique(status)) == {0, 1, 2, 3}
    assert sum(r["inside"] for r in rays) > 0, "no ray starts inside the box"
    hit = np.concatenate([r["status"].ravel() == 1 for r in rays])
    depth = np.concatenate([r["depth"].ravel() for r in rays])
    assert np.isfinite(depth[hit]).all() and np.isnan(depth[~hit]).all()
    nz = np.concatenate([r["normal"][2].ravel() for r in rays])
    assert np.isfinite(nz[hit]).any() and np.isnan(nz[~hit]).all()


@pytest.mark.parametrize("case", LIVE, ids=repr)
def test_surface_points_are_not_vacuous(case):
    res = case.reference()
    for key, cnt in res["crossings"].items():
        assert cnt > 0, key
    assert res["refused"] > 0 and res["count"] == sum(res["crossings"].values()) == len(res["cloud"])
    assert np.all(np.diff(res["cloud"]["pixel"].astype(np.int64)) >= 0)
    assert np.isnan(res["cloud"]["nx"]).any() and np.isfinite(res["cloud"]["nx"]).any()
    assert 0 < case.capacity() + (case.cap == "zero") <= res["count"]
