"""The restatement of the plane-field carry (tests/carry_ref.py) against algebra and analytic geometry, without a
GPU, and the case table of the GPU test: every exit, state and tie it is meant to cover occurs in it."""
import numpy as np
import pytest

import carry_cases as cc
import carry_ref as cr
import fuse_cases as fc
import register_cases as rc


def _field(abc, w, h):
    f = np.zeros((h, w, 6))
    f[..., 2] = 1.0
    f[..., 3:6] = abc
    return f


def test_baseline_shift_is_view_propagation():
    """R = I, t = (-B, 0, 0) into the pair's own view-1 camera: the carried plane is (a, b, c) / (1 - a); a >= 1 has no contender"""
    cal = (117.0, 64.8, 32.8, 0.2, 3.5)
    ks, kt = cr.camera(cal, 0), cr.camera(cal, 1)
    R, t = np.eye(3), np.array([-0.2, 0.0, 0.0])
    rng = np.random.default_rng(3)
    for _ in range(200):
        a, b, c = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(1.0, 30.0)
        pa, pb, pc, hq = cr.plane(ks, kt, R, t, np.float64(a), np.float64(b), np.float64(c))
        assert hq > 0.0
        for got, want in zip((pa, pb, pc), (a / (1 - a), b / (1 - a), c / (1 - a))):
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (a, b, c, got, want)
    for a in (1.0, 1.5, 40.0):
        res = cr.carry(_field((a, 0.1, 20.0), 9, 7), ks, kt, R, t, 9, 7, 1e9)
        assert not (res["state"] == 1).any() and set(np.unique(res["exit"])) <= {cr.EXITS.index(e) for e in ("hq", "tt", "behind", "outside")}


def test_identity_returns_every_plane():
    cal = (117.0, 64.8, 32.8, 0.2, -1.25)
    rng = np.random.default_rng(4)
    w, h = 23, 11
    f = _field((0.0, 0.0, 0.0), w, h)
    f[..., 3] = rng.uniform(-0.3, 0.3, (h, w))
    f[..., 4] = rng.uniform(-0.3, 0.3, (h, w))
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    f[..., 5] = rng.uniform(5.0, 30.0, (h, w)) - f[..., 3] * x - f[..., 4] * y  # a disparity in 5 .. 30 at the pixel itself
    for v in (0, 1):
        k = cr.camera(cal, v)
        res = cr.carry(f, k, k, np.eye(3), np.zeros(3), w, h, 64, fill=0)
        assert (res["state"] == 1).all()
        assert np.array_equal(res["source"].ravel(), np.arange(w * h))
        got, want = res["planes"][..., 3:6], f[..., 3:6]
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


def test_relative_pose():
    Rs, ts = fc.rot(3.0, -7.0, 11.0), np.array([0.3, -0.2, 0.7])
    Rt, tt = fc.rot(-2.0, 5.0, 1.0), np.array([-0.1, 0.4, 0.2])
    R, t = cr.relative_pose(Rs, ts, Rt, tt)
    X = np.array([0.4, -0.3, 2.5])
    assert np.allclose(Rt @ (R @ X + t) + tt, Rs @ X + ts, atol=1e-14)
    R1, t1 = cr.view1_motion(R, t, 0.2, 0.3)
    Xs1 = X - np.array([0.2, 0.0, 0.0])  # the same point in the source's view-1 camera
    assert np.allclose(R1 @ Xs1 + t1, (R @ X + t) - np.array([0.3, 0.0, 0.0]), atol=1e-14)


@pytest.mark.parametrize("w,h", [(130, 67), (300, 220)])
def test_corner_against_analytic_geometry(w, h):
    """the rendered three-plane corner, source at the identity, target at register_cases.TRUE: every carried pixel with S = 1 equals the
    analytic plane of the target view, except where its winner came from another surface than the one visible there"""
    cal = cc.calib(w, h)
    src, src_index, _ = cc.analytic(cal, 0, w, h, rc.CORNER)
    dst, dst_index, _ = cc.analytic(cal, 0, w, h, rc.CORNER, rc.TRUE)
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    max_dis = 1.5 * np.nanmax((dst[..., 3] * x + dst[..., 4] * y) + dst[..., 5])
    R, t = cr.relative_pose(np.eye(3), np.zeros(3), *rc.TRUE)
    k = cr.camera(cal, 0)
    res = cr.carry(src, k, k, R, t, w, h, max_dis)
    carried = res["state"] == 1
    other = carried & (src_index.ravel()[np.maximum(res["source"], 0)] != dst_index)  # creases and occlusion edges
    check = carried & ~other
    d = np.abs(res["planes"][..., 3:6] - dst[..., 3:6])[check]
    scale = np.maximum(1.0, np.abs(dst[..., 5][check]))
    print(f"{w}x{h}: covered {carried.mean():.4f}, left out {other.sum() / carried.sum():.4f}, max |da| {d[:, 0].max():.3g} |db| {d[:, 1].max():.3g} "
          f"|dc|/max(1,|c|) {(d[:, 2] / scale).max():.3g}")
    assert d[:, 0].max() <= 1e-12 and d[:, 1].max() <= 1e-12
    assert np.all(d[:, 2] <= 1e-12 * scale)
    assert other.sum() <= 0.01 * carried.sum()
    assert carried.mean() >= 0.85


def test_table_is_not_vacuous():
    exits, states = set(), set()
    depth_ties = fill_ties = 0
    for case in cc.CASES:
        ref = case.reference()
        exits |= set(np.unique(ref["exit"]).tolist())
        states |= set(np.unique(ref["state"]).tolist())
        depth_ties += ref["depth_ties"]
        fill_ties += ref["fill_ties"]
    assert exits == set(range(len(cr.EXITS))), [e for i, e in enumerate(cr.EXITS) if i not in exits]
    assert states == {0, 1, 2}
    assert depth_ties > 0 and fill_ties > 0
    half = cc.BY_NAME["half_300x220_150x110"].reference()
    assert (half["state"] == 1).all()  # four contenders per target pixel, the smallest m wins: the even column of the even row
    yy, xx = np.divmod(half["source"], 300)
    assert np.array_equal(xx, np.broadcast_to(2 * np.arange(150)[None, :], (110, 150))) and np.array_equal(yy, np.broadcast_to(2 * np.arange(110)[:, None], (110, 150)))
    stretch = cc.BY_NAME["stretch_64x48_130x67"].reference()
    assert (stretch["state"] == 2).mean() > 0.2
    assert (cc.BY_NAME["nothing_130x67"].reference()["state"] == 0).all()
    assert cr.EXITS.index("hq") in cc.BY_NAME["behind_130x67"].reference()["exit"]
    rz = cc.BY_NAME["rz180_130x67"].reference()
    first, last = rz["source"][rz["state"] == 1][[0, -1]]
    assert first > last  # the raster order is reversed
