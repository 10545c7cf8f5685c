"""-m "not gpu": the host derivation of the rectification R (cspm_rectify_compute; include/cspm.h "rectification")
against the numpy restatement tests/rectify_ref.py bit for bit, the restatement's own properties (an orthonormal R0 that takes camera
1's centre to (baseline, 0, 0); the exact identity rig; an epipolar known answer written independently of the map code) and every
CSPM_ERR_ARG the derivation answers.  cspm_rectify_compute is host logic: all of this runs without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import rectify_ref as rr
from crossscalepatchmatch_amd import capi

N_RIGS = 200


def _rigs(n=N_RIGS, seed=2310):
    rng = np.random.default_rng(seed)
    return [rr.random_rig(rng) for _ in range(n)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_rect(got, want):
    """a capi.Rectification against the restatement's dict, bit for bit"""
    return (np.array_equal(_bits(list(got.R0)), _bits(want["R0"].reshape(9))) and np.array_equal(_bits(list(got.R1)), _bits(want["R1"].reshape(9))) and
            np.array_equal(_bits([got.f, got.cx, got.cy, got.baseline]), _bits([want["f"], want["cx"], want["cy"], want["baseline"]])) and
            (got.w, got.h) == (want["w"], want["h"]))


def test_compute_matches_the_restatement_bit_for_bit():
    for k, rig in enumerate(_rigs()):
        kw = {} if k % 3 else dict(f=55.0 + k % 7, w=130, h=37)  # every third rig: a chosen focal length and size, automatic principal point
        if k % 5 == 0:
            kw.update(cx=31.25, cy=math.nan)  # a chosen cx beside an automatic cy
        want, want_calib = rr.compute(rig, **kw)
        got, calib = capi.rectify_compute(rr.capi_rig(rig), **kw)
        assert _same_rect(got, want), k
        assert np.array_equal(_bits([calib.f, calib.cx, calib.cy, calib.baseline, calib.doffs]), _bits(want_calib)), k
        assert calib.doffs == 0.0


def _library_rect(rig):
    """cspm_rectify_compute's answer in the restatement's form"""
    got, _ = capi.rectify_compute(rr.capi_rig(rig))
    return {"R0": np.array(list(got.R0)).reshape(3, 3), "R1": np.array(list(got.R1)).reshape(3, 3), "f": got.f, "cx": got.cx, "cy": got.cy,
            "baseline": got.baseline, "w": got.w, "h": got.h}


@pytest.mark.parametrize("source", ["restatement", "library"])
def test_rotation_properties(source):
    for rig in _rigs():
        rect = rr.compute(rig)[0] if source == "restatement" else _library_rect(rig)
        for R in (rect["R0"], rect["R1"]):
            assert abs(np.linalg.det(R) - 1.0) <= 1e-14
            assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-14
        C1 = -rig["R"].T @ rig["T"]
        B = rect["baseline"]
        assert np.max(np.abs(rect["R0"] @ C1 - np.array([B, 0.0, 0.0]))) <= 1e-14 * B
        # camera 1's frame: its own centre is the origin, so R1 (R C1 + T) = 0 and both views look along the same rectified axes
        assert np.max(np.abs(rect["R1"] @ rig["R"] - rect["R0"])) <= 1e-14


def test_identity_rig_is_exact():
    rig = rr.identity_rig()
    for rect, calib in (rr.compute(rig),):
        assert np.array_equal(rect["R0"], np.eye(3)) and np.array_equal(rect["R1"], np.eye(3))
        assert (rect["f"], rect["cx"], rect["cy"], rect["baseline"], rect["w"], rect["h"]) == (64.0, 23.5, 17.5, 0.25, 48, 36)
        assert calib == (64.0, 23.5, 17.5, 0.25, 0.0)
    got, calib = capi.rectify_compute(rr.capi_rig(rig))
    assert _same_rect(got, rect)
    raw = np.random.default_rng(3).integers(0, 256, (36, 48, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:36, 0:48]
    for v in (0, 1):
        bgr, sx, sy, valid = rr.rectify(rig, rect, v, raw)
        assert np.array_equal(sx, xx.astype(np.float64)) and np.array_equal(sy, yy.astype(np.float64))
        assert valid.all()
        assert np.array_equal(bgr, raw)  # the last row and column included: x1, y1 are clamped and tx = ty = 0


def _project(cam, P):
    """a forward projection written here, independently of the map code: pinhole + Brown-Conrady, plain numpy"""
    a, b = P[0] / P[2], P[1] / P[2]
    r2 = a * a + b * b
    rad = 1 + cam["k1"] * r2 + cam["k2"] * r2 ** 2 + cam["k3"] * r2 ** 3
    ad = a * rad + 2 * cam["p1"] * a * b + cam["p2"] * (r2 + 2 * a * a)
    bd = b * rad + cam["p1"] * (r2 + 2 * b * b) + 2 * cam["p2"] * a * b
    return cam["fx"] * ad + cam["skew"] * bd + cam["cx"], cam["fy"] * bd + cam["cy"]


@pytest.mark.parametrize("source", ["restatement", "library"])
def test_epipolar_known_answer(source):
    """a 3-D point seen at (x, y) with disparity d in the rectified pair: its forward projections into the two raw cameras are the map's
    entries at (x, y) of view 0 and at (x - d, y) of view 1.  Bar 1e-9 px: 2.8e-14 px was measured on these rigs; the bar leaves room
    for other rigs, not for the code under test."""
    worst = 0.0
    rng = np.random.default_rng(99)
    for rig in _rigs(40):
        rect = rr.compute(rig)[0] if source == "restatement" else _library_rect(rig)  # library: its rotations and projection under the map
        f, cx, cy, B = rect["f"], rect["cx"], rect["cy"], rect["baseline"]
        maps = [rr.rect_map(rig, rect, v) for v in (0, 1)]
        for _ in range(25):
            d = int(rng.integers(1, 12))
            x, y = int(rng.integers(d, rect["w"])), int(rng.integers(0, rect["h"]))
            Z = f * B / d
            P = np.array([(x - cx) * Z / f, (y - cy) * Z / f, Z])
            X0 = rect["R0"].T @ P
            X1 = rig["R"] @ X0 + rig["T"]
            for v, (X, xm) in enumerate(((X0, x), (X1, x - d))):
                px, py = _project(rig["cam"][v], X)
                worst = max(worst, abs(px - maps[v][0][y, xm]), abs(py - maps[v][1][y, xm]))
    print(f"epipolar known answer: worst deviation {worst:.3g} px")
    assert worst <= 1e-9


def _rc(rig, **kw):
    L = capi.load_library()
    p = capi.rect_params(**kw)
    rect, calib = capi.Rectification(), capi.Calib()
    rc = L.cspm_rectify_compute(C.byref(rig) if rig is not None else None, C.byref(p), C.byref(rect), C.byref(calib))
    return rc, L.cspm_last_error(None).decode()


def _ident(**over):
    c = rr.camera(64.0, 64.0, 23.5, 17.5)
    kw = dict(cam0=c, cam1=c, R=np.eye(3), T=(-0.25, 0.0, 0.0), raw_w=48, raw_h=36)
    kw.update(over)
    return rr.make_rig(**kw)


ERRORS = {
    "camera 1 on the left": _ident(T=(0.25, 0.0, 0.0)),
    "a vertical rig": _ident(T=(-0.1, -0.25, 0.0)),
    "a rig along the optical axis": _ident(T=(-0.1, 0.0, -0.25)),
    "T = 0": _ident(T=(0.0, 0.0, 0.0)),
    "NaN in a camera": _ident(cam1=rr.camera(64.0, 64.0, math.nan, 17.5)),
    "NaN in R": _ident(R=np.array([[1, 0, 0], [0, math.nan, 0], [0, 0, 1.0]])),
    "infinite T": _ident(T=(-math.inf, 0.0, 0.0)),
    "fx = 0": _ident(cam0=rr.camera(0.0, 64.0, 23.5, 17.5)),
    "fy < 0": _ident(cam1=rr.camera(64.0, -64.0, 23.5, 17.5)),
    "an empty raw image": _ident(raw_w=0),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_errors(name):
    rig = ERRORS[name]
    with pytest.raises(rr.RigError):
        rr.compute(rig)
    rc, msg = _rc(rr.capi_rig(rig))
    assert rc == -1 and msg.startswith("rectification"), (rc, msg)  # CSPM_ERR_ARG with a message


def test_parameter_errors_and_optional_outputs():
    rig = rr.capi_rig(rr.identity_rig())
    assert _rc(None)[0] == -1
    for kw in (dict(f=math.inf), dict(cx=math.inf), dict(cy=-math.inf), dict(w=1 << 16, h=1 << 15)):
        rc, msg = _rc(rig, **kw)
        assert rc == -1 and msg, kw
    assert _rc(rig, w=1, h=1)[0] == 0
    L = capi.load_library()
    assert L.cspm_rectify_compute(C.byref(rig), None, None, None) == 0  # NULL params = automatic; both outputs optional
    p = capi.RectParams(1.0, 2.0, 3.0, 4, 5)
    assert L.cspm_rect_default_params(C.byref(p)) == 0
    assert p.f <= 0.0 and math.isnan(p.cx) and math.isnan(p.cy) and p.w <= 0 and p.h <= 0
    assert L.cspm_rect_default_params(None) == -1
