"""Specification G of DESIGN.md section 19 (include/cspm.h "reprojection") restated on the CPU, twice:
reproject_pixel -- one pixel in Python floats, line by line as the specification writes it;
reproject       -- elementwise numpy with the same association, plus the cloud builder.
Every product, sum, quotient and square root is one IEEE f64 operation (Python floats and numpy f64 never contract)."""
import math

import numpy as np

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                  ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"), ("pixel", "<u4")])
assert POINT.itemsize == 32

DEFAULTS = dict(z_near=0.0, z_far=math.inf, min_cos=0.0, left_frame=0)
NAN = float("nan")


def check_args(calib, z_near=0.0, z_far=math.inf, min_cos=0.0, **_):
    """the validity rules of the calibration and the parameters: True when an entry would accept them"""
    f, cx, cy, B, doffs = calib
    if not all(math.isfinite(v) for v in (f, cx, cy, B, doffs)) or not f > 0 or not B > 0:
        return False
    return z_near >= 0.0 and z_far >= z_near and 0.0 <= min_cos <= 1.0


def _div(a, b):
    """IEEE division of Python floats: no ZeroDivisionError"""
    return float(np.float64(a) / np.float64(b))


def reproject_pixel(calib, v, x, y, D, V=1, A=None, Bs=None, z_near=0.0, z_far=math.inf, min_cos=0.0, left_frame=0):
    """-> dict(ok, keep, X, Y, Z, N (three floats, NaN without slopes), cos)"""
    f, cx, cy, baseline, doffs = (float(t) for t in calib)
    cxv = cx + float(v) * doffs
    fB = f * baseline
    D = float(D)
    with np.errstate(all="ignore"):
        t = D + doffs
        ok = V != 0 and math.isfinite(D) and t > 0.0
        Z = _div(fB, t)
        u = float(x) - cxv
        wv = float(y) - cy
        X = _div(u * Z, f)
        Y = _div(wv * Z, f)
        if left_frame and v == 1:
            X = X + baseline
        ok = ok and Z >= z_near and Z <= z_far
        N = (NAN, NAN, NAN)
        cos = NAN
        keep = ok
        if A is not None:
            A, Bs = float(A), float(Bs)
            n0 = A * f
            n1 = Bs * f
            n2 = (t - A * u) - Bs * wv
            s = (n0 * n0 + n1 * n1) + n2 * n2
            ln = math.sqrt(s) if s >= 0.0 else NAN  # s is a sum of squares: negative never, NaN stays NaN
            N = (_div(-n0, ln), _div(-n1, ln), _div(-n2, ln))
            cos = _div(f * t, ln * math.sqrt((u * u + wv * wv) + f * f))
            keep = ok and (min_cos == 0.0 or cos >= min_cos)
    return dict(ok=bool(ok), keep=bool(keep), X=X, Y=Y, Z=Z, N=N, cos=cos)


def reproject(calib, v, D, V=None, A=None, Bs=None, img=None, z_near=0.0, z_far=math.inf, min_cos=0.0, left_frame=0, cap=None):
    """D (h, w) f64; V (h, w) or None; A, Bs (h, w) f64 or None; img (h, w, 3) uint8 BGR or None.
    -> dict(depth (h, w), xyz (3, h, w), normal (3, h, w) or None, keep (h, w) uint8, cos, ok, count, cloud (POINT records, the first
    `cap` kept pixels in raster order; cap None = all))"""
    f, cx, cy, baseline, doffs = (np.float64(t) for t in calib)
    D = np.asarray(D, np.float64)
    h, w = D.shape
    cxv = cx + np.float64(v) * doffs
    fB = f * baseline
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        t = D + doffs
        ok = np.isfinite(D) & (t > 0.0)
        if V is not None:
            ok &= np.asarray(V) != 0
        Z = fB / t
        u = np.broadcast_to(x - cxv, D.shape)
        wv = np.broadcast_to(y - cy, D.shape)
        X = (u * Z) / f
        Y = (wv * Z) / f
        if left_frame and v == 1:
            X = X + baseline
        ok = ok & (Z >= z_near) & (Z <= z_far)
        keep = ok.copy()
        normal = cos = None
        if A is not None:
            A = np.asarray(A, np.float64)
            Bs = np.asarray(Bs, np.float64)
            n0 = A * f
            n1 = Bs * f
            n2 = (t - A * u) - Bs * wv
            ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            N = np.stack([-n0 / ln, -n1 / ln, -n2 / ln])
            cos = (f * t) / (ln * np.sqrt((u * u + wv * wv) + f * f))
            if min_cos != 0.0:
                keep &= cos >= min_cos
            normal = np.where(ok[None], N, np.nan)
    depth = np.where(ok, Z, np.nan)
    xyz = np.where(ok[None], np.stack([X, Y, Z]), np.nan)
    idx = np.flatnonzero(keep.ravel())
    count = len(idx)
    if cap is not None:
        idx = idx[:cap]
    cloud = np.zeros(len(idx), POINT)
    with np.errstate(all="ignore"):
        cloud["x"] = X.ravel()[idx].astype(np.float32)
        cloud["y"] = Y.ravel()[idx].astype(np.float32)
        cloud["z"] = Z.ravel()[idx].astype(np.float32)
        for k, name in enumerate(("nx", "ny", "nz")):
            cloud[name] = N[k].ravel()[idx].astype(np.float32) if A is not None else np.float32(np.nan)
    cloud["pixel"] = idx
    if img is not None:
        flat = np.asarray(img, np.uint8).reshape(-1, 3)
        cloud["b"], cloud["g"], cloud["r"], cloud["a"] = flat[idx, 0], flat[idx, 1], flat[idx, 2], 255
    return dict(depth=depth, xyz=xyz, normal=normal, keep=keep.astype(np.uint8), cos=cos, ok=ok, count=count, cloud=cloud)


def same_bits(a, b):
    """equal as bit patterns except that any NaN equals any NaN (payloads are not part of G); -0.0 differs from +0.0"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    ints = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(ints)[~na], b.view(ints)[~nb]))


def same_cloud(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == POINT and b.dtype == POINT and a.shape == b.shape and all(same_bits(a[n], b[n]) for n in POINT.names)


def render_plane(calib, v, w, h, m, hh):
    """the 3-D plane m . P = hh (P in view 0's camera frame, hh > 0) seen by view v of a rectified pair -> (D, A, Bs).
    Camera v sits at (v B, 0, 0): in its own frame the plane is m . P_v = h_v = hh - v B m0, its principal point is cx + v doffs, and
    with X = (x - cxv) Z / f, Y = (y - cy) Z / f, d + doffs = f B / Z the plane is the disparity plane d = a x + b y + c,
    a = B m0 / h_v, b = B m1 / h_v, c = (B / h_v) (m2 f - m0 cxv - m1 cy) - doffs."""
    f, cx, cy, B, doffs = (float(t) for t in calib)
    hv = hh - v * B * m[0]
    cxv = cx + v * doffs
    a, b = B * m[0] / hv, B * m[1] / hv
    c = (B / hv) * (m[2] * f - m[0] * cxv - m[1] * cy) - doffs
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    return a * x + b * y + c, np.full((h, w), a), np.full((h, w), b)
