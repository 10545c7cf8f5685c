"""CPU restatement of the plane fit (include/cspm.h "plane fitting"), written from the specification:
F(D, V, I, radius, max_diff, min_support, use_guide, max_dis) -> (planes, fitted), a local weighted least-squares plane per pixel.

fit_pixel() is the specification line by line for one pixel, in Python floats (IEEE f64, one rounding per operation).  fit() is the
same arithmetic for a whole map: the taps are visited one after the other in the specified order and every step is an elementwise
numpy operation over all pixels at once -- numpy rounds every elementwise f64 product and sum on its own and never contracts a
multiply and an add, so each pixel sees exactly fit_pixel()'s chain (tests/test_fit_ref.py holds the two to each other bit for bit).
tests/test_gpu_fit.py holds the HIP entries to fit() with array_equal.  It never imports the GPU package."""
import math

import numpy as np

LUT = np.array([math.exp(-i * 1.0 / 10.0) for i in range(766)])  # libm, like the library's table
DEFAULTS = dict(radius=5, max_diff=1.5, min_support=6, use_guide=1)
EPS = 0.00000001
DET_RATIO = 1e-6


def nodes(D, V=None):
    n = np.isfinite(np.asarray(D, dtype=np.float64))
    if V is not None:
        n &= np.asarray(V) != 0
    return n


def _plane(a, b, c0, dp, x, y, max_dis):
    """the output plane of one pixel from its solution, in Python floats"""
    t = dp + c0
    z = t if t > 0.0 else 0.0
    z = z if z < float(max_dis) else float(max_dis)
    m0, m1, m2 = -a, -b, 1.0
    s = m0 * m0
    s += m1 * m1
    s += m2 * m2
    inv = 1.0 / max(math.sqrt(s), EPS)
    nx, ny, nz = m0 * inv, m1 * inv, m2 * inv
    denom = max(abs(nz), EPS)  # Plane::update_param
    if nz < 0.0:
        denom = -denom
    pa = -nx / denom
    pb = -ny / denom
    s = nx * float(x)
    s += ny * float(y)
    s += nz * z
    return nx, ny, nz, pa, pb, s / denom


def fit_pixel(D, V, I, x, y, max_dis, radius=5, max_diff=1.5, min_support=6, use_guide=1):
    """one pixel, the specification as written.  Returns (six floats, fitted)."""
    D = np.asarray(D, dtype=np.float64)
    h, w = D.shape
    node = nodes(D, V)
    if not node[y, x]:
        return (math.nan,) * 6, 0
    guided = bool(use_guide) and I is not None
    dp = float(D[y, x])
    Sw = Su = Sv = Suu = Suv = Svv = Se = Sue = Sve = 0.0
    n = 0
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            qx, qy = x + i, y + j
            if not (0 <= qx < w and 0 <= qy < h) or not node[qy, qx]:
                continue
            e = float(D[qy, qx]) - dp
            if not abs(e) <= max_diff:
                continue
            wq = 1.0
            if guided:
                k = sum(abs(int(I[qy, qx, ch]) - int(I[y, x, ch])) for ch in range(3))
                wq = float(LUT[k])
            u, v = float(i), float(j)
            Sw = Sw + wq * 1.0
            Su = Su + wq * u
            Sv = Sv + wq * v
            Suu = Suu + wq * (u * u)
            Suv = Suv + wq * (u * v)
            Svv = Svv + wq * (v * v)
            Se = Se + wq * e
            Sue = Sue + wq * (u * e)
            Sve = Sve + wq * (v * e)
            n += 1
    C00 = Svv * Sw - Sv * Sv
    C01 = Suv * Sw - Sv * Su
    C02 = Suv * Sv - Svv * Su
    C11 = Suu * Sw - Su * Su
    C12 = Suu * Sv - Suv * Su
    C22 = Suu * Svv - Suv * Suv
    det = (Suu * C00 - Suv * C01) + Su * C02
    a = b = c0 = 0.0
    if n >= min_support and det > DET_RATIO * ((Suu * Svv) * Sw):
        a = ((C00 * Sue - C01 * Sve) + C02 * Se) / det
        b = ((C11 * Sve - C01 * Sue) - C12 * Se) / det
        c0 = ((C02 * Sue - C12 * Sve) + C22 * Se) / det
    return _plane(a, b, c0, dp, x, y, max_dis), 1


def solve(D, V, I, radius=5, max_diff=1.5, min_support=6, use_guide=1):
    """the sums and the solve of every pixel: (a, b, c0, n, degenerate, node), each (h, w).  a, b, c0 are 0 where the fit is
    degenerate; everything is meaningless outside `node`."""
    D = np.asarray(D, dtype=np.float64)
    h, w = D.shape
    r = int(radius)
    node = nodes(D, V)
    guided = bool(use_guide) and I is not None
    Dn = np.full((h + 2 * r, w + 2 * r), np.nan)  # non-nodes and the outside folded to NaN: such a tap never passes the <= test
    Dn[r:r + h, r:r + w] = np.where(node, D, np.nan)
    if guided:
        Ip = np.zeros((h + 2 * r, w + 2 * r, 3), np.int64)
        Ip[r:r + h, r:r + w] = np.asarray(I).astype(np.int64)
        Ic = Ip[r:r + h, r:r + w]
    Dp = Dn[r:r + h, r:r + w]
    S = [np.zeros((h, w)) for _ in range(9)]
    n = np.zeros((h, w), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                e = Dn[r + j:r + j + h, r + i:r + i + w] - Dp
                ok = np.abs(e) <= max_diff
                if not ok.any():
                    continue
                if guided:
                    k = np.abs(Ip[r + j:r + j + h, r + i:r + i + w] - Ic).sum(axis=2)
                    wq = LUT[k]
                else:
                    wq = np.ones((h, w))
                u, v = float(i), float(j)
                for idx, t in enumerate((1.0, u, v, u * u, u * v, v * v, e, u * e, v * e)):
                    S[idx] = np.where(ok, S[idx] + wq * t, S[idx])
                n += ok
        Sw, Su, Sv, Suu, Suv, Svv, Se, Sue, Sve = S
        C00 = Svv * Sw - Sv * Sv
        C01 = Suv * Sw - Sv * Su
        C02 = Suv * Sv - Svv * Su
        C11 = Suu * Sw - Su * Su
        C12 = Suu * Sv - Suv * Su
        C22 = Suu * Svv - Suv * Suv
        det = (Suu * C00 - Suv * C01) + Su * C02
        good = (n >= min_support) & (det > DET_RATIO * ((Suu * Svv) * Sw))
        safe = np.where(good, det, 1.0)
        a = np.where(good, ((C00 * Sue - C01 * Sve) + C02 * Se) / safe, 0.0)
        b = np.where(good, ((C11 * Sve - C01 * Sue) - C12 * Se) / safe, 0.0)
        c0 = np.where(good, ((C02 * Sue - C12 * Sve) + C22 * Se) / safe, 0.0)
    return a, b, c0, n, ~good, node


def fit(D, V=None, I=None, max_dis=0, radius=5, max_diff=1.5, min_support=6, use_guide=1):
    """cspm_fit_planes_host: ((h, w, 6) planes in the layout of cspm_get_planes, (h, w) uint8 fitted)"""
    D = np.asarray(D, dtype=np.float64)
    h, w = D.shape
    a, b, c0, _, _, node = solve(D, V, I, radius, max_diff, min_support, use_guide)
    xs = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(node, D, 0.0) + c0
        z = np.where(t > 0.0, t, 0.0)
        z = np.where(z < float(max_dis), z, float(max_dis))
        m0, m1, m2 = -a, -b, np.ones((h, w))
        s = m0 * m0
        s = s + m1 * m1
        s = s + m2 * m2
        inv = 1.0 / np.maximum(np.sqrt(s), EPS)
        nx, ny, nz = m0 * inv, m1 * inv, m2 * inv
        denom = np.maximum(np.abs(nz), EPS)
        denom = np.where(nz < 0.0, -denom, denom)
        pa = -nx / denom
        pb = -ny / denom
        s = nx * xs
        s = s + ny * ys
        s = s + nz * z
        pc = s / denom
    planes = np.stack([nx, ny, nz, pa, pb, pc], axis=-1)
    planes[~node] = np.nan
    return planes, node.astype(np.uint8)


def fit_fields(fields, images, max_dis, **params):
    """cspm_fit_planes(merge = 0) on both views: fields[v] (h, w, 6), images[v] the level-0 BGR image.  D is the stored field's
    a*x + b*y + c in the order of cspm_get_disparity_f64.  Returns (replaced, candidates, masks) per view: the field with every fitted
    pixel's plane replaced (any other keeps its own), and what merge = 1 offers to cspm_merge_planes_host instead."""
    out, cands, masks = [], [], []
    for f, img in zip(fields, images):
        f = np.asarray(f, dtype=np.float64)
        h, w = f.shape[:2]
        xs = np.arange(w, dtype=np.float64)[None, :]
        ys = np.arange(h, dtype=np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            d = f[..., 3] * xs
            d = d + f[..., 4] * ys
            d = d + f[..., 5] * 1.0
        planes, fitted = fit(d, None, img, max_dis, **params)
        out.append(np.where(fitted[..., None] != 0, planes, f))
        cands.append(planes)
        masks.append(fitted)
    return out, cands, masks
