"""CPU restatement of the superpixel segment planes (include/cspm.h "segment planes"), written from the
specification: the grid SLIC S(I, s, m, T) -> (labels, centres, counts) and the robust per-segment plane fit
P(D, V, labels, s, max_dis, tau, R, min_support) -> (segment planes, inliers, per-pixel planes, fitted).

Everything the specification does in integers is int64 numpy here (np.add.at, never a float accumulation), so the sums are exact
whatever the order; everything it does in f64 is one elementwise numpy operation per specified operation -- numpy rounds every
product and sum on its own and never contracts a multiply and an add.  tests/test_gpu_seg.py holds the HIP entries to these
functions with array_equal.  It never imports the GPU package."""
import numpy as np

DEFAULTS = dict(step=16, compactness=20, iters=5, tau=1.0, rounds=3, min_support=6)
EPS = 0.00000001
DET_RATIO = 1e-6
MAX_ABS_D = 32768.0


def grid(w, h, step):
    """(nx, ny, K)"""
    s = int(step)
    nx, ny = -(-int(w) // s), -(-int(h) // s)
    return nx, ny, nx * ny


def home_cells(w, h, step):
    """the home cell of every pixel: (hx, hy), each (h, w) int64"""
    s = int(step)
    nx, ny, _ = grid(w, h, s)
    hx = np.minimum(nx - 1, np.arange(w, dtype=np.int64) // s)
    hy = np.minimum(ny - 1, np.arange(h, dtype=np.int64) // s)
    return np.broadcast_to(hx[None, :], (h, w)), np.broadcast_to(hy[:, None], (h, w))


def labels_obey_3x3(labels, step):
    """every label names an existing segment whose home cell is within one cell of its pixel's"""
    labels = np.asarray(labels).astype(np.int64)
    h, w = labels.shape
    nx, ny, K = grid(w, h, step)
    hx, hy = home_cells(w, h, step)
    ok = (labels >= 0) & (labels < K)
    gx, gy = labels % nx, labels // nx
    return bool(np.all(ok & (np.abs(gx - hx) <= 1) & (np.abs(gy - hy) <= 1)))


def segment(I, step=16, compactness=20, iters=5):
    """S: I (h, w, 3) uint8 BGR.  Returns (labels (h, w) int32 of the last ASSIGN, centres (K, 5) int64 in 1/16 units
    (cx, cy, cb, cg, cr) and counts (K,) int64 of the UPDATE after it)."""
    I = np.asarray(I)
    h, w = I.shape[:2]
    s, m = int(step), int(compactness)
    nx, ny, K = grid(w, h, s)
    k = np.arange(K, dtype=np.int64)
    px = np.minimum(w - 1, (k % nx) * s + s // 2)
    py = np.minimum(h - 1, (k // nx) * s + s // 2)
    cen = np.empty((K, 5), np.int64)
    cen[:, 0], cen[:, 1] = 16 * px, 16 * py
    cen[:, 2:] = 16 * I[py, px].astype(np.int64)
    val = np.empty((h, w, 5), np.int64)  # 16 * (x, y, B, G, R)
    val[..., 0] = 16 * np.arange(w, dtype=np.int64)[None, :]
    val[..., 1] = 16 * np.arange(h, dtype=np.int64)[:, None]
    val[..., 2:] = 16 * I.astype(np.int64)
    hx, hy = home_cells(w, h, s)
    labels = np.full((h, w), -1, np.int64)
    counts = np.zeros(K, np.int64)
    for _ in range(int(iters)):
        best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
        labels = np.full((h, w), -1, np.int64)
        for dy in (-1, 0, 1):          # gy outer, gx inner, ascending
            for dx in (-1, 0, 1):
                gx, gy = hx + dx, hy + dy
                exists = (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny)
                kk = np.where(exists, gy * nx + gx, 0)
                d = val - cen[kk]
                dc = d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3] + d[..., 4] * d[..., 4]
                ds = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
                dist = dc * (s * s) + ds * (m * m)
                take = exists & (dist < best)  # the first candidate with the strictly smallest Dist
                best = np.where(take, dist, best)
                labels = np.where(take, kk, labels)
        flat = labels.ravel()
        counts = np.bincount(flat, minlength=K).astype(np.int64)
        sums = np.zeros((K, 5), np.int64)
        np.add.at(sums, flat, val.reshape(-1, 5))
        n = counts[:, None]
        cen = np.where(n > 0, (2 * sums + n) // (2 * np.maximum(n, 1)), cen)
    return labels.astype(np.int32), cen, counts


def _solve(S, min_support):
    """the cofactor solve of cspm_fit_planes on the nine sums (K, 9) int64: (a, b, c0, good)"""
    Sw, Su, Sv, Suu, Suv, Svv, Se, Sue, Sve = (S[:, i].astype(np.float64) for i in range(9))  # each sum converted once
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        C00 = Svv * Sw - Sv * Sv
        C01 = Suv * Sw - Sv * Su
        C02 = Suv * Sv - Svv * Su
        C11 = Suu * Sw - Su * Su
        C12 = Suu * Sv - Suv * Su
        C22 = Suu * Svv - Suv * Suv
        det = (Suu * C00 - Suv * C01) + Su * C02
        good = (S[:, 0] >= min_support) & (det > DET_RATIO * ((Suu * Svv) * Sw))
        safe = np.where(good, det, 1.0)
        scale = 2.0 ** -16
        a = (((C00 * Sue - C01 * Sve) + C02 * Se) / safe) * scale
        b = (((C11 * Sve - C01 * Sue) - C12 * Se) / safe) * scale
        c0 = (((C02 * Sue - C12 * Sve) + C22 * Se) / safe) * scale
    return a, b, c0, good


def fit_segments(D, V, labels, step=16, max_dis=0, tau=1.0, rounds=3, min_support=6, **_):
    """P: D (h, w) f64, V (h, w) or None, labels (h, w) obeying the 3 x 3 property.  Returns (seg_planes (K, 3) f64 (a, b, c), NaN for an
    unfitted segment; inliers (K,) int32, 0 for an unfitted segment; planes (h, w, 6) in the layout of cspm_get_planes; fitted (h, w)
    uint8)."""
    D = np.asarray(D, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    h, w = D.shape
    s, R = int(step), int(rounds)
    assert labels.shape == D.shape and labels_obey_3x3(labels, s)
    nx, ny, K = grid(w, h, s)
    with np.errstate(invalid="ignore"):
        node = np.abs(D) <= MAX_ABS_D  # false for NaN and inf
    if V is not None:
        node &= np.asarray(V) != 0
    ox = (labels % nx) * s
    oy = (labels // nx) * s
    u = np.arange(w, dtype=np.int64)[None, :] - ox
    v = np.arange(h, dtype=np.int64)[:, None] - oy
    uf, vf = u.astype(np.float64), v.astype(np.float64)
    q = np.zeros((h, w), np.int64)
    q[node] = np.rint(D[node] * 65536.0).astype(np.int64)
    one = np.ones((h, w), np.int64)
    terms = np.stack([one, u, v, u * u, u * v, v * v, q, u * q, v * q], axis=-1)

    def sums(sel):
        S = np.zeros((K, 9), np.int64)
        np.add.at(S, labels[sel], terms[sel])
        return S

    S = sums(node)  # round 0: every member node
    a, b, c0, good = _solve(S, min_support)
    fitted = good.copy()
    active = good.copy()
    a, b, c0 = np.where(good, a, 0.0), np.where(good, b, 0.0), np.where(good, c0, 0.0)
    inl = np.where(good, S[:, 0], 0)
    for r in range(1, R + 1):
        thr = float(tau) * float(2 ** (R - r))
        with np.errstate(invalid="ignore", over="ignore"):
            res = np.abs(D - ((a[labels] * uf + b[labels] * vf) + c0[labels]))
            sel = node & active[labels] & (res <= thr)
        S = sums(sel)
        na, nb, nc0, good = _solve(S, min_support)
        good &= active
        a, b, c0 = np.where(good, na, a), np.where(good, nb, b), np.where(good, nc0, c0)
        inl = np.where(good, S[:, 0], inl)
        active = good  # a degenerate later round stops and keeps the previous plane
    kk = np.arange(K, dtype=np.int64)
    sox, soy = ((kk % nx) * s).astype(np.float64), ((kk // nx) * s).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (c0 - a * sox) - b * soy
    seg_planes = np.where(fitted[:, None], np.stack([a, b, c], axis=-1), np.nan)

    pa_, pb_, pc0 = a[labels], b[labels], c0[labels]
    xs = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    ys = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (pa_ * uf + pb_ * vf) + pc0
        z = np.where(t > 0.0, t, 0.0)
        z = np.where(z < float(max_dis), z, float(max_dis))
        m0, m1, m2 = -pa_, -pb_, np.ones((h, w))
        sq = m0 * m0
        sq = sq + m1 * m1
        sq = sq + m2 * m2
        inv = 1.0 / np.maximum(np.sqrt(sq), EPS)
        nxn, nyn, nzn = m0 * inv, m1 * inv, m2 * inv
        denom = np.maximum(np.abs(nzn), EPS)  # Plane::update_param
        denom = np.where(nzn < 0.0, -denom, denom)
        pa = -nxn / denom
        pb = -nyn / denom
        sq = nxn * xs
        sq = sq + nyn * ys
        sq = sq + nzn * z
        pc = sq / denom
    planes = np.stack([nxn, nyn, nzn, pa, pb, pc], axis=-1)
    pix_fitted = fitted[labels]
    planes[~pix_fitted] = np.nan
    return seg_planes, inl.astype(np.int32), planes, pix_fitted.astype(np.uint8)


def segment_planes_fields(fields, images, max_dis, **params):
    """cspm_segment_planes on both views: fields[v] (h, w, 6), images[v] the level-0 BGR image.  D is the stored field's a*x + b*y + c
    in the order of cspm_get_disparity_f64, V all 1.  Returns (replaced, candidates, masks, labels) per view: the field with the
    planes of fitted segments replaced (merge = 0), and what merge = 1 offers to cspm_merge_planes_host instead."""
    p = {**DEFAULTS, **params}
    out, cands, masks, labs = [], [], [], []
    for f, img in zip(fields, images):
        f = np.asarray(f, dtype=np.float64)
        h, w = f.shape[:2]
        xs = np.arange(w, dtype=np.float64)[None, :]
        ys = np.arange(h, dtype=np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            d = f[..., 3] * xs
            d = d + f[..., 4] * ys
            d = d + f[..., 5] * 1.0
        labels, _, _ = segment(img, p["step"], p["compactness"], p["iters"])
        _, _, planes, fitted = fit_segments(d, None, labels, p["step"], max_dis, p["tau"], p["rounds"], p["min_support"])
        out.append(np.where(fitted[..., None] != 0, planes, f))
        cands.append(planes)
        masks.append(fitted)
        labs.append(labels)
    return out, cands, masks, labs
