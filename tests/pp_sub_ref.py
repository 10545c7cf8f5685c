"""CPU restatement of the sub-pixel PostProcessing, written from the specification.

Every f64 sum the specification orders is a serial chain here too: np.cumsum adds left to right and np.add.at applies its updates
one by one in index order (np.sum / np.add.reduce are pairwise and are not used).  numpy does not contract a multiply and an add.
Vectorised per row (check, fill) and per inconsistent pixel (median): a 741x500 pair takes seconds.
"""
import math

import numpy as np

WND = 35            # WeightedMedian's window
THRESH = 0.5        # LeftRightCheck's threshold
LUT = np.array([math.exp(-i * 1.0 / 10.0) for i in range(766)])  # WMF_GAMMA = 10; libm, like the library's table

_MAGIC = 6755399441055744.0


def round2int(d):
    """commfunc.h Round2Int: the low 32 bits of d + 1.5 * 2^52, as a signed integer (round half to even)"""
    s = np.ascontiguousarray(np.asarray(d, np.float64) + _MAGIC)
    return (s.view(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)


def plane_disp(abc):
    """d(x, y) of a (h, w, 3) field of (a, b, c) at every pixel's own position: a*x, += b*y, += c*1.0"""
    h, w = abc.shape[:2]
    return plane_disp_at(abc[..., 0], abc[..., 1], abc[..., 2], np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None])


def plane_disp_at(a, b, c, x, y):
    d = a * x
    d = d + b * y
    d = d + c * 1.0
    return d


def lr_check(d, v):
    """step 1: the consistency masks; d = [d_left, d_right] raw maps"""
    h, w = d[v].shape
    x = np.arange(w, dtype=np.int64)[None, :]
    ox = x + (2 * v - 1) * round2int(d[v])
    inside = (ox >= 0) & (ox < w)
    other = np.take_along_axis(d[1 - v], np.clip(ox, 0, w - 1), axis=1)
    return inside & (np.abs(d[v] - other) <= THRESH) & (d[v] > 0.0)


def fill(abc, d, valid, max_dis):
    """step 2: inconsistent pixels take the plane of the nearest consistent column of their row, evaluated at the pixel"""
    h, w = d.shape
    cols = np.broadcast_to(np.arange(w, dtype=np.int64)[None, :], (h, w))
    left = np.maximum.accumulate(np.where(valid, cols, -1), axis=1)                          # -1: none
    right = np.minimum.accumulate(np.where(valid, cols, w)[:, ::-1], axis=1)[:, ::-1]         # w: none
    xs = cols.astype(np.float64)
    ys = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    rows = np.broadcast_to(np.arange(h)[:, None], (h, w))

    def at(col):
        cc = np.clip(col, 0, w - 1)
        return plane_disp_at(abc[rows, cc, 0], abc[rows, cc, 1], abc[rows, cc, 2], xs, ys)

    dl, dr = at(left), at(right)
    has_l, has_r = left >= 0, right < w
    cand = np.where(has_l & has_r, np.where(dl <= dr, dl, dr), np.where(has_l, dl, dr))
    cand = np.where(cand < 0.0, 0.0, np.where(cand > float(max_dis), float(max_dis), cand))
    out = d.copy()
    hole = ~valid & (has_l | has_r)
    out[hole] = cand[hole]
    return out


def weighted_median_pixel(vals, wgts):
    """step 3 for one pixel: vals / wgts = the window's contributions in window order.  Returns None without a contribution."""
    if len(vals) == 0:
        return None
    sum_wgt = np.cumsum(wgts)[-1]
    median_wgt = sum_wgt / 2.0
    if not median_wgt > 0.0:
        return None
    uniq, inv = np.unique(vals, return_inverse=True)  # ascending distinct values (all > 0: like their bit patterns)
    bins = np.zeros(len(uniq))
    np.add.at(bins, inv.ravel(), wgts)                # each bin: its weights in window order, one by one
    run = np.cumsum(bins)                             # 0.0 + bin == bin
    hit = np.nonzero(run >= median_wgt)[0]
    return uniq[hit[0]] if len(hit) else None


def weighted_median(img, d_raw, filled, valid):
    h, w = d_raw.shape
    half = WND // 2
    col = img.astype(np.int64)
    out = filled.copy()
    for y, x in zip(*np.nonzero(~valid)):
        y0, y1, x0, x1 = max(0, y - half), min(h, y + half + 1), max(0, x - half), min(w, x + half + 1)
        m = valid[y0:y1, x0:x1]
        if not m.any():
            continue
        sad = np.abs(col[y0:y1, x0:x1] - col[y, x]).sum(axis=2)
        u = weighted_median_pixel(d_raw[y0:y1, x0:x1][m], LUT[sad[m]])  # boolean indexing keeps row-major = window order
        if u is not None:
            out[y, x] = u
    return out


def postprocess_f64(abc_l, abc_r, img_l, img_r, max_dis):
    """abc_v: (h, w, 3) plane parameters (a, b, c); img_v: (h, w, 3) u8 BGR.  Returns (l, r, l_valid, r_valid): f64 maps, u8 masks."""
    abc = [np.ascontiguousarray(abc_l, dtype=np.float64), np.ascontiguousarray(abc_r, dtype=np.float64)]
    img = [np.asarray(img_l), np.asarray(img_r)]
    d = [plane_disp(abc[0]), plane_disp(abc[1])]
    valid = [lr_check(d, v) for v in (0, 1)]
    out = []
    for v in (0, 1):
        filled = fill(abc[v], d[v], valid[v], max_dis)
        out.append(weighted_median(img[v], d[v], filled, valid[v]))
    return out[0], out[1], valid[0].astype(np.uint8), valid[1].astype(np.uint8)


def fronto_field(disp):
    """(h, w, 3) plane parameters of a fronto-parallel field with the given disparities"""
    disp = np.asarray(disp, dtype=np.float64)
    abc = np.zeros(disp.shape + (3,))
    abc[..., 2] = disp
    return abc
