"""CPU restatement of the median filter, written from the specification: a clamped gather of the (2r+1)^2
window, a sort by key, then the rank.

M8(D, r), u8 with cn interleaved channels: out[y][x][c] = the element of 0-based rank 2r^2 + 2r among D[clamp(y+j)][clamp(x+i)][c],
i, j in -r .. r.  Defined for every w, h >= 1.
M64(D, r), f64: the same window; a NaN tap does not vote; a NaN centre stays (the same bits); otherwise the tap of 0-based rank
(n - 1) // 2 among the n voting taps in the order of the order-preserving 64-bit key of the bit pattern (-inf < finite < +inf,
-0.0 < +0.0).  The output is a tap's own bits.

Also the recorded cases of the reference's filter (tests/golden/refmedian_<case>.npz, written by tests/golden/make_refmedian.py) and
the compositions with the post-processing restatements.
"""
import os

import numpy as np

import pp_sub_ref as ps

MAX_RADIUS = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SIGN = np.uint64(1 << 63)
_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def gather(a, r):
    """(h, w, ...) -> (h, w, (2r+1)^2, ...): every pixel's window, row-major, coordinates clamped to the image"""
    h, w = a.shape[:2]
    ys = np.clip(np.arange(h)[:, None] + np.arange(-r, r + 1)[None, :], 0, h - 1)  # (h, side)
    xs = np.clip(np.arange(w)[:, None] + np.arange(-r, r + 1)[None, :], 0, w - 1)  # (w, side)
    win = a[ys[:, None, :, None], xs[None, :, None, :]]                             # (h, w, side, side, ...)
    return win.reshape((h, w, (2 * r + 1) ** 2) + a.shape[2:])


def median_u8(img, r):
    """M8; img (h, w) or (h, w, cn) uint8"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3) and r >= 1
    win = np.sort(gather(a, r), axis=2)
    return np.ascontiguousarray(win[:, :, 2 * r * r + 2 * r])


def f64_key(d):
    """the order-preserving 64-bit key of every f64 bit pattern"""
    u = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    return np.where(u & _SIGN != 0, ~u, u | _SIGN)


def f64_unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k & _SIGN != 0, k ^ _SIGN, ~k).view(np.float64)


def median_f64(d, r):
    """M64; d (h, w) float64"""
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert d.ndim == 2 and r >= 1
    nan = np.isnan(d)
    keys = np.where(nan, _ONES, f64_key(d))      # a NaN sorts behind every voting tap (the all-ones key is a NaN's own)
    win = np.sort(gather(keys, r), axis=2)
    votes = (~gather(nan, r)).sum(axis=2)
    rank = np.where(votes > 0, (votes - 1) // 2, 0)
    picked = np.take_along_axis(win, rank[:, :, None], axis=2)[:, :, 0]
    out = f64_unkey(picked).copy()
    out.view(np.uint64)[nan] = d.view(np.uint64)[nan]
    return out


def postprocess_f64_median(abc_l, abc_r, img_l, img_r, max_dis, r):
    """pp_sub_ref.postprocess_f64 as it is, then M64 on both maps; the masks are the unfiltered run's"""
    l, rr, lv, rv = ps.postprocess_f64(abc_l, abc_r, img_l, img_r, max_dis)
    if r > 0:
        l, rr = median_f64(l, r), median_f64(rr, r)
    return l, rr, lv, rv


def postprocess_u8_median(pm, r):
    """the 8-bit composition on an oracle PatchMatch (oracle/pyoracle.py) that holds a finished plane field: its PlaneToDisp and
    PostProcessing as they are, then M8 with one channel on both maps.  Returns (l, r) uint8."""
    pm.plane_to_disp()
    pm.postprocess()
    maps = [pm.dis(0), pm.dis(1)]
    if r > 0:
        maps = [median_u8(m, r) for m in maps]
    return maps[0], maps[1]


# ---- the recorded cases of the reference's filter: (w, h, r, channels, memsize) ----------------------------------------------------
KIB512 = 512 * 1024
CASES = [(5, 5, 2, 1, KIB512), (5, 9, 2, 1, KIB512), (15, 15, 7, 1, KIB512), (70, 33, 2, 1, KIB512), (130, 67, 1, 1, KIB512),
         (130, 67, 2, 1, KIB512), (65, 17, 7, 1, KIB512), (64, 40, 3, 3, KIB512), (300, 40, 2, 1, 544 * 40), (130, 67, 2, 1, 130 * 67)]
KINDS = ("levels", "saturated")


def case_name(w, h, r, cn, memsize, kind):
    return f"{w}x{h}_r{r}_c{cn}_m{memsize}_{kind}"


def case_input(w, h, r, cn, memsize, kind):
    """the case's input image: a 6-level map 3k + 100, k in 0 .. 5, or a saturated one drawn from {0, 15, 16, 240, 255}"""
    rng = np.random.default_rng([w, h, r, cn, memsize % 65521, KINDS.index(kind)])
    shape = (h, w) if cn == 1 else (h, w, cn)
    if kind == "levels":
        return (3 * rng.integers(0, 6, shape) + 100).astype(np.uint8)
    return np.array([0, 15, 16, 240, 255], np.uint8)[rng.integers(0, 5, shape)]


def golden_path(name):
    return os.path.join(GOLDEN, f"refmedian_{name}.npz")


def all_cases():
    return [c + (k,) for c in CASES for k in KINDS]
