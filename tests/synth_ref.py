"""Specification N of DESIGN.md section 20 (include/cspm.h "view synthesis") restated on the CPU, twice:
synthesize_loop -- one pixel at a time in Python floats, line by line as the specification writes it;
synthesize      -- numpy over whole maps with the same association (candidates sorted instead of depth-tested).
Every product, sum and quotient is one IEEE f64 operation (Python floats and numpy f64 never contract)."""
import math

import numpy as np

DEFAULTS = dict(views=3, max_stretch=4.0, merge_diff=1.0, fill=1)
NAN = float("nan")
_MAGIC = 6755399441055744.0  # Round2Int: round half to even by the magic-number sum


def check_args(t, w, h, views=3, max_stretch=4.0, merge_diff=1.0, fill=1, strides=(), **_):
    """the validity rules of N's scalar arguments: True when an entry would accept them"""
    if not (0.0 <= t <= 1.0) or views not in (1, 2, 3):
        return False
    if not max_stretch >= 1.0 or not merge_diff >= 0.0:
        return False
    if w < 1 or h < 1 or w * h >= 2 ** 31:
        return False
    return all(s >= 3 * w for s in strides)


def sigmas(t):
    t = float(t)
    return (-t, 1.0 - t)


def f64_key(d):
    """the order-preserving 64-bit key of f64 bit patterns: -inf < finite < +inf, -0.0 < +0.0"""
    b = np.asarray(d, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def _round_u8(c):
    """saturated Round2Int of an f64 colour"""
    r = int(np.float64(c + _MAGIC).view(np.int64) & 0xFFFFFFFF)
    if r >= 1 << 31:
        r -= 1 << 32
    return min(max(r, 0), 255)


# ---- the per-pixel restatement ------------------------------------------------------------------------------------------------------
def _source(x, D, V, A, sigma, max_stretch, w):
    """step 1 for one source pixel -> None or (D, a, g, u, hi, first)"""
    D = float(D)
    if V == 0 or not math.isfinite(D) or not D >= 0.0:
        return None
    a = float(A) if math.isfinite(A) else 0.0
    g = 1.0 + sigma * a
    if not (g > 0.0 and g <= max_stretch):
        return None
    u = float(x) + sigma * D
    half = 0.5 * g
    lo = u - half
    hi = u + half
    if not lo <= float(w - 1):
        return None
    first = 0 if lo <= 0.0 else int(math.ceil(lo))
    return D, a, g, u, hi, first


def _at(src, x, xp):
    D, a, g, u, hi, first = src
    xs = float(x) + (float(xp) - u) / g
    dp = D + a * (xs - float(x))
    return xs, dp


def _key1(d):
    return int(f64_key(np.float64(d)))


def synthesize_loop(t, D, V, A, I, views=3, max_stretch=4.0, merge_diff=1.0, fill=1):
    """D, V, A, I: pairs (view 0, view 1); D[v] (h, w) f64, V[v] (h, w) or None, A[v] (h, w) f64 or None, I[v] (h, w, 3) uint8; the
    entries of a view that `views` does not name may be None.  -> dict(bgr (h, w, 3) uint8, disp (h, w) f64, mask (h, w) uint8,
    holes = the mask before the fill, colour (h, w, 3) = the f64 colour before rounding and before the fill, NaN in holes)"""
    v_any = 0 if views & 1 else 1
    h, w = np.asarray(D[v_any]).shape
    sg = sigmas(t)
    w0, w1 = 1.0 - float(t), float(t)
    bgr = np.zeros((h, w, 3), np.uint8)
    disp = np.full((h, w), np.nan)
    mask = np.zeros((h, w), np.uint8)
    colour = np.full((h, w, 3), np.nan)
    for y in range(h):
        best = [[None] * w, [None] * w]  # per view and target column: (key of d', -x) -> greatest wins
        for v in (0, 1):
            if not views >> v & 1:
                continue
            for x in range(w):
                src = _source(x, D[v][y, x], 1 if V[v] is None else V[v][y, x], 0.0 if A[v] is None else A[v][y, x], sg[v], max_stretch, w)
                if src is None:
                    continue
                xp = src[5]
                while xp < w and float(xp) < src[4]:
                    xs, dp = _at(src, x, xp)
                    cand = (_key1(dp), -x, xs, dp)
                    if best[v][xp] is None or cand[:2] > best[v][xp][:2]:
                        best[v][xp] = cand
                    xp += 1
        for xp in range(w):
            Z, C = [None, None], [None, None]
            for v in (0, 1):
                if best[v][xp] is None:
                    continue
                _, _, xs, dp = best[v][xp]
                i0 = math.floor(xs)
                f = xs - float(i0)
                ia, ib = min(max(i0, 0), w - 1), min(max(i0 + 1, 0), w - 1)
                fa = 1.0 - f
                C[v] = [fa * float(I[v][y, ia, ch]) + f * float(I[v][y, ib, ch]) for ch in range(3)]
                Z[v] = dp
            if Z[0] is not None and Z[1] is not None:
                if abs(Z[0] - Z[1]) <= merge_diff:
                    m, Zm, Cm = 3, w0 * Z[0] + w1 * Z[1], [w0 * C[0][ch] + w1 * C[1][ch] for ch in range(3)]
                elif Z[0] >= Z[1]:
                    m, Zm, Cm = 1, Z[0], C[0]
                else:
                    m, Zm, Cm = 2, Z[1], C[1]
            elif Z[0] is not None:
                m, Zm, Cm = 1, Z[0], C[0]
            elif Z[1] is not None:
                m, Zm, Cm = 2, Z[1], C[1]
            else:
                continue
            mask[y, xp], disp[y, xp] = m, Zm
            bgr[y, xp] = [_round_u8(c) for c in Cm]
            colour[y, xp] = Cm
    holes = mask.copy()
    if fill:
        for y in range(h):
            for xp in range(w):
                if holes[y, xp] != 0:
                    continue
                L = next((i for i in range(xp - 1, -1, -1) if holes[y, i] != 0), None)
                R = next((i for i in range(xp + 1, w) if holes[y, i] != 0), None)
                if L is None and R is None:
                    continue
                src = L
                if L is None or (R is not None and disp[y, R] < disp[y, L]):
                    src = R
                bgr[y, xp], disp[y, xp], mask[y, xp] = bgr[y, src], disp[y, src], 4
    return dict(bgr=bgr, disp=disp, mask=mask, holes=holes, colour=colour)


# ---- the vectorised restatement -----------------------------------------------------------------------------------------------------
def _view_winners(D, V, A, sigma, max_stretch, ties=None):
    """steps 1 and 2 of one view -> (have (h, w) bool, xs (h, w), Z (h, w)); ties: a list that receives the number of target pixels
    whose two best candidates have bit-equal d' (the tie rule decided them)"""
    D = np.asarray(D, np.float64)
    h, w = D.shape
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    with np.errstate(all="ignore"):
        usable = np.isfinite(D) & (D >= 0.0)
        if V is not None:
            usable &= np.asarray(V) != 0
        a = np.zeros((h, w)) if A is None else np.asarray(A, np.float64)
        a = np.where(np.isfinite(a), a, 0.0)
        g = 1.0 + sigma * a
        u = x + sigma * D
        half = 0.5 * g
        lo = u - half
        hi = u + half
        used = usable & (g > 0.0) & (g <= max_stretch) & (lo <= float(w - 1))
        first = np.where(used, np.where(lo <= 0.0, 0.0, np.ceil(np.where(used, lo, 0.0))), float(w))
        cells, keys, xsrc, xss, dps = [], [], [], [], []
        rows = np.broadcast_to(np.arange(h)[:, None], (h, w))
        k = 0
        while True:
            xp = first + float(k)
            ok = used & (xp < float(w)) & (xp < hi)
            if not ok.any():
                break
            xs = x + (xp - u) / g
            dp = D + a * (xs - x)
            cells.append((rows[ok] * w + xp[ok].astype(np.int64)))
            keys.append(f64_key(dp[ok]))
            xsrc.append(x[ok].astype(np.int64))
            xss.append(xs[ok])
            dps.append(dp[ok])
            k += 1
    have = np.zeros(h * w, bool)
    XS = np.zeros(h * w)
    Z = np.zeros(h * w)
    if cells:
        cells, keys, xsrc, xss, dps = (np.concatenate(q) for q in (cells, keys, xsrc, xss, dps))
        order = np.lexsort((xsrc, ~keys, cells))  # by cell, then the greatest key, then the smallest source x
        cs = cells[order]
        lead = np.ones(len(cs), bool)
        lead[1:] = cs[1:] != cs[:-1]
        sel = order[lead]
        if ties is not None:
            ks = keys[order]
            ties.append(int(np.sum(~lead[1:] & lead[:-1] & (ks[1:] == ks[:-1]))))
        have[cells[sel]] = True
        XS[cells[sel]] = xss[sel]
        Z[cells[sel]] = dps[sel]
    return have.reshape(h, w), XS.reshape(h, w), Z.reshape(h, w)


def _colour(I, xs):
    h, w = xs.shape
    i0 = np.floor(xs)
    f = xs - i0
    ia = np.clip(i0, 0, w - 1).astype(np.int64)
    ib = np.clip(i0 + 1.0, 0, w - 1).astype(np.int64)
    rows = np.arange(h)[:, None]
    Ia = np.asarray(I)[rows, ia].astype(np.float64)
    Ib = np.asarray(I)[rows, ib].astype(np.float64)
    return (1.0 - f)[..., None] * Ia + f[..., None] * Ib


def synthesize(t, D, V, A, I, views=3, max_stretch=4.0, merge_diff=1.0, fill=1, ties=None):
    """the same arguments and results as synthesize_loop; ties: see _view_winners"""
    v_any = 0 if views & 1 else 1
    h, w = np.asarray(D[v_any]).shape
    sg = sigmas(t)
    w0, w1 = np.float64(1.0 - float(t)), np.float64(t)
    have, Z, C = [], [], []
    for v in (0, 1):
        if views >> v & 1:
            hv, xs, z = _view_winners(D[v], V[v], A[v], sg[v], max_stretch, ties)
            have.append(hv), Z.append(z), C.append(_colour(I[v], xs))
        else:
            have.append(np.zeros((h, w), bool)), Z.append(np.zeros((h, w))), C.append(np.zeros((h, w, 3)))
    with np.errstate(all="ignore"):
        both = have[0] & have[1]
        close = both & (np.abs(Z[0] - Z[1]) <= merge_diff)
        one = np.where(both, Z[0] >= Z[1], have[0])  # view 0 alone
        mask = np.where(close, 3, np.where(have[0] | have[1], np.where(one, 1, 2), 0)).astype(np.uint8)
        Zm = np.where(close, w0 * Z[0] + w1 * Z[1], np.where(one, Z[0], Z[1]))
        Cm = np.where(close[..., None], w0 * C[0] + w1 * C[1], np.where(one[..., None], C[0], C[1]))
    disp = np.where(mask != 0, Zm, np.nan)
    bgr = np.where((mask != 0)[..., None], np.clip(np.rint(Cm), 0, 255), 0).astype(np.uint8)  # rint = round half to even = Round2Int here
    holes = mask.copy()
    colour = np.where((mask != 0)[..., None], Cm, np.nan)
    if fill:
        idx = np.broadcast_to(np.arange(w)[None, :], (h, w))
        L = np.maximum.accumulate(np.where(holes != 0, idx, -1), axis=1)
        R = np.minimum.accumulate(np.where(holes != 0, idx, w)[:, ::-1], axis=1)[:, ::-1]
        rows = np.broadcast_to(np.arange(h)[:, None], (h, w))
        hasL, hasR = L >= 0, R < w
        Lc, Rc = np.clip(L, 0, w - 1), np.clip(R, 0, w - 1)
        with np.errstate(all="ignore"):
            right = hasR & (~hasL | (disp[rows, Rc] < disp[rows, Lc]))
        src = np.where(right, Rc, Lc)
        todo = (holes == 0) & (hasL | hasR)
        bgr = np.where(todo[..., None], bgr[rows, src], bgr)
        disp = np.where(todo, disp[rows, src], disp)
        mask = np.where(todo, 4, mask).astype(np.uint8)
    return dict(bgr=bgr, disp=disp, mask=mask, holes=holes, colour=colour)


def same_bits(a, b):
    """equal as bit patterns except that any NaN equals any NaN (payloads are not part of N); -0.0 differs from +0.0"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    ints = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(ints)[~na], b.view(ints)[~nb]))


def same_result(a, b):
    return all(same_bits(a[k], b[k]) for k in ("bgr", "disp", "mask"))


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 5), (63, 3), (64, 4), (65, 5), (255, 1), (256, 1), (257, 1), (130, 67)]
TS = (0.0, 0.25, 0.5, 1.0)


def random_case(w, h, seed, dmax=40.0):
    """a random pair of inputs: disparities in [0, dmax] in smooth runs with jumps, half of them dyadic; view 1's map is view 0's warped
    into view 1 (so that the two views agree on much of the target) with noise, random where nothing lands; then NaN, +-inf, negative and
    V = 0 holes; slopes in +-0.3 plus non-finite and steep ones; random images -> (D, V, A, I), each a pair"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, dmax, (h, 1)) + np.cumsum(rng.uniform(-0.6, 0.6, (h, w)), axis=1)
    steps = np.cumsum(rng.random((h, w)) < 0.08, axis=1) * rng.uniform(-6.0, 6.0)
    d0 = np.clip(base + steps, 0.0, dmax)
    d1 = rng.uniform(0.0, dmax, (h, w))
    for y in range(h):
        best = np.full(w, -1.0)
        for x in range(w):
            xr = int(round(x - d0[y, x]))
            if 0 <= xr < w and d0[y, x] > best[xr]:
                best[xr] = d0[y, x]
        d1[y] = np.where(best >= 0.0, np.clip(best + rng.uniform(-0.7, 0.7, w), 0.0, dmax), d1[y])
    D, V, A, I = [], [], [], []
    for v, d in enumerate((d0, d1)):
        dyadic = rng.random((h, w)) < 0.5
        d = np.where(dyadic, np.round(d * 4.0) / 4.0, d)
        r = rng.random((h, w))
        d = np.where(r < 0.02, np.nan, d)
        d = np.where((r >= 0.02) & (r < 0.03), np.inf, d)
        d = np.where((r >= 0.03) & (r < 0.04), -np.inf, d)
        d = np.where((r >= 0.04) & (r < 0.06), -d - 0.5, d)
        a = rng.uniform(-0.3, 0.3, (h, w))
        r = rng.random((h, w))
        a = np.where(r < 0.03, np.nan, a)
        a = np.where((r >= 0.03) & (r < 0.05), np.inf, a)
        a = np.where((r >= 0.05) & (r < 0.10), rng.uniform(-12.0, 12.0, (h, w)), a)
        D.append(d), A.append(a)
        V.append((rng.random((h, w)) >= 0.15).astype(np.uint8))
        I.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return D, V, A, I


def shape_case(shape):
    """the random case the CPU and the GPU tests use for a shape (the seed is a function of the shape)"""
    w, h = shape
    return random_case(w, h, 1000 + 7 * w + h)


# planes (a, c) whose rendering at t = 1 from view 0 (D = a x + c over 200 columns, A = a) contains target pixels that two neighbouring
# source pixels claim with bit-equal d': found by a random search over two-decimal values, kept because the tie rule needs a case
TIE_PLANES = [(-0.94, 208.19), (-1.76, 367.14), (-0.66, 163.15), (-0.72, 181.1), (-1.7, 370.95), (-0.16, 43.66), (-0.38, 121.31)]


def tie_case():
    """-> (D, A, I): one row per TIE_PLANES entry, 200 columns, a random image"""
    w = 200
    x = np.arange(w, dtype=np.float64)[None, :]
    D = np.concatenate([a * x + c for a, c in TIE_PLANES])
    A = np.concatenate([np.full((1, w), a) for a, _ in TIE_PLANES])
    I = np.random.default_rng(12).integers(0, 256, (len(TIE_PLANES), w, 3), dtype=np.uint8)
    return D, A, I
