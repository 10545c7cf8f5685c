"""The chain engine's choice of code path in a raster sweep, restated on the CPU (csrc/cspm_chain.h): per pyramid level and candidate pair
the window geometry of make_chain_level and the all-valid decision of chain_passes (the four window corners of EVERY candidate inside
[1 + 2^-20, D_s - 2^-20] -> chain_tap_value<SRC, true>, no clamp, no validity test, no select; otherwise both candidates take the general
taps), and per sweep pixel the LEAF of sweep_candidates and of the three-way dispatch behind it, from the field before the sweep, the
field after it, the direction and the trust flag.  CASES are small plane fields BUILT to take every one of those leaves on purpose:

 (a) "emitter / probe" fields, trust 0: pixels with (x + y) even are emitters (stored cost -1: they never accept and keep their built
     plane), pixels with (x + y) odd are probes (stored cost 1e300: they accept the better of their candidates and store its exact cost).
     Both predecessors of a probe are emitters, in both sweep directions, so a probe's candidate pair is what the builder wrote.  The
     emitters of an anti-diagonal x + y = 2u share one recipe (A, B): those in odd columns hold A, those in even columns B.  The probes
     between two emitter diagonals see (A, B) in even columns and (B, A) in odd ones -- every recipe is met with its slots swapped.
 (b) "block" fields, trust 1 and trust 0: piecewise constant fields of rectangles and stripes at least two pixels wide, in which the left
     predecessor, the upper one, both or neither hold the pixel's own plane bit for bit.

tests/test_chain_path_ref.py holds the table non-vacuous on the CPU (with the oracle's costs, tests/chain_cases.py),
tests/test_gpu_chain_paths.py holds the device to the oracle on it.  This file imports neither the GPU package nor the oracle.

Plain numpy arithmetic restates the corner test (the device forms the corners with one fma each): the builder asserts that every corner
value of every built candidate stays 2^-30 away from both thresholds (GUARD), so one rounding cannot change a classification."""
import collections

import numpy as np

import rows_path_ref as rp

Geom = rp.Geom  # w h max_dis wnd scale_num (0: single scale, the stored a, b, c)
K_ROW_MOD, K_CHAIN_ROWS = 7, 9
EPS20, GUARD = 2.0 ** -20, 2.0 ** -30
EMITTER_COST, PROBE_COST = -1.0, 1e300

# ---- make_chain_level and the all-valid decision ----------------------------------------------------------------------------------

Window = collections.namedtuple("Window", "level W H D cx cy r_lo nrows passes nsteps has_valid x0 x1 y0 y1")


def level_windows(g, x, y):
    """make_chain_level at every level for the window centred on pixel (x, y): first window row inside the image, rows inside, chain
    passes (9 rows each), steps (7 columns each), and the columns / rows the corner test uses (x1 covers the last step's masked taps)"""
    half = g.wnd // 2
    n = 2 * half + 1
    out, cx, cy = [], int(x), int(y)
    for s, (W, H, D) in enumerate(rp.level_dims(g)):
        ox0, oy0 = cx - half, cy - half
        r_lo = max(0, -oy0)
        nrows = min(n - 1, H - 1 - oy0) - r_lo + 1
        nsteps = (n + K_ROW_MOD - 1) // K_ROW_MOD
        out.append(Window(s, W, H, D, cx, cy, r_lo, nrows, (nrows + K_CHAIN_ROWS - 1) // K_CHAIN_ROWS, nsteps, D >= 2,
                          ox0, ox0 + K_ROW_MOD * nsteps - 1, oy0 + r_lo, oy0 + r_lo + nrows - 1))
        cx, cy = cx // 2, cy // 2
    return out


Level = collections.namedtuple("Level", "D has_valid ok qmin qmax guard")


def classify(g, xs, ys, planes):
    """planes (N, 6) norm+param, each evaluated as a candidate at pixel (xs[i], ys[i]).  Per level: `ok` -- the candidate's four corners
    lie inside [1 + 2^-20, D - 2^-20] and the level has a valid disparity at all; qmin / qmax over the corners; guard -- the corners'
    smallest distance from either threshold (inf where the level takes no decision).  The per-level plane: eval_pixel_pair's
    plane_param at the halved centre and disparity (pre_cs_pc.cc:139-149,183-185)."""
    P = np.asarray(planes, np.float64).reshape(-1, 6)
    nx, ny, nz, pa, pb, pc = (np.ascontiguousarray(P[:, k]) for k in range(6))
    cx, cy = np.asarray(xs, np.int64).copy(), np.asarray(ys, np.int64).copy()
    half = g.wnd // 2
    n = 2 * half + 1
    nsteps = (n + K_ROW_MOD - 1) // K_ROW_MOD
    out = []
    with np.errstate(all="ignore"):
        cur = pa * cx + pb * cy + pc
        for W, H, D in rp.level_dims(g):
            a, b, c = rp.plane_param(nx, ny, nz, cx.astype(np.float64), cy.astype(np.float64), cur) if g.scale_num else (pa, pb, pc)
            ox0, oy0 = cx - half, cy - half
            r_lo = np.maximum(0, -oy0)
            nrows = np.minimum(n - 1, H - 1 - oy0) - r_lo + 1
            x0, x1 = ox0.astype(np.float64), (ox0 + K_ROW_MOD * nsteps - 1).astype(np.float64)
            y0, y1 = (oy0 + r_lo).astype(np.float64), (oy0 + r_lo + nrows - 1).astype(np.float64)
            t0, t1 = b * y0 + c, b * y1 + c
            q = np.stack([a * x0 + t0, a * x1 + t0, a * x0 + t1, a * x1 + t1])
            qmin, qmax = np.fmin.reduce(q), np.fmax.reduce(q)
            lo, hi = 1.0 + EPS20, float(D) - EPS20
            ok = (qmin >= lo) & (qmax <= hi) & (D >= 2)
            guard = np.minimum(np.abs(q - lo), np.abs(q - hi)).min(0) if D >= 2 else np.full(len(P), np.inf)
            assert not np.isnan(q).any(), "a built plane gives a NaN corner"
            out.append(Level(D, D >= 2, ok, qmin, qmax, guard))
            cur, cx, cy = cur / 2.0, cx // 2, cy // 2
    return out


def level_paths(g, x, y, cands):
    """the path of every level for the candidates `cands` (one or two (6,) planes) evaluated together at (x, y): ["allv" | "general: why"]"""
    per = [classify(g, [x], [y], c) for c in cands]
    out = []
    for s in range(len(per[0])):
        if not per[0][s].has_valid:
            out.append(f"general: D = {per[0][s].D} < 2")
            continue
        bad = [f"candidate {k} leaves [1 + 2^-20, {per[0][s].D} - 2^-20] (corners {p[s].qmin[0]!r} .. {p[s].qmax[0]!r})" for k, p in enumerate(per) if not p[s].ok[0]]
        out.append("general: " + "; ".join(bad) if bad else "allv")
    return out


# ---- sweep_candidates and the dispatch --------------------------------------------------------------------------------------------

LEAVES = ["corner", "row/eval", "row/own", "col/eval", "col/own", "pair", "same01", "own0", "own1", "own0+own1"]
CORNER, ROW_EVAL, ROW_OWN, COL_EVAL, COL_OWN, PAIR, SAME01, OWN0, OWN1, OWN01 = range(10)
# what the dispatch behind sweep_candidates runs: eval0 && eval1 (chain_passes<SRC, 2>), eval0 alone, eval1 alone (chain_passes<SRC, 1>,
# the costs swapped), nothing.  own0 && own1 is `own` together with same01: == is transitive, either two of the three give the third
DISPATCH = {CORNER: "none", ROW_EVAL: "eval0", ROW_OWN: "none", COL_EVAL: "eval1", COL_OWN: "none", PAIR: "eval0 && eval1", SAME01: "eval0",
            OWN0: "eval1", OWN1: "eval0", OWN01: "none"}


def leaf_name(leaf):
    return f"{LEAVES[leaf]} [{DISPATCH[leaf]}]"


def _shift(F, inc, axis):
    """the field of the predecessors along `axis` (1: x, 0: y) in sweep direction inc; the first sweep row / column gets garbage that
    have0 / have1 mask"""
    return np.roll(F, inc, axis=axis)


def sweep_leaves(F, F2, inc, trust):
    """F (h, w, 6): the field before the sweep, F2: after it (a pixel's candidates are its predecessors' FINAL planes), inc +1 / -1,
    trust: Pm::trust_cost.  Returns (leaf (h, w), c0 (h, w, 6), c1 (h, w, 6), same_bits (h, w)): sweep_candidates' slots -- with one
    predecessor missing both hold the other -- and whether the two slots agree bit for bit (same01 is ==: +0.0 equals -0.0)."""
    F, F2 = np.asarray(F, np.float64), np.asarray(F2, np.float64)
    h, w = F.shape[:2]
    xs = np.arange(w) if inc > 0 else w - 1 - np.arange(w)  # sweep coordinates
    ys = np.arange(h) if inc > 0 else h - 1 - np.arange(h)
    have0 = np.broadcast_to((xs > 0)[None, :], (h, w))
    have1 = np.broadcast_to((ys > 0)[:, None], (h, w))
    px, py = _shift(F2, inc, 1), _shift(F2, inc, 0)
    c0 = np.where(have0[..., None], px, py)
    c1 = np.where(have1[..., None], py, px)
    same01 = np.all(c0 == c1, -1)
    own0 = np.all(c0 == F, -1) & bool(trust)
    own1 = np.all(c1 == F, -1) & bool(trust)
    eval0 = have0 & ~own0
    eval1 = have1 & ~own1 & ~(have0 & same01)
    leaf = np.full((h, w), -1)
    both = have0 & have1
    leaf[~have0 & ~have1] = CORNER
    leaf[have0 & ~have1] = ROW_EVAL
    leaf[have0 & ~have1 & own0] = ROW_OWN
    leaf[~have0 & have1] = COL_EVAL
    leaf[~have0 & have1 & own1] = COL_OWN
    leaf[both] = PAIR
    leaf[both & same01] = SAME01
    leaf[both & own0] = OWN0
    leaf[both & own1] = OWN1
    leaf[both & own0 & own1] = OWN01
    assert (leaf >= 0).all()
    # the restated eval flags and the leaf's dispatch say the same
    want0 = np.isin(leaf, [ROW_EVAL, PAIR, SAME01, OWN1])
    want1 = np.isin(leaf, [COL_EVAL, PAIR, OWN0])
    assert np.array_equal(eval0, want0) and np.array_equal(eval1, want1)
    same_bits = np.all(np.ascontiguousarray(c0).view(np.uint64) == np.ascontiguousarray(c1).view(np.uint64), -1)
    return leaf, c0, c1, same_bits


# ---- (a) emitter / probe fields ---------------------------------------------------------------------------------------------------

THIN_NORMS = ((0.6, 0.8, 1e-9), (0.6, -0.8, -1e-12))  # |nz| < kDoubleEps: the clamped denominator, slopes of 1e7 and more, finite


def make_plane(spec, x, y):
    kind = spec[0]
    if kind == "fp":     # fronto-parallel at d, as Plane::param() gives it: a = b = -0.0
        return np.array([0.0, 0.0, 1.0, -0.0, -0.0, spec[1]])
    if kind == "fpz":    # the same plane with the other zero signs: == says equal, the bits differ
        return np.array([-0.0, -0.0, 1.0, 0.0, 0.0, spec[1]])
    if kind == "sl":     # slopes a, b, disparity d at the emitter's own pixel
        _, d, a, b = spec
        return rp.planes_from_slopes(a, b, np.array([[float(d)]]), np.array([[float(x)]]), np.array([[float(y)]]))[0, 0]
    if kind == "thin":
        nx, ny, nz = THIN_NORMS[spec[1]]
        pa, pb, pc = rp.plane_param(np.float64(nx), np.float64(ny), np.float64(nz), np.float64(x), np.float64(y), np.float64(spec[2]))
        return np.array([nx, ny, nz, pa, pb, pc])
    raise ValueError(kind)


def recipes_of(g):
    """the (A, B) recipes of a geometry.  sL: the coarsest level with a valid disparity; fronto-parallel planes at d in [2^sL, 2^sL * D_sL)
    are all-valid on every level that has one (2^s * D_s does not grow with s)."""
    dims = rp.level_dims(g)
    D = [d for _, _, d in dims]
    sL = max(s for s in range(len(D)) if D[s] >= 2)
    lo_all, hi_all = float(2 ** sL), float(2 ** sL * D[sL])

    def f(t):
        return lo_all + t * (hi_all - lo_all)

    sc = 2.0 ** sL
    R = [
        (("fp", f(0.16)), ("fp", f(0.57))),                           # all-valid on every level
        (("sl", f(0.45), 0.004, -0.006), ("fp", f(0.3))),
        (("sl", f(0.5), -0.003, 0.002), ("sl", f(0.62), 0.002, 0.005)),
        (("fp", 0.5), ("fp", f(0.39))),                               # mixed: A invalid everywhere
        (("fp", float(D[0]) - 2.0 ** -21), ("fp", f(0.24))),          # level 0: corner at D - 2^-21, valid taps, general
        (("fp", 1.0 + 2.0 ** -21), ("fp", f(0.65))),                  # level 0: corner at 1 + 2^-21
        (("fp", 1.0 + 2.0 ** -19), ("fp", f(0.1))),                   # level 0: corner at 1 + 2^-19, all-valid there
        (("fp", sc * (D[sL] - 2.0 ** -19)), ("fp", f(0.34))),         # level sL: corner at D_sL - 2^-19, all-valid
        (("fp", 1.0), ("fp", f(0.52))),                               # taps exactly 1.0 on level 0: valid, general
        (("fp", float(D[0])), ("fp", f(0.27))),                       # taps exactly D: not valid, max_cost (D even: on level 1 as well)
        (("thin", 0, f(0.5)), ("fp", f(0.2))),                        # |nz| ~ 0
        (("thin", 1, f(0.4)), ("sl", f(0.55), 0.003, 0.003)),
        (("fp", f(0.61)), ("fp", f(0.61))),                           # same01, bit for bit
        (("fp", f(0.41)), ("fpz", f(0.41))),                          # same01 under ==, the zero signs differ
        (("sl", 0.4 * hi_all, 0.01, 0.02), ("fp", f(0.8))),
        (("fp", f(0.9)), ("fp", f(0.05))),
    ]
    if sL >= 1:
        R += [
            (("fp", sc * (1.0 + 2.0 ** -21)), ("fp", f(0.88))),       # level sL: corner at 1 + 2^-21
            (("fp", sc * (1.0 + 2.0 ** -19)), ("fp", f(0.49))),       # level sL: corner at 1 + 2^-19
            (("fp", sc), ("fp", f(0.13))),                            # taps exactly 1.0 on level sL
            (("fp", sc * 0.625), ("fp", f(0.86))),                    # fails on level sL only
            (("fp", sc * 0.7), ("fp", sc * 0.55)),                    # both fail on level sL only
            (("fp", 2.0 + 0.3), ("fp", f(0.7))),                      # fails on every coarse level from 2 on (where there is one)
        ]
    return R


def _last_valid(g):
    D = [d for _, _, d in rp.level_dims(g)]
    sL = max(s for s in range(len(D)) if D[s] >= 2)
    return D, sL


def border_leaf_built(g):
    """Level s + 1 sees the plane of level s with its disparities halved, over a window that covers the finer one in image terms, against
    the narrower range -- EXCEPT at the image border: rows are clipped to the image and the centre is halved with a floor, so at the odd
    row y = 1 the fine window reaches one row above its centre (offset -1) and the coarse one, centred on row 0, none.  A plane whose
    disparity grows towards the top by more than its distance from D there leaves the range at level 0 only -- where D is 2^sL * D_sL, so
    that a disparity just below D halves into every coarse range (with max_dis 40 and five levels the coarsest range ends at 32: the slope
    would have to be above 8 per row, and the rows below leave the range on every level)."""
    D, sL = _last_valid(g)
    return bool(g.scale_num) and sL >= 1 and 2 ** sL * D[sL] == D[0] and g.h >= 3 and g.wnd // 2 > 1


def border_planes(g):
    """(border planes, partners): y-sloped planes with the disparity D - 0.1 .. D - 0.04 at row 1 and D + 0.02 or more at row 0, b <= -0.12
    -- level 0 general, every coarse level all-valid (its window starts at its centre row, 0); partners all-valid on every level, some
    of them as far from any surface as the border planes are, so that either may win"""
    D, sL = _last_valid(g)
    lo_all, hi_all = float(2 ** sL), float(2 ** sL * D[sL])
    S = [("sl", D[0] - 0.1, 0.0, -0.2), ("sl", D[0] - 0.07, 0.0, -0.15), ("sl", D[0] - 0.04, 0.0, -0.12), ("sl", D[0] - 0.1, 0.0, -0.17)]
    Q = [("fp", lo_all + t * (hi_all - lo_all)) for t in (0.97, 0.35, 0.99, 0.6, 0.93, 0.2, 0.985)]
    return S, Q


def probe_field(g, view):
    """(field (h, w, 6), stored cost (h, w)) of the emitter / probe case of geometry g, view `view`"""
    R = recipes_of(g)
    F = np.zeros((g.h, g.w, 6))
    for y in range(g.h):
        for x in range(g.w):
            if (x + y) % 2 == 0:
                a, b = R[((x + y) // 2 + 7 * view) % len(R)]
                F[y, x] = make_plane(a if x % 2 else b, x, y)
    if border_leaf_built(g):
        # "Fails on level 0 but on no coarse level" (border_planes): the probes of row 1.  Left part of the row: the emitters of row 1
        # hold a border plane (candidate 0 of the probe to their right going forwards, of the one to their left going backwards), those of
        # rows 0 and 2 an all-valid partner.  Right part: the emitters of rows 0 and 2 hold the border plane (candidate 1 forwards and
        # backwards), those of row 1 the partner.
        S, Q = border_planes(g)
        for x in range(g.w // 8, g.w - g.w // 8):
            left = x < g.w // 2
            for y in (0, 1, 2):
                if (x + y) % 2 == 0:
                    k = x // 2 + view
                    special = (y == 1) == left
                    F[y, x] = make_plane(S[k % len(S)], x, 1) if special else make_plane(Q[k % len(Q)], x, y)
    # A probe's own plane is never kept (its stored cost is 1e300).  Four probes in five hold, bit for bit, the plane of their left,
    # upper, right or lower emitter: a candidate that equals the own plane must be evaluated all the same, because cspm_set_planes
    # leaves Pm::trust_cost at 0 -- a sweep that took own0 / own1 there would leave the 1e300 standing.
    for y in range(g.h):
        for x in range(g.w):
            if (x + y) % 2:
                dx, dy = ((-1, 0), (0, -1), (1, 0), (0, 1), (0, 0))[(x // 2 + y // 2) % 5]
                inside = 0 <= x + dx < g.w and 0 <= y + dy < g.h and (dx, dy) != (0, 0)
                F[y, x] = F[y + dy, x + dx] if inside else make_plane(("fp", 0.37 * g.max_dis), x, y)
    xx, yy = np.meshgrid(np.arange(g.w), np.arange(g.h))
    return F, np.where((xx + yy) % 2 == 0, EMITTER_COST, PROBE_COST)


def probe_tags(g, F, inc):
    """per pixel of a kind-(a) field swept in direction inc: {tag: (h, w) bool} over the PROBES, from the restatement alone (the
    emitters keep their planes, so the field after the sweep is not needed to know a probe's candidates), and the smallest guard
    distance of any candidate at any level"""
    h, w = F.shape[:2]
    leaf, c0, c1, same_bits = sweep_leaves(F, F, inc, False)
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    probe = (xx + yy) % 2 == 1
    L0 = classify(g, xx.ravel(), yy.ravel(), c0.reshape(-1, 6))
    L1 = classify(g, xx.ravel(), yy.ravel(), c1.reshape(-1, 6))
    nl = len(L0)
    sh = (h, w)
    ok0 = np.stack([l.ok.reshape(sh) for l in L0])
    ok1 = np.stack([l.ok.reshape(sh) for l in L1])
    hv = np.array([l.has_valid for l in L0])
    pair = probe & (leaf == PAIR)
    gen = ~(ok0 & ok1)  # per level: general
    ngen = gen[hv].sum(0)
    T = {}
    T["pair: all-valid on every level"] = pair & (ngen == 0)
    T["pair: candidate 0 alone fails"] = pair & np.any(~ok0 & ok1 & hv[:, None, None], 0)
    T["pair: candidate 1 alone fails"] = pair & np.any(ok0 & ~ok1 & hv[:, None, None], 0)
    if hv.sum() >= 2:
        T["pair: fails on one level only"] = pair & (ngen == 1)
        T["pair: fails on one coarse level only"] = pair & (ngen == 1) & ~gen[0]
    if not hv.all():
        T["pair: a level with D < 2"] = pair.copy()

    def corner(which, val_of, allv, levels):
        m = np.zeros(sh, bool)
        for s in levels:
            if not hv[s]:
                continue
            for L in (L0, L1):
                q = (L[s].qmin if which == "min" else L[s].qmax).reshape(sh)
                m |= (q == val_of(L[s].D)) & (gen[s] != allv)
        return pair & m

    lv0, lvc = [0], list(range(1, nl))
    T["pair: level 0 corner at 1 + 2^-21 (general)"] = corner("min", lambda D: 1.0 + 2.0 ** -21, False, lv0)
    T["pair: level 0 corner at D - 2^-21 (general)"] = corner("max", lambda D: D - 2.0 ** -21, False, lv0)
    T["pair: level 0 corner at 1 + 2^-19 (all-valid)"] = corner("min", lambda D: 1.0 + 2.0 ** -19, True, lv0)
    T["pair: a corner at D_s - 2^-19 (all-valid)"] = corner("max", lambda D: D - 2.0 ** -19, True, range(nl))
    # "taps exactly ...": all four corners at the value, i.e. a fronto-parallel plane, which is what the builder writes for these leaves
    # (qmax == 1.0 with every corner in the general range below it, qmin == D likewise); a sloped recipe would not be tagged here
    T["pair: level 0 taps exactly 1.0"] = corner("max", lambda D: 1.0, False, lv0)
    T["pair: level 0 taps exactly D"] = corner("min", lambda D: float(D), False, lv0)
    if hv[1:].any():
        T["pair: coarse corner at 1 + 2^-21 (general)"] = corner("min", lambda D: 1.0 + 2.0 ** -21, False, lvc)
        T["pair: coarse corner at 1 + 2^-19 (all-valid)"] = corner("min", lambda D: 1.0 + 2.0 ** -19, True, lvc)
        T["pair: coarse taps exactly 1.0"] = corner("max", lambda D: 1.0, False, lvc)
        T["pair: coarse taps exactly D_s"] = corner("min", lambda D: float(D), False, lvc)
    if border_leaf_built(g):
        T["pair: fails on level 0 but on no coarse level"] = pair & gen[0] & ~np.any(gen[1:] & hv[1:, None, None], 0)
    thin = (np.abs(c0[..., 2]) < rp.K_DOUBLE_EPS) | (np.abs(c1[..., 2]) < rp.K_DOUBLE_EPS)
    T["pair: |nz| ~ 0"] = pair & thin
    T["same01: bit for bit"] = probe & (leaf == SAME01) & same_bits
    T["same01: +0.0 against -0.0"] = probe & (leaf == SAME01) & ~same_bits
    trusted = sweep_leaves(F, F, inc, True)[0]  # where own0 / own1 WOULD hold: the probe's own plane is a candidate's, trust is 0
    T["trust 0: the own plane is candidate 0's, evaluated all the same"] = probe & np.isin(trusted, [OWN0, OWN01, ROW_OWN])
    T["trust 0: the own plane is candidate 1's, evaluated all the same"] = probe & np.isin(trusted, [OWN1, OWN01, COL_OWN])
    T["first sweep row (x-predecessor only)"] = probe & (leaf == ROW_EVAL)
    T["first sweep column (y-predecessor only)"] = probe & (leaf == COL_EVAL)
    guard = min(float(l.guard.reshape(sh)[probe].min()) for l in L0 + L1)
    return T, guard, leaf


# ---- (b) block fields -------------------------------------------------------------------------------------------------------------

def block_field(g, view, seed, guide=None):
    """a piecewise constant field: a grid of rectangles 2 .. 7 pixels wide and high, each holding one plane of a small palette (equal
    neighbours merge) or, with a `guide` disparity map (h, w), three times in five the fronto-parallel plane at the guide's value in the
    rectangle's middle, rounded to 1/8 -- planes that a sweep does not flood with one winner --, crossed by stripes (whole bands of the grid)"""
    rng = np.random.default_rng(seed + view)
    dims = rp.level_dims(g)
    D = [d for _, _, d in dims]
    sL = max(s for s in range(len(D)) if D[s] >= 2)
    lo_all, hi_all = float(2 ** sL), float(2 ** sL * D[sL])
    pal = [make_plane(("fp", lo_all + t * (hi_all - lo_all)), 0, 0) for t in (0.1, 0.3, 0.5, 0.7, 0.9)]
    pal += [make_plane(("sl", lo_all + 0.4 * (hi_all - lo_all), 0.004, -0.003), g.w // 2, g.h // 2),
            make_plane(("sl", lo_all + 0.6 * (hi_all - lo_all), -0.005, 0.004), g.w // 2, g.h // 2),
            make_plane(("fp", 0.3 * hi_all), 0, 0), make_plane(("fp", 0.55 * hi_all), 0, 0)]

    def cuts(n):
        out = [0]
        while out[-1] < n:
            out.append(out[-1] + int(rng.integers(2, 8)))
        out[-1] = n
        if out[-1] - out[-2] < 2:
            out.pop(-2)
        return out

    F = np.zeros((g.h, g.w, 6))
    xc, yc = cuts(g.w), cuts(g.h)
    for j in range(len(yc) - 1):
        for i in range(len(xc) - 1):
            k, u = int(rng.integers(len(pal))), float(rng.uniform())
            if guide is not None and u < 0.6:
                d = guide[(yc[j] + yc[j + 1]) // 2, (xc[i] + xc[i + 1]) // 2]
                d = min(max(np.rint(8.0 * (d if np.isfinite(d) else lo_all)) / 8.0, 1.5), g.max_dis - 1.5)
                F[yc[j]:yc[j + 1], xc[i]:xc[i + 1]] = make_plane(("fp", float(d)), 0, 0)
            else:
                F[yc[j]:yc[j + 1], xc[i]:xc[i + 1]] = pal[k]
    for k in range(2):  # stripes: a whole band of rows and a whole band of columns of the grid, one plane each
        j, i = int(rng.integers(len(yc) - 1)), int(rng.integers(len(xc) - 1))
        F[yc[j]:yc[j + 1], :] = pal[int(rng.integers(len(pal)))]
        F[:, xc[i]:xc[i + 1]] = pal[int(rng.integers(len(pal)))]
    return F


SHORTCUT_LEAVES = (OWN0, OWN1, OWN01, ROW_OWN, COL_OWN)

# ---- the cases --------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name kind geom seed lam fold")  # kind "probe" / "block"; fold: also run under CSPM_OPT_SWEEP_FOLD

G5 = Geom(48, 40, 16, 35, 5)     # levels 24x20 .. 3x3 shorter than the window: 1-4 passes, rows clipped at both ends; level 4 has D = 1
G3 = Geom(48, 40, 16, 35, 3)
GSS = Geom(48, 40, 16, 35, 0)    # four waves share a window's passes; clipped windows leave waves without one
G45 = Geom(80, 12, 16, 45, 2)    # window 45: five steps of 7 + 3 columns, a level of 12 rows, shorter than two pass groups
G45T = Geom(12, 80, 8, 45, 0)    # window 45 down a tall image: five passes for four waves; the level is narrower than one step group
G9 = Geom(40, 30, 8, 9, 3)       # window 9: 7 * nsteps = 14 > 9, the corner test covers the masked columns of the last step
GWIDE = Geom(30, 30, 40, 35, 5)  # max_dis > width: off-image columns on both sides

CASES = [
    Case("probe_5lv", "probe", G5, 51, 0.3, True),
    Case("probe_3lv", "probe", G3, 51, 0.3, False),
    Case("probe_ss", "probe", GSS, 51, 0.0, False),
    Case("probe_w45", "probe", G45, 52, 0.3, False),
    Case("probe_w45_tall", "probe", G45T, 53, 0.0, False),
    Case("probe_w9", "probe", G9, 54, 0.3, False),
    Case("probe_wide_dis", "probe", GWIDE, 55, 0.3, True),
    Case("block_5lv", "block", G5, 51, 0.3, True),
    Case("block_ss", "block", GSS, 51, 0.0, False),
    Case("block_w9", "block", G9, 54, 0.3, False),
]
BY_NAME = {c.name: c for c in CASES}
# the other cost sources take these (the all-valid, mixed, margin and exact-boundary probes of the five-level geometry are all in it)
SOURCE_CASE = "probe_5lv"
# one case of each kind with one workgroup per row band (CSPM_OPT_SWEEP_GRID = 8): dependent items follow one another
GRID_CASES = ("probe_5lv", "block_5lv")


def case_fields(case, guides=(None, None)):
    """[(field, stored cost or None)] per view; a block field's start costs are the oracle's re-score (tests/chain_cases.py), its
    guides the pair's own disparity maps"""
    if case.kind == "probe":
        return [probe_field(case.geom, v) for v in (0, 1)]
    return [(block_field(case.geom, v, case.seed, guides[v]), None) for v in (0, 1)]
