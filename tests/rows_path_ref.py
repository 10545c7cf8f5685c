"""The row engine's choice of code path, restated on the CPU (csrc/cspm_rows.h level_rows, the fused GRD cost): which LEAF of the
decision every level pass of a k_rescore launch takes, from the geometry and the plane field alone -- the wave layout of row_item /
k_rescore / eval_rows_view (64 consecutive columns of a row, tail lanes shadow the last pixel, at level s the centre is (x >> s, y >> s)
and the plane is re-derived with plane_param), strip_capacity / own_capacity / wave_lds_bytes, fits() / span32(), the NQP / NQE / NQD
pitches, the cluster cut and the four-corner range test.  sweep() lists the leaves any geometry can reach, CASES are small constructed
plane fields that take every one of them on purpose.  tests/test_rows_path_ref.py holds this file to the device's own counters
(tests/golden/row_paths.json, recorded by tools/row_paths.py), tests/test_gpu_row_paths.py holds the device to the oracle on CASES.

leaf = kind | two table buffers << 3 | padded pitch << 4 | weight table << 5 | edge << 6 (g_pathstat in cspm_rows.h)."""
import collections
import fractions
import functools

import numpy as np

K_WAVE, K_STRIP_REGS, K_ROW_MOD = 64, 6, 7
K_DOUBLE_EPS = 0.00000001
EPS20 = 2.0 ** -20
KINDS = ["unstaged", "general_range_failed", "general_too_many", "full_computed", "full_dma", "range_computed", "range_dma", "cluster_dma"]
UNSTAGED, GEN_RANGE, GEN_MANY, FULL_COMP, FULL_DMA, RANGE_COMP, RANGE_DMA, CLUSTER_DMA = range(8)
TBUF2, PADDED, WTAB, EDGE = 8, 16, 32, 64


def leaf_name(leaf):
    k = leaf & 7
    s = KINDS[k]
    if k >= FULL_COMP:
        if k in (FULL_DMA, RANGE_DMA, CLUSTER_DMA):
            s += "/2buf" if leaf & TBUF2 else "/1buf"
        s += "/padded" if leaf & PADDED else "/unpadded"
        s += "/wtab" if leaf & WTAB else "/pertap"
    return s + ("/edge" if leaf & EDGE else "/interior")


# ---- the LDS budget (cspm_rows.h:68-80) ---------------------------------------------------------------------------------------------

def strip_capacity(max_dis, half):
    want = K_WAVE + 2 * half + max_dis + 2
    return min(want, K_STRIP_REGS * K_WAVE)


def own_capacity(half):
    return K_WAVE + 2 * half + 2


def strip_set_bytes(cap, ocap):
    return (cap * 16 + ocap * 12 + 15) // 16 * 16


def wave_lds_bytes(cap, ocap):
    return max(2 * strip_set_bytes(cap, ocap), (cap + ocap) * 16)


Geom = collections.namedtuple("Geom", "w h max_dis wnd scale_num")  # scale_num 0: single-scale (one level, the stored a, b, c)


def level_dims(g):
    """[(W, H, D)] per level (cspm_api.hip: pre_cs_pc.cc:36-55)"""
    out, (w, h, d) = [], (g.w, g.h, g.max_dis)
    for s in range(max(g.scale_num, 1)):
        if s:
            w, h, d = (w + 1) // 2, (h + 1) // 2, d // 2
        out.append((w, h, d))
    return out


# ---- the decision of one level pass (cspm_rows.h level_rows, "the wave's span of centres" .. the end of the computed-table choice) ----

Pass = collections.namedtuple("Pass", "leaf nd pitch tbuf why")


def decide(max_dis, wnd, D, W, H, view, cmin, cmax, have_cvol, lanes):
    """lanes() -> (safe, fl, fh) lists of the wave's 64 lanes (the range test's per-lane result), called only where the device runs
    the test.  Returns the Pass of the wave."""
    half = wnd // 2
    n = 2 * half + 1
    cap, ocap = strip_capacity(max_dis, half), own_capacity(half)
    edge = (cmin - half < 0) or (cmax + half >= W)
    e = EDGE if edge else 0
    s_len = cmax - cmin + 2 * half + D + (1 if view == 0 else 2)
    o_len = cmax - cmin + 2 * half + 1
    staged = s_len <= cap and o_len <= ocap
    if not (staged and D >= 2):
        return Pass(UNSTAGED | e, 0, 0, 0, "unstaged" if not staged else "D < 2")
    ncent, NQ = cmax - cmin + 1, o_len
    lds_room = wave_lds_bytes(cap, ocap) - 64
    own_bytes = (NQ * 8 + 15) // 16 * 16 + (NQ * 4 + 15) // 16 * 16
    wtab_bytes = ncent * n * 8 + ncent * 4
    NQP = (NQ + 31) // 32 * 32 if ncent >= 48 else (NQ + 15) // 32 * 32 + 16 if ncent >= 24 else NQ
    p2 = (NQ * 4 + 15) // 16 * 16
    full_fits = (NQ + D) * 16 + own_bytes + NQ * D * 8 + wtab_bytes <= lds_room
    range_ok, f_lo, f_hi, fl, fh = False, 1, 1, None, None
    if (not full_fits or have_cvol) and D < 512:
        safe, fl, fh = lanes()  # lists
        f_lo, f_hi = min(fl), max(fh)
        range_ok = all(safe)
    nd = f_hi - f_lo + 1
    NQE = (NQ + 3) & ~3
    NQD = max(NQP, NQE)
    cvW = W + 2 * (wnd // 2 + 2)

    def span32(n_):
        return n_ * H * cvW * 8 < (1 << 32)

    def fits(nb, n_, pit, wt):
        return nb * n_ * pit * 8 + 2 * p2 + (wtab_bytes if wt else 0) <= lds_room and n_ * (pit // 2) <= 12 * K_WAVE and span32(n_)

    def table(kind, nb, pit, wt, nrows, why):
        return Pass(kind | (TBUF2 if nb == 2 else 0) | (PADDED if pit == NQD else 0) | (WTAB if wt else 0) | e, nrows, pit, nb, why)

    if have_cvol:
        for nb in (2, 1):
            if range_ok:
                small = not edge and ncent <= K_WAVE
                for cond, pit, wt in ((small, NQD, False), (small, NQE, False), (True, NQD, True), (not edge, NQD, False), (True, NQE, True),
                                      (not edge, NQE, False)):
                    if cond and fits(nb, nd, pit, wt):
                        return table(RANGE_DMA, nb, pit, wt, nd, "range")
            if full_fits:
                for pit in (NQD, NQE):
                    if fits(nb, D, pit, True):
                        return table(FULL_DMA, nb, pit, True, D, "full")
        if range_ok and nd > 2:
            cut = (f_lo + f_hi + 1) // 2
            in_a, in_b = [h < cut for h in fh], [l >= cut for l in fl]
            if all(x or y for x, y in zip(in_a, in_b)):
                a_hi = max(h if x else f_lo for h, x in zip(fh, in_a))
                bl = min(l if y else f_hi for l, y in zip(fl, in_b))
                nt = (a_hi - f_lo + 1) + (f_hi - bl + 1)
                if nt < nd and span32(f_hi - f_lo + 1):
                    for nb in (2, 1):
                        for cond, pit, wt in ((True, NQD, True), (not edge, NQD, False), (True, NQE, True), (not edge, NQE, False)):
                            if cond and fits(nb, nt, pit, wt):
                                return table(CLUSTER_DMA, nb, pit, wt, nt, f"cluster cut {cut}: {a_hi - f_lo + 1} + {f_hi - bl + 1} of {nd}")
    if full_fits:
        padded = (NQ + D) * 16 + own_bytes + NQP * D * 8 + wtab_bytes <= lds_room
        pit = NQP if padded else NQ
        return Pass(FULL_COMP | (PADDED if pit == NQP else 0) | WTAB | e, D, pit, 0, "full computed")
    if range_ok and NQ + nd <= K_STRIP_REGS * K_WAVE:
        strip_bytes = (NQ + nd) * 16 + own_bytes
        for cond, pit, wt in ((True, NQP, True), (not edge, NQP, False), (True, NQ, True), (not edge, NQ, False)):
            need = strip_bytes + pit * nd * 8 + (wtab_bytes if wt else p2)
            if cond and need <= lds_room:
                return Pass(RANGE_COMP | (PADDED if pit == NQP else 0) | (WTAB if wt else 0) | e, nd, pit, 0, "range computed")
    return Pass((GEN_MANY if range_ok else GEN_RANGE) | e, nd, 0, 0, "too many disparities" if range_ok else "range test failed")


# ---- the sweep: which leaves can any geometry reach? ----------------------------------------------------------------------------------

SWEEP_WND, SWEEP_DIS, SWEEP_LEVELS = (9, 35), (16, 32, 128, 320), 5


@functools.lru_cache(maxsize=None)
def sweep():
    """{leaf: {(window, max_dis, level): witness}} over window x max_dis x level x ncent x nd x edge x cvol x view x (the range test
    fails: nd 0; passes with one interval of nd disparities; passes with two clusters of nt < nd table rows).  An interior wave has
    exactly 64 >> s centres at level s (segments start at multiples of 64; a shorter tail wave touches the right border), an edge wave
    1 .. 64 >> s.  A lane's interval holds at least two disparities: nd >= 2, and two clusters hold nt >= 4.  Every cluster leaf is reached at nd = D if at all (the plain tables, tried first, fit the less the larger nd).  The
    image is taken 4096 wide and 40 rows high: W enters the decision through `edge` only and H through span32() (see UNREACHABLE)."""
    seen = {}
    for wnd in SWEEP_WND:
        for max_dis in SWEEP_DIS:
            for s in range(SWEEP_LEVELS):
                D = max_dis >> s
                full = max(K_WAVE >> s, 1)
                for edge in (False, True):
                    for ncent in (range(1, full + 1) if edge else (full,)):
                        cmin = 0 if edge else 1024
                        for cvol in (False, True):
                            for view in (0, 1):
                                for nd in (0,) + tuple(range(2, max(D, 2) + 1)):
                                    for nt in (0,) + (tuple(range(4, nd)) if nd == D else ()):
                                        if nd == 0:    # the range test fails in some lane
                                            lanes = ([False, True], [1, 1], [1, 1])
                                        elif nt == 0:  # one lane spans the interval
                                            lanes = ([True], [1], [nd])
                                        else:
                                            lanes = ([True, True], [1, nd - (nt - nt // 2) + 1], [nt // 2, nd])
                                        p = decide(max_dis, wnd, D, 4096, 40, view, cmin, cmin + ncent - 1, cvol, lambda: lanes)
                                        seen.setdefault(p.leaf, {}).setdefault((wnd, max_dis, s), dict(ncent=ncent, nd=nd, nt=nt, cvol=cvol, view=view))
                                    if p.leaf & 7 == UNSTAGED:
                                        break
    return seen


# leaves that no geometry reaches, with the inequality that excludes them
UNREACHABLE = {
    "span32() false (any DMA table refused for its 32-bit offsets)":
        "needs n_ * H * cvW * 8 >= 2^32 with n_ * (pitch / 2) <= 768 rows-pieces: the host refuses table volumes when 64 slabs span 4 GiB "
        "(cspm_api.hip fits32), so the table would need more than 64 rows of a pitch >= 2 * half + 4 >= 12 entries -- at most 128 rows, "
        "i.e. a level image of H * cvW >= 2^22 entries; the leaf it would lead to (a computed table or general taps) is reached otherwise",
    "range tables at D >= 512":
        "D < 512 guards the range test (the disparity's linearity bound 2^-43 holds below 2^9): range_ok stays false, such a level takes "
        "general_range_failed, and it is unstaged anyway (s_len >= 64 + D > 384 slots)",
}


# ---- the wave layout and the four-corner range test, per launch -----------------------------------------------------------------------

def _fma_exact(a, b, c):
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def _corner(a, qx, rt, j):
    """tap_disp(a, j, group_disp(a, qx, rt)) = fma(a, j, fma(a, qx, rt)) per lane.  numpy has no fused multiply-add: the unfused value
    differs from the device's by < 2^-40 relative, so lanes whose value lies within 2^-30 of a point where the decision changes
    (an integer -+ 2^-20) are recomputed exactly."""
    with np.errstate(all="ignore"):
        q = a * j + (a * qx + rt)
        lo, hi = q - EPS20, q + EPS20
        flag = np.isfinite(q) & (np.abs(q) < 2.0 ** 20) & ((np.abs(lo - np.rint(lo)) < 2.0 ** -30) | (np.abs(hi - np.rint(hi)) < 2.0 ** -30))
    for i in np.flatnonzero(flag):
        q.flat[i] = _fma_exact(a.flat[i], j, _fma_exact(a.flat[i], qx.flat[i], rt.flat[i]))
    return q


def plane_param(nx, ny, nz, px, py, pz):
    with np.errstate(all="ignore"):
        denom = np.maximum(np.abs(nz), K_DOUBLE_EPS)
        denom = np.where(nz < 0.0, -denom, denom)
        s = nx * px
        s = s + ny * py
        s = s + nz * pz
        return -nx / denom, -ny / denom, s / denom


def planes_from_slopes(a, b, d, xs, ys):
    """(h, w, 6) norm+param field of the planes through (xs, ys, d) -- image columns and rows of the pixels, (h, w) like d -- with slopes
    a, b: the normal (-a, -b, 1) / length, the parameters as plane_param gives them back (what Plane(norm, point).param() holds)"""
    a, b = np.broadcast_to(np.asarray(a, np.float64), d.shape), np.broadcast_to(np.asarray(b, np.float64), d.shape)
    ln = np.sqrt(a * a + b * b + 1.0)
    nx, ny, nz = -a / ln, -b / ln, 1.0 / ln
    pa, pb, pc = plane_param(nx, ny, nz, np.asarray(xs, np.float64), np.asarray(ys, np.float64), d.astype(np.float64))
    return np.stack([nx, ny, nz, pa, pb, pc], -1)


def launch_leaves(g, have_cvol, view, field):
    """every level pass of view `view` of a k_rescore launch over `field` ((h, w, 6) norm+param): [(level, y, x0, Pass)]"""
    return [(s, y, x0, decide(g.max_dis, g.wnd, D, W, H, view, cmin, cmax, have_cvol, lambda: (safe, fl, fh)))
            for s, y, x0, (W, H, D), cmin, cmax, safe, fl, fh, _ in launch_lanes(g, field)]


def launch_lanes(g, field):
    """the range test of every level pass: [(level, y, x0, (W, H, D), cmin, cmax, safe, fl, fh, unsafe_corners)], the last four lists over
    the wave's 64 lanes (unsafe_corners: how many of the lane's four window corners leave [1 + 2^-20, D - 2^-20])"""
    half = g.wnd // 2
    n = 2 * half + 1
    jl = (n - 1) % K_ROW_MOD
    segs = (g.w + K_WAVE - 1) // K_WAVE
    x = np.minimum(np.arange(segs * K_WAVE), g.w - 1)  # tail lanes shadow the last pixel
    f = np.asarray(field, np.float64)[:, x, :]
    ys = np.broadcast_to(np.arange(g.h)[:, None], (g.h, x.size))
    xs = np.broadcast_to(x[None, :], (g.h, x.size))
    out = []
    for s, (W, H, D) in enumerate(level_dims(g)):
        cx, cy = xs >> s, ys >> s
        if g.scale_num > 0:
            with np.errstate(all="ignore"):
                cur = f[..., 3] * xs + f[..., 4] * ys + f[..., 5]
                for _ in range(s):
                    cur = cur / 2.0
            a, b, c = plane_param(f[..., 0], f[..., 1], f[..., 2], cx.astype(np.float64), cy.astype(np.float64), cur)
        else:
            a, b, c = f[..., 3], f[..., 4], f[..., 5]
        a, b, c = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)
        dy_lo, dy_hi = np.maximum(0, half - cy), np.minimum(n - 1, H - 1 - cy + half)
        qx0 = (cx - half).astype(np.float64)
        with np.errstate(all="ignore"):
            rt0 = b * (cy - half + dy_lo).astype(np.float64) + c
            rt1 = b * (cy - half + dy_hi).astype(np.float64) + c
            qx1 = qx0 + float(n - 1 - jl)
            q = np.stack([_corner(a, qx0, rt0, 0.0), _corner(a, qx1, rt0, float(jl)), _corner(a, qx0, rt1, 0.0), _corner(a, qx1, rt1, float(jl))])
            # fmin / fmax ignore a NaN operand; a NaN result (all four) compares false
            qmin, qmax = np.fmin.reduce(q), np.fmax.reduce(q)
            safe = (qmin >= 1.0 + EPS20) & (qmax <= float(D) - EPS20)
            nbad = (~((q >= 1.0 + EPS20) & (q <= float(D) - EPS20))).sum(0)
            fl = np.where(safe, (np.where(safe, qmin, 1.0) - EPS20).astype(np.int64), 1)
            fh = np.where(safe, np.minimum((np.where(safe, qmax, 1.0) + EPS20).astype(np.int64) + 1, D), 1)
        for y in range(g.h):
            for k in range(segs):
                sl = slice(k * K_WAVE, (k + 1) * K_WAVE)
                cw = cx[y, sl]
                out.append((s, y, k * K_WAVE, (W, H, D), int(cw.min()), int(cw.max()), safe[y, sl].tolist(), fl[y, sl].tolist(), fh[y, sl].tolist(),
                            nbad[y, sl].tolist()))
    return out


def histogram(passes):
    """{(level, leaf): count}"""
    return dict(collections.Counter((s, p.leaf) for s, _, _, p in passes))


# ---- constructed cases ----------------------------------------------------------------------------------------------------------------
# A case: a geometry, a cost source ("tables": table_volumes on, "computed": table_volumes off, "volumes": kSrcVolume -- no fused cells,
# the decision does not run), and per view a field made of per-segment recipes: segment k (64 columns) of every row gets recipe[k % len].

Case = collections.namedtuple("Case", "name geom seed fields phases")
SOURCES = ("tables", "computed", "volumes")


def _stairs(w, h, base, nd):
    """fronto-parallel planes whose 64 lanes of a segment step through nd - 1 consecutive half-integer disparities base + 0.5 + k: the wave
    touches nd integer disparities at level 0 and every integer between has a lane on it (no cluster cut without a straddling lane)"""
    lane = np.arange(w) % K_WAVE
    steps = max(nd - 2, 0)
    d = base + 0.5 + (lane * (steps + 1) // K_WAVE if steps else 0 * lane)
    return np.broadcast_to(d.astype(np.float64)[None, :], (h, w)).copy()


def _segment_field(w, h, recipes, D, wnd):
    """recipes: per segment a dict(kind=..., ...) -> (h, w, 6)"""
    out = np.zeros((h, w, 6))
    segs = (w + K_WAVE - 1) // K_WAVE
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    for k in range(segs):
        r = recipes[k % len(recipes)]
        sl = slice(k * K_WAVE, min((k + 1) * K_WAVE, w))
        ww = sl.stop - sl.start
        lane = np.arange(ww)
        kind = r["kind"]
        a = b = 0.0
        X, Y = xs[:, sl], ys[:, sl]
        if kind == "flat":          # fronto-parallel at d (k + 0.5: nd = 2, integer k: nd = 3)
            d = np.full((h, ww), float(r["d"]))
        elif kind == "stairs":      # nd integer disparities from base + 1 down to ... (see _stairs)
            d = _stairs(ww, h, r["base"], r["nd"])
        elif kind == "xslant":      # one plane, slope a in x, disparity d at the segment's first column
            a = r["a"]
            d = r["d"] + a * (X - sl.start)
        elif kind == "yslant":
            b = r["b"]
            d = r["d"] + b * Y
        elif kind == "step":        # two (three) far-apart fronto-parallel surfaces, the step at lane `at` (and `at2`)
            d = np.where(lane[None, :] < r["at"], float(r["lo"]), float(r["hi"])) * np.ones((h, 1))
            if "at2" in r:
                d = np.where(lane[None, :] >= r["at2"], float(r["hi2"]), d)
        elif kind == "parts":       # runs of lanes, each stepping through `steps` consecutive disparities from d_first, as seen at level `level`
            d = np.zeros(ww)
            at = 0
            for cnt, d_first, steps in r["parts"]:
                i = np.arange(min(cnt, ww - at))
                d[at:at + i.size] = (d_first + i * steps // cnt) * 2.0 ** r.get("level", 0)
                at += i.size
            assert at == ww, (at, ww)
            d = np.broadcast_to(d[None, :], (h, ww)).copy()
        elif kind == "corner":      # every lane its own slanted plane whose full window leaves [1, D] at ONE corner only, by 0.05: near 1 or near D
            a, b = r["a"], r["b"]       # (|a| != |b|: the next corner lies 34 * min(|a|, |b|) further in)
            reach = (wnd // 2) * (abs(a) + abs(b))
            d = np.full((h, ww), 1.0 + reach - 0.05 if r["near"] == "lo" else D - reach + 0.05)
        elif kind == "thin_nz":     # one lane in four with |nz| < kDoubleEps, the others flat
            d = np.full((h, ww), float(r["d"]))
        elif kind == "huge":        # one lane in four with a NaN-free but huge slope, the others flat
            d = np.full((h, ww), float(r["d"]))
        else:
            raise ValueError(kind)
        f = planes_from_slopes(a, b, d, X, Y)
        if kind in ("flat", "stairs", "parts", "step", "thin_nz", "huge"):
            f[..., 0:2] = 0.0
            f[..., 2] = 1.0
            f[..., 3:5] = -0.0
            f[..., 5] = d
        if kind == "step" and "straddle" in r:  # ONE lane whose own interval of disparities straddles the cut: a gently slanted plane through
            c = r["straddle"]                   # the middle of the two surfaces at the lane's own pixel, all four corners inside the range
            f[:, c, :] = planes_from_slopes(r["sa"], 0.0, np.full((h, 1), 0.5 * (r["lo"] + r["hi"])), X[:, c:c + 1], Y[:, c:c + 1])[:, 0, :]
        if kind == "thin_nz":
            m = lane % 4 == 1
            nz = 0.5 * K_DOUBLE_EPS
            nx = np.sqrt(1.0 - nz * nz)
            one = np.ones_like(d[:, m])
            pa, pb, pc = plane_param(nx * one, 0.0 * one, nz * one, xs[:, sl][:, m], ys[:, sl][:, m], d[:, m])
            f[:, m, :] = np.stack([nx * one, 0.0 * one, nz * one, pa, pb, pc], -1)
        if kind == "huge":
            m = lane % 4 == 2
            f[:, m, :] = planes_from_slopes(1e6, -3e5, d[:, m], X[:, m], Y[:, m])
        out[:, sl, :] = f
    return out


def _case(name, geom, seed, left, right, phases=False):
    return Case(name, geom, seed, (tuple(left), tuple(right)), phases)


def F(d):
    return dict(kind="flat", d=d)


def S(base, nd):
    return dict(kind="stairs", base=base, nd=nd)


def P(parts, level=0):
    return dict(kind="parts", parts=parts, level=level)


G32 = Geom(320, 40, 32, 35, 3)
G128 = Geom(320, 40, 128, 35, 3)
G320 = Geom(200, 36, 320, 35, 2)
G9 = Geom(320, 36, 32, 9, 3)
G9_128 = Geom(200, 36, 128, 9, 2)
GSS = Geom(200, 36, 32, 35, 0)
G9_128C = Geom(242, 36, 128, 9, 2)  # a 50-column tail wave; level 1 (121 wide) has interior waves
G9_320 = Geom(200, 36, 320, 9, 2)
G128_4 = Geom(400, 36, 128, 35, 4)  # level 3 (50 wide) has one interior wave, the segment at x = 192
GTAIL = Geom(147, 36, 32, 35, 3)   # the narrowest image with an interior level-0 wave; a 19-column tail wave
GTAIL9 = Geom(203, 36, 16, 9, 2)   # an 11-column tail wave under a small window

CASES = [
    _case("flat_half_and_integer", G32, 21, [F(7.5), F(8.0), F(20.5), F(12.0), F(3.5)], [F(9.0), F(6.5), F(15.0), F(22.5), F(4.0)]),
    _case("nd_thresholds_32", G32, 22, [S(2, 4), S(3, 2), S(2, 3), S(1, 4), S(4, 12)], [S(2, 14), S(2, 5), S(1, 6), S(1, 7), S(1, 30)], True),
    _case("nd_thresholds_32_b", G32, 23, [S(2, 9), S(2, 8), S(2, 9), S(2, 12), S(2, 18)], [S(2, 5), S(2, 16), S(1, 22), S(1, 26), S(1, 28)]),
    _case("nd_thresholds_128", G128, 24, [S(10, 3), S(10, 4), S(10, 5), S(10, 6), S(10, 8)], [S(10, 9), S(10, 8), S(10, 9), S(10, 11), S(10, 20)], True),
    _case("nd_thresholds_128_b", G128, 25, [S(30, 7), S(30, 12), S(30, 13), S(30, 16), S(30, 40)], [S(30, 18), S(30, 22), S(30, 26), S(30, 30), S(30, 60)]),
    _case("slants", G32, 26,
          [dict(kind="xslant", a=0.02, d=6.3), dict(kind="xslant", a=0.06, d=5.3), dict(kind="xslant", a=-0.1, d=20.3),
           dict(kind="yslant", b=0.11, d=6.3), dict(kind="yslant", b=-0.3, d=20.3)],
          [dict(kind="yslant", b=0.05, d=6.3), dict(kind="xslant", a=0.15, d=4.3), dict(kind="xslant", a=0.2, d=3.3),
           dict(kind="yslant", b=0.4, d=5.3), dict(kind="xslant", a=-0.03, d=12.3)]),
    _case("steps", G32, 27,
          [dict(kind="step", at=20, lo=3.5, hi=27.5), dict(kind="step", at=32, lo=4.5, hi=25.5), dict(kind="step", at=63, lo=5.5, hi=28.5),
           dict(kind="step", at=1, lo=2.5, hi=29.5), dict(kind="step", at=40, lo=3.5, hi=26.5)],
          [dict(kind="step", at=33, lo=4.5, hi=27.5), dict(kind="step", at=20, lo=2.5, hi=14.5, at2=44, hi2=28.5),
           dict(kind="step", at=31, lo=3.5, hi=27.5, straddle=40, sa=0.05), dict(kind="step", at=50, lo=2.5, hi=29.5, straddle=7, sa=-0.04),
           dict(kind="step", at=10, lo=6.0, hi=24.0)], True),
    _case("steps_128", G128, 28,
          [dict(kind="step", at=20, lo=10.5, hi=100.5), dict(kind="step", at=32, lo=20.5, hi=90.5), dict(kind="step", at=47, lo=30.0, hi=110.0),
           dict(kind="step", at=5, lo=12.5, hi=120.5), dict(kind="step", at=40, lo=3.5, hi=60.5)],
          [dict(kind="step", at=10, lo=20.0, hi=84.0), dict(kind="step", at=20, lo=10.5, hi=50.5, at2=44, hi2=110.5),
           dict(kind="step", at=31, lo=10.5, hi=100.5, straddle=31, sa=0.05), dict(kind="step", at=50, lo=8.5, hi=99.5, straddle=63, sa=-0.3),
           dict(kind="step", at=33, lo=4.5, hi=127.0 - 2.5)]),
    _case("unsafe_corners", G32, 29,
          [dict(kind="corner", a=0.01, b=-0.02, near="lo"), dict(kind="corner", a=0.01, b=0.02, near="lo"), dict(kind="corner", a=-0.01, b=0.02, near="hi"),
           dict(kind="thin_nz", d=9.5), dict(kind="huge", d=11.5)],
          [dict(kind="huge", d=5.5), dict(kind="corner", a=0.012, b=0.03, near="hi"), dict(kind="thin_nz", d=14.0),
           dict(kind="corner", a=-0.012, b=0.02, near="lo"), dict(kind="corner", a=0.02, b=0.03, near="hi")], True),
    _case("beyond_the_strip_320", G320, 30, [F(40.5), S(60, 5), S(20, 12), F(100.0)], [S(30, 3), F(250.5), S(100, 8), F(9.5)]),
    _case("window9", G9, 31, [F(7.5), S(2, 6), S(2, 12), S(1, 20), S(1, 30)], [S(2, 24), F(6.0), S(1, 28), S(2, 16), S(3, 9)]),
    _case("window9_steps", G9, 32,
          [dict(kind="step", at=20, lo=3.5, hi=27.5), S(1, 26), dict(kind="step", at=32, lo=2.5, hi=29.5), S(1, 31), S(1, 22)],
          [S(1, 27), dict(kind="step", at=40, lo=2.5, hi=14.5, at2=50, hi2=29.5), S(1, 29), dict(kind="step", at=9, lo=4.0, hi=25.0), S(1, 18)]),
    _case("window9_128", G9_128, 33, [S(10, 4), S(10, 30), S(10, 60), S(5, 110)], [S(10, 20), S(10, 45), S(4, 90), S(10, 8)]),
    _case("window9_128_clusters", G9_128C, 37,
          [F(20.5), P([(32, 2.5, 5), (32, 40.5, 5)], 1), P([(32, 2.5, 6), (32, 40.5, 6)], 1), F(9.0)],
          [P([(32, 10.5, 1), (32, 16.5, 1)]), P([(32, 2.5, 1), (32, 40.5, 1)], 1), S(10, 7), P([(25, 10.5, 1), (25, 30.5, 1)])]),
    _case("window9_320_clusters", G9_320, 38, [F(40.5), P([(32, 2.5, 16), (32, 60.5, 16)], 1), S(30, 9), F(7.5)],
          [S(20, 4), P([(32, 4.5, 10), (32, 70.5, 10)], 1), F(100.0), F(33.5)]),
    _case("four_levels_128", G128_4, 39, [F(20.5), S(10, 6), S(30, 12), dict(kind="huge", d=41.5), F(90.0), S(50, 30), F(8.5)],
          [S(10, 9), F(64.0), dict(kind="thin_nz", d=17.5), S(20, 5), S(40, 16), dict(kind="huge", d=100.5), F(3.5)]),
    _case("single_scale", GSS, 34, [F(7.5), S(2, 9), dict(kind="step", at=30, lo=3.5, hi=27.5), S(1, 14)],
          [dict(kind="step", at=22, lo=2.5, hi=28.5), F(12.0), S(2, 6), S(2, 17)]),
    _case("tail_wave", GTAIL, 35, [F(7.5), S(2, 8), S(2, 5)], [S(2, 12), F(9.0), S(1, 20)]),
    _case("tail_wave_window9", GTAIL9, 36, [S(1, 6), S(1, 12), F(5.5), S(1, 14)], [S(1, 10), F(7.0), S(1, 15), S(1, 3)]),
]
# (case, view, first column) of the waves with ONE lane whose interval straddles the cluster cut, all else fit for a two-cluster table
STRADDLE_WAVES = (("steps", 1, 128), ("steps", 1, 192), ("steps_128", 1, 128), ("steps_128", 1, 192))
# (view, first column) of the interior segments of "unsafe_corners" whose lanes leave the range at one window corner only
ONE_CORNER_WAVES = ((0, 64), (0, 128), (1, 64), (1, 192))
# the fields the issue asks for beyond the GRD cells: nd = 2 and the cluster field also under kSrcVolume and single-scale
VOLUME_CASES = ("flat_half_and_integer", "steps", "single_scale")


def case_fields(case):
    g = case.geom
    return [_segment_field(g.w, g.h, case.fields[v], g.max_dis, g.wnd) for v in (0, 1)]


def case_passes(case, source):
    """[(view, level, y, x0, Pass)] of the rescore launch of `case` under cost source `source`"""
    if source == "volumes":
        return []
    fields = case_fields(case)
    return [(v,) + p for v in (0, 1) for p in launch_leaves(case.geom, source == "tables", v, fields[v])]


def case_histogram(case, source):
    """{"view/level/leaf": count}, the layout of tests/golden/row_paths.json"""
    return {f"{v}/{s}/{leaf}": c for (v, s, leaf), c in sorted(collections.Counter((v, s, p.leaf) for v, s, _, _, p in case_passes(case, source)).items())}
