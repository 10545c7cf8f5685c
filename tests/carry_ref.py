"""CPU restatement of the plane-field carry (include/cspm.h "plane-field carry"): the specification C in numpy
f64, every product, sum, quotient, floor and square root one IEEE operation in the association cspm.h states.  tests/test_gpu_carry.py
holds the HIP entries to it bit for bit; tests/test_carry_ref.py checks the restatement itself without a GPU.  It never imports the GPU
package.

A calibration is (f, cx, cy, baseline, doffs); a carry camera is camera(calib, view).  A field is (h, w, 6) doubles, norm then param,
the layout of cspm_get_planes, of which the carry reads the param part."""
import numpy as np

DEFAULTS = dict(fill=1)
EPS = 1e-8
# where a source pixel leaves steps 1 - 6, in the order of the steps; "contender" = it leaves none of them
EXITS = ("mask", "nonfinite", "tt", "behind", "outside", "hq", "plane_nonfinite", "z", "contender")


def camera(calib, view):
    f, cx, cy, B, doffs = (float(v) for v in calib)
    return dict(f=f, cxv=cx + float(view) * doffs, cy=cy, B=B, doffs=doffs, fB=f * B)


def relative_pose(Rs, ts, Rt, tt):
    """cspm_carry_relative_pose: two camera -> world poses into X_t = R X_s + t"""
    Rs, Rt = np.asarray(Rs, np.float64).reshape(3, 3), np.asarray(Rt, np.float64).reshape(3, 3)
    ts, tt = np.asarray(ts, np.float64).reshape(3), np.asarray(tt, np.float64).reshape(3)
    d = ts - tt
    R, t = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = (Rt[0, i] * Rs[0, j] + Rt[1, i] * Rs[1, j]) + Rt[2, i] * Rs[2, j]
        t[i] = (Rt[0, i] * d[0] + Rt[1, i] * d[1]) + Rt[2, i] * d[2]
    return R, t


def view1_motion(R, t, B_s, B_t):
    """the motion between the two view-1 cameras from the one between the view-0 cameras, as cspm_carry_planes shifts it"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    t1 = np.array([t[i] + R[i, 0] * float(B_s) for i in range(3)])
    t1[0] = t1[0] - float(B_t)
    return R, t1


def plane(ks, kt, R, t, a, b, c):
    """steps 4 and 5 on arrays: (a', b', c', hq)"""
    n0, n1 = a * ks["f"], b * ks["f"]
    n2 = ((a * ks["cxv"] + b * ks["cy"]) + c) + ks["doffs"]
    r = [(R[i, 0] * n0 + R[i, 1] * n1) + R[i, 2] * n2 for i in range(3)]
    hq = ks["fB"] + ((r[0] * t[0] + r[1] * t[1]) + r[2] * t[2])
    pa = (kt["B"] * r[0]) / hq
    pb = (kt["B"] * r[1]) / hq
    pc = (((kt["fB"] * r[2]) / hq - pa * kt["cxv"]) - pb * kt["cy"]) - kt["doffs"]
    return pa, pb, pc, hq


def splat(field, mask, ks, kt, R, t, w_t, h_t, max_dis):
    """steps 1 - 6 for every source pixel: dict(exit (h_s, w_s) indices into EXITS, g, depth, a, b, c (the carried plane))"""
    f = np.asarray(field, np.float64)
    h_s, w_s = f.shape[:2]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    a, b, c = f[..., 3], f[..., 4], f[..., 5]
    x = np.broadcast_to(np.arange(w_s, dtype=np.float64)[None, :], (h_s, w_s))
    y = np.broadcast_to(np.arange(h_s, dtype=np.float64)[:, None], (h_s, w_s))
    exit_ = np.full((h_s, w_s), len(EXITS) - 1, np.int64)
    live = np.ones((h_s, w_s), bool)

    def leave(name, cond):
        nonlocal live
        out = live & ~cond
        exit_[out] = EXITS.index(name)
        live = live & cond

    with np.errstate(all="ignore"):
        leave("mask", np.ones((h_s, w_s), bool) if mask is None else np.asarray(mask) != 0)
        leave("nonfinite", np.isfinite(a) & np.isfinite(b) & np.isfinite(c))
        D = (a * x + b * y) + c
        tt = D + ks["doffs"]
        leave("tt", tt > 0.0)
        Z = ks["fB"] / tt
        u, wv = x - ks["cxv"], y - ks["cy"]
        X = (u * Z) / ks["f"]
        Y = (wv * Z) / ks["f"]
        Q = [((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z) + t[i] for i in range(3)]
        leave("behind", Q[2] > 0.0)
        pu = (kt["f"] * Q[0]) / Q[2] + kt["cxv"]
        pv = (kt["f"] * Q[1]) / Q[2] + kt["cy"]
        fx, fy = np.floor(pu + 0.5), np.floor(pv + 0.5)
        leave("outside", (fx >= 0.0) & (fx <= float(w_t - 1)) & (fy >= 0.0) & (fy <= float(h_t - 1)))
        pa, pb, pc, hq = plane(ks, kt, R, t, a, b, c)
        leave("hq", hq > 0.0)
        leave("plane_nonfinite", np.isfinite(pa) & np.isfinite(pb) & np.isfinite(pc))
        z = (pa * fx + pb * fy) + pc
        leave("z", (z >= 0.0) & (z <= float(max_dis)))
    g = np.full((h_s, w_s), -1, np.int64)
    g[live] = fy[live].astype(np.int64) * w_t + fx[live].astype(np.int64)
    return dict(exit=exit_, g=g, depth=np.where(live, Q[2], np.nan), a=pa, b=pb, c=pc)


def finish(pa, pb, x, y, z):
    """the output record of a pixel: the normal from (a', b'), Plane(normal, (x, y, z)) as fit_ref.fit finishes"""
    with np.errstate(all="ignore"):
        ln = np.sqrt((pa * pa + pb * pb) + 1.0)
        inv = 1.0 / np.maximum(ln, EPS)
        nx, ny, nz = (-pa) * inv, (-pb) * inv, 1.0 * inv
        denom = np.maximum(np.abs(nz), EPS)
        denom = np.where(nz < 0.0, -denom, denom)
        fa = -nx / denom
        fb = -ny / denom
        s = nx * x
        s = s + ny * y
        s = s + nz * z
        fc = s / denom
    return np.stack([nx, ny, nz, fa, fb, fc], axis=-1)


def carry(field, ks, kt, R, t, w_t, h_t, max_dis, mask=None, fill=1):
    """C: dict(planes (h_t, w_t, 6), state (h_t, w_t) uint8, source (h_t, w_t) int32, exit (h_s, w_s), depth_ties, fill_ties)
    depth_ties: target pixels whose two nearest contenders have bit-equal depths; fill_ties: filled pixels that chose among equal z."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    sp = splat(field, mask, ks, kt, R, t, w_t, h_t, max_dis)
    n_t = w_t * h_t
    m = np.flatnonzero(sp["g"].ravel() >= 0)
    g, depth = sp["g"].ravel()[m], sp["depth"].ravel()[m]
    order = np.lexsort((m, depth, g))  # by g, then the depth, then m
    g, depth, m = g[order], depth[order], m[order]
    first = np.ones(len(g), bool)
    first[1:] = g[1:] != g[:-1]
    win = np.full(n_t, -1, np.int64)
    win[g[first]] = m[first]
    second = np.flatnonzero(~first & np.roll(first, 1)) if len(g) else np.zeros(0, np.int64)
    depth_ties = int(np.sum(depth[second] == depth[second - 1])) if len(second) else 0
    win = win.reshape(h_t, w_t)

    x = np.broadcast_to(np.arange(w_t, dtype=np.float64)[None, :], (h_t, w_t))
    y = np.broadcast_to(np.arange(h_t, dtype=np.float64)[:, None], (h_t, w_t))
    A, B, C_ = sp["a"].ravel(), sp["b"].ravel(), sp["c"].ravel()
    state = np.where(win >= 0, 1, 0).astype(np.uint8)
    source = win.copy()
    safe = np.maximum(win, 0)
    with np.errstate(all="ignore"):
        pa, pb = A[safe], B[safe]
        z = (pa * x + pb * y) + C_[safe]
    fill_ties = 0
    if fill:
        best_z = np.full((h_t, w_t), np.inf)
        best_w = np.full((h_t, w_t), -1, np.int64)
        ties = np.zeros((h_t, w_t), bool)
        for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            wq = np.full((h_t, w_t), -1, np.int64)  # the neighbour's winner, -1 outside the image
            ys, yd = (slice(max(oy, 0), h_t + min(oy, 0)), slice(max(-oy, 0), h_t + min(-oy, 0)))
            xs, xd = (slice(max(ox, 0), w_t + min(ox, 0)), slice(max(-ox, 0), w_t + min(-ox, 0)))
            wq[yd, xd] = win[ys, xs]
            sq = np.maximum(wq, 0)
            with np.errstate(all="ignore"):
                zq = (A[sq] * x + B[sq] * y) + C_[sq]
            ok = (win < 0) & (wq >= 0) & (zq >= 0.0) & (zq <= float(max_dis))
            ties |= ok & (best_w >= 0) & (zq == best_z)
            take = ok & ((best_w < 0) | (zq < best_z))
            ties &= ~(take & (best_w >= 0))  # a strictly smaller z ends an earlier tie
            best_z = np.where(take, zq, best_z)
            best_w = np.where(take, wq, best_w)
        filled = best_w >= 0
        state[filled] = 2
        source = np.where(filled, best_w, source)
        sf = np.maximum(best_w, 0)
        pa = np.where(filled, A[sf], pa)
        pb = np.where(filled, B[sf], pb)
        z = np.where(filled, best_z, z)
        fill_ties = int(np.sum(ties & filled))
    planes = finish(pa, pb, x, y, z)
    planes[state == 0] = np.nan
    return dict(planes=planes, state=state, source=source.astype(np.int32), exit=sp["exit"], depth_ties=depth_ties, fill_ties=fill_ties)


def carry_fields(fields, calib_s, calib_t, R, t, w_t, h_t, max_dis, fill=1):
    """cspm_carry_planes' candidates: view v of the source carried into view v of the target, (R, t) between the view-0 cameras.
    Returns (candidates, masks) per view: what merge = 1 offers to cspm_merge_planes_host."""
    cands, masks = [], []
    for v in (0, 1):
        Rv, tv = (np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)) if v == 0 else view1_motion(R, t, calib_s[3], calib_t[3])
        res = carry(fields[v], camera(calib_s, v), camera(calib_t, v), Rv, tv, w_t, h_t, max_dis, None, fill)
        cands.append(res["planes"])
        masks.append(res["state"])
    return cands, masks
