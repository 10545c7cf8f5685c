"""Specification F of DESIGN.md section 25 (include/cspm.h "depth-map fusion") restated on the CPU: elementwise numpy f64 over the
pixels of one reference view, one operation per line in the association the specification writes, the views and the passes as Python
loops.  Every product, sum, quotient, floor and square root is one IEEE f64 operation (numpy f64 never contracts).
fuse() also tallies by which `continue` of step 4 every loop iteration left: the case table's non-vacuity is checked on that."""
import numpy as np

from geom_ref import POINT, same_bits, same_cloud  # noqa: F401  (re-exported: the fusion tests compare with the same helpers)

DEFAULTS = dict(max_reproj=2.0, max_rel_depth=0.01, min_cos=0.0, min_views=2, suppress=1)
EXITS = ("behind", "outside", "hole", "behind_back", "reproj", "depth", "normal", "consistent")
S_KEPT, S_SUPPRESSED = 0x40, 0x80


def check_args(views, max_reproj=2.0, max_rel_depth=0.01, min_cos=0.0, min_views=2, **_):
    """the validity rules: True when an entry would accept the views' cameras and the parameters"""
    if not 1 <= len(views) <= 64:
        return False
    for v in views:
        R, t = np.asarray(v["R"], np.float64).reshape(3, 3), np.asarray(v["t"], np.float64).reshape(3)
        vals = [v["f"], v["cx"], v["cy"], *R.ravel(), *t]
        if not all(np.isfinite(vals)) or not v["f"] > 0:
            return False
        if not np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-6:
            return False
        if (v.get("normal") is None) != (views[0].get("normal") is None):
            return False
    return bool(max_reproj >= 0.0 and max_rel_depth >= 0.0 and 0.0 <= min_cos <= 1.0 and 0 <= min_views <= 63)


def _cam(v):
    return (np.float64(v["f"]), np.float64(v["cx"]), np.float64(v["cy"]), np.asarray(v["R"], np.float64).reshape(3, 3),
            np.asarray(v["t"], np.float64).reshape(3))


def _world(cam, x, y, Z):
    """world(k, back(k, x, y, Z))"""
    f, cx, cy, R, t = cam
    u = x - cx
    wv = y - cy
    X = (u * Z) / f
    Y = (wv * Z) / f
    return [((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z) + t[i] for i in range(3)]


def _to_cam(cam, W):
    _, _, _, R, t = cam
    d = [W[0] - t[0], W[1] - t[1], W[2] - t[2]]
    return [(R[0, j] * d[0] + R[1, j] * d[1]) + R[2, j] * d[2] for j in range(3)]


def _proj(cam, Q):
    f, cx, cy, _, _ = cam
    pu = (f * Q[0]) / Q[2] + cx
    pv = (f * Q[1]) / Q[2] + cy
    return pu, pv


def _rot(cam, n):
    R = cam[3]
    return [(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)]


def _finite3(N):
    return np.isfinite(N[0]) & np.isfinite(N[1]) & np.isfinite(N[2])


def fuse(views, w, h, max_reproj=2.0, max_rel_depth=0.01, min_cos=0.0, min_views=2, suppress=1, cap=None):
    """views: dicts with depth (h, w), f, cx, cy, R (3, 3), t (3,) and optionally normal (3, h, w), bgr (h, w, 3) uint8.
    -> dict(cloud (POINT records, the first `cap`; None = all), count, view_counts (K,) uint32, state (K, h, w) uint8,
            exits {name: iterations that left step 4 there}, points64 (count, 3): the f64 means SP/den before the cast to float)"""
    K, n = len(views), w * h
    cams = [_cam(v) for v in views]
    depth = [np.asarray(v["depth"], np.float64).reshape(n) for v in views]
    normals = views[0].get("normal") is not None
    nrm = [np.asarray(v["normal"], np.float64).reshape(3, n) for v in views] if normals else None
    any_image = any(v.get("bgr") is not None for v in views)
    bgr = [np.asarray(v["bgr"], np.uint8).reshape(n, 3).astype(np.int64) if v.get("bgr") is not None else np.zeros((n, 3), np.int64) for v in views]
    mr2 = np.float64(max_reproj) * np.float64(max_reproj)
    mrd, mc = np.float64(max_rel_depth), np.float64(min_cos)
    used = np.zeros((K, n), np.uint8)
    state = np.zeros((K, n), np.uint8)
    exits = dict.fromkeys(EXITS, 0)
    m = np.arange(n)
    x = (m % w).astype(np.float64)
    y = (m // w).astype(np.float64)
    clouds, means, view_counts = [], [], np.zeros(K, np.uint32)
    with np.errstate(all="ignore"):
        for r in range(K):
            Z = depth[r]
            valid = np.isfinite(Z) & (Z > 0.0)                                  # step 1
            supp = valid & (used[r] != 0) if suppress else np.zeros(n, bool)     # step 2
            act = valid & ~supp
            P = _world(cams[r], x, y, Z)                                         # step 3
            SP = [P[i].copy() for i in range(3)]
            SN = [np.zeros(n) for _ in range(3)]
            if normals:
                Nr = _rot(cams[r], nrm[r])
                fin = _finite3(Nr)
                SN = [np.where(fin, Nr[i], 0.0) for i in range(3)]
            SC = bgr[r].copy()
            c = np.zeros(n, np.int64)
            marks = []
            for k in range(K):                                                   # step 4
                if k == r:
                    continue
                go = act.copy()

                def leave(name, cond, go=go):
                    out = go & ~cond
                    exits[name] += int(out.sum())
                    go &= cond

                Q = _to_cam(cams[k], P)
                leave("behind", Q[2] > 0.0)
                pu, pv = _proj(cams[k], Q)
                fx = np.floor(pu + 0.5)
                fy = np.floor(pv + 0.5)
                leave("outside", (fx >= 0.0) & (fx <= float(w - 1)) & (fy >= 0.0) & (fy <= float(h - 1)))
                mk = np.where(go, fy, 0.0).astype(np.int64) * w + np.where(go, fx, 0.0).astype(np.int64)
                Zk = depth[k][mk]
                leave("hole", np.isfinite(Zk) & (Zk > 0.0))
                Pk = _world(cams[k], fx, fy, Zk)
                Q2 = _to_cam(cams[r], Pk)
                leave("behind_back", Q2[2] > 0.0)
                pu2, pv2 = _proj(cams[r], Q2)
                ex = pu2 - x
                ey = pv2 - y
                leave("reproj", ex * ex + ey * ey <= mr2)
                leave("depth", np.abs(Q2[2] - Z) <= mrd * Z)
                if normals:
                    Nk = _rot(cams[k], nrm[k][:, mk])
                    if mc > 0.0:
                        leave("normal", (Nr[0] * Nk[0] + Nr[1] * Nk[1]) + Nr[2] * Nk[2] >= mc)
                exits["consistent"] += int(go.sum())
                c += go
                for i in range(3):
                    SP[i] = np.where(go, SP[i] + Pk[i], SP[i])
                if normals:
                    add = go & _finite3(Nk)
                    for i in range(3):
                        SN[i] = np.where(add, SN[i] + Nk[i], SN[i])
                SC += np.where(go[:, None], bgr[k][mk], 0)
                marks.append((k, go, mk))
            kept = act & (c >= min_views)                                        # step 5
            state[r] = np.where(act, c | np.where(kept, S_KEPT, 0), np.where(supp, S_SUPPRESSED, 0)).astype(np.uint8)
            if suppress:                                                         # step 6
                for k, go, mk in marks:
                    used[k][mk[go & kept]] = 1
            idx = np.flatnonzero(kept)                                           # step 7
            view_counts[r] = len(idx)
            rec = np.zeros(len(idx), POINT)
            den = (c[idx] + 1).astype(np.float64)
            for i, name in enumerate(("x", "y", "z")):
                rec[name] = (SP[i][idx] / den).astype(np.float32)
            if normals:
                s0, s1, s2 = SN[0][idx], SN[1][idx], SN[2][idx]
                ln = np.sqrt((s0 * s0 + s1 * s1) + s2 * s2)
                for i, name in enumerate(("nx", "ny", "nz")):
                    rec[name] = (SN[i][idx] / ln).astype(np.float32)
            else:
                rec["nx"] = rec["ny"] = rec["nz"] = np.float32(np.nan)
            if any_image:
                d1 = c[idx] + 1
                for i, name in enumerate(("b", "g", "r")):
                    rec[name] = (2 * SC[idx, i] + d1) // (2 * d1)
                rec["a"] = 255
            rec["pixel"] = idx
            clouds.append(rec)
            means.append(np.stack([SP[i][idx] / den for i in range(3)], -1))
    cloud = np.concatenate(clouds) if clouds else np.zeros(0, POINT)
    count = len(cloud)
    if cap is not None:
        cloud = cloud[:cap]
    return dict(cloud=cloud, count=count, view_counts=view_counts, state=state.reshape(K, h, w), exits=exits,
                points64=np.concatenate(means) if means else np.zeros((0, 3)))
