"""Specification R of DESIGN.md section 26 (include/cspm.h "depth-view registration") restated on the CPU: elementwise numpy f64 over the
samples of the source view, one operation per line in the association the specification writes, the targets and the iterations as Python
loops, the reduction tree over arrays, the solve and the update in scalar f64.  Every product, sum, quotient, floor and fabs is one IEEE
f64 operation (numpy f64 never contracts).  register() also tallies by which exit every (sample, target) iteration left the pair loop:
the case table's non-vacuity is checked on that."""
import numpy as np

from fuse_ref import _cam, _finite3, _proj, _rot, _to_cam, _world

DEFAULTS = dict(iters=8, stride=1, max_dist=0.5, huber=0.05, min_cos=0.0, min_pairs=100, pivot_rel=1e-8)
EXITS = ("behind", "outside", "hole", "normal_nonfinite", "far", "normal", "pair")
BLOCK, SUMS, MAX_ITERS = 256, 29, 64
REC = np.dtype([("pairs", "<f8"), ("cost", "<f8"), ("rot2", "<f8"), ("trans2", "<f8"), ("status", "<i4")])


def check_args(views, src, targets, iters=8, stride=1, max_dist=0.5, huber=0.05, min_cos=0.0, min_pairs=100, pivot_rel=1e-8):
    """the validity rules of the registration's own arguments (the views' cameras: fuse_ref.check_args)"""
    K = len(views)
    if not 0 <= src < K or targets == 0 or targets >> K or (targets >> src) & 1:
        return False
    return bool(1 <= iters <= MAX_ITERS and stride >= 1 and max_dist >= 0.0 and huber >= 0.0 and 0.0 <= min_cos <= 1.0 and min_pairs >= 0
                and 0.0 <= pivot_rel < 1.0)


def tree(v):
    """v (..., 256, q): for s = 128 .. 1: v[i] = v[i] + v[i + s], i < s -> (..., q)"""
    v = np.array(v, np.float64)
    s = v.shape[-2] // 2
    with np.errstate(all="ignore"):
        while s >= 1:
            v = v[..., :s, :] + v[..., s:2 * s, :]
            s //= 2
    return v[..., 0, :]


def reduce_samples(acc):
    """acc (samples, 29) -> (29,): blocks of 256 samples (missing ones all 0.0), the tree per block, lane j the running sum of the
    partials j, j + 256, .. from 0.0, the tree over the lanes"""
    n = acc.shape[0]
    nb = max((n + BLOCK - 1) // BLOCK, 0)
    pad = np.zeros((nb * BLOCK, acc.shape[1]))
    pad[:n] = acc
    part = tree(pad.reshape(nb, BLOCK, -1))
    u = np.zeros((BLOCK, acc.shape[1]))
    with np.errstate(all="ignore"):
        for B in range(nb):
            u[B % BLOCK] = u[B % BLOCK] + part[B]
    return tree(u)


def solve(S, min_pairs, pivot_rel):
    """the 29 sums -> (status, xi): LDL^T without pivoting in scalar f64"""
    f = np.float64
    A = np.zeros((6, 6))
    q = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = S[q]
            q += 1
    bv = S[21:27]
    if S[28] < f(min_pairs):
        return 1, None
    L = np.zeros((6, 6))
    D = np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j, j]
            for k in range(j):
                dj = dj - (L[j, k] * L[j, k]) * D[k]
            D[j] = dj
            if not dj > f(pivot_rel) * A[j, j]:
                return 2, None
            for i in range(j + 1, 6):
                l = A[i, j]
                for k in range(j):
                    l = l - (L[i, k] * L[j, k]) * D[k]
                L[i, j] = l / dj
        y = np.zeros(6)
        for i in range(6):
            v = bv[i]
            for k in range(i):
                v = v - L[i, k] * y[k]
            y[i] = v
        xi = np.zeros(6)
        for i in range(6):
            xi[i] = y[i] / D[i]
        for i in range(5, -1, -1):
            v = xi[i]
            for k in range(i + 1, 6):
                v = v - L[k, i] * xi[k]
            xi[i] = v
    if not np.all(np.isfinite(xi)):
        return 3, None
    return 0, xi


def cayley(om):
    """E of the update, each entry in the written association"""
    f = np.float64
    a0, a1, a2 = f(0.5) * om[0], f(0.5) * om[1], f(0.5) * om[2]
    s = (a0 * a0 + a1 * a1) + a2 * a2
    p, q = f(1.0) - s, f(1.0) + s
    two = f(2.0)
    return np.array([[(p + two * (a0 * a0)) / q, (two * (a0 * a1) - two * a2) / q, (two * (a0 * a2) + two * a1) / q],
                     [(two * (a0 * a1) + two * a2) / q, (p + two * (a1 * a1)) / q, (two * (a1 * a2) - two * a0) / q],
                     [(two * (a0 * a2) - two * a1) / q, (two * (a1 * a2) + two * a0) / q, (p + two * (a2 * a2)) / q]])


def sample_sums(views, w, h, src, targets, R, t, stride, max_dist, huber, min_cos, exits=None):
    """one iteration's per-sample sums (ws*hs, 29) under the source pose (R, t)"""
    n = w * h
    cams = [_cam(v) for v in views]
    depth = [np.asarray(v["depth"], np.float64).reshape(n) for v in views]
    nrm = [np.asarray(v["normal"], np.float64).reshape(3, n) for v in views]
    cs = (cams[src][0], cams[src][1], cams[src][2], np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3))
    ws, hs = (w + stride - 1) // stride, (h + stride - 1) // stride
    q = np.arange(ws * hs)
    xi_, yi_ = (q % ws) * stride, (q // ws) * stride
    m = yi_ * w + xi_
    x, y = xi_.astype(np.float64), yi_.astype(np.float64)
    md2 = np.float64(max_dist) * np.float64(max_dist)
    hub, mc = np.float64(huber), np.float64(min_cos)
    acc = np.zeros((SUMS, ws * hs))
    with np.errstate(all="ignore"):
        Z = depth[src][m]
        valid = np.isfinite(Z) & (Z > 0.0)
        P = _world(cs, x, y, Z)
        Lv = [P[i] - cs[4][i] for i in range(3)]
        Ns = _rot(cs, nrm[src][:, m]) if mc > 0.0 else None
        for k in range(len(views)):
            if not (targets >> k) & 1:
                continue
            go = valid.copy()

            def leave(name, cond, go=go):
                if exits is not None:
                    exits[name] += int((go & ~cond).sum())
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
            N = _rot(cams[k], nrm[k][:, mk])
            leave("normal_nonfinite", _finite3(N))
            d = [Pk[0] - P[0], Pk[1] - P[1], Pk[2] - P[2]]
            leave("far", (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= md2)
            if mc > 0.0:
                leave("normal", (Ns[0] * N[0] + Ns[1] * N[1]) + Ns[2] * N[2] >= mc)
            if exits is not None:
                exits["pair"] += int(go.sum())
            r = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]
            J = [Lv[1] * N[2] - Lv[2] * N[1], Lv[2] * N[0] - Lv[0] * N[2], Lv[0] * N[1] - Lv[1] * N[0], N[0], N[1], N[2]]
            ar = np.abs(r)
            wt = np.where((hub == 0.0) | (ar <= hub), 1.0, hub / ar)
            g = [wt * J[a] for a in range(6)]
            upd = []
            for a in range(6):
                for b in range(a, 6):
                    upd.append(g[a] * J[b])
            for a in range(6):
                upd.append(g[a] * r)
            upd.append((wt * r) * r)
            upd.append(np.ones_like(r))
            for i in range(SUMS):
                acc[i] = np.where(go, acc[i] + upd[i], acc[i])
    return acc.T.copy()


def register(views, w, h, src, targets, R0=None, t0=None, iters=8, stride=1, max_dist=0.5, huber=0.05, min_cos=0.0, min_pairs=100, pivot_rel=1e-8):
    """views as for fuse_ref.fuse (with normals); targets a bit mask.  -> dict(R (3, 3), t (3,), iters (REC records), exits)"""
    R = np.array(views[src]["R"] if R0 is None else R0, np.float64).reshape(3, 3)
    t = np.array(views[src]["t"] if t0 is None else t0, np.float64).reshape(3)
    recs = np.zeros(iters, REC)
    exits = dict.fromkeys(EXITS, 0)
    for it in range(iters):
        S = reduce_samples(sample_sums(views, w, h, src, targets, R, t, stride, max_dist, huber, min_cos, exits))
        status, xi = solve(S, min_pairs, pivot_rel)
        recs[it] = (S[28], S[27], 0.0, 0.0, status)
        if status == 0:
            recs[it]["rot2"] = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]
            recs[it]["trans2"] = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]
            E = cayley(xi[:3])
            R = np.array([[(E[i, 0] * R[0, j] + E[i, 1] * R[1, j]) + E[i, 2] * R[2, j] for j in range(3)] for i in range(3)])
            t = np.array([t[i] + xi[3 + i] for i in range(3)])
    return dict(R=R, t=t, iters=recs, exits=exits)


def same_result(got, want):
    """pose and records bit for bit; NaN positions must agree, NaN payloads need not"""
    from fuse_ref import same_bits
    ok = same_bits(np.asarray(got["R"], np.float64).reshape(9), want["R"].reshape(9)) and same_bits(np.asarray(got["t"], np.float64), want["t"])
    ok = ok and len(got["iters"]) == len(want["iters"]) and np.array_equal(got["iters"]["status"], want["iters"]["status"])
    return bool(ok and all(same_bits(np.ascontiguousarray(got["iters"][k]), np.ascontiguousarray(want["iters"][k])) for k in ("pairs", "cost", "rot2", "trans2")))
