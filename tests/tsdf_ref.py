"""Specification T of DESIGN.md section 28 (include/cspm.h "TSDF fusion") restated on the CPU: elementwise numpy over the voxels of
the volume (integration, surface points) or the pixels of a raycast, one operation per line in the association the specification
writes, the views and the march as Python loops.  Every product, sum, quotient, floor and square root is one IEEE f64 operation (numpy
f64 never contracts); the casts to f32 round to nearest even like the device's.
The functions also tally what the case table's non-vacuity is checked on: the exit every voxel of an integration took, the status of
every ray and the rays that start inside the box, the crossings per axis and direction and the neighbours refused for W = 0."""
import numpy as np

from fuse_ref import _cam, _proj, _rot, _to_cam
from geom_ref import POINT, same_bits  # noqa: F401  (re-exported: the TSDF tests compare with the same helpers)

DEFAULTS = dict(trunc=0.0, max_weight=64.0, min_cos=0.0, step_rel=0.5)
EXITS = ("behind", "outside", "hole", "occluded", "grazing", "updated")
MAX_STEPS = 1 << 20


def check_params(origin, voxel, dims, trunc=0.0, max_weight=64.0, min_cos=0.0, step_rel=0.5):
    """the validity rules of cspm_tsdf_params"""
    nx, ny, nz = dims
    return bool(np.all(np.isfinite(origin)) and np.isfinite(voxel) and voxel > 0 and min(dims) >= 1 and nx * ny * nz < 2 ** 31 and np.isfinite(trunc)
                and trunc >= 0 and 1 <= max_weight <= 2 ** 24 and 0 <= min_cos <= 1 and 0 < step_rel <= 1)


def lerp(a, b, t):
    return a + t * (b - a)


def new_volume(origin, voxel, dims, trunc=0.0, max_weight=64.0, min_cos=0.0, step_rel=0.5):
    """a cleared volume: D = 1, W = 0, colour (b, g, r, has) = 0"""
    nx, ny, nz = (int(d) for d in dims)
    nvox = nx * ny * nz
    voxel = np.float64(voxel)
    trunc = np.float64(4.0) * voxel if trunc == 0.0 else np.float64(trunc)
    return dict(origin=np.asarray(origin, np.float64), voxel=voxel, dims=(nx, ny, nz), trunc=trunc, max_weight=np.float64(max_weight),
                min_cos=np.float64(min_cos), step=np.float64(step_rel) * trunc, D=np.ones(nvox, np.float32), W=np.zeros(nvox, np.float32),
                C=np.zeros((nvox, 4), np.uint8))


def _indices(vol):
    nx, ny, nz = vol["dims"]
    v = np.arange(nx * ny * nz, dtype=np.int64)
    return v % nx, (v // nx) % ny, v // (nx * ny)


def _centre(vol, a, idx):
    return vol["origin"][a] + (idx.astype(np.float64) + 0.5) * vol["voxel"]


def integrate(vol, view, w, h):
    """one view (a dict as for fuse_ref.fuse) into the volume, in place -> {exit: voxels that left there}"""
    n = w * h
    cam = _cam(view)
    f, cx, cy = cam[0], cam[1], cam[2]
    depth = np.asarray(view["depth"], np.float64).reshape(n)
    nrm = np.asarray(view["normal"], np.float64).reshape(3, n) if view.get("normal") is not None else None
    bgr = np.asarray(view["bgr"], np.uint8).reshape(n, 3) if view.get("bgr") is not None else None
    idx = _indices(vol)
    exits = dict.fromkeys(EXITS, 0)
    with np.errstate(all="ignore"):
        C = [_centre(vol, a, idx[a]) for a in range(3)]
        go = np.ones(len(C[0]), bool)

        def leave(name, cond):
            exits[name] += int((go & ~cond).sum())
            np.logical_and(go, cond, out=go)

        Q = _to_cam(cam, C)
        leave("behind", Q[2] > 0.0)
        pu, pv = _proj(cam, Q)
        fx = np.floor(pu + 0.5)
        fy = np.floor(pv + 0.5)
        leave("outside", (fx >= 0.0) & (fx <= float(w - 1)) & (fy >= 0.0) & (fy <= float(h - 1)))
        m = np.where(go, fy, 0.0).astype(np.int64) * w + np.where(go, fx, 0.0).astype(np.int64)
        Z = depth[m]
        leave("hole", np.isfinite(Z) & (Z > 0.0))
        sdf = Z - Q[2]
        leave("occluded", sdf >= -vol["trunc"])
        if nrm is not None and vol["min_cos"] > 0.0:
            n0, n1, n2 = nrm[0][m], nrm[1][m], nrm[2][m]
            u = fx - cx
            wv = fy - cy
            X = (u * Z) / f
            Y = (wv * Z) / f
            num = (n0 * X + n1 * Y) + n2 * Z
            ln = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            ls = np.sqrt((X * X + Y * Y) + Z * Z)
            c = (-num) / (ln * ls)
            leave("grazing", c >= vol["min_cos"])
        exits["updated"] = int(go.sum())
        d = sdf / vol["trunc"]
        d = np.where(d > 1.0, 1.0, d)
        Wo = vol["W"].astype(np.float64)
        Wn = Wo + 1.0
        Dn = ((vol["D"].astype(np.float64) * Wo + d) / Wn).astype(np.float32)
        Wf = np.where(Wn > vol["max_weight"], vol["max_weight"], Wn).astype(np.float32)
        vol["D"] = np.where(go, Dn, vol["D"])
        vol["W"] = np.where(go, Wf, vol["W"])
        if bgr is not None:
            paint = go & (sdf <= vol["trunc"])
            Wc = np.where(vol["C"][:, 3] != 0, Wo, 0.0)
            den = Wc + 1.0
            for a in range(3):
                co = vol["C"][:, a].astype(np.float64)
                cn = bgr[m, a].astype(np.float64)
                new = np.floor((co * Wc + cn) / den + 0.5)
                vol["C"][:, a] = np.where(paint, new, co).astype(np.uint8)
            vol["C"][:, 3] = np.where(paint, 1, vol["C"][:, 3])
            exits["painted"] = int(paint.sum())
    return exits


def _locate(vol, P):
    """-> ok, base, fr: the cell of the points P (three arrays)"""
    nx, ny, nz = vol["dims"]
    ok = np.ones(len(P[0]), bool)
    c, fr = [], []
    for a, na in enumerate((nx, ny, nz)):
        g = (P[a] - vol["origin"][a]) / vol["voxel"] - 0.5
        fl = np.floor(g)
        ok &= (fl >= 0.0) & (fl <= float(na - 2))
        c.append(np.where(ok, fl, 0.0).astype(np.int64))
        fr.append(g - fl)
    return ok, (c[2] * ny + c[1]) * nx + c[0], fr


def _corner(vol, base, q):
    nx, ny, _ = vol["dims"]
    return base + (q & 1) + ((q >> 1) & 1) * nx + (q >> 2) * nx * ny


def _trilinear(d, fr):
    c00, c10 = lerp(d[0], d[1], fr[0]), lerp(d[2], d[3], fr[0])
    c01, c11 = lerp(d[4], d[5], fr[0]), lerp(d[6], d[7], fr[0])
    return lerp(lerp(c00, c10, fr[1]), lerp(c01, c11, fr[1]), fr[2])


def _sample(vol, P):
    """-> known, base, fr, d (the eight corners' D as f64; garbage where not known)"""
    ok, base, fr = _locate(vol, P)
    base = np.where(ok, base, 0)
    known = ok.copy()
    nvox = len(vol["D"])
    corners = [np.minimum(_corner(vol, base, q), nvox - 1) for q in range(8)]
    for q in range(8):
        known &= vol["W"][corners[q]] > 0.0
    d = [vol["D"][corners[q]].astype(np.float64) for q in range(8)]
    return known, corners, fr, d


def raycast(vol, cam, w, h, z_near=0.0):
    """cam: a dict with f, cx, cy, R, t -> dict(depth (h, w), normal (3, h, w), bgr (h, w, 3), status (h, w), inside: the rays that start
    inside the box (they enter it at z_near))"""
    n = w * h
    k = _cam(cam)
    f, cx, cy, R, t = k
    nx, ny, nz = vol["dims"]
    p = np.arange(n)
    x = (p % w).astype(np.float64)
    y = (p // w).astype(np.float64)
    status = np.zeros(n, np.uint8)
    depth = np.full(n, np.nan)
    normal = np.full((3, n), np.nan)
    px = np.zeros((n, 3), np.uint8)
    with np.errstate(all="ignore"):
        dirs = _rot(k, [(x - cx) / f, (y - cy) / f, np.ones(n)])
        l0 = np.full(n, np.float64(z_near))
        l1 = np.full(n, np.inf)
        inb = np.full(n, min(nx, ny, nz) >= 2)
        for a, na in enumerate((nx, ny, nz)):
            lo = vol["origin"][a] + 0.5 * vol["voxel"]
            hi = vol["origin"][a] + (np.float64(na) - 0.5) * vol["voxel"]
            zero = dirs[a] == 0.0
            inb &= ~zero | ((t[a] >= lo) & (t[a] <= hi))
            ta = (lo - t[a]) / dirs[a]
            tb = (hi - t[a]) / dirs[a]
            swap = ta > tb
            ta, tb = np.where(swap, tb, ta), np.where(swap, ta, tb)
            l0 = np.where(~zero & (ta > l0), ta, l0)
            l1 = np.where(~zero & (tb < l1), tb, l1)
        inb &= l0 <= l1
        inside = int((inb & (l0 == np.float64(z_near))).sum())
        status[inb] = 2
        act = np.flatnonzero(inb)
        has_prev = np.zeros(n, bool)
        prev = np.zeros(n)
        lam_prev = np.zeros(n)
        lam_hit = np.full(n, np.nan)
        step = vol["step"]
        m = 0
        while len(act) and m < MAX_STEPS:
            lam = l0[act] + np.float64(m) * step
            act = act[lam <= l1[act]]
            if not len(act):
                break
            lam = l0[act] + np.float64(m) * step
            P = [t[a] + lam * dirs[a][act] for a in range(3)]
            known, _, fr, d = _sample(vol, P)
            cur = _trilinear(d, fr)
            unknown = act[~known]
            has_prev[unknown] = False
            pos = known & (cur > 0.0)
            has_prev[act[pos]] = True
            prev[act[pos]] = cur[pos]
            lam_prev[act[pos]] = lam[pos]
            end = known & ~(cur > 0.0)
            e = act[end]
            hit = has_prev[e]
            status[e] = np.where(hit, 1, 3)
            lh = lam_prev[e] + (step * prev[e]) / (prev[e] - cur[end])
            lam_hit[e] = np.where(hit, lh, np.nan)
            act = act[~end]
            m += 1
        hits = np.flatnonzero(status == 1)
        depth[hits] = lam_hit[hits]
        if len(hits):
            lam = lam_hit[hits]
            P = [t[a] + lam * dirs[a][hits] for a in range(3)]
            known, corners, fr, d = _sample(vol, P)
            g0 = lerp(lerp(d[1] - d[0], d[3] - d[2], fr[1]), lerp(d[5] - d[4], d[7] - d[6], fr[1]), fr[2])
            g1 = lerp(lerp(d[2] - d[0], d[3] - d[1], fr[0]), lerp(d[6] - d[4], d[7] - d[5], fr[0]), fr[2])
            g2 = lerp(lerp(d[4] - d[0], d[5] - d[1], fr[0]), lerp(d[6] - d[2], d[7] - d[3], fr[0]), fr[1])
            ln = np.sqrt((g0 * g0 + g1 * g1) + g2 * g2)
            nw = [g0 / ln, g1 / ln, g2 / ln]
            for j in range(3):
                nj = (R[0, j] * nw[0] + R[1, j] * nw[1]) + R[2, j] * nw[2]
                normal[j, hits] = np.where(known, nj, np.nan)
            coloured = known.copy()
            for q in range(8):
                coloured &= vol["C"][corners[q], 3] != 0
            for a in range(3):
                c = [vol["C"][corners[q], a].astype(np.float64) for q in range(8)]
                val = np.floor(_trilinear(c, fr) + 0.5)
                px[hits, a] = np.where(coloured, val, 0.0).astype(np.uint8)
    return dict(depth=depth.reshape(h, w), normal=normal.reshape(3, h, w), bgr=px.reshape(h, w, 3), status=status.reshape(h, w), inside=inside)


def _gradient(vol, v, idx):
    """the central differences of D at the voxels v (with their indices idx): (3, len(v)), NaN where a neighbour is missing or unknown"""
    nx, ny, nz = vol["dims"]
    stride = (1, nx, nx * ny)
    nvox = len(vol["D"])
    G = []
    for a, na in enumerate((nx, ny, nz)):
        ok = (idx[a] >= 1) & (idx[a] + 1 < na)
        hi = np.clip(v + stride[a], 0, nvox - 1)
        lo = np.clip(v - stride[a], 0, nvox - 1)
        ok = ok & (vol["W"][hi] > 0.0) & (vol["W"][lo] > 0.0)
        G.append(np.where(ok, vol["D"][hi].astype(np.float64) - vol["D"][lo].astype(np.float64), np.nan))
    return G


def points(vol, cap=None):
    """-> dict(cloud (POINT records, the first `cap`; None = all), count, crossings {(axis, 'down' | 'up'): n} ('down': D > 0 at the voxel,
    <= 0 at its neighbour), refused: in-volume neighbours of a known voxel that have W = 0, points64 (count, 3): the f64 positions)"""
    nx, ny, nz = vol["dims"]
    dims, stride = (nx, ny, nz), (1, nx, nx * ny)
    nvox = nx * ny * nz
    idx = _indices(vol)
    v = np.arange(nvox, dtype=np.int64)
    known = vol["W"] > 0.0
    pos = vol["D"] > 0.0
    keys, crossings, refused = [], {}, 0
    for a in range(3):
        inside = idx[a] + 1 < dims[a]
        nb = np.minimum(v + stride[a], nvox - 1)
        refused += int((known & inside & ~known[nb]).sum())
        f = known & inside & known[nb] & (pos != pos[nb])
        crossings[(a, "down")] = int((f & pos).sum())
        crossings[(a, "up")] = int((f & ~pos).sum())
        keys.append(v[f] * 3 + a)
    keys = np.sort(np.concatenate(keys))
    va, ax = keys // 3, keys % 3
    vb = va + np.asarray(stride, np.int64)[ax]
    ia = [idx[e][va] for e in range(3)]
    ib = [ia[e] + (ax == e) for e in range(3)]
    rec = np.zeros(len(keys), POINT)
    with np.errstate(all="ignore"):
        Da = vol["D"][va].astype(np.float64)
        Db = vol["D"][vb].astype(np.float64)
        t = Da / (Da - Db)
        Ga, Gb = _gradient(vol, va, ia), _gradient(vol, vb, ib)
        P = [lerp(_centre(vol, e, ia[e]), _centre(vol, e, ib[e]), t) for e in range(3)]
        G = [lerp(Ga[e], Gb[e], t) for e in range(3)]
        ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
        for e, name in enumerate(("x", "y", "z")):
            rec[name] = P[e].astype(np.float32)
        for e, name in enumerate(("nx", "ny", "nz")):
            rec[name] = (G[e] / ln).astype(np.float32)
        both = (vol["C"][va, 3] != 0) & (vol["C"][vb, 3] != 0)
        for e, name in enumerate(("b", "g", "r")):
            val = np.floor(lerp(vol["C"][va, e].astype(np.float64), vol["C"][vb, e].astype(np.float64), t) + 0.5)
            rec[name] = np.where(both, val, 0.0).astype(np.uint8)
        rec["a"] = np.where(both, 255, 0)
    rec["pixel"] = va
    count = len(rec)
    return dict(cloud=rec if cap is None else rec[:cap], count=count, crossings=crossings, refused=refused,
                points64=np.stack(P, -1) if count else np.zeros((0, 3)))


def fuse(views, w, h, origin, voxel, dims, cap=None, **params):
    """the one-shot entry: every view integrated in list order into a cleared volume, then the surface points.
    -> dict(D, W, C, cloud, count, exits (summed over the views), crossings, refused, vol)"""
    vol = new_volume(origin, voxel, dims, **params)
    exits = dict.fromkeys(EXITS, 0)
    for view in views:
        for name, cnt in integrate(vol, view, w, h).items():
            exits[name] = exits.get(name, 0) + cnt
    out = points(vol, cap)
    out.update(D=vol["D"], W=vol["W"], C=vol["C"], exits=exits, vol=vol)
    return out
