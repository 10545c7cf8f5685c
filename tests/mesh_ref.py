"""Specification M of DESIGN.md section 24 (include/cspm.h "triangle meshes") restated on the CPU, twice:
mesh_py -- quad by quad in Python floats, line by line as the specification writes it, on geom_ref.reproject_pixel;
mesh    -- elementwise numpy with the same association, on geom_ref.reproject.
Every product, sum and difference is one IEEE f64 operation (Python floats and numpy f64 never contract)."""
import math

import numpy as np

import geom_ref as gr

POINT = gr.POINT
FACE = np.dtype([("v", "<u4", 3)])
assert FACE.itemsize == 12

# the corners of the four triangles as (dx, dy) from the quad origin, in the order the specification writes them
MAIN = (((0, 0), (0, 1), (1, 1)), ((0, 0), (1, 1), (1, 0)))
ANTI = (((0, 0), (0, 1), (1, 0)), ((1, 0), (0, 1), (1, 1)))


def check_args(max_diff=1.0, **_):
    """True when an entry would accept the mesh parameters"""
    return max_diff >= 0.0


def _geom(params):
    return {k: params[k] for k in ("z_near", "z_far", "min_cos", "left_frame") if k in params}


def _slopes_py(A, Bs, y, x):
    if A is None:
        return 0.0, 0.0
    a, b = float(A[y, x]), float(Bs[y, x])
    return (a, b) if math.isfinite(a) and math.isfinite(b) else (0.0, 0.0)


def mesh_py(calib, v, D, V=None, A=None, Bs=None, img=None, max_diff=1.0, all_vertices=0, vertex_cap=None, face_cap=None, **params):
    """one quad at a time.  -> dict(quad (h, w) uint8, n_vertices, n_faces, vertices (POINT), faces (FACE), vert (h, w) bool)"""
    D = np.asarray(D, np.float64)
    h, w = D.shape
    tau = float(max_diff)
    g = _geom(params)
    pix = [[gr.reproject_pixel(calib, v, x, y, D[y, x], 1 if V is None else int(V[y, x] != 0), None if A is None else A[y, x],
                               None if A is None else Bs[y, x], **g) for x in range(w)] for y in range(h)]
    K = lambda p: pix[p[1]][p[0]]["keep"]

    def pred(s, t):
        a, b = _slopes_py(A, Bs, s[1], s[0])
        return (float(D[s[1], s[0]]) + a * float(t[0] - s[0])) + b * float(t[1] - s[1])

    def E(s, t):
        return abs(pred(s, t) - float(D[t[1], t[0]])) <= tau and abs(pred(t, s) - float(D[s[1], s[0]])) <= tau

    Q = np.zeros((h, w), np.uint8)
    tris = []  # corner pixels of the emitted triangles, in face order
    used = np.zeros((h, w), bool)
    for y in range(h - 1):
        for x in range(w - 1):
            p00, p10, p01, p11 = (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
            main_ok, anti_ok = K(p00) and K(p11), K(p10) and K(p01)
            if not main_ok and not anti_ok:
                continue
            if main_ok and not anti_ok:
                anti = False
            elif anti_ok and not main_ok:
                anti = True
            else:
                anti = not (abs(float(D[y, x]) - float(D[y + 1, x + 1])) <= abs(float(D[y, x + 1]) - float(D[y + 1, x])))
            q = 4 if anti else 0
            for k, tri in enumerate(ANTI if anti else MAIN):
                c = [(x + dx, y + dy) for dx, dy in tri]
                if all(K(p) for p in c) and E(c[0], c[1]) and E(c[1], c[2]) and E(c[2], c[0]):
                    q |= 1 << k
                    tris.append(c)
                    for p in c:
                        used[p[1], p[0]] = True
            Q[y, x] = q
    vert = np.array([[bool(K((x, y))) and (bool(all_vertices) or bool(used[y, x])) for x in range(w)] for y in range(h)], bool).reshape(h, w)
    number = {}
    recs = []
    for y in range(h):
        for x in range(w):
            if vert[y, x]:
                number[(x, y)] = len(recs)
                p = pix[y][x]
                r = np.zeros((), POINT)
                with np.errstate(all="ignore"):
                    r["x"], r["y"], r["z"] = np.float32(p["X"]), np.float32(p["Y"]), np.float32(p["Z"])
                    r["nx"], r["ny"], r["nz"] = (np.float32(t) for t in p["N"])
                r["pixel"] = y * w + x
                if img is not None:
                    r["b"], r["g"], r["r"], r["a"] = img[y, x, 0], img[y, x, 1], img[y, x, 2], 255
                recs.append(r)
    vertices = np.array(recs, POINT) if recs else np.zeros(0, POINT)
    faces = np.zeros(len(tris), FACE)
    for k, c in enumerate(tris):
        faces["v"][k] = [number[p] for p in c]
    nv, nf = len(vertices), len(faces)
    return dict(quad=Q, n_vertices=nv, n_faces=nf, vertices=vertices[:vertex_cap], faces=faces[:face_cap], vert=vert)


def mesh(calib, v, D, V=None, A=None, Bs=None, img=None, max_diff=1.0, all_vertices=0, vertex_cap=None, face_cap=None, **params):
    """D (h, w) f64; V, A, Bs, img as for geom_ref.reproject; the geometry parameters in params.
    -> dict(quad, n_vertices, n_faces, vertices, faces, vert, keep (h, w) bool, xyz (3, h, w) the f64 points, normal (3, h, w) or None,
    vmap (h, w) int64: the vertex number, -1 elsewhere)"""
    D = np.asarray(D, np.float64)
    h, w = D.shape
    tau = np.float64(max_diff)
    res = gr.reproject(calib, v, D, V, A, Bs, img, **_geom(params))
    K = res["keep"].astype(bool)
    if A is None:
        a = b = np.zeros((h, w))
    else:
        A, Bs = np.asarray(A, np.float64), np.asarray(Bs, np.float64)
        fin = np.isfinite(A) & np.isfinite(Bs)
        a, b = np.where(fin, A, 0.0), np.where(fin, Bs, 0.0)
    Q = np.zeros((h, w), np.uint8)
    corner = lambda M, d: M[d[1]:h - 1 + d[1], d[0]:w - 1 + d[0]]  # the map at offset d from every quad origin

    def E(s, t):
        dx, dy = np.float64(t[0] - s[0]), np.float64(t[1] - s[1])
        Ds, Dt = corner(D, s), corner(D, t)
        pst = (Ds + corner(a, s) * dx) + corner(b, s) * dy
        pts = (Dt + corner(a, t) * (-dx)) + corner(b, t) * (-dy)
        return (np.abs(pst - Dt) <= tau) & (np.abs(pts - Ds) <= tau)

    emitted = np.zeros((max(h - 1, 0), max(w - 1, 0), 2), bool)
    corners = np.zeros((max(h - 1, 0), max(w - 1, 0), 2, 3), np.int64)  # pixel indices of the chosen split's corners
    if h > 1 and w > 1:
        with np.errstate(all="ignore"):
            k00, k10, k01, k11 = (corner(K, d) for d in ((0, 0), (1, 0), (0, 1), (1, 1)))
            main_ok, anti_ok = k00 & k11, k10 & k01
            tie = np.abs(corner(D, (0, 0)) - corner(D, (1, 1))) <= np.abs(corner(D, (1, 0)) - corner(D, (0, 1)))
            anti = np.where(main_ok & anti_ok, ~tie, anti_ok)
            some = main_ok | anti_ok
            oy, ox = np.mgrid[0:h - 1, 0:w - 1]
            for split, tris in ((False, MAIN), (True, ANTI)):
                sel = some & (anti == split)
                for k, tri in enumerate(tris):
                    ok = sel & corner(K, tri[0]) & corner(K, tri[1]) & corner(K, tri[2]) & E(tri[0], tri[1]) & E(tri[1], tri[2]) & E(tri[2], tri[0])
                    emitted[..., k] |= ok
                    for j, d in enumerate(tri):
                        corners[..., k, j] = np.where(sel, (oy + d[1]) * w + (ox + d[0]), corners[..., k, j])
            Q[:h - 1, :w - 1] = emitted[..., 0] * 1 + emitted[..., 1] * 2 + (some & anti) * 4
    used = np.zeros(h * w, bool)
    used[corners[emitted].ravel()] = True
    vert = K & (used.reshape(h, w) | bool(all_vertices))
    vmap = np.full(h * w, -1, np.int64)
    idx = np.flatnonzero(vert.ravel())
    vmap[idx] = np.arange(len(idx))
    cloud = res["cloud"]  # every kept pixel in raster order
    vertices = cloud[vert.ravel()[cloud["pixel"]]]
    faces = np.zeros(int(emitted.sum()), FACE)
    faces["v"] = vmap[corners[emitted]]
    nv, nf = len(vertices), len(faces)
    return dict(quad=Q, n_vertices=nv, n_faces=nf, vertices=vertices[:vertex_cap], faces=faces[:face_cap], vert=vert, keep=K, xyz=_points(calib, v, D, params),
                normal=res["normal"], vmap=vmap.reshape(h, w))


def _points(calib, v, D, params):
    """the f64 points (X, Y, Z) of every pixel, not masked: G's arithmetic"""
    f, cx, cy, baseline, doffs = (np.float64(t) for t in calib)
    h, w = D.shape
    with np.errstate(all="ignore"):
        Z = (f * baseline) / (D + doffs)
        X = ((np.arange(w, dtype=np.float64)[None, :] - (cx + np.float64(v) * doffs)) * Z) / f
        Y = ((np.arange(h, dtype=np.float64)[:, None] - cy) * Z) / f
        if params.get("left_frame") and v == 1:
            X = X + baseline
    return np.stack([X, Y, Z])


def same_mesh(got, want, what=""):
    """the quad bytes, both counts, the vertex records and the faces, bit for bit (any NaN equals any NaN); returns a message or None"""
    for name in ("n_vertices", "n_faces"):
        if name in got and got[name] != want[name]:
            return f"{what}: {name} {got[name]} != {want[name]}"
    if "quad" in got and not np.array_equal(got["quad"], want["quad"]):
        return f"{what}: quad bytes differ in {int(np.sum(got['quad'] != want['quad']))} places"
    if "vertices" in got and not gr.same_cloud(got["vertices"], want["vertices"]):
        return f"{what}: vertices"
    if "faces" in got and not (got["faces"].dtype == FACE and np.array_equal(got["faces"]["v"], want["faces"]["v"])):
        return f"{what}: faces"
    return None
