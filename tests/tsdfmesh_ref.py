"""Specification MC of DESIGN.md section 29 (include/cspm.h "TSDF meshes") restated on the CPU on top of tsdf_ref.points: the case table
derived from the specification's rule (nothing is read from the committed header), the faces of a volume as numpy arrays, and the
topological helpers the tests share (directed edges, Euler characteristic, signed volume)."""
import functools

import numpy as np

import tsdf_ref as tr

FACE = np.dtype([("v", "<u4", 3)])
assert FACE.itemsize == 12
MAX_TRIS = 5


def corner_offsets(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_axis(e):
    return e >> 2


def edge_corners(e):
    """the two corner numbers of edge e = 4*a + u + 2*w, the lower one first"""
    a, u, w = e >> 2, e & 1, (e >> 1) & 1
    o = [0, 0, 0]
    others = [i for i in range(3) if i != a]
    o[others[0]], o[others[1]] = u, w
    lo = o[0] | o[1] << 1 | o[2] << 2
    return lo, lo | 1 << a


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def cube_faces():
    """[(axis, side, [four corner numbers counter-clockwise seen from outside])]"""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            ring = [(side << a) | (ob << b) | (oc << c) for ob, oc in ((0, 0), (1, 0), (1, 1), (0, 1))]
            out.append((a, side, ring if side else ring[::-1]))
    return out


def face_segments(case, ring):
    """the marching-squares segments of one cube face: [(entering edge, leaving edge)], one per maximal run of positive corners"""
    s = [(case >> c) & 1 for c in ring]
    segs = []
    for i in range(4):
        if s[i] or not s[(i + 1) % 4]:
            continue
        j = (i + 1) % 4                      # the run starts at corner j = i + 1
        while s[(j + 1) % 4]:
            j = (j + 1) % 4
        segs.append((EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))], EDGE_OF[frozenset((ring[j], ring[(j + 1) % 4]))]))
    return segs


def sign_change_edges(case):
    return [e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1]


def case_triangles(case):
    nxt = {}
    for _, _, ring in cube_faces():
        for e_in, e_out in face_segments(case, ring):
            assert e_in not in nxt
            nxt[e_in] = e_out
    assert sorted(nxt) == sorted(nxt.values()) == sign_change_edges(case)
    tris, done = [], set()
    for start in sorted(nxt):
        if start in done:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        done.update(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i + 1], loop[i]))
    return tris


@functools.lru_cache(maxsize=None)
def table():
    """-> a tuple of 256 tuples of triangles (three edge numbers each)"""
    return tuple(tuple(case_triangles(case)) for case in range(256))


@functools.lru_cache(maxsize=None)
def table_arrays():
    """-> counts (256,), edges (256, 5, 3) (unused entries 0)"""
    counts = np.zeros(256, np.int64)
    edges = np.zeros((256, MAX_TRIS, 3), np.int64)
    for case, tris in enumerate(table()):
        counts[case] = len(tris)
        for t, tri in enumerate(tris):
            edges[case, t] = tri
    return counts, edges


def flags(vol):
    """(3, nvox) bool: voxel v's +x, +y, +z neighbour is a counted neighbour of T's surface points"""
    nx, ny, nz = vol["dims"]
    dims, stride = (nx, ny, nz), (1, nx, nx * ny)
    nvox = nx * ny * nz
    v = np.arange(nvox, dtype=np.int64)
    idx = (v % nx, (v // nx) % ny, v // (nx * ny))
    known = vol["W"] > 0.0
    pos = vol["D"] > 0.0
    f = np.zeros((3, nvox), bool)
    for a in range(3):
        nb = np.minimum(v + stride[a], nvox - 1)
        f[a] = known & (idx[a] + 1 < dims[a]) & known[nb] & (pos != pos[nb])
    return f


def cells(vol):
    """-> v0 (the corner-0 voxels of the KNOWN cells in flat order), case (their cases), n_cells (all cells), unknown (int)"""
    nx, ny, nz = vol["dims"]
    if min(nx, ny, nz) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0, 0
    v = np.arange(nx * ny * nz, dtype=np.int64)
    i, j, k = v % nx, (v // nx) % ny, v // (nx * ny)
    v0 = v[(i <= nx - 2) & (j <= ny - 2) & (k <= nz - 2)]
    known = np.ones(len(v0), bool)
    case = np.zeros(len(v0), np.int64)
    for c in range(8):
        dx, dy, dz = corner_offsets(c)
        q = v0 + dx + dy * nx + dz * nx * ny
        known &= vol["W"][q] > 0.0
        case |= (vol["D"][q] > 0.0).astype(np.int64) << c
    return v0[known], case[known], len(v0), int((~known).sum())


def mesh(vol, vertex_cap=None, face_cap=None):
    """-> dict(vertices (POINT records, the first vertex_cap), n_vertices, faces (FACE records, the first face_cap), n_faces, all_faces
    (n_faces, 3) int64, cases (the known cells' cases), cell_of_face, unknown_cells)"""
    pts = tr.points(vol, vertex_cap)
    nx, ny, nz = vol["dims"]
    f = flags(vol)
    per_voxel = f.sum(0)
    first = np.cumsum(per_voxel) - per_voxel
    assert int(per_voxel.sum()) == pts["count"]
    v0, case, n_cells, unknown = cells(vol)
    counts, edges = table_arrays()
    cnt = counts[case]
    out = np.full((len(v0), MAX_TRIS, 3), -1, np.int64)
    for t in range(MAX_TRIS):
        for m in range(3):
            e = edges[case, t, m]
            a, u, w = e >> 2, e & 1, (e >> 1) & 1
            o0 = np.where(a == 0, 0, u)
            o1 = np.where(a == 0, u, np.where(a == 1, 0, w))
            o2 = np.where(a == 2, 0, w)
            vu = v0 + o0 + o1 * nx + o2 * nx * ny
            num = first[vu] + np.where(a >= 1, f[0][vu], 0) + np.where(a >= 2, f[1][vu], 0)
            assert np.all(f[a, vu][cnt > t])       # a sign-change edge of a known cell is a counted neighbour
            out[:, t, m] = np.where(cnt > t, num, -1)
    keep = np.arange(MAX_TRIS)[None, :] < cnt[:, None]
    all_faces = out[keep]
    cell_of_face = np.repeat(v0, cnt)
    rec = np.zeros(len(all_faces), FACE)
    rec["v"] = all_faces
    return dict(vertices=pts["cloud"], n_vertices=pts["count"], faces=rec if face_cap is None else rec[:face_cap], n_faces=len(all_faces),
                all_faces=all_faces, cases=case, cell_of_face=cell_of_face, unknown_cells=unknown, n_cells=n_cells, points64=pts["points64"])


def volume(D, W=None, C=None, origin=(0.0, 0.0, 0.0), voxel=1.0):
    """a tsdf_ref volume around the given field D of shape (nz, ny, nx)"""
    D = np.asarray(D, np.float32)
    nz, ny, nx = D.shape
    vol = tr.new_volume(origin, voxel, (nx, ny, nz))
    vol["D"] = D.reshape(-1).copy()
    vol["W"] = np.ones(D.size, np.float32) if W is None else np.asarray(W, np.float32).reshape(-1).copy()
    if C is not None:
        vol["C"] = np.asarray(C, np.uint8).reshape(-1, 4).copy()
    return vol


def directed_edges(faces):
    """{(a, b): how often the directed edge a -> b occurs in the faces}"""
    out = {}
    for tri in np.asarray(faces).reshape(-1, 3).tolist():
        for m in range(3):
            key = (tri[m], tri[(m + 1) % 3])
            out[key] = out.get(key, 0) + 1
    return out


def euler(faces):
    """V_used - E + F of the faces"""
    faces = np.asarray(faces).reshape(-1, 3)
    und = {frozenset(k) for k in directed_edges(faces)}
    return len(np.unique(faces)) - len(und) + len(faces)


def signed_volume(faces, xyz):
    """the sum of the signed tetrahedra (origin, v0, v1, v2): positive when the normals (v1 - v0) x (v2 - v0) point out of the solid"""
    p = xyz[np.asarray(faces).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def noise_volume(seed=7, dims=(33, 17, 9)):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(nz, ny, nx)).astype(np.float32)


def sphere_field(n, radius, centre=None):
    """D < 0 inside a sphere: the solid is where D <= 0, the free space outside"""
    c = (n - 1) / 2.0 if centre is None else centre
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    return (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - radius).astype(np.float32)


def torus_field(n, R, r):
    c = (n - 1) / 2.0
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    q = np.sqrt((x - c) ** 2 + (y - c) ** 2) - R
    return (np.sqrt(q * q + (z - c) ** 2) - r).astype(np.float32)
