"""The case table of the fusion tests, shared by test_fuse_ref.py (CPU: the table is not vacuous) and
test_gpu_fuse.py (GPU: the library against tests/fuse_ref.py bit for bit).

Scenes are rendered analytically by ray-plane intersection: exact depth along the optical axis, the plane's normal in the camera frame
(facing the camera) and a colour that is a function of the world point.  A GPU case then spoils its maps on purpose -- holes (NaN, inf,
0, negative), speckles of tiny depth, patches of 3 % and of 50 % wrong depth, random and non-finite normals -- so that every state of a
pixel and every exit of the specification's loop occurs in it."""
import functools
import math

import numpy as np

import fuse_ref as fr

PLANE = (np.array([0.10, -0.05, 1.0]) / np.linalg.norm([0.10, -0.05, 1.0]), 4.0)  # n . P = d: a slanted plane about 4 units away


def rot(rx=0.0, ry=0.0, rz=0.0):
    """R = Rz Ry Rx, angles in degrees"""
    ax, ay, az = (math.radians(a) for a in (rx, ry, rz))
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def camera(w, h, k=0, R=None, t=(0.0, 0.0, 0.0), vary=True):
    """view k's pinhole camera: f, cx, cy differ per view when `vary`"""
    s = float(k) if vary else 0.0
    return dict(f=0.9 * max(w, h, 8) * (1.0 + 0.03 * s), cx=0.5 * (w - 1) + 0.3 + 0.5 * s, cy=0.5 * (h - 1) - 0.2 + 0.25 * s,
                R=np.eye(3) if R is None else np.asarray(R, np.float64), t=np.asarray(t, np.float64))


def colour(P):
    """an 8-bit BGR colour of the world point"""
    b = np.clip(128.0 + 30.0 * P[0], 0, 255)
    g = np.clip(128.0 + 30.0 * P[1], 0, 255)
    r = np.clip(40.0 * P[2], 0, 255)
    return np.stack([b, g, r], -1).astype(np.uint8)


def render(cam, w, h, planes):
    """planes: (n, d, box) with box None or (xmin, xmax, ymin, ymax) limiting the plane in world x, y.  The nearest hit in front of the
    camera wins.  -> depth (h, w) (NaN: no hit), normal (3, h, w) in the camera frame facing the camera, bgr (h, w, 3)"""
    x = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1))
    y = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    d_cam = np.stack([(x - cam["cx"]) / cam["f"], (y - cam["cy"]) / cam["f"], np.ones((h, w))])
    d_w = np.einsum("ij,jhw->ihw", cam["R"], d_cam)
    depth = np.full((h, w), np.inf)
    normal = np.full((3, h, w), np.nan)
    bgr = np.zeros((h, w, 3), np.uint8)
    with np.errstate(all="ignore"):
        for n, d, box in planes:
            s = (d - n @ cam["t"]) / np.einsum("i,ihw->hw", n, d_w)
            P = cam["t"][:, None, None] + s[None] * d_w
            hit = np.isfinite(s) & (s > 0.0) & (s < depth)
            if box is not None:
                hit &= (P[0] >= box[0]) & (P[0] <= box[1]) & (P[1] >= box[2]) & (P[1] <= box[3])
            nc = cam["R"].T @ n
            nc = np.where(np.einsum("i,ihw->hw", nc, d_cam)[None] > 0.0, -nc[:, None, None], nc[:, None, None])
            depth = np.where(hit, s, depth)
            normal = np.where(hit[None], nc, normal)
            bgr = np.where(hit[..., None], colour(P), bgr)
    depth[~np.isfinite(depth)] = np.nan
    return depth, normal, bgr


def view(cam, depth, normal=None, bgr=None):
    v = dict(cam, depth=depth)
    if normal is not None:
        v["normal"] = normal
    if bgr is not None:
        v["bgr"] = bgr
    return v


def poses(K, thin, rng, special=False):
    """camera -> world poses: view 0 the identity, view 1 a pure translation (forwards too, so that near speckles lie behind it), then
    rotations about all three axes up to 15 degrees (about y only for a thin image, whose rows must stay rows).  `special`: the last two
    views are a camera behind the surface and one that sees none of it."""
    out = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.3, 0.0 if thin else 0.05, 0.5]))]
    for k in range(2, K):
        if thin:
            R, t = rot(ry=rng.uniform(-8, 8)), np.array([rng.uniform(-0.4, 0.4), 0.0, rng.choice([0.5, 0.0, -0.3])])
        else:
            R = rot(rng.uniform(-3, 3), rng.uniform(-8, 8), rng.uniform(-15, 15))
            t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.1, 0.1), rng.choice([0.5, 0.0, -0.3])])
        out.append((R, t))
    out = out[:K]
    if special and K >= 5:
        out[K - 2] = (np.eye(3), np.array([0.0, 0.0, 8.0]))       # behind the plane, looking away from it
        out[K - 1] = (rot(ry=90.0), np.array([30.0, 0.0, 0.0]))   # far to the side, looking along +x
    return out


def spoil(depth, normal, rng, k):
    """holes, speckles and wrong patches, in place"""
    h, w = depth.shape
    u = rng.uniform(size=(h, w))
    depth[u < 0.03] = np.nan
    depth[(u >= 0.03) & (u < 0.045)] = np.inf
    depth[(u >= 0.045) & (u < 0.06)] = 0.0
    depth[(u >= 0.06) & (u < 0.075)] = -3.0
    depth[(u >= 0.075) & (u < 0.12)] = 0.2                      # near speckles: behind a camera that stands further forward
    depth[(u >= 0.12) & (u < 0.20)] *= 1.03                     # passes the reprojection test, fails the depth test
    depth[(u >= 0.20) & (u < 0.28)] *= 1.5                      # fails the reprojection test
    if normal is not None:
        q = rng.uniform(size=(h, w))
        rnd = rng.normal(size=(3, h, w))
        rnd /= np.linalg.norm(rnd, axis=0)
        normal[:, q < 0.10] = rnd[:, q < 0.10]
        normal[0, (q >= 0.10) & (q < 0.13)] = np.nan
        normal[1, (q >= 0.13) & (q < 0.15)] = np.inf


@functools.lru_cache(maxsize=None)
def scene(kind, w, h, K, seed=0, normals=True, images="all", vary=True, special=False):
    """-> a tuple of K view dicts.  kind: plane, occlusion, blob (exact renders), spoiled (the plane, spoiled), random (random maps),
    identical (K copies of one spoiled view).  images: all, none, some (every second view)."""
    rng = np.random.default_rng(1000 * seed + 7 * w + 13 * h + K)
    thin = h < 8
    pp = poses(K, thin, rng, special)
    planes = [(PLANE[0], PLANE[1], None)]
    if kind == "occlusion":
        planes.append((np.array([0.0, 0.0, 1.0]), 2.5, (-0.6, 0.2, -1.0, 1.0)))  # a front rectangle that hides part of the back plane
    views = []
    for k in range(K):
        R, t = pp[0] if kind == "identical" else pp[k]
        cam = camera(w, h, 0 if kind == "identical" else k, R, t, vary)
        if kind == "random":
            depth = rng.uniform(1.0, 8.0, (h, w))
            normal = rng.normal(size=(3, h, w))
            normal /= np.linalg.norm(normal, axis=0)
            bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        else:
            depth, normal, bgr = render(cam, w, h, planes)
        if kind == "blob" and k == 1:
            depth[h // 4:h // 2, w // 4:w // 2] *= 1.2
        if kind in ("spoiled", "random") or (kind == "identical" and k == 0):
            spoil(depth, normal, rng, k)
        if kind == "identical" and k > 0:
            depth, normal, bgr = views[0]["depth"], views[0].get("normal", normal), views[0].get("bgr", bgr)
        with_image = images == "all" or (images == "some" and k % 2 == 1)
        views.append(view(cam, depth, normal if normals else None, bgr if with_image else None))
    return tuple(views)


class Case:
    def __init__(self, name, w, h, K, kind="spoiled", degenerate=False, cap="exact", seed=0, normals=True, images="all", vary=True, special=False, **params):
        self.name, self.w, self.h, self.K, self.kind, self.degenerate, self.cap = name, w, h, K, kind, degenerate, cap
        self.scene_args = (kind, w, h, K, seed, normals, images, vary, special)
        self.params = dict(fr.DEFAULTS, **params)

    def views(self):
        return list(scene(*self.scene_args))

    def reference(self):
        """fuse_ref's result with every record (computed once per case and shared; nobody writes into it)"""
        return _reference(self)

    def capacity(self):
        count = self.reference()["count"]
        return {"exact": count, "zero": 0, "short": max(count - 1, 0)}[self.cap]

    def reachable_exits(self):
        """the exits of step 4 this case's inputs can reach"""
        if self.K < 2:
            return ()
        with_normal_test = self.scene_args[5] and self.params["min_cos"] > 0.0
        return tuple(e for e in fr.EXITS if e != "normal" or with_normal_test)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _reference(case):
    return fr.fuse(case.views(), case.w, case.h, **case.params)


def _table():
    cases = []
    shapes = [(1, 1), (7, 5), (63, 3), (64, 4), (65, 5), (257, 1), (130, 67)]
    combos = [dict(suppress=1, min_views=2, min_cos=0.0), dict(suppress=0, min_views=1, min_cos=0.9), dict(suppress=1, min_views=1, min_cos=0.9),
              dict(suppress=0, min_views=2, min_cos=0.0), dict(suppress=1, min_views=0, min_cos=0.0), dict(suppress=0, min_views=0, min_cos=0.9)]
    n = 0
    for w, h in shapes:
        tiny = w * h < 64
        for K in ((1, 2, 3, 5) if (w, h) in ((7, 5), (130, 67)) else (2, 3, 5)):
            c = combos[n % len(combos)]
            cases.append(Case(f"{w}x{h}_K{K}_s{c['suppress']}v{c['min_views']}c{c['min_cos']}", w, h, K, degenerate=tiny or K == 1, seed=n,
                              special=K == 5 and not tiny, cap=("exact", "zero", "short")[n % 3], **c))
            n += 1
    w, h = 130, 67
    for i, c in enumerate(combos):  # every parameter combination at one size, the optional inputs varied with it
        cases.append(Case(f"{w}x{h}_K3_combo{i}", w, h, 3, seed=50 + i, normals=i % 2 == 0, images=("all", "none", "some")[i % 3], **c))
    cases.append(Case("130x67_K5_nonormals_someimages", w, h, 5, seed=60, normals=False, images="some", special=True, cap="short"))
    cases.append(Case("130x67_K3_random", w, h, 3, kind="random", degenerate=True, seed=61, min_cos=0.9))  # random maps never agree: nothing is kept
    cases.append(Case("130x67_K3_loose", w, h, 3, seed=62, max_reproj=6.0, max_rel_depth=0.05, min_views=1))
    cases.append(Case("130x67_K3_plane", w, h, 3, kind="plane", degenerate=True, seed=63))
    cases.append(Case("130x67_K3_occlusion", w, h, 3, kind="occlusion", degenerate=True, seed=64))
    cases.append(Case("130x67_K3_blob", w, h, 3, kind="blob", degenerate=True, seed=65))
    cases.append(Case("130x67_K3_identical", w, h, 3, kind="identical", degenerate=True, seed=66, min_views=1))
    cases.append(Case("7x5_K64", 7, 5, 64, degenerate=True, seed=67, min_views=3))
    cases.append(Case("512x513_K2", 512, 513, 2, seed=68, min_views=1))  # two passes of the scan's workgroup per view, with a carry
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
