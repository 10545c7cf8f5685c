"""The case table of the TSDF tests, shared by test_tsdf_ref.py (CPU: the properties of the specification and
that the table is not vacuous) and test_gpu_tsdf.py (GPU: the library against tests/tsdf_ref.py bit for bit).

The scenes are fuse_cases' analytic renders -- the slanted plane, the occluding rectangle, the wrong-depth blob -- spoiled on purpose:
holes (NaN, inf, 0, negative), speckles of 10 % too small a depth (columns of voxels whose sign differs from their neighbours': lateral
crossings in both directions), random and non-finite normals.  The poses: the identity, a translation, rotations up to 15 degrees, a
camera inside the volume, one behind the surface looking back at it, one that sees none of the volume."""
import functools

import numpy as np

import fuse_cases as fc
import tsdf_ref as tr

# camera -> world poses in the order a case takes them
POSES = [(np.eye(3), np.zeros(3)),
         (np.eye(3), np.array([0.1, 0.0, 3.45])),                 # inside every volume but the thinnest: voxels lie behind it
         (np.eye(3), np.array([0.3, 0.05, 0.5])),
         (fc.rot(3.0, -8.0, 15.0), np.array([0.4, -0.1, 0.0])),
         (fc.rot(ry=180.0), np.array([0.0, 0.0, 8.0])),           # behind the surface, looking back at it
         (fc.rot(ry=90.0), np.array([30.0, 0.0, 0.0]))]           # sees none of the volume
THIN_POSES = [POSES[0], POSES[1], (np.eye(3), np.array([0.3, 0.0, 0.5])), (fc.rot(ry=-8.0), np.array([0.4, 0.0, 0.0])), POSES[4], POSES[5]]
# the raycast cameras of every case: the first view's, a 15 degree rotation, inside the volume, behind the surface, seeing nothing
RAY_POSES = [POSES[0], (fc.rot(ry=15.0), np.array([-0.8, 0.0, 0.2])), (fc.rot(2.0, 5.0, -10.0), np.array([0.1, 0.05, 3.45])), POSES[4], POSES[5]]

# dims -> (voxel, origin): every volume holds part of the plane (z about 4 at the optical axis)
VOLUMES = {(1, 1, 1): (0.5, (-0.25, -0.25, 3.75)),
           (3, 2, 2): (0.4, (-0.6, -0.4, 3.6)),
           (64, 4, 3): (0.1, (-3.2, -0.2, 3.85)),
           (65, 5, 2): (0.1, (-3.25, -0.25, 3.9)),
           (257, 1, 2): (0.03, (-3.855, -0.015, 3.97)),
           (33, 17, 9): (0.2, (-3.3, -1.7, 3.0)),
           (96, 96, 64): (0.05, (-2.4, -2.4, 2.3))}   # 2304 workgroups: three passes of the scan's workgroup, with a carry


def spoil(depth, normal, rng):
    """holes, speckles and bad normals, in place"""
    h, w = depth.shape
    u = rng.uniform(size=(h, w))
    depth[u < 0.02] = np.nan
    depth[(u >= 0.02) & (u < 0.03)] = np.inf
    depth[(u >= 0.03) & (u < 0.04)] = 0.0
    depth[(u >= 0.04) & (u < 0.05)] = -3.0
    depth[(u >= 0.05) & (u < 0.10)] *= 0.9
    if normal is not None:
        q = rng.uniform(size=(h, w))
        rnd = rng.normal(size=(3, h, w))
        rnd /= np.linalg.norm(rnd, axis=0)
        normal[:, q < 0.10] = rnd[:, q < 0.10]
        normal[0, (q >= 0.10) & (q < 0.13)] = np.nan
        normal[1, (q >= 0.13) & (q < 0.15)] = np.inf


@functools.lru_cache(maxsize=None)
def scene(kind, w, h, K, seed, normals, images, spoiled):
    """-> a tuple of K view dicts.  kind: plane, occlusion, blob, identical (K copies of the first view).  images: all, none, some."""
    rng = np.random.default_rng(2000 * seed + 7 * w + 13 * h + K)
    pp = THIN_POSES if h < 8 else POSES
    planes = [(fc.PLANE[0], fc.PLANE[1], None)]
    if kind == "occlusion":
        planes.append((np.array([0.0, 0.0, 1.0]), 2.5, (-0.6, 0.2, -1.0, 1.0)))
    views = []
    for k in range(K):
        R, t = pp[0] if kind == "identical" else pp[k % len(pp)]
        cam = fc.camera(w, h, 0 if kind == "identical" else k, R, t)
        depth, normal, bgr = fc.render(cam, w, h, planes)
        if kind == "blob" and k == 1:
            depth[h // 4:h // 2, w // 4:w // 2] *= 1.2
        if kind == "identical" and k > 0:
            depth, normal = views[0]["depth"], views[0].get("normal", normal)
        elif spoiled:
            spoil(depth, normal, rng)
        with_image = images == "all" or (images == "some" and k % 2 == 1)
        views.append(fc.view(cam, depth, normal if normals else None, bgr if with_image else None))
    return tuple(views)


class Case:
    def __init__(self, name, dims, w, h, K, kind="plane", degenerate=False, cap="exact", seed=0, normals=True, images="all", spoiled=True, **params):
        self.name, self.dims, self.w, self.h, self.K, self.kind, self.degenerate, self.cap = name, tuple(dims), w, h, K, kind, degenerate, cap
        self.scene_args = (kind, w, h, K, seed, normals, images, spoiled)
        self.voxel, self.origin = VOLUMES[self.dims]
        self.params = dict(tr.DEFAULTS, **params)

    def views(self):
        return list(scene(*self.scene_args))

    def ray_cameras(self):
        """the cameras the case's volume is raycast from, at the image size of its views"""
        return [fc.camera(self.w, self.h, 0, R, t) for R, t in RAY_POSES]

    def reference(self):
        """tsdf_ref's volume and every record (computed once per case and shared; nobody writes into it)"""
        return _reference(self)

    def raycasts(self):
        """tsdf_ref's raycasts of the reference volume from ray_cameras() (computed once, shared)"""
        return _raycasts(self)

    def capacity(self):
        count = self.reference()["count"]
        return {"exact": count, "zero": 0, "short": max(count - 1, 0)}[self.cap]

    def reachable_exits(self):
        with_normal_test = self.scene_args[5] and self.params["min_cos"] > 0.0
        return tuple(e for e in tr.EXITS if e != "grazing" or with_normal_test)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _reference(case):
    return tr.fuse(case.views(), case.w, case.h, case.origin, case.voxel, case.dims, **case.params)


@functools.lru_cache(maxsize=None)
def _raycasts(case):
    vol = case.reference()["vol"]
    return tuple(tr.raycast(vol, cam, case.w, case.h, 0.0 if i % 2 == 0 else 0.25) for i, cam in enumerate(case.ray_cameras()))


def _table():
    cases = []
    kinds = ("plane", "occlusion", "blob")
    caps = ("exact", "zero", "short")
    n = 0
    # every volume and every image size, the degenerate ones included (a dimension of 1, fewer voxels than a wave, a 1 x 1 image)
    for dims, (w, h) in (((1, 1, 1), (1, 1)), ((3, 2, 2), (7, 5)), ((64, 4, 3), (65, 5)), ((65, 5, 2), (65, 5)), ((257, 1, 2), (65, 5)),
                         ((33, 17, 9), (7, 5)), ((33, 17, 9), (1, 1)), ((3, 2, 2), (130, 67))):
        for K in (2, 3):
            cases.append(Case(f"{'x'.join(map(str, dims))}_{w}x{h}_K{K}", dims, w, h, K, kind=kinds[n % 3], degenerate=True, seed=n, cap=caps[n % 3],
                              min_cos=(0.0, 0.5)[n % 2], step_rel=(0.5, 1.0)[(n // 2) % 2]))
            n += 1
    # the crosses at the size every path is taken at: K, normals, images, min_cos, step_rel, capacities; trunc given and defaulted
    dims, w, h = (33, 17, 9), 130, 67
    for K in (1, 2, 3, 5):
        for j, (normals, images) in enumerate(((True, "all"), (False, "none"), (True, "some"))):
            mc = (0.0, 0.5)[(n + j) % 2] if normals else 0.0
            cases.append(Case(f"33x17x9_130x67_K{K}_n{int(normals)}_{images}_c{mc}", dims, w, h, K, kind=kinds[n % 3], degenerate=K == 1, seed=n,
                              normals=normals, images=images, cap=caps[n % 3], min_cos=mc, step_rel=(0.5, 1.0)[n % 2], trunc=(0.5, 0.0, 0.35)[n % 3]))
            n += 1
    cases.append(Case("33x17x9_130x67_K3_saturated", dims, w, h, 3, seed=n, max_weight=2.0, trunc=0.5))            # three views, the weight stops at 2
    cases.append(Case("33x17x9_130x67_K3_identical", dims, w, h, 3, kind="identical", degenerate=True, seed=n + 1, trunc=0.5))
    cases.append(Case("33x17x9_130x67_K5_clean", dims, w, h, 5, degenerate=True, spoiled=False, seed=n + 2, trunc=0.5, min_cos=0.5))
    cases.append(Case("96x96x64_130x67_K2", (96, 96, 64), w, h, 2, kind="occlusion", seed=n + 3, cap="short", trunc=0.15))
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
