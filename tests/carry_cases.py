"""The case table of the carry tests, shared by test_carry_ref.py (CPU: the restatement against analytic
geometry, the table is not vacuous) and test_gpu_carry.py (GPU: the library against tests/carry_ref.py bit for bit).

Scenes are rendered by fuse_cases.render: the three-plane corner of register_cases, a single plane, a fronto-parallel wall.  The source
field is the ANALYTIC plane field of the rendered view -- per pixel the disparity plane of the surface that is visible there -- so that
pixels of one surface hold bit-equal planes (depth ties and fill ties then really occur).  A spoiled case damages it on purpose."""
import functools

import numpy as np

import carry_ref as cr
import fuse_cases as fc
import register_cases as rc

B = 0.2  # the baseline of every case
WALL = [(np.array([0.0, 0.0, 1.0]), 3.0, None)]  # fronto-parallel for a camera at the identity


def calib(w, h, doffs=0.0, focal=1.0):
    """(f, cx, cy, baseline, doffs) of fuse_cases.camera(vary=False) at this size; focal scales f"""
    cam = fc.camera(w, h, vary=False)
    return (cam["f"] * focal, cam["cx"], cam["cy"], B, doffs)


def analytic(cal, view, w, h, planes, pose=(np.eye(3), np.zeros(3))):
    """the plane field a camera sees: (field (h, w, 6) with NaN where nothing is hit, index (h, w) of the visible plane or -1).
    pose: camera -> world.  World plane n . P = d is nc . P_cam = dc with nc = R^T n, dc = d - n . t, and in disparity space
    a = B nc0 / dc, b = B nc1 / dc, c = f B nc2 / dc - a cxv - b cy - doffs."""
    k = cr.camera(cal, view)
    R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    cam = dict(f=k["f"], cx=k["cxv"], cy=k["cy"], R=R, t=t)
    depth = np.stack([np.nan_to_num(fc.render(cam, w, h, [p])[0], nan=np.inf) for p in planes])
    index = np.where(np.isfinite(depth.min(axis=0)), depth.argmin(axis=0), -1)
    abc = np.full((len(planes), 3), np.nan)
    for i, (n, d, _) in enumerate(planes):
        nc, dc = R.T @ n, d - n @ t
        a, b = k["B"] * nc[0] / dc, k["B"] * nc[1] / dc
        abc[i] = (a, b, k["fB"] * nc[2] / dc - a * k["cxv"] - b * k["cy"] - k["doffs"])
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    sel = abc[np.maximum(index, 0)]
    field = cr.finish(sel[..., 0], sel[..., 1], x, y, (sel[..., 0] * x + sel[..., 1] * y) + sel[..., 2])
    field[..., 3:6] = sel  # the param part is the analytic plane itself, bit-equal within a surface
    field[index < 0] = np.nan
    return field, index, abc


def spoil(field, k, rng):
    """damaged planes, in place, and a mask: every exit of steps 1 and 2, slopes beyond any range, disparities out of range"""
    h, w = field.shape[:2]
    u = rng.uniform(size=(h, w))
    mask = (u >= 0.05).astype(np.uint8)
    field[(u >= 0.05) & (u < 0.08), 3] = np.nan
    field[(u >= 0.08) & (u < 0.10), 4] = np.inf
    field[(u >= 0.10) & (u < 0.12), 5] = -np.inf
    field[(u >= 0.12) & (u < 0.16), 5] = -1e3                       # tt < 0
    field[(u >= 0.16) & (u < 0.19), 3:6] = (0.0, 0.0, -k["doffs"])  # tt == 0
    field[(u >= 0.19) & (u < 0.23), 3] = 1e306                      # n and hq stay finite, c' does not
    field[(u >= 0.23) & (u < 0.26), 3] = -1e306
    field[(u >= 0.26) & (u < 0.29), 3] = 1e308                      # a * f overflows
    field[(u >= 0.29) & (u < 0.33), 5] += 40.0                      # a surface too near: z > max_dis or behind the target
    field[(u >= 0.33) & (u < 0.37), 3] = 0.999                      # a slope at the edge of visibility
    return mask


RZ180 = (fc.rot(rz=180.0), np.array([0.02, -0.01, 0.05]))
BEHIND = (fc.rot(ry=180.0), np.array([0.0, 0.0, 8.0]))    # beyond the surface, looking back at it: hq <= 0
NOTHING = (fc.rot(ry=90.0), np.array([30.0, 0.0, 0.0]))   # far to the side, looking away
BACKWARD = (np.eye(3), np.array([-0.01, 0.0, -0.05]))     # a small step back: a point at the camera centre still projects inside


class Case:
    """src, dst: (w, h); pose: the target camera -> world pose (the source stands at the identity); view: (source view, target view);
    baseline_shift: the pair's own other view (R = I, t = (-B, 0, 0)) instead of a pose"""

    def __init__(self, name, src, dst, planes=rc.CORNER, pose=rc.TRUE, fill=1, doffs=0.0, focal_t=1.0, view=(0, 0), spoiled=False, seed=0,
                 max_dis=None, baseline_shift=False):
        self.name, self.src, self.dst, self.fill, self.view = name, src, dst, fill, view
        self.planes, self.pose, self.doffs, self.focal_t, self.spoiled, self.seed, self.baseline_shift = planes, pose, doffs, focal_t, spoiled, seed, baseline_shift
        self._max_dis = max_dis

    def inputs(self):
        return _inputs(self)

    def reference(self):
        """carry_ref's result (computed once per case and shared; nobody writes into it)"""
        return _reference(self)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _inputs(case):
    (ws, hs), (wt, ht) = case.src, case.dst
    cal_s, cal_t = calib(ws, hs, case.doffs), calib(wt, ht, case.doffs, case.focal_t)
    if case.baseline_shift:
        cal_t = cal_s
        R, t = np.eye(3), np.array([-B, 0.0, 0.0])
    else:
        R, t = cr.relative_pose(np.eye(3), np.zeros(3), case.pose[0], case.pose[1])
    field, index, _ = analytic(cal_s, case.view[0], ws, hs, case.planes)
    with np.errstate(invalid="ignore"):
        x, y = np.arange(ws, dtype=np.float64)[None, :], np.arange(hs, dtype=np.float64)[:, None]
        top = np.nanmax(np.append(((field[..., 3] * x + field[..., 4] * y) + field[..., 5]).ravel(), 1.0))
    max_dis = int(np.ceil(1.5 * top)) if case._max_dis is None else case._max_dis
    mask = None
    if case.spoiled:
        mask = spoil(field, cr.camera(cal_s, case.view[0]), np.random.default_rng(100 + case.seed))
    return dict(field=field, mask=mask, calib_s=cal_s, calib_t=cal_t, view_s=case.view[0], view_t=case.view[1], R=R, t=t, w_t=wt, h_t=ht,
                max_dis=max_dis, fill=case.fill, index=index)


@functools.lru_cache(maxsize=None)
def _reference(case):
    i = case.inputs()
    return cr.carry(i["field"], cr.camera(i["calib_s"], i["view_s"]), cr.camera(i["calib_t"], i["view_t"]), i["R"], i["t"], i["w_t"], i["h_t"],
                    i["max_dis"], i["mask"], i["fill"])


def _table():
    cases = []
    same = [(1, 1), (7, 5), (64, 4), (65, 5), (257, 1), (130, 67)]
    for n, (w, h) in enumerate(same):
        cases.append(Case(f"corner_{w}x{h}", (w, h), (w, h), fill=1 if n % 2 or (w, h) == (130, 67) else 0))
        cases.append(Case(f"spoiled_{w}x{h}", (w, h), (w, h), pose=BACKWARD, spoiled=True, seed=n, fill=1 - n % 2))
    cases.append(Case("corner_130x67_nofill", (130, 67), (130, 67), fill=0))
    cases.append(Case("corner_130x67_tight", (130, 67), (130, 67), max_dis=9))  # the nearest surfaces exceed max_dis
    # half the focal length on a fronto-parallel wall: four contenders of bit-equal depth per target pixel, the smallest m must win
    cases.append(Case("half_300x220_150x110", (300, 220), (150, 110), planes=WALL, pose=(np.eye(3), np.zeros(3)), focal_t=1.0))
    cases.append(Case("stretch_64x48_130x67", (64, 48), (130, 67)))  # stretch and holes: the fill works
    cases.append(Case("stretch_64x48_130x67_nofill", (64, 48), (130, 67), fill=0))
    for w, h in ((7, 5), (130, 67)):
        cases.append(Case(f"rz180_{w}x{h}", (w, h), (w, h), pose=RZ180))  # the raster order is reversed
    cases.append(Case("behind_130x67", (130, 67), (130, 67), pose=BEHIND))
    cases.append(Case("behind_65x5_wall", (65, 5), (65, 5), planes=WALL, pose=BEHIND))
    cases.append(Case("nothing_130x67", (130, 67), (130, 67), pose=NOTHING))
    cases.append(Case("view0to1_130x67_doffs", (130, 67), (130, 67), doffs=3.5, view=(0, 1), baseline_shift=True))
    cases.append(Case("view0to1_65x5_doffs_spoiled", (65, 5), (65, 5), doffs=-2.25, view=(0, 1), baseline_shift=True, spoiled=True, seed=9))
    cases.append(Case("view1_130x67_doffs", (130, 67), (130, 67), doffs=3.5, view=(1, 1)))
    return cases


BOX = (np.array([0.0, 0.0, 1.0]), 2.5, (-0.6, 0.2, -1.0, 1.0))  # fuse_cases' front rectangle: it hides part of the corner
FRAME_SCENE = rc.CORNER + [BOX]


def texture(P):
    """an 8-bit BGR texture of the world point: enough structure for a matching cost to tell disparities apart"""
    out = []
    for k in range(3):
        v = 128.0 + 55.0 * np.sin(9.0 * P[0] + 3.0 * P[2] + k) * np.sin(11.0 * P[1] + 0.7 * k) + 45.0 * np.sin(23.0 * P[0] + 17.0 * P[1] + 5.0 * P[2] + 2.0 * k)
        out.append(np.clip(v, 0, 255))
    return np.stack(out, -1).astype(np.uint8)


def render_image(cal, view, w, h, pose, planes=None):
    """the textured image view `view` of the pair at `pose` (camera -> world of its view 0) sees, and its exact disparity map"""
    k = cr.camera(cal, view)
    R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    centre = t + R[:, 0] * (k["B"] * view)  # view 1 stands one baseline to the right
    cam = dict(f=k["f"], cx=k["cxv"], cy=k["cy"], R=R, t=centre)
    depth, _, _ = fc.render(cam, w, h, FRAME_SCENE if planes is None else planes)
    x = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1))
    y = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    ray = np.einsum("ij,jhw->ihw", R, np.stack([(x - k["cxv"]) / k["f"], (y - k["cy"]) / k["f"], np.ones((h, w))]))
    P = centre[:, None, None] + np.nan_to_num(depth)[None] * ray
    img = texture(P)
    img[~np.isfinite(depth)] = 0
    return img, k["fB"] / depth - k["doffs"]


@functools.lru_cache(maxsize=None)
def frames(w=96, h=64, n=2, step=1.0):
    """n stereo frames of a rig that moves from the identity towards register_cases.TRUE and beyond, `step` of that motion per frame:
    dict(calib, poses [(R, t)], pairs [(left, right)], truth [(left disparity, right disparity)])"""
    cal = calib(w, h)
    poses = [(fc.rot(1.5 * step * i, -3.0 * step * i, 2.0 * step * i), rc.TRUE[1] * (step * i)) for i in range(n)]
    views = [[render_image(cal, v, w, h, p) for v in (0, 1)] for p in poses]
    return dict(calib=cal, poses=poses, pairs=[(f[0][0], f[1][0]) for f in views], truth=[(f[0][1], f[1][1]) for f in views])


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
