"""numpy restatement of the specification R (include/cspm.h "rectification"): the host derivation, the map and
the remap, every operation one IEEE f64 operation in the written association.  Test infrastructure: the product never imports it.

A rig is a dict: cam = two dicts with fx, fy, cx, cy, skew, k1, k2, p1, p2, k3; R (3, 3) with X1 = R X0 + T; T (3,); raw_w, raw_h.
A rectification is a dict: R0, R1 (3, 3), f, cx, cy, baseline, w, h."""
import math

import numpy as np

CAM_KEYS = ("fx", "fy", "cx", "cy", "skew", "k1", "k2", "p1", "p2", "k3")


class RigError(ValueError):
    """what cspm_rectify_compute answers with CSPM_ERR_ARG"""


def camera(fx, fy, cx, cy, skew=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    return dict(zip(CAM_KEYS, (float(v) for v in (fx, fy, cx, cy, skew, k1, k2, p1, p2, k3))))


def make_rig(cam0, cam1, R, T, raw_w, raw_h):
    return {"cam": (dict(cam0), dict(cam1)), "R": np.array(R, np.float64).reshape(3, 3), "T": np.array(T, np.float64).reshape(3),
            "raw_w": int(raw_w), "raw_h": int(raw_h)}


def _cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def compute(rig, f=0.0, cx=math.nan, cy=math.nan, w=0, h=0):
    """the derivation: (rectification, calib) with calib = (f, cx, cy, baseline, 0.0); python floats are IEEE doubles"""
    cams = rig["cam"]
    R = [[float(rig["R"][i][j]) for j in range(3)] for i in range(3)]
    T = [float(t) for t in rig["T"]]
    vals = [c[k] for c in cams for k in CAM_KEYS] + [v for row in R for v in row] + T
    if not all(math.isfinite(v) for v in vals):
        raise RigError("non-finite rig")
    if any(not (c["fx"] > 0.0 and c["fy"] > 0.0) for c in cams):
        raise RigError("fx, fy must be positive")
    if T == [0.0, 0.0, 0.0]:
        raise RigError("T is zero")
    raw_w, raw_h = rig["raw_w"], rig["raw_h"]
    if raw_w < 1 or raw_h < 1 or raw_w * raw_h >= 2 ** 31:
        raise RigError("raw size")
    C1 = [-((R[0][j] * T[0] + R[1][j] * T[1]) + R[2][j] * T[2]) for j in range(3)]
    baseline = math.sqrt((C1[0] * C1[0] + C1[1] * C1[1]) + C1[2] * C1[2])
    if not (baseline > 0.0 and math.isfinite(baseline)):
        raise RigError("baseline")
    e1 = [c / baseline for c in C1]
    if not (e1[0] > 0.0 and abs(e1[0]) >= abs(e1[1]) and abs(e1[0]) >= abs(e1[2])):
        raise RigError("camera 1 must be to the right of camera 0 and the rig horizontal")
    zm = [R[2][0], R[2][1], 1.0 + R[2][2]]
    c = _cross(zm, e1)
    n = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not (n > 0.0 and math.isfinite(n)):
        raise RigError("the mean optical axis is parallel to the baseline")
    e2 = [v / n for v in c]
    e3 = _cross(e1, e2)
    R0 = [e1, e2, e3]
    R1 = [[(R0[i][0] * R[j][0] + R0[i][1] * R[j][1]) + R0[i][2] * R[j][2] for j in range(3)] for i in range(3)]
    if math.isinf(f) or math.isinf(cx) or math.isinf(cy):
        raise RigError("infinite parameter")
    fo = f if f > 0.0 else 0.25 * (((cams[0]["fx"] + cams[0]["fy"]) + cams[1]["fx"]) + cams[1]["fy"])
    wo = w if w > 0 else raw_w
    ho = h if h > 0 else raw_h
    if wo * ho >= 2 ** 31:
        raise RigError("w * h")
    q = []
    for v, Rv in enumerate((R0, R1)):
        k = cams[v]
        yn = (float(raw_h - 1) / 2.0 - k["cy"]) / k["fy"]
        xn = ((float(raw_w - 1) / 2.0 - k["cx"]) - k["skew"] * yn) / k["fx"]
        P = [(Rv[i][0] * xn + Rv[i][1] * yn) + Rv[i][2] for i in range(3)]
        with np.errstate(all="ignore"):
            q.append((float(np.float64(fo * P[0]) / np.float64(P[2])), float(np.float64(fo * P[1]) / np.float64(P[2]))))
    cxo = float(wo - 1) / 2.0 - 0.5 * (q[0][0] + q[1][0]) if math.isnan(cx) else cx
    cyo = float(ho - 1) / 2.0 - 0.5 * (q[0][1] + q[1][1]) if math.isnan(cy) else cy
    if not all(math.isfinite(v) for v in [fo, cxo, cyo, baseline] + [v for row in R0 + R1 for v in row]):
        raise RigError("non-finite rectification")
    rect = {"R0": np.array(R0, np.float64), "R1": np.array(R1, np.float64), "f": fo, "cx": cxo, "cy": cyo, "baseline": baseline, "w": wo, "h": ho}
    return rect, (fo, cxo, cyo, baseline, 0.0)


def rect_map(rig, rect, view):
    """M_v over the whole rectified image: sx, sy (h, w) f64 as computed (also where invalid or NaN), front and valid (h, w) bool"""
    Rv = rect["R1" if view else "R0"]
    k = rig["cam"][view]
    w, h = rect["w"], rect["h"]
    with np.errstate(all="ignore"):
        x = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1))
        y = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
        u = (x - rect["cx"]) / rect["f"]
        wv = (y - rect["cy"]) / rect["f"]
        X = (Rv[0, 0] * u + Rv[1, 0] * wv) + Rv[2, 0]
        Y = (Rv[0, 1] * u + Rv[1, 1] * wv) + Rv[2, 1]
        Z = (Rv[0, 2] * u + Rv[1, 2] * wv) + Rv[2, 2]
        front = Z > 0.0
        a = X / Z
        b = Y / Z
        r2 = a * a + b * b
        rad = 1.0 + r2 * (k["k1"] + r2 * (k["k2"] + r2 * k["k3"]))
        ad = a * rad + ((2.0 * k["p1"]) * a * b + k["p2"] * (r2 + 2.0 * a * a))
        bd = b * rad + (k["p1"] * (r2 + 2.0 * b * b) + (2.0 * k["p2"]) * a * b)
        sx = (k["fx"] * ad + k["skew"] * bd) + k["cx"]
        sy = k["fy"] * bd + k["cy"]
        valid = front & (sx >= 0.0) & (sx <= float(rig["raw_w"] - 1)) & (sy >= 0.0) & (sy <= float(rig["raw_h"] - 1))
    return sx, sy, front, valid


def round2int(v):
    """the project's Round2Int: round half to even through the 2^52 + 2^51 constant (|v| < 2^31)"""
    return ((v + 6755399441055744.0).view(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def remap(raw, sx, sy, valid):
    """raw (raw_h, raw_w, 3) u8 through a map: (h, w, 3) u8, invalid pixels (0, 0, 0)"""
    raw = np.asarray(raw)
    raw_h, raw_w = raw.shape[:2]
    sxs, sys_ = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
    x0 = np.floor(sxs).astype(np.int64)
    y0 = np.floor(sys_).astype(np.int64)
    x1 = np.minimum(x0 + 1, raw_w - 1)
    y1 = np.minimum(y0 + 1, raw_h - 1)
    tx = (sxs - x0)[..., None]
    ty = (sys_ - y0)[..., None]
    img = raw.astype(np.float64)
    i00, i01, i10, i11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top = i00 + tx * (i01 - i00)
    bot = i10 + tx * (i11 - i10)
    val = np.ascontiguousarray(top + ty * (bot - top))
    out = np.clip(round2int(val), 0, 255).astype(np.uint8)
    out[~valid] = 0
    return out


def rectify(rig, rect, view, raw):
    """(bgr, sx, sy, valid u8) of one view: what cspm_rectify_host returns"""
    sx, sy, _, valid = rect_map(rig, rect, view)
    return remap(raw, sx, sy, valid), sx, sy, valid.astype(np.uint8)


# ---- the rigs the tests share ----
def rotation(axis, deg):
    """Rodrigues' formula (test data only: the specification itself needs no trigonometry)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def random_rig(rng, raw_w=67, raw_h=45, f=60.0, max_deg=6.0, distortion=True):
    """the issue's family: rotations up to max_deg about a random axis, baseline direction (1, +-0.1, +-0.1), cameras jittered round
    fx = fy = f, |k1| <= 0.1, |k2| <= 0.02, |p1|, |p2|, |k3| <= 0.005"""
    cams = []
    for _ in range(2):
        d = [rng.uniform(-0.1, 0.1), rng.uniform(-0.02, 0.02), rng.uniform(-0.005, 0.005), rng.uniform(-0.005, 0.005),
             rng.uniform(-0.005, 0.005)] if distortion else [0.0] * 5
        cams.append(camera(f * rng.uniform(0.97, 1.03), f * rng.uniform(0.97, 1.03), (raw_w - 1) / 2.0 + rng.uniform(-2, 2),
                           (raw_h - 1) / 2.0 + rng.uniform(-2, 2), rng.uniform(-0.05, 0.05), *d))
    R = rotation(rng.normal(size=3), rng.uniform(-max_deg, max_deg))
    C1 = rng.uniform(0.1, 0.5) * np.array([1.0, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    return make_rig(cams[0], cams[1], R, -R @ C1, raw_w, raw_h)


def identity_rig():
    """both cameras fx = fy = 64, cx = 23.5, cy = 17.5, no distortion, R = I, T = (-0.25, 0, 0), 48 x 36: everything exact"""
    c = camera(64.0, 64.0, 23.5, 17.5)
    return make_rig(c, c, np.eye(3), (-0.25, 0.0, 0.0), 48, 36)


def behind_rig():
    """both cameras fx = fy = 8, 64 x 48, camera 1 yawed 100 degrees about y, baseline (0.2, 0, 0): rays behind camera 1"""
    c = camera(8.0, 8.0, 31.5, 23.5)
    R = rotation((0.0, 1.0, 0.0), 100.0)
    return make_rig(c, c, R, -R @ np.array([0.2, 0.0, 0.0]), 64, 48)


# ---- the same rigs and rectifications as the binding's structures ----
def capi_rig(rig):
    from crossscalepatchmatch_amd import capi
    cams = [[c[k] for k in CAM_KEYS] for c in rig["cam"]]
    return capi.make_rig(cams[0], cams[1], rig["R"], rig["T"], rig["raw_w"], rig["raw_h"])


def capi_rect(rect):
    from crossscalepatchmatch_amd import capi
    r = capi.Rectification()
    r.R0[:] = [float(v) for v in rect["R0"].reshape(9)]
    r.R1[:] = [float(v) for v in rect["R1"].reshape(9)]
    r.f, r.cx, r.cy, r.baseline, r.w, r.h = rect["f"], rect["cx"], rect["cy"], rect["baseline"], rect["w"], rect["h"]
    return r
