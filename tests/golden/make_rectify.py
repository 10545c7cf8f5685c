"""Regenerates tests/golden/rectify/: a small rig file and a raw pair for tests/test_rectify_cli.py.  The project's own data: the
synthetic 96 x 64 pair of crossscalepatchmatch_amd.synth, "un-rectified" by the rig's distortion-free homographies (the small
distortion coefficients of the rig file are ignored here: the test compares against the restatement of R, not against the pair this
started from).  Run from the repository root:  python tests/golden/make_rectify.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pngio  # noqa: E402
import rectify_ref as rr  # noqa: E402
from crossscalepatchmatch_amd import synth  # noqa: E402

W, H, D = 96, 64, 16


def unrectify(img, K, Rv, rect):
    """the raw view of a distortion-free camera K whose rectified image (projection f, cx, cy; X_rect = Rv X_cam) is img: bilinear, border replicated"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    yn = (yy - K["cy"]) / K["fy"]
    xn = ((xx - K["cx"]) - K["skew"] * yn) / K["fx"]
    P = [Rv[i, 0] * xn + Rv[i, 1] * yn + Rv[i, 2] for i in range(3)]
    sx = np.clip(rect["f"] * P[0] / P[2] + rect["cx"], 0, img.shape[1] - 1)
    sy = np.clip(rect["f"] * P[1] / P[2] + rect["cy"], 0, img.shape[0] - 1)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    x1, y1 = np.minimum(x0 + 1, img.shape[1] - 1), np.minimum(y0 + 1, img.shape[0] - 1)
    tx, ty = (sx - x0)[..., None], (sy - y0)[..., None]
    f = img.astype(np.float64)
    top = f[y0, x0] + tx * (f[y0, x1] - f[y0, x0])
    bot = f[y1, x0] + tx * (f[y1, x1] - f[y1, x0])
    return np.clip(np.rint(top + ty * (bot - top)), 0, 255).astype(np.uint8)


def main():
    out = os.path.join(HERE, "rectify")
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(2024)
    rig = rr.random_rig(rng, raw_w=W, raw_h=H, f=90.0, max_deg=2.0)
    for c in rig["cam"]:  # a gentle lens: most of the rectified image has a source
        for k in ("k1", "k2", "p1", "p2", "k3"):
            c[k] *= 0.25
    rect, _ = rr.compute(rig)
    l, r, _, _ = synth.make_pair(W, H, D, regions=3, seed=12)
    for name, img, v in (("l_raw.png", l, 0), ("r_raw.png", r, 1)):
        raw = unrectify(img, rig["cam"][v], rect["R1" if v else "R0"], rect)
        pngio.write_png(os.path.join(out, name), raw[..., ::-1])  # BGR -> the file's RGB
    g = lambda v: repr(float(v))  # noqa: E731
    with open(os.path.join(out, "rig.txt"), "w") as f:
        f.write("# two 96 x 64 cameras, camera 1 to the right of camera 0: X1 = R*X0 + T\n")
        for v, c in enumerate(rig["cam"]):
            f.write(f"cam{v}=[{g(c['fx'])} {g(c['skew'])} {g(c['cx'])}; 0 {g(c['fy'])} {g(c['cy'])}; 0 0 1]\n")
            f.write(f"dist{v}=[{' '.join(g(c[k]) for k in ('k1', 'k2', 'p1', 'p2', 'k3'))}]\n")
        f.write("R=[" + "; ".join(" ".join(g(x) for x in row) for row in rig["R"]) + "]\n")
        f.write("T=[" + " ".join(g(x) for x in rig["T"]) + "]\n")
        f.write(f"width={W}\nheight={H}\n")


if __name__ == "__main__":
    main()
