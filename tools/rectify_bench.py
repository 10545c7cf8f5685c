"""What the rectification front end (include/cspm.h "rectification") costs and what it does to a match: JSON lines.

    python tools/rectify_bench.py [--repeats 9] [--warmup 3] [--iters 3] [--no-motorcycle] [--no-quality]

Timing, at the C3 geometry (1242 x 375, synthetic) and the 741 x 500 Motorcycle pair, rectified size = raw size:
    set_rectification   the two map launches (k_rect_map per view), rebuilt for every measurement (the stored rectification is dropped first)
    set_images_raw      the remap bracket (k_pack_bgr + k_rect_remap per view) plus the two brackets of the path it shares with ...
    set_images          ... cspm_set_images: k_pack_bgr per view
each the sum of the library's own hipEvent brackets of the call (CSPM_K_MISC, cspm_get_timing) on the context's stream, one call per
measurement after --warmup calls, median and min - max of --repeats; `wall_ms` is the host's clock round the whole synchronous call, the
host-to-device copy of the pair included.  Bytes: what the launches must move, from the shapes --
    map     17 out per pixel and view
    remap   3 in + 4 out per raw pixel (pack), 17 in per pixel, 4 x 4 gathered per valid pixel, 3 out per pixel
    pack    3 in + 4 out per pixel and view (cspm_set_images' own launches)
-- and the share of the 8 TB/s HBM peak that time and those bytes amount to.  These are launches of a few microseconds: the figure is
launch overhead and latency, not bandwidth, and the JSON says so (`launches`).

Quality, one figure that needs no new data: the C3 pair is "un-rectified" by a distortion-free rotated rig -- each raw view is the
closed-form homography K_v R_v^T K_rect^-1 of the original view, resampled bilinearly on the host --, rectified on the device and
matched; bad-2.0 of the left map beside the untouched pair's, over the pixels with ground truth and, for both, over those that the
rectification also has a source for.  Two resamplings (one here, one on the device) blur the pair: the difference is what that costs."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second, the MI355X's specified peak


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def bench_rig(capi, w, h):
    """a distortion-free rig of the pair's size: two slightly different cameras, camera 1 rotated by 1.5 degrees, a slanted baseline"""
    f = 0.9 * w
    R = rot((0.3, 1.0, 0.2), 1.5)
    C1 = np.array([0.2, 0.006, -0.004])
    return capi.make_rig((f, 1.01 * f, (w - 1) / 2 + 3.0, (h - 1) / 2 - 2.0), (0.99 * f, f, (w - 1) / 2 - 4.0, (h - 1) / 2 + 1.5), R, -R @ C1, w, h)


def unrectify(img, cam, Rv, rect):
    """the raw view of a distortion-free camera whose rectified image is img: the homography K_rect Rv K_v^-1 per raw pixel, bilinear,
    black where the rectified image has nothing"""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    yn = (yy - cam.cy) / cam.fy
    xn = ((xx - cam.cx) - cam.skew * yn) / cam.fx
    P = [Rv[3 * i] * xn + Rv[3 * i + 1] * yn + Rv[3 * i + 2] for i in range(3)]
    sx, sy = rect.f * P[0] / P[2] + rect.cx, rect.f * P[1] / P[2] + rect.cy
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = (sx - x0)[..., None], (sy - y0)[..., None]
    f = img.astype(np.float64)
    top = f[y0, x0] + tx * (f[y0, x1] - f[y0, x0])
    bot = f[y1, x0] + tx * (f[y1, x1] - f[y1, x0])
    out = np.clip(np.rint(top + ty * (bot - top)), 0, 255).astype(np.uint8)
    out[~inside] = 0
    return out


def stats(times):
    return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "repeats": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd, synth

    scenes = []
    c3 = synth.make_config("C3")
    scenes.append(("C3", c3[1], c3[2]))
    full = None if args.no_motorcycle else rd.load_full()
    if full is not None:
        scenes.append(("motorcycle", full[1], full[2]))
    ctx = cs.StereoContext(0)
    note = "launch- and latency-bound at this size: the share of peak is what is left of bandwidth, not a roof that was hit"
    for name, l, r in scenes:
        h, w = l.shape[:2]
        n = w * h
        rig = bench_rig(capi, w, h)
        rect, _ = capi.rectify_compute(rig)
        ctx.enable_timing(True)

        def measure(call, before=None):
            ms, wall = [], []
            for k in range(args.warmup + args.repeats):
                if before:
                    before()
                ctx.synchronize()
                ctx.reset_timing()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                t1 = time.perf_counter()
                t = ctx.timing()["misc"]
                if k >= args.warmup:
                    ms.append(t["ms"])
                    wall.append((t1 - t0) * 1e3)
            return ms, wall, t["launches"]

        ms, wall, brackets = measure(lambda: ctx.set_rectification(rig, rect), before=lambda: ctx.set_rectification(None))
        moved = 2 * n * 17
        row = {"scene": name, "size": f"{w}x{h}", "call": "set_rectification", "launches": 2, "brackets": brackets, "bytes_moved": moved, "pixels": n}
        row.update(stats(ms))
        row.update({"wall_ms_median": round(statistics.median(wall), 4), "share_of_hbm_peak": round(moved / (row["ms_median"] * 1e-3) / HBM_PEAK, 5), "note": note})
        print(json.dumps(row), flush=True)
        valid = sum(int(ctx.rect_map(v)[2].sum()) for v in (0, 1))
        for call, fn, launches, moved in (("set_images_raw", lambda: ctx.set_images_raw(l, r), 6, 2 * n * 7 + 2 * n * 20 + 16 * valid + 2 * n * 7),
                                          ("set_images", lambda: ctx.set_images(l, r), 2, 2 * n * 7)):
            ms, wall, brackets = measure(fn)
            row = {"scene": name, "size": f"{w}x{h}", "call": call, "launches": launches, "brackets": brackets, "bytes_moved": moved, "pixels": n}
            row.update(stats(ms))
            row.update({"wall_ms_median": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                        "share_of_hbm_peak": round(moved / (row["ms_median"] * 1e-3) / HBM_PEAK, 5), "valid_fraction": round(valid / (2 * n), 4), "note": note})
            print(json.dumps(row), flush=True)
        ctx.enable_timing(False)
        ctx.set_rectification(None)

    if not args.no_quality:
        cfg, l, r, gl, _ = c3
        h, w = l.shape[:2]
        rig = bench_rig(capi, w, h)
        # the rectified frame IS the original pair's: same size, f = w, the principal point at the centre
        rect, calib = capi.rectify_compute(rig, f=float(w), cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)
        raws = [unrectify(img, rig.cam[v], list(rect.R1 if v else rect.R0), rect) for v, img in enumerate((l, r))]

        def match(set_images):
            set_images()
            ctx.build_cost_grd(cfg["max_dis"], 35, cfg["scale_num"], cfg["reg_lambda"])
            ctx.patchmatch(args.iters, seed=12345)
            return ctx.disparity_f64(0)

        plain = match(lambda: ctx.set_images(l, r))
        ctx.set_rectification(rig, rect)
        rectified = match(lambda: ctx.set_images_raw(*raws))
        mask = ctx.rect_map(0)[2] != 0
        back = ctx.level_image(0, 0)
        gt_masked = np.where(mask, gl, np.nan)
        print(json.dumps({"scene": "C3", "size": f"{w}x{h}", "quality": "bad-2.0 of the left raw plane disparities, %", "iters": args.iters,
                          "untouched_pair": round(100 * synth.bad_fraction(plain, gl, 2.0), 3),
                          "unrectified_then_rectified_on_device": round(100 * synth.bad_fraction(rectified, gl, 2.0), 3),
                          "untouched_pair_where_rectification_has_a_source": round(100 * synth.bad_fraction(plain, gt_masked, 2.0), 3),
                          "rectified_where_rectification_has_a_source": round(100 * synth.bad_fraction(rectified, gt_masked, 2.0), 3),
                          "valid_fraction_left": round(float(mask.mean()), 4),
                          "mean_abs_difference_of_the_rectified_left_image_from_the_original": round(float(np.mean(np.abs(back[mask].astype(int) - l[mask].astype(int)))), 3),
                          "rig": "distortion-free, camera 1 rotated 1.5 degrees, baseline direction (0.2, 0.006, -0.004)"}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
