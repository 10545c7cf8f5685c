"""What view synthesis (include/cspm.h "view synthesis") costs and what it is good for: one JSON line per case.

    python tools/synth_bench.py [--repeats 9] [--warmup 3] [--no-motorcycle] [--no-quality]

Timing: ms per cspm_synthesize_device call at t = 0.5 on the C3 geometry (1242 x 375, synthetic) and the 741 x 500 Motorcycle pair, after
one PatchMatch iteration, source RAW: views 3 and 1, with and without the fill, every output requested.  Time: the library's own hipEvent
bracket around the call's launches on the context's stream (CSPM_K_MISC, cspm_get_timing), one call per measurement, after --warmup
calls; median and min - max of --repeats.  A call is one launch per view of the disparity snapshot and one of the row kernel.

Quality on Motorcycle: view 1 rendered from view 0 alone (t = 1, views = 1) against the real right photograph, with the fill and
without it: PSNR over all pixels (fill on), over the pixels the warp itself reached (the mask before the fill), and the hole fraction
before the fill.  Fields: RAW after 1 iteration, RAW after 3 iterations, PP (after 3); each with the plane slopes and, as the contrast
the feature exists for, with the slopes dropped (A = NULL through cspm_synthesize_host on the same maps).  No figure is a pass bar."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def psnr(a, b, where=None):
    import numpy as np
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    if where is not None:
        d = d[where]
    mse = float(d.mean()) if d.size else math.nan
    return round(10.0 * math.log10(255.0 * 255.0 / mse), 3) if mse > 0 else math.inf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd, synth

    scenes = []
    c, l, r, _, _ = synth.make_config("C3")
    scenes.append(("C3", c, l, r))
    full = None if args.no_motorcycle else rd.load_full()
    if full is not None:
        scenes.append(("motorcycle", full[0], full[1], full[2]))
    ctx = cs.StereoContext(0)
    for name, c, l, r in scenes:
        h, w = l.shape[:2]
        n = w * h
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        ctx.patchmatch(1)
        ctx.synchronize()
        bgr = torch.empty((h, 3 * w), dtype=torch.uint8, device="cuda")
        disp = torch.empty((h, w), dtype=torch.float64, device="cuda")
        mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.enable_timing(True)
        for views in (3, 1):
            for fill in (1, 0):
                times = []
                for k in range(args.warmup + args.repeats):
                    ctx.reset_timing()
                    ctx.synthesize_device(0.5, capi.GEOM_RAW, d_bgr=bgr.data_ptr(), d_disp=disp.data_ptr(), d_mask=mask.data_ptr(), views=views, fill=fill)
                    ctx.synchronize()
                    t = ctx.timing()["misc"]
                    assert t["launches"] == 1 and t["evals"] == n, t
                    if k >= args.warmup:
                        times.append(t["ms"])
                holes = float((mask == 0).float().mean().item())
                print(json.dumps({"part": "timing", "scene": name, "size": f"{w}x{h}", "t": 0.5, "views": views, "fill": fill,
                                  "ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                                  "repeats": len(times), "launches": (2 if views == 3 else 1) + 1, "pixels": n, "holes_left": round(holes, 5)}), flush=True)
        ctx.enable_timing(False)
        if name != "motorcycle" or args.no_quality:
            continue
        fields = []  # (label, D of view 0, A of view 0)
        planes = ctx.get_planes(0)[0]
        fields.append(("RAW, 1 iteration", ctx.disparity_f64(0), planes[..., 3].copy()))
        ctx.patchmatch(3)
        planes = ctx.get_planes(0)[0]
        fields.append(("RAW, 3 iterations", ctx.disparity_f64(0), planes[..., 3].copy()))
        maps = ctx.postprocess_f64(valid=True)
        fields.append(("PP, 3 iterations", maps[0], np.where(maps[2] != 0, planes[..., 3], 0.0)))
        for label, D, A in fields:
            for slopes in (True, False):
                kw = dict(slope_a=(A if slopes else None, None), views=1)
                filled = capi.synthesize_host(1.0, (D, None), (l, None), fill=1, **kw)
                raw = capi.synthesize_host(1.0, (D, None), (l, None), fill=0, **kw)
                reached = raw["mask"] != 0
                print(json.dumps({"part": "quality", "scene": name, "size": f"{w}x{h}", "field": label, "slopes": slopes, "t": 1.0, "views": 1,
                                  "psnr_all_filled": psnr(filled["bgr"], r), "psnr_all_holes_black": psnr(raw["bgr"], r), "psnr_unfilled_pixels": psnr(raw["bgr"], r, reached),
                                  "hole_fraction_before_fill": round(float(np.mean(~reached)), 5)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
