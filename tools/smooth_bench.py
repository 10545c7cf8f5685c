"""What the edge-aware global smoother of the sub-pixel post-processing does to accuracy and time: the first
six synthetic C3 pairs (1242x375, D = 128, seeds 2000 .. 2005) and, where the checkout has it, Motorcycle 741x500 D = 64, each after
PatchMatch with seed 12345 and 3 iterations.  Per pair, for smoothing off and for lambda x fill_conf (sigma_color and iterations at
their defaults): bad-2.0 of the left f64 post-processed map, its mean absolute error over the pixels with ground truth, and the
CSPM_K_POST milliseconds of cspm_postprocess_f64_device (three repeats after a warm-up: median, minimum, maximum).  One JSON line per
pair and setting, then one markdown table of the means per input.

    python tools/smooth_bench.py [--lambdas 25,100,400] [--fill_confs 0,0.25,1] [--pairs 6] [--reps 3] [--median 0]
With --lambdas "" the script touches nothing the smoother added (no setter is called), so the same file run against a checkout of the
parent commit gives the row to compare the off row with: equal errors, times within the spread of the repeats.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mean_abs_error(disp, gt):
    known = np.isfinite(gt)  # the pixels synth.bad_fraction counts
    return float(np.mean(np.abs(disp[known] - gt[known])))


def measure(ctx, torch, name, l, r, gt, D, settings, reps):
    from crossscalepatchmatch_amd import capi, synth
    h, w = l.shape[:2]
    ctx.set_images(l, r)
    ctx.build_cost_grd(D, 35, 5, 0.3)
    ctx.patchmatch(3, seed=12345, schedule=capi.SCHED_RASTER)
    ctx.synchronize()
    o64 = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    rows = []
    for setting in settings:
        if setting is not None:
            ctx.set_pp_smooth(lam=setting[0], fill_conf=setting[1])
        row = {"pair": name, "w": w, "h": h, "max_dis": D, "lambda": setting[0] if setting else 0.0, "fill_conf": setting[1] if setting else None}
        ctx.enable_timing(True)
        ctx.postprocess_f64_device(o64[0].data_ptr(), o64[1].data_ptr())  # warm-up: code objects, first-use allocations
        ctx.synchronize()
        ms = []
        for _ in range(reps):
            ctx.reset_timing()
            ctx.postprocess_f64_device(o64[0].data_ptr(), o64[1].data_ptr())
            ctx.synchronize()
            ms.append(ctx.timing()["post"]["ms"])
        ctx.enable_timing(False)
        row["post_ms"] = [float(np.median(ms)), min(ms), max(ms)]
        left = o64[0].cpu().numpy()
        row["bad2"] = synth.bad_fraction(left, gt, 2.0)
        row["mae"] = mean_abs_error(left, gt)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if any(s is not None for s in settings):
        ctx.set_pp_smooth(lam=0)
    return rows


def table(rows):
    """means over the pairs of an input, one line per setting"""
    out = ["| input | lambda | fill_conf | bad-2.0 f64 | mean abs error | post ms f64 (min-max) |", "|---|---|---|---|---|---|"]
    keys = []
    for r in rows:
        k = (r["input"], r["lambda"], r["fill_conf"])
        if k not in keys:
            keys.append(k)
    for k in keys:
        g = [r for r in rows if (r["input"], r["lambda"], r["fill_conf"]) == k]
        m = lambda f: float(np.mean([f(r) for r in g]))  # noqa: E731
        out.append(f"| {k[0]} ({len(g)}) | {'off' if k[2] is None else f'{k[1]:g}'} | {'' if k[2] is None else f'{k[2]:g}'} | {100 * m(lambda r: r['bad2']):.3f} % | "
                   f"{m(lambda r: r['mae']):.4f} | {m(lambda r: r['post_ms'][0]):.3f} ({m(lambda r: r['post_ms'][1]):.3f}-{m(lambda r: r['post_ms'][2]):.3f}) |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lambdas", default="25,100,400")
    ap.add_argument("--fill_confs", default="0,0.25,1")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--median", type=int, default=0, help="radius of the median filter in front of the smoother")
    a = ap.parse_args()
    settings = [None] + [(float(x), float(f)) for x in a.lambdas.split(",") if x for f in a.fill_confs.split(",") if f]
    import torch
    if not torch.cuda.is_available():
        sys.exit("smooth_bench needs a GPU")
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import realdata, synth
    ctx = cs.StereoContext(0)
    if a.median:
        ctx.set_pp_median(a.median)
    rows = []
    for i in range(a.pairs):
        cfg, l, r, gl, _ = synth.make_config("C3", index=i)
        for row in measure(ctx, torch, f"C3 seed {cfg['seed'] + i}", l, r, gl, cfg["max_dis"], settings, a.reps):
            rows.append(dict(row, input="C3 synthetic"))
    full = realdata.load_full()
    if full is not None:
        cfg, l, r, gt = full
        for row in measure(ctx, torch, "Motorcycle", l, r, gt, cfg["max_dis"], settings, a.reps):
            rows.append(dict(row, input="Motorcycle"))
    ctx.close()
    print(table(rows), flush=True)


if __name__ == "__main__":
    main()
