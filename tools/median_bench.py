"""What the median filter of the post-processing does to accuracy and time: the first six synthetic C3 pairs
(1242x375, D = 128, seeds 2000 .. 2005) and, where the checkout has it, Motorcycle 741x500 D = 64, each after PatchMatch with seed
12345 and 3 iterations.  Per pair and radius: bad-2.0 of the left 8-bit and f64 post-processed maps and the CSPM_K_POST milliseconds
of cspm_postprocess_device and cspm_postprocess_f64_device (three repeats after a warm-up: median, minimum, maximum).  One JSON line
per pair and radius, then one markdown table of the means per input.

    python tools/median_bench.py [--radii 0,1,2,3] [--pairs 6] [--reps 3]
With --radii 0 the script touches nothing the filter added, so the same file run in a checkout of the parent commit gives the row to
compare the r = 0 row with: equal bad-2.0, times within the spread of the repeats.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(ctx, torch, name, l, r, gt, D, dis_scale, radii, reps):
    from crossscalepatchmatch_amd import capi, synth
    h, w = l.shape[:2]
    ctx.set_images(l, r)
    ctx.build_cost_grd(D, 35, 5, 0.3)
    ctx.patchmatch(3, seed=12345, schedule=capi.SCHED_RASTER)
    ctx.synchronize()
    o8 = [torch.zeros((h, w), dtype=torch.uint8, device="cuda:0") for _ in (0, 1)]
    o64 = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    calls = (("u8", lambda: ctx.postprocess_device(dis_scale, o8[0].data_ptr(), o8[1].data_ptr())),
             ("f64", lambda: ctx.postprocess_f64_device(o64[0].data_ptr(), o64[1].data_ptr())))
    rows = []
    for radius in radii:
        if radius:
            ctx.set_pp_median(radius)
        row = {"pair": name, "w": w, "h": h, "max_dis": D, "r": radius}
        ctx.enable_timing(True)
        for key, call in calls:
            call()  # warm-up: code objects, first-use allocations
            ctx.synchronize()
            ms = []
            for _ in range(reps):
                ctx.reset_timing()
                call()
                ctx.synchronize()
                ms.append(ctx.timing()["post"]["ms"])
            row[key + "_post_ms"] = [float(np.median(ms)), min(ms), max(ms)]
        ctx.enable_timing(False)
        row["bad2_u8"] = synth.bad_fraction(o8[0].cpu().numpy() / float(dis_scale), gt, 2.0)
        row["bad2_f64"] = synth.bad_fraction(o64[0].cpu().numpy(), gt, 2.0)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if any(radii):
        ctx.set_pp_median(0)
    return rows


def table(rows):
    """means over the pairs of an input, one line per radius"""
    out = ["| input | r | bad-2.0 8-bit | bad-2.0 f64 | post ms 8-bit (min-max) | post ms f64 (min-max) |", "|---|---|---|---|---|---|"]
    keys = []
    for r in rows:
        k = (r["input"], r["r"])
        if k not in keys:
            keys.append(k)
    for k in keys:
        g = [r for r in rows if (r["input"], r["r"]) == k]
        m = lambda f: float(np.mean([f(r) for r in g]))  # noqa: E731
        out.append(f"| {k[0]} ({len(g)}) | {k[1]} | {100 * m(lambda r: r['bad2_u8']):.3f} % | {100 * m(lambda r: r['bad2_f64']):.3f} % | "
                   f"{m(lambda r: r['u8_post_ms'][0]):.3f} ({m(lambda r: r['u8_post_ms'][1]):.3f}-{m(lambda r: r['u8_post_ms'][2]):.3f}) | "
                   f"{m(lambda r: r['f64_post_ms'][0]):.3f} ({m(lambda r: r['f64_post_ms'][1]):.3f}-{m(lambda r: r['f64_post_ms'][2]):.3f}) |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radii", default="0,1,2,3")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    radii = [int(s) for s in a.radii.split(",")]
    import torch
    if not torch.cuda.is_available():
        sys.exit("median_bench needs a GPU")
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import realdata, synth
    ctx = cs.StereoContext(0)
    rows = []
    for i in range(a.pairs):
        cfg, l, r, gl, _ = synth.make_config("C3", index=i)
        for row in measure(ctx, torch, f"C3 seed {cfg['seed'] + i}", l, r, gl, cfg["max_dis"], cfg["dis_scale"], radii, a.reps):
            rows.append(dict(row, input="C3 synthetic"))
    full = realdata.load_full()
    if full is not None:
        cfg, l, r, gt = full
        for row in measure(ctx, torch, "Motorcycle", l, r, gt, cfg["max_dis"], cfg["dis_scale"], radii, a.reps):
            rows.append(dict(row, input="Motorcycle"))
    ctx.close()
    print(table(rows), flush=True)


if __name__ == "__main__":
    main()
