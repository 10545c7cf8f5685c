"""Time of the sub-pixel PostProcessing (cspm_postprocess_f64_device) against the 8-bit one (cspm_postprocess_device) on the SAME
plane field, from the library's CSPM_K_POST timers: a C3-size synthetic pair (1242x375, D = 128) and, where the checkout has it,
the full Motorcycle pair with its bad-2.0 figures.  One JSON line per pair.

    python tools/pp_sub_bench.py [--reps 10]
Under rocprofv3 --kernel-trace --stats the same run gives the kernels' shares.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(ctx, torch, name, l, r, D, dis_scale, reps, gt=None):
    from crossscalepatchmatch_amd import capi, realdata
    h, w = l.shape[:2]
    ctx.set_images(l, r)
    ctx.build_cost_grd(D, 35, 5, 0.3)
    ctx.patchmatch(3, seed=12345, schedule=capi.SCHED_RASTER)
    ctx.synchronize()
    o8 = [torch.zeros((h, w), dtype=torch.uint8, device="cuda:0") for _ in (0, 1)]
    o64 = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    out = {"pair": name, "w": w, "h": h, "max_dis": D, "reps": reps}
    ctx.enable_timing(True)
    for key, call in (("u8", lambda: ctx.postprocess_device(dis_scale, o8[0].data_ptr(), o8[1].data_ptr())),
                      ("f64", lambda: ctx.postprocess_f64_device(o64[0].data_ptr(), o64[1].data_ptr()))):
        call()  # warm-up: code objects, first-use allocations
        ctx.synchronize()
        ctx.reset_timing()
        for _ in range(reps):
            call()
        ctx.synchronize()
        t = ctx.timing()["post"]
        out[key + "_post_ms"] = t["ms"] / t["launches"]
    ctx.enable_timing(False)
    res = ctx.postprocess_f64(valid=True)
    out["inconsistent_pixels"] = [int((res[2] == 0).sum()), int((res[3] == 0).sum())]
    if gt is not None:
        out["bad2_raw_f64"] = realdata.bad_fraction(ctx.disparity_f64(0), gt, 2.0)
        out["bad2_pp_f64"] = realdata.bad_fraction(res[0], gt, 2.0)
        out["bad2_pp_u8"] = realdata.bad_fraction(ctx.postprocess(dis_scale)[0] / float(dis_scale), gt, 2.0)
        for t in (0.5, 1.0):
            out[f"bad{t}_pp_f64"] = realdata.bad_fraction(res[0], gt, t)
            out[f"bad{t}_pp_u8"] = realdata.bad_fraction(ctx.postprocess(dis_scale)[0] / float(dis_scale), gt, t)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pp_sub_bench needs a GPU")
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import realdata, synth
    ctx = cs.StereoContext(0)
    cfg, l, r, _, _ = synth.make_config("C3")
    measure(ctx, torch, "C3 synthetic", l, r, cfg["max_dis"], cfg["dis_scale"], a.reps)
    full = realdata.load_full()
    if full is not None:
        cfg, l, r, gt = full
        measure(ctx, torch, "Motorcycle", l, r, cfg["max_dis"], cfg["dis_scale"], a.reps, gt)
    ctx.close()


if __name__ == "__main__":
    main()
