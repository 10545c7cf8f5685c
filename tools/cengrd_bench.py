"""Cost and accuracy of the CENGRD matching cost next to GRD and CEN at the C3 geometry: one JSON line per cost and measurement.

    python tools/cengrd_bench.py [--costs GRD,CEN,CENGRD,GRD_fused,CEN_fused,CENGRD_fused] [--modes ctor,run,quality] [--pairs 20] [--inflight 2] [--repeats 3]
                                 [--quality-pairs 6] [--config C3] [--no-motorcycle]

Costs: GRD and CEN are built with CSPM_OPT_GRD_VOLUMES = 1 (materialised f64 volumes: the PatchMatch kernels are then the same
volume-sourced instantiations CENGRD runs); GRD_fused is the default fused GRD cost (the bench.py headline), CEN_fused the fused census
cost, CENGRD_fused the CENGRD cost with CSPM_OPT_CENGRD_FUSED = 1 (no volumes: the cells are computed inside the PatchMatch kernels).
The fused-CENGRD comparison of DESIGN.md section 13 is ONE run of
    python tools/cengrd_bench.py --costs CENGRD,CENGRD_fused,GRD_fused,CEN_fused --modes run
Modes:
  ctor     the cost constructor alone, per pair, on one context: host clock around build + synchronise (images already on the device),
           and the summed device time of the constructor's kernels (CSPM_K_GRD).  For the per-kernel split run this mode alone under
           `rocprofv3 --kernel-trace --stats`.
  run      `pairs` distinct synthetic pairs (synth.make_config) with `inflight` contexts in flight (one host thread each), timed from
           the first cost construction to the last pair's maps: constructor + 3 iterations + both 8-bit maps per pair -> ms per pair,
           `repeats` times (the spread is the noise floor a difference has to clear).
  quality  bad-2.0 of the left map, raw (PlaneToDisp) and post-processed, on the first `quality-pairs` synthetic pairs and on the
           741x500 Motorcycle pair (D = 64, 5 levels, lambda 0.3) -- as they are, and with the RIGHT image radiometrically altered:
           right' = saturate_u8(round(0.8 * right + 20)) (gain 0.8, offset +20; no random component: the pairs are those of
           synth.make_config(config, i), i = 0 .., whose seeds are the config's seed + i; PatchMatch seed 12345)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAIN, OFFSET = 0.8, 20.0


def alter(img):
    """gain and offset on an 8-bit image, saturating"""
    return np.clip(np.rint(GAIN * img.astype(np.float64) + OFFSET), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--costs", default="GRD,CEN,CENGRD")
    ap.add_argument("--modes", default="ctor,run,quality")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quality-pairs", type=int, default=6)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--no-motorcycle", action="store_true")
    args = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import realdata as rd, synth

    pairs = [synth.make_config(args.config, i) for i in range(args.pairs)]
    cfg = pairs[0][0]
    ctxs = [cs.StereoContext(0) for _ in range(args.inflight)]
    modes = args.modes.split(",")
    label = f"{args.config}: {cfg['w']}x{cfg['h']} max_dis={cfg['max_dis']} scale_num={cfg['scale_num']} reg_lambda={cfg['reg_lambda']}"

    def build(ctx, cost, c):
        a = (c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        if cost == "GRD":
            ctx.build_cost_grd(*a, volumes=True)
        elif cost == "GRD_fused":
            ctx.build_cost_grd(*a, volumes=False)
        elif cost == "CEN":
            ctx.build_cost_cen(*a, volumes=True)
        elif cost == "CEN_fused":
            ctx.build_cost_cen(*a, volumes=False)
        elif cost == "CENGRD":
            ctx.build_cost_cengrd(*a, fused=False)
        elif cost == "CENGRD_fused":
            ctx.build_cost_cengrd(*a, fused=True)
        else:
            raise ValueError(f"unknown cost {cost!r} (GRD, GRD_fused, CEN, CEN_fused, CENGRD or CENGRD_fused)")

    def run(k, c, l, r, cost, iters=3):
        ctx = ctxs[k]
        ctx.set_images(l, r)
        build(ctx, cost, c)
        ctx.patchmatch(iters)
        return ctx.disparity_u8(0, c["dis_scale"]), ctx.disparity_u8(1, c["dis_scale"])

    for cost in args.costs.split(","):
        c0, l0, r0 = pairs[0][0], pairs[0][1], pairs[0][2]
        for k in range(len(ctxs)):  # warm-up: buffers of this geometry, kernels loaded
            run(k, c0, l0, r0, cost, iters=1)
        if "ctor" in modes:
            ctx = ctxs[0]
            ctx.enable_timing(True)
            host_ms = []
            ctx.reset_timing()
            for c, l, r, _, _ in pairs:
                ctx.set_images(l, r)  # synchronises: the upload is not part of the constructor
                t0 = time.perf_counter()
                build(ctx, cost, c)
                ctx.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1000.0)
            kernels = ctx.timing()["grd"]
            ctx.enable_timing(False)
            print(json.dumps({"cost": cost, "mode": "ctor", "config": label, "pairs": len(pairs),
                              "ctor_host_ms_per_pair_median": round(float(np.median(host_ms)), 3),
                              "ctor_host_ms_per_pair_min_max": [round(min(host_ms), 3), round(max(host_ms), 3)],
                              "ctor_kernel_ms_per_pair": round(kernels["ms"] / len(pairs), 3),
                              "ctor_kernel_launches_per_pair": kernels["launches"] / len(pairs)}), flush=True)
        if "run" in modes:
            times = []
            for _ in range(args.repeats):
                def worker(k):
                    for i in range(k, len(pairs), len(ctxs)):
                        run(k, pairs[i][0], pairs[i][1], pairs[i][2], cost)

                t0 = time.perf_counter()
                th = [threading.Thread(target=worker, args=(k,)) for k in range(len(ctxs))]
                for t in th:
                    t.start()
                for t in th:
                    t.join()
                times.append(round((time.perf_counter() - t0) * 1000.0 / len(pairs), 2))
            print(json.dumps({"cost": cost, "mode": "run", "config": label, "pairs": len(pairs), "inflight": len(ctxs),
                              "ms_per_pair_repeats": times, "ms_per_pair_median": float(np.median(times))}), flush=True)
        if "quality" in modes:
            out = {"cost": cost, "mode": "quality", "config": label, "synthetic_pairs": min(args.quality_pairs, len(pairs)),
                   "right_image_alteration": f"saturate_u8(round({GAIN} * right + {OFFSET:g}))"}
            full = None if args.no_motorcycle else rd.load_full()
            for tag, f in (("", lambda im: im), ("_altered", alter)):
                raw, post = [], []
                for c, l, r, gt, _ in pairs[:args.quality_pairs]:
                    dl, _ = run(0, c, l, f(r), cost)
                    pl, _ = ctxs[0].postprocess(c["dis_scale"])
                    raw.append(synth.bad_fraction(dl.astype(np.float64) / c["dis_scale"], gt, 2.0))
                    post.append(synth.bad_fraction(pl.astype(np.float64) / c["dis_scale"], gt, 2.0))
                out[f"synthetic{tag}_bad2_raw"] = round(float(np.mean(raw)), 4)
                out[f"synthetic{tag}_bad2_post_processed"] = round(float(np.mean(post)), 4)
                if full is not None:
                    fc, l, r, gt = full
                    dl, _ = run(0, fc, l, f(r), cost)
                    pl, _ = ctxs[0].postprocess(fc["dis_scale"])
                    out[f"motorcycle_741x500{tag}_bad2_raw"] = round(rd.bad_fraction(dl.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
                    out[f"motorcycle_741x500{tag}_bad2_post_processed"] = round(rd.bad_fraction(pl.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
            print(json.dumps(out), flush=True)
    for ctx in ctxs:
        ctx.close()


if __name__ == "__main__":
    main()
