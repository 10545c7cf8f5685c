"""Cost and accuracy of the spatial-propagation schedules at the C3 geometry: one JSON line per variant.

    python tools/propagation_bench.py [--variants raster,redblack,diffuse4,diffuse8,diffuse20,diffuse8r2] [--pairs 20] [--inflight 2]
                                      [--reps 3] [--config C3] [--no-motorcycle] [--no-warm] [--lib PATH]

Variants: raster = CSPM_SCHED_RASTER; redblack = CSPM_SCHED_REDBLACK with 4 neighbours, 1 round; diffuseK[rR] = CSPM_SCHED_DIFFUSE
with K neighbours and R rounds (1 when absent).  Per variant, modelled on tools/warm_start_bench.py: 20 distinct synthetic pairs
(synth.make_config) with two contexts in flight (one host thread each), GRD cost (5 levels, lambda 0.3) + 3 iterations + both 8-bit
maps per pair, timed from the first cost construction to the last pair's maps -> ms per pair, `reps` times after a warm-up (median,
min and max are reported); the CSPM_K_SPATIAL bracket per propagation of one pair that has the GPU to itself (hipEvents, median of
`reps` runs); bad-2.0 of the left map against the synthetic ground truth, raw and post-processed; the same for the 741x500 Motorcycle
pair (D = 64); and both again for BOX local stereo + 1 warm iteration under the variant's schedule.
--lib: another build of the library (the parent commit's, for the unchanged default path); it has to be given before anything is loaded."""
import argparse
import json
import os
import re
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pm_kw(variant):
    if variant == "raster":
        return dict(schedule=0)
    if variant == "redblack":
        return dict(schedule=1, rb_rounds=1, rb_neighbours=4)
    m = re.fullmatch(r"diffuse(\d+)(?:r(\d+))?", variant)
    if not m:
        raise SystemExit(f"unknown variant {variant!r}")
    return dict(schedule=2, rb_neighbours=int(m.group(1)), rb_rounds=int(m.group(2) or 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="raster,redblack,diffuse4,diffuse8,diffuse20,diffuse8r2")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-warm", action="store_true")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.lib:
        os.environ["CSPM_LIB"] = os.path.abspath(args.lib)
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd, synth

    pairs = [synth.make_config(args.config, i) for i in range(args.pairs)]
    cfg = pairs[0][0]
    ctxs = [cs.StereoContext(0) for _ in range(args.inflight)]
    full = None if args.no_motorcycle else rd.load_full()

    def enqueue(ctx, c, l, r, kw, warm=False):
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        if warm:
            ctx.local_stereo(capi.CA_BOX)
            ctx.patchmatch_warm(1, **kw)
        else:
            ctx.patchmatch(3, **kw)

    def bad_pair(ctx, c, l, r, gt, kw, warm, bad):
        """(raw, post-processed) bad-2.0 of the left map"""
        enqueue(ctx, c, l, r, kw, warm)
        raw = ctx.disparity_u8(0, c["dis_scale"])
        post, _ = ctx.postprocess(c["dis_scale"])
        return [bad(m.astype(np.float64) / c["dis_scale"], gt, 2.0) for m in (raw, post)]

    for variant in args.variants.split(","):
        kw = pm_kw(variant)

        def run(k, p):
            c, l, r, _, _ = p
            enqueue(ctxs[k], c, l, r, kw)
            return ctxs[k].disparity_u8(0, c["dis_scale"]), ctxs[k].disparity_u8(1, c["dis_scale"])

        for k in range(len(ctxs)):  # warm-up: buffers of this geometry, kernels loaded
            run(k, pairs[0])
        ms = []
        for _ in range(args.reps):
            def worker(k):
                for i in range(k, len(pairs), len(ctxs)):
                    run(k, pairs[i])

            t0 = time.perf_counter()
            th = [threading.Thread(target=worker, args=(k,)) for k in range(len(ctxs))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            ms.append((time.perf_counter() - t0) * 1000.0 / len(pairs))
        # the spatial bracket of one pair alone
        solo = []
        ctx = ctxs[0]
        ctx.enable_timing(True)
        for _ in range(args.reps):
            ctx.reset_timing()
            c, l, r, _, _ = pairs[0]
            enqueue(ctx, c, l, r, kw)
            ctx.synchronize()
            solo.append(ctx.timing()["spatial"]["ms"] / 3.0)
        ctx.enable_timing(False)
        out = {"variant": variant, "lib": args.lib or "this tree",
               "config": f"{args.config}: {cfg['w']}x{cfg['h']} max_dis={cfg['max_dis']} GRD scale_num={cfg['scale_num']} reg_lambda={cfg['reg_lambda']}",
               "pairs": len(pairs), "inflight": len(ctxs), "reps": args.reps, "ms_per_pair": round(float(np.median(ms)), 2),
               "ms_per_pair_min_max": [round(min(ms), 2), round(max(ms), 2)], "spatial_ms_per_propagation_solo": round(float(np.median(solo)), 2)}
        modes = [("cold3", False)] + ([] if args.no_warm else [("box_warm1", True)])
        for tag, warm in modes:
            b = np.mean([bad_pair(ctxs[0], p[0], p[1], p[2], p[3], kw, warm, synth.bad_fraction) for p in pairs], axis=0)
            out[f"synthetic_bad2_{tag}_raw_post"] = [round(float(x), 4) for x in b]
            if full is not None:
                fc, l, r, gt = full
                out[f"motorcycle_741x500_bad2_{tag}_raw_post"] = [round(x, 4) for x in bad_pair(ctxs[0], fc, l, r, gt, kw, warm, rd.bad_fraction)]
        print(json.dumps(out), flush=True)
    for ctx in ctxs:
        ctx.close()


if __name__ == "__main__":
    main()
