"""Cost and accuracy of FITTED PatchMatch starts (include/cspm.h "plane fitting") at the C3 geometry: one JSON line
per variant.

    python tools/fit_bench.py [--variants cold3,box_warm1,box_warm2,box_seed1,box_fit_warm1,box_fit_warm2,box_fitmerge_seed1] [--pairs 20]
                              [--inflight 2] [--config C3] [--no-motorcycle] [--no-kernel-times] [--fit_radius 5] [--fit_max_diff 1.5]

The variants of tools/seed_bench.py -- coldK = cspm_patchmatch with K iterations; box_warmK = BOX local stereo, then K warm iterations;
box_seedK = BOX local stereo, keep-init, then K iterations; prev_seedK -- plus the fitted ones: box_fit_warmK = BOX local stereo,
cspm_fit_planes(merge = 0) over its fronto-parallel field, then K warm iterations (cspm_main --warm_ca=BOX --fit_radius=R);
box_fitmerge_seedK = BOX local stereo, cspm_fit_planes(merge = 1) (a fitted plane wins only where it costs less), keep-init, then K
iterations (cspm_main --seed_ca=BOX --fit_radius=R --fit_merge).
Measured as in tools/seed_bench.py: 20 distinct synthetic pairs with two contexts in flight -> ms per pair and bad-2.0 of the left map;
the 741x500 Motorcycle pair against its ground truth, raw and post-processed.  Last line: what the k_fit_planes bracket of one view
(the disparity snapshot and the fit, CSPM_K_MISC) takes on one pair of the configuration (hipEvent brackets, cspm_get_timing)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="cold3,box_warm1,box_warm2,box_seed1,box_fit_warm1,box_fit_warm2,box_fitmerge_seed1")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-kernel-times", action="store_true")
    ap.add_argument("--fit_radius", type=int, default=5)
    ap.add_argument("--fit_max_diff", type=float, default=1.5)
    args = ap.parse_args()
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
    prev = [cs.StereoContext(0) for _ in range(args.inflight)]  # prev_seed: the contexts that hold the stand-in for the previous frame

    def build(ctx, c, l, r):
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])

    def enqueue(k, c, l, r, variant):
        """the variant on context k, enqueued (asynchronous)"""
        ctx = ctxs[k]
        build(ctx, c, l, r)
        fit = dict(radius=args.fit_radius, max_diff=args.fit_max_diff)
        if variant.startswith("box_fit_warm"):
            ctx.local_stereo(capi.CA_BOX)
            ctx.fit_planes(merge=False, **fit)
            ctx.patchmatch_warm(int(variant[12:]))
        elif variant.startswith("box_fitmerge_seed"):
            ctx.local_stereo(capi.CA_BOX)
            ctx.fit_planes(merge=True, **fit)
            ctx.pm_init_keep()
            ctx.patchmatch_warm(int(variant[17:]))
        elif variant.startswith("cold"):
            ctx.patchmatch(int(variant[4:]))
        elif variant.startswith("box_warm"):
            ctx.local_stereo(capi.CA_BOX)
            ctx.patchmatch_warm(int(variant[8:]))
        elif variant.startswith("box_seed"):
            ctx.local_stereo(capi.CA_BOX)
            ctx.pm_init_keep()
            ctx.patchmatch_warm(int(variant[8:]))
        elif variant.startswith("prev_seed"):
            build(prev[k], c, l, r)
            prev[k].patchmatch(1, seed=777)
            capi.seeded_patchmatch(ctx, int(variant[9:]), [prev[k]])
        else:
            raise ValueError(variant)

    def run(k, p, variant):
        c, l, r, _, _ = p
        enqueue(k, c, l, r, variant)
        return ctxs[k].disparity_u8(0, c["dis_scale"]), ctxs[k].disparity_u8(1, c["dis_scale"])

    for variant in args.variants.split(","):
        for k in range(len(ctxs)):  # warm-up: buffers of this geometry, kernels loaded
            run(k, pairs[0], variant)
        maps = [None] * len(pairs)

        def worker(k):
            for i in range(k, len(pairs), len(ctxs)):
                maps[i] = run(k, pairs[i], variant)

        t0 = time.perf_counter()
        th = [threading.Thread(target=worker, args=(k,)) for k in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        ms = (time.perf_counter() - t0) * 1000.0 / len(pairs)
        bad = float(np.mean([synth.bad_fraction(maps[i][0].astype(np.float64) / pairs[i][0]["dis_scale"], pairs[i][3], 2.0)
                             for i in range(len(pairs))]))
        out = {"variant": variant, "config": f"{args.config}: {cfg['w']}x{cfg['h']} max_dis={cfg['max_dis']} GRD scale_num={cfg['scale_num']} "
                                             f"reg_lambda={cfg['reg_lambda']}", "pairs": len(pairs), "inflight": len(ctxs),
               "fit_radius": args.fit_radius, "fit_max_diff": args.fit_max_diff, "ms_per_pair": round(ms, 2), "synthetic_bad2_left": round(bad, 4)}
        full = None if args.no_motorcycle else rd.load_full()
        if full is not None:
            fc, l, r, gt = full
            enqueue(0, fc, l, r, variant)
            raw = ctxs[0].disparity_u8(0, fc["dis_scale"])
            lo, _ = ctxs[0].postprocess(fc["dis_scale"])
            out["motorcycle_741x500_bad2_raw"] = round(rd.bad_fraction(raw.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
            out["motorcycle_741x500_bad2_post_processed"] = round(rd.bad_fraction(lo.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
        print(json.dumps(out), flush=True)

    if not args.no_kernel_times:
        c, l, r, _, _ = pairs[0]
        ctx = ctxs[0]
        build(ctx, c, l, r)
        ctx.enable_timing(True)
        best = None
        for _ in range(5):
            ctx.local_stereo(capi.CA_BOX)  # the same starting field for every repetition
            ctx.synchronize()
            ctx.reset_timing()
            ctx.fit_planes(merge=False, radius=args.fit_radius, max_diff=args.fit_max_diff)
            ctx.synchronize()
            t = ctx.timing()["misc"]
            assert t["launches"] == 2, t
            best = t["ms"] / 2 if best is None else min(best, t["ms"] / 2)
        ctx.enable_timing(False)
        print(json.dumps({"k_fit_planes_ms_per_view": round(best, 3), "fit_radius": args.fit_radius, "config": args.config,
                          "note": "best of 5, the snapshot and the fit of one view, one pair alone on the GPU"}), flush=True)
    for ctx in ctxs + prev:
        ctx.close()


if __name__ == "__main__":
    main()
