"""Cost and effect of SEGMENT PLANES (include/cspm.h "segment planes") at the C3 geometry and on Motorcycle: one
JSON line per measurement.

    python tools/seg_bench.py [--pairs 6] [--inflight 2] [--config C3] [--no-motorcycle] [--no-call-times] [--no-variants]
                              [--steps 8,16,32] [--step 16] [--variants ...]

1. ms per cspm_segment_planes call, merge 0 and 1, for every --steps value: hipEvent brackets (cspm_get_timing: CSPM_K_MISC for the
   snapshot, the segmentation and the fit of both views, plus CSPM_K_INIT for the merge launches), the median of 9 calls on the same
   buffers -- the field of one cold iteration is put back (and, for merge 1, re-scored) before every call, outside the brackets.
2. bad-2.0 of the left map, raw and post-processed, and ms per pair (wall clock, --inflight contexts) for the variants
       cold3                       cspm_patchmatch(3)
       cold3_seg                   ... then cspm_segment_planes(merge = 1)
       cold3_seg_warm1             ... then one warm iteration          (cspm_main --seg_step=S)
       cold2_seg_warm1             two cold iterations, the merge, one warm iteration
       box_fit_warm1               BOX local stereo, cspm_fit_planes(merge = 0), one warm iteration
       box_fit_warm1_seg_warm1     ... then the merge and one more warm iteration
   at --step, over --pairs synthetic pairs of the configuration and the 741x500 Motorcycle pair.  Nothing here is a pass bar."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = "cold3,cold3_seg,cold3_seg_warm1,cold2_seg_warm1,box_fit_warm1,box_fit_warm1_seg_warm1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default=VARIANTS)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", default="8,16,32")
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-call-times", action="store_true")
    ap.add_argument("--no-variants", action="store_true")
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
    full = None if args.no_motorcycle else rd.load_full()
    config = f"{args.config}: {cfg['w']}x{cfg['h']} max_dis={cfg['max_dis']} GRD scale_num={cfg['scale_num']} reg_lambda={cfg['reg_lambda']}"

    def build(ctx, c, l, r):
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])

    if not args.no_call_times:
        inputs = [(config, pairs[0][0], pairs[0][1], pairs[0][2])]
        if full is not None:
            inputs.append(("Motorcycle 741x500", full[0], full[1], full[2]))
        ctx = ctxs[0]
        for name, c, l, r in inputs:
            build(ctx, c, l, r)
            ctx.patchmatch(1)
            start = [ctx.get_planes(v) for v in (0, 1)]
            for step in (int(s) for s in args.steps.split(",")):
                for merge in (0, 1):
                    ms = []
                    for rep in range(10):  # the first call allocates the scratch: not counted
                        for v in (0, 1):
                            ctx.set_planes(v, *start[v])
                        if merge:
                            ctx.rescore_planes()
                        ctx.synchronize()
                        ctx.enable_timing(True)
                        ctx.reset_timing()
                        ctx.segment_planes(merge=bool(merge), step=step)
                        ctx.synchronize()
                        t = ctx.timing()
                        ctx.enable_timing(False)
                        assert t["misc"]["launches"] == 2 and t["init"]["launches"] == 2 * merge, t
                        if rep:
                            ms.append((t["misc"]["ms"], t["init"]["ms"]))
                    tot = sorted(a + b for a, b in ms)
                    print(json.dumps({"segment_planes_ms_per_call": round(tot[len(tot) // 2], 3), "min": round(tot[0], 3), "max": round(tot[-1], 3),
                                      "segmentation_and_fit_ms": round(sorted(a for a, _ in ms)[len(ms) // 2], 3),
                                      "merge_ms": round(sorted(b for _, b in ms)[len(ms) // 2], 3), "merge": merge, "step": step,
                                      "segments": capi.segment_count(c["w"], c["h"], step), "input": name,
                                      "note": "median of 9 calls on the same buffers, both views, one pair alone on the GPU"}), flush=True)

    def enqueue(k, c, l, r, variant):
        """the variant on context k, enqueued (asynchronous)"""
        ctx = ctxs[k]
        build(ctx, c, l, r)
        seg = dict(step=args.step)
        if variant == "cold3":
            ctx.patchmatch(3)
        elif variant == "cold3_seg":
            ctx.patchmatch(3)
            ctx.segment_planes(merge=True, **seg)
        elif variant == "cold3_seg_warm1":
            ctx.patchmatch(3)
            ctx.segment_planes(merge=True, **seg)
            ctx.patchmatch_warm(1)
        elif variant == "cold2_seg_warm1":
            ctx.patchmatch(2)
            ctx.segment_planes(merge=True, **seg)
            ctx.patchmatch_warm(1)
        elif variant in ("box_fit_warm1", "box_fit_warm1_seg_warm1"):
            ctx.local_stereo(capi.CA_BOX)
            ctx.fit_planes(merge=False)
            ctx.patchmatch_warm(1)
            if variant.endswith("seg_warm1"):
                ctx.segment_planes(merge=True, **seg)
                ctx.patchmatch_warm(1)
        else:
            raise ValueError(variant)

    def run(k, p, variant):
        c, l, r, _, _ = p
        enqueue(k, c, l, r, variant)
        raw = ctxs[k].disparity_u8(0, c["dis_scale"])
        post, _ = ctxs[k].postprocess(c["dis_scale"])
        return raw, post

    for variant in ([] if args.no_variants else args.variants.split(",")):
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
        bad = [float(np.mean([synth.bad_fraction(maps[i][j].astype(np.float64) / pairs[i][0]["dis_scale"], pairs[i][3], 2.0)
                              for i in range(len(pairs))])) for j in (0, 1)]
        out = {"variant": variant, "config": config, "pairs": len(pairs), "inflight": len(ctxs), "seg_step": args.step,
               "ms_per_pair_with_postprocessing": round(ms, 2), "synthetic_bad2_raw": round(bad[0], 4), "synthetic_bad2_post_processed": round(bad[1], 4)}
        if full is not None:
            fc, l, r, gt = full
            run(0, (fc, l, r, None, None), variant)  # warm-up at this geometry
            ctxs[0].synchronize()
            t0 = time.perf_counter()
            raw, lo = run(0, (fc, l, r, None, None), variant)
            out["motorcycle_741x500_ms_with_postprocessing"] = round((time.perf_counter() - t0) * 1000.0, 2)
            out["motorcycle_741x500_bad2_raw"] = round(rd.bad_fraction(raw.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
            out["motorcycle_741x500_bad2_post_processed"] = round(rd.bad_fraction(lo.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
        print(json.dumps(out), flush=True)
    for ctx in ctxs:
        ctx.close()


if __name__ == "__main__":
    main()
