"""Cost and accuracy of warm-started PatchMatch at the C3 geometry: one JSON line per variant.

    python tools/warm_start_bench.py [--variants cold3,cold2,cold1,box_warm1,box_warm2,gf_warm1,c2f_3_1] [--pairs 20] [--inflight 2]
                                     [--config C3] [--no-motorcycle]

Variants: coldK = cspm_patchmatch with K iterations (the bench.py headline is cold3); box_warmK / gf_warmK = local stereo with BOX / GF
aggregation, then K warm iterations (cspm_patchmatch_warm); c2f_C_F = C iterations on the half-size pair (the level-1 images,
max_dis (max_dis+1)//2), the planes carried up (cspm_upsample_planes), then F warm iterations on the full pair (capi.coarse_to_fine).
Per variant: 20 distinct synthetic pairs (synth.make_config) with two contexts in flight (one host thread each), timed from the first
cost construction to the last pair's maps: GRD cost (5 levels, lambda 0.3) + the variant + both 8-bit maps (PlaneToDisp) per pair ->
ms per pair; bad-2.0 of the left map against the synthetic ground truth; and the 741x500 Motorcycle pair (D = 64, 5 levels,
lambda 0.3) with post-processing against its ground truth."""
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
    ap.add_argument("--variants", default="cold3,cold2,cold1,box_warm1,box_warm2,gf_warm1,c2f_3_1")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=2)
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
    from crossscalepatchmatch_amd import capi, realdata as rd, synth

    pairs = [synth.make_config(args.config, i) for i in range(args.pairs)]
    cfg = pairs[0][0]
    ctxs = [cs.StereoContext(0) for _ in range(args.inflight)]
    coarse = [cs.StereoContext(0) for _ in range(args.inflight)]  # the half-size contexts of c2f, kept like the full ones
    codes = {"box": capi.CA_BOX, "gf": capi.CA_GF}

    def enqueue(k, c, l, r, variant):
        """the variant on context k, enqueued (asynchronous)"""
        ctx = ctxs[k]
        if variant.startswith("c2f_"):
            ci, fi = (int(t) for t in variant[4:].split("_"))
            capi.coarse_to_fine(l, r, c["max_dis"], ci, fi, "GRD", 35, c["scale_num"], c["reg_lambda"], ctx=ctx, coarse_ctx=coarse[k])
            return
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        if variant.startswith("cold"):
            ctx.patchmatch(int(variant[4:]))
        else:
            name, it = variant.split("_warm")
            ctx.local_stereo(codes[name])
            ctx.patchmatch_warm(int(it))

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
               "ms_per_pair": round(ms, 2), "synthetic_bad2_left": round(bad, 4)}
        full = None if args.no_motorcycle else rd.load_full()
        if full is not None:
            fc, l, r, gt = full
            enqueue(0, fc, l, r, variant)
            lo, _ = ctxs[0].postprocess(fc["dis_scale"])
            out["motorcycle_741x500_bad2_post_processed"] = round(rd.bad_fraction(lo.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
        print(json.dumps(out), flush=True)
    for ctx in ctxs + coarse:
        ctx.close()


if __name__ == "__main__":
    main()
