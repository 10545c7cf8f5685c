"""Timing of local stereo (cost aggregation + cross-scale WTA, cspm_local_stereo) at the C3 geometry: one JSON line per method.

    python tools/local_stereo_bench.py [--methods BOX,GF,BF] [--pairs 20] [--inflight 2] [--config C3]

Per method: 20 distinct synthetic pairs (synth.make_config) with two contexts in flight (one host thread each), timed from the
first cost construction to the last pair's maps: GRD cost (5 levels, lambda 0.3) + local stereo + both 8-bit maps (PlaneToDisp)
per pair -> ms per pair and Mpix/s (left-view pixels); bad-2.0 of the left map against the synthetic ground truth; and the
741x500 Motorcycle pair (D = 64, 5 levels, lambda 0.3) with post-processing against its ground truth.  Also the per-class
launch times of one C3 pair alone (CSPM_K_MISC holds the aggregation and WTA launches)."""
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
    ap.add_argument("--methods", default="BOX,GF,BF")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--config", default="C3")
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
    codes = {"BOX": capi.CA_BOX, "GF": capi.CA_GF, "BF": capi.CA_BF}

    def run(ctx, p, method):
        c, l, r, gl, _ = p
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        ctx.local_stereo(codes[method])
        return ctx.disparity_u8(0, c["dis_scale"]), ctx.disparity_u8(1, c["dis_scale"])

    for method in args.methods.split(","):
        for ctx in ctxs:  # warm-up: buffers of this geometry, kernels loaded
            run(ctx, pairs[0], method)
        maps = [None] * len(pairs)

        def worker(k):
            for i in range(k, len(pairs), len(ctxs)):
                maps[i] = run(ctxs[k], pairs[i], method)

        t0 = time.perf_counter()
        th = [threading.Thread(target=worker, args=(k,)) for k in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        ms = (time.perf_counter() - t0) * 1000.0 / len(pairs)
        bad = float(np.mean([synth.bad_fraction(maps[i][0].astype(np.float64) / pairs[i][0]["dis_scale"], pairs[i][3], 2.0)
                             for i in range(len(pairs))]))
        # one pair alone, per kernel class
        ctx = ctxs[0]
        ctx.enable_timing(True)
        ctx.reset_timing()
        run(ctx, pairs[1], method)
        tm = {k: round(v["ms"], 3) for k, v in ctx.timing().items() if v["launches"]}
        ctx.enable_timing(False)
        out = {"method": method, "config": f"{args.config}: {cfg['w']}x{cfg['h']} max_dis={cfg['max_dis']} GRD scale_num={cfg['scale_num']} "
                                           f"reg_lambda={cfg['reg_lambda']}", "pairs": len(pairs), "inflight": len(ctxs),
               "ms_per_pair": round(ms, 2), "mpix_per_s": round(cfg["w"] * cfg["h"] / ms / 1000.0, 2), "synthetic_bad2_left": round(bad, 4),
               "one_pair_kernel_ms": tm}
        full = rd.load_full()
        if full is not None:
            fc, l, r, gt = full
            ctx.set_images(l, r)
            ctx.build_cost_grd(fc["max_dis"], 35, fc["scale_num"], fc["reg_lambda"])
            ctx.local_stereo(codes[method])
            lo, _ = ctx.postprocess(fc["dis_scale"])
            out["motorcycle_741x500_bad2_post_processed"] = round(rd.bad_fraction(lo.astype(np.float64) / fc["dis_scale"], gt, 2.0), 4)
        print(json.dumps(out), flush=True)
    for ctx in ctxs:
        ctx.close()


if __name__ == "__main__":
    main()
