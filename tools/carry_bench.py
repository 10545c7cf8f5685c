"""What the plane-field carry (include/cspm.h "plane-field carry") costs and what a carried start is worth: one JSON
line per case.

    python tools/carry_bench.py [--repeats 9] [--warmup 3] [--frames 8] [--no-motorcycle] [--no-sequence] [--parent DIR [--bench-runs 3]]

(a) The carry call alone: two rendered frames (tests/carry_cases.py) at 1242 x 375 and 741 x 500, frame 0 matched with one iteration,
    cspm_carry_planes(merge = 0) into frame 1's context.  Time: the library's own hipEvent brackets (CSPM_K_MISC, one per view; each a
    memset and three launches), summed per call; --warmup calls, then the median and min - max of --repeats.  Repeated calls on the same
    fields: WARM-CACHE figures.
(b) A rendered sequence: --frames frames at 741 x 500 of the textured corner with a box in front, exact ground truth, the rig moving a
    0.4 of register_cases.TRUE per frame (the printed pixel motion).  Per method the host clock from cspm_set_images to the
    synchronise behind the sub-pixel post-processing, mean over frames 1 .. (frame 0 is always cold 3), after one untimed pass over
    the sequence; bad-2.0 of the left view against the truth, raw (the plane disparities) and post-processed.
(c) Motorcycle: the left field after three iterations carried into the right view (R = I, t = (-B, 0, 0)): coverage, and the share of
    carried pixels within 1 px of the right view's own field.
(d) With --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 6 --warmup 2 in this tree and in DIR,
    alternating, --bench-runs times each, every run a fresh process."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CAL_MC = (3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4)  # the Motorcycle calibration at quarter size (741 wide)
STEP = 0.4  # of register_cases.TRUE per frame: a pixel moves by 5 .. 20 px


def _bad(disp, gt, thresh=2.0):
    m = np.isfinite(gt)
    return round(float(np.mean(~(np.abs(disp[m] - gt[m]) <= thresh))), 5)


def _motion(cr, fr, i, j):
    return cr.relative_pose(*fr["poses"][i], *fr["poses"][j])


def call_alone(cs, capi, cc, cr, args):
    for w, h in ((1242, 375), (741, 500)):
        fr = cc.frames(w, h, 2, STEP)
        D = int(np.ceil(np.nanmax(fr["truth"][0][0]))) + 8
        src, dst = cs.StereoContext(0), cs.StereoContext(0)
        for ctx, pair in ((src, fr["pairs"][0]), (dst, fr["pairs"][1])):
            ctx.set_images(*pair)
            ctx.build_cost_grd(D, 35, 5, 0.3)
            ctx.patchmatch(1)
        R, t = _motion(cr, fr, 0, 1)
        dst.synchronize()
        dst.enable_timing(True)
        times = []
        for i in range(args.warmup + args.repeats):
            dst.reset_timing()
            dst.carry_planes_from(src, fr["calib"], fr["calib"], R, t, merge=False)
            dst.synchronize()
            tm = dst.timing()["misc"]
            assert tm["launches"] == 2, tm
            if i >= args.warmup:
                times.append(tm["ms"])
        dst.enable_timing(False)
        fields = [src.get_planes(v)[0] for v in (0, 1)]
        _, masks = cr.carry_fields(fields, fr["calib"], fr["calib"], R, t, w, h, D)
        print(json.dumps(dict(case="carry call alone, merge = 0, both views", size=f"{w}x{h}", max_dis=D, ms_median=round(statistics.median(times), 4),
                              ms_min=round(min(times), 4), ms_max=round(max(times), 4), repeats=len(times), launches_per_call=6, memsets_per_call=2,
                              winners=round(float(np.mean([(m == 1).mean() for m in masks])), 4), filled=round(float(np.mean([(m == 2).mean() for m in masks])), 4),
                              note="repeated calls on the same fields: warm-cache figures")), flush=True)
        src.close()
        dst.close()


def sequence(cs, capi, cc, cr, args):
    w, h, n = 741, 500, args.frames
    fr = cc.frames(w, h, n, STEP)
    D = int(np.ceil(max(np.nanmax(tr[0]) for tr in fr["truth"]))) + 8
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    flow = []
    for i in range(1, n):  # how far the pixels of frame i - 1 move: through the exact planes of the view
        R, t = _motion(cr, fr, i - 1, i)
        k = cr.camera(fr["calib"], 0)
        Z = k["fB"] / fr["truth"][i - 1][0]
        P = np.stack([(x - k["cxv"]) * Z / k["f"], (y - k["cy"]) * Z / k["f"], Z])
        Q = np.einsum("ij,jhw->ihw", R, P) + t[:, None, None]
        flow.append(np.hypot(k["f"] * Q[0] / Q[2] + k["cxv"] - x, k["f"] * Q[1] / Q[2] + k["cy"] - y))
    flow = np.stack(flow)
    print(json.dumps(dict(case="rendered sequence", size=f"{w}x{h}", frames=n, max_dis=D, pixel_motion_median=round(float(np.nanmedian(flow)), 2),
                          pixel_motion_p05=round(float(np.nanpercentile(flow, 5)), 2), pixel_motion_p95=round(float(np.nanpercentile(flow, 95)), 2))), flush=True)
    ctxs = [cs.StereoContext(0), cs.StereoContext(0)]
    rng = np.random.default_rng(7)

    def perturbed(R, t):
        """what cspm_fuse_register left on Motorcycle: 0.03 degrees about a random axis, 0.2 % of the baseline in a random direction"""
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = np.radians(0.03)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dR = np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
        d = rng.normal(size=3)
        return dR @ R, t + 0.002 * fr["calib"][3] * d / np.linalg.norm(d)

    def start(ctx, i):
        ctx.set_images(*fr["pairs"][i])
        ctx.build_cost_grd(D, 35, 5, 0.3)

    def cold(iters):
        def run(ctx, prev, i):
            ctx.patchmatch(iters)
        return run

    def box_fit_warm(ctx, prev, i):
        ctx.local_stereo(capi.CA_BOX)
        ctx.fit_planes(merge=False)
        ctx.patchmatch_warm(1)

    def carried(iters, noisy=False):
        def run(ctx, prev, i):
            R, t = _motion(cr, fr, i - 1, i)
            if noisy:
                R, t = perturbed(R, t)
            ctx.pm_init()
            ctx.carry_planes_from(prev, fr["calib"], fr["calib"], R, t, merge=True)
            ctx.patchmatch_warm(iters)
        return run

    methods = [("cold 3", cold(3)), ("cold 1", cold(1)), ("BOX + fit + warm 1", box_fit_warm), ("init + carry + warm 1", carried(1)),
               ("init + carry + warm 2", carried(2)), ("init + carry + warm 1, poses perturbed by 0.03 deg and 0.2 % of the baseline", carried(1, True))]
    for name, run in methods:
        for timed in (False, True):  # one untimed pass over the sequence first
            ms, raw, pp = [], [], []
            for i in range(n):
                ctx, prev = ctxs[i & 1], ctxs[(i - 1) & 1]
                ctx.synchronize()
                t0 = time.perf_counter()
                start(ctx, i)
                if i == 0:
                    ctx.patchmatch(3)
                else:
                    run(ctx, prev, i)
                lp, _ = ctx.postprocess_f64()
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if timed and i > 0:
                    ms.append(dt)
                    raw.append(_bad(ctx.disparity_f64(0), fr["truth"][i][0]))
                    pp.append(_bad(lp, fr["truth"][i][0]))
        print(json.dumps(dict(case="rendered sequence", method=name, frames_timed=len(ms), ms_per_pair_mean=round(statistics.mean(ms), 3), ms_per_pair_min=round(min(ms), 3),
                              ms_per_pair_max=round(max(ms), 3), bad2_raw_mean=round(statistics.mean(raw), 5), bad2_pp_mean=round(statistics.mean(pp), 5),
                              bad2_raw_last=raw[-1], bad2_pp_last=pp[-1], timed="set_images .. synchronise behind postprocess_f64, host clock")), flush=True)
    for c in ctxs:
        c.close()


def motorcycle(cs, capi, rd, cr):
    full = rd.load_full()
    if full is None:
        print(json.dumps({"case": "motorcycle", "skipped": "the pair is not in this checkout"}))
        return
    c, l, r, _ = full
    h, w = l.shape[:2]
    ctx = cs.StereoContext(0)
    ctx.set_images(l, r)
    ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
    ctx.patchmatch(3)
    left = ctx.get_planes(0)[0]
    own = ctx.disparity_f64(1)
    res = capi.carry_plane_field(left, CAL_MC, 0, CAL_MC, 1, w, h, c["max_dis"], np.eye(3), np.array([-CAL_MC[3], 0.0, 0.0]))
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        d = (res["planes"][..., 3] * x + res["planes"][..., 4] * y) + res["planes"][..., 5]
        close = np.abs(d - own) <= 1.0
    S = res["state"]
    print(json.dumps(dict(case="motorcycle left field carried into the right view", size=f"{w}x{h}", pm_iters=3, winners=round(float((S == 1).mean()), 4),
                          filled=round(float((S == 2).mean()), 4), none=round(float((S == 0).mean()), 4),
                          winners_within_1px_of_right_field=round(float(close[S == 1].mean()), 4),
                          carried_within_1px_of_right_field=round(float(close[S != 0].mean()), 4))), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--no-call", action="store_true")
    ap.add_argument("--no-sequence", action="store_true")
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--bench-runs", type=int, default=3)
    args = ap.parse_args()
    if args.parent:  # before this process opens the GPU: the children run alone
        from register_bench import bench_against
        bench_against(os.path.abspath(args.parent), args.bench_runs)
    import torch
    torch.cuda.init()
    import carry_cases as cc
    import carry_ref as cr
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd
    if not args.no_call:
        call_alone(cs, capi, cc, cr, args)
    if not args.no_sequence:
        sequence(cs, capi, cc, cr, args)
    if not args.no_motorcycle:
        motorcycle(cs, capi, rd, cr)


if __name__ == "__main__":
    main()
