"""What depth-view registration (include/cspm.h "depth-view registration") costs and what it recovers: one JSON line
per case.

    python tools/register_bench.py [--repeats 9] [--warmup 3] [--no-motorcycle] [--parent DIR [--bench-runs 3] [--parent-first]]

(a) The corner scene of tests/register_cases.py rendered at 1242 x 375 (C3's size) and 741 x 500 (Motorcycle's), four views pushed with
    cspm_fuse_push_maps; view 1 registered from the start pose of the tests (2.07 degrees and 0.071 units off) against 1 and 3 targets,
    strides 1, 2 and 4, 8 iterations.  Time: the library's own hipEvent bracket around the call's 16 launches (CSPM_K_MISC,
    cspm_get_timing), --warmup calls, then the median and min - max of --repeats.  Repeated calls on the same views: WARM-CACHE figures.
    Also reported: the pose error before and after.
(b) The 741 x 500 Motorcycle pair after 3 PatchMatch iterations, both views pushed (cspm_fuse_push; RAW, and PP with consistent pixels
    only).  The true pose of the right view is the translation by the baseline.  It is registered against the left view from a start
    that is off by 1 degree (about the axis (1, 1, 1)) and by 2 % of the baseline.  The world unit is the calibration's (millimetres),
    so max_dist and huber are given in baselines: max_dist = 1 baseline, huber = 0.1 baseline; strides 1 and 4 then 1.
(c) With --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 6 --warmup 2 in this tree and in DIR,
    alternating, --bench-runs times each, every run a fresh process."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAL_MC = (3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4)  # the Motorcycle calibration at quarter size (741 wide)


def _err(R, t, R_true, t_true):
    dR = np.asarray(R).reshape(3, 3) @ R_true.T
    return (float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))), float(np.linalg.norm(np.asarray(t) - t_true)))


def _timed(ctx, args, call):
    times, res = [], None
    for i in range(args.warmup + args.repeats):
        ctx.reset_timing()
        res = call()
        t = ctx.timing()["misc"]
        assert t["launches"] == 1, t
        if i >= args.warmup:
            times.append(t["ms"])
    return res, dict(ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4), repeats=len(times))


def rendered(ctx, args):
    import register_cases as rc
    for w, h in ((1242, 375), (741, 500)):
        views = rc.scene("corner", w, h, 3)
        ctx.fuse_begin(w, h, len(views))
        for v in views:
            ctx.fuse_push_maps(v["depth"], v["f"], v["cx"], v["cy"], v["R"], v["t"], normal=v["normal"])
        ctx.enable_timing(True)
        rot0, tr0 = rc.pose_error(*rc.START)
        for targets in ([0], [0, 2, 3]):
            for stride in (1, 2, 4):
                res, tm = _timed(ctx, args, lambda: ctx.fuse_register(rc.SRC, targets, iters=8, stride=stride))
                rot1, tr1 = rc.pose_error(res["R"], res["t"])
                print(json.dumps(dict(case="rendered corner", size=f"{w}x{h}", targets=len(targets), stride=stride, iters=8, launches=16, **tm,
                                      samples=-(-w // stride) * -(-h // stride), pairs_last=float(res["iters"]["pairs"][-1]),
                                      status=[int(s) for s in res["iters"]["status"]], rot_deg_before=round(rot0, 5), rot_deg_after=round(rot1, 5),
                                      trans_before=round(tr0, 6), trans_after=round(tr1, 6), note="repeated calls on the same views: warm-cache figures")),
                      flush=True)
        ctx.enable_timing(False)
        ctx.fuse_end()


def motorcycle(ctx, capi, rd, args):
    full = rd.load_full()
    if full is None:
        print(json.dumps({"case": "motorcycle", "skipped": "the pair is not in this checkout"}))
        return
    c, l, r, _ = full
    h, w = l.shape[:2]
    B = CAL_MC[3]
    eye, zero = np.eye(3), np.zeros(3)
    R_true, t_true = eye, np.array([B, 0.0, 0.0])
    ax = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    a = np.radians(1.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R0 = eye + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)
    t0 = t_true + 0.02 * B * np.array([0.6, 0.0, 0.8])
    ctx.set_images(l, r)
    ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(3)
    for source, name, kw in ((capi.GEOM_RAW, "RAW", {}), (capi.GEOM_PP, "PP", dict(consistent_only=1))):
        ctx.fuse_begin(w, h, 2)
        for v in (0, 1):
            ctx.fuse_push(v, CAL_MC, eye, zero, source, **kw)
        for schedule in ((1,), (4, 1)):
            R, t, recs = R0, t0, []
            for stride in schedule:
                res = ctx.fuse_register(1, [0], R0=R, t0=t, iters=8, stride=stride, max_dist=B, huber=0.1 * B)
                R, t = res["R"], res["t"]
                recs.append(res["iters"])
            rot0, tr0 = _err(R0, t0, R_true, t_true)
            rot1, tr1 = _err(R, t, R_true, t_true)
            print(json.dumps(dict(case="motorcycle right view against left", size=f"{w}x{h}", pm_iters=3, source=name, strides=list(schedule), iters_each=8,
                                  rot_deg_before=round(rot0, 5), rot_deg_after=round(rot1, 5), trans_before_in_baselines=round(tr0 / B, 5),
                                  trans_after_in_baselines=round(tr1 / B, 5), pairs_last=float(recs[-1]["pairs"][-1]),
                                  cost_first=float(recs[0]["cost"][0]), cost_last=float(recs[-1]["cost"][-1]),
                                  status=[int(s) for it in recs for s in it["status"]], params="max_dist 1 baseline, huber 0.1 baseline, min_cos 0")), flush=True)
        ctx.fuse_end()


def bench_against(parent, runs, parent_first=False):
    """bench.py in this tree and in `parent`, alternating; every run a fresh child process"""
    values = {"this": [], "parent": []}
    order = (("this", ROOT), ("parent", parent))
    for _ in range(runs):
        for name, top in (order[::-1] if parent_first else order):
            p = subprocess.run([sys.executable, os.path.join(top, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2"], cwd=top, capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
            if p.returncode != 0 or not line:
                print(json.dumps({"case": "bench.py", "tree": name, "failed": (p.stdout + p.stderr)[-400:]}), flush=True)
                return
            res = json.loads(line[-1])
            values[name].append(res["ms_per_step"])
            print(json.dumps({"case": "bench.py", "tree": name, "ms_per_step": round(res["ms_per_step"], 3), "value": round(res["value"], 4), "unit": res["unit"]}),
                  flush=True)
    print(json.dumps({"case": "bench.py summary", **{k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in values.items()}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-motorcycle", action="store_true")
    ap.add_argument("--no-rendered", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-first", action="store_true", help="with --parent: the parent's run comes first in every round")
    args = ap.parse_args()
    if args.parent:  # before this process opens the GPU: the children run alone
        bench_against(os.path.abspath(args.parent), args.bench_runs, args.parent_first)
    import torch
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd
    ctx = cs.StereoContext(0)
    if not args.no_rendered:
        rendered(ctx, args)
    if not args.no_motorcycle:
        motorcycle(ctx, capi, rd, args)
    ctx.close()


if __name__ == "__main__":
    main()
