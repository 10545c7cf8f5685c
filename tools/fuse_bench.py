"""What depth-map fusion (include/cspm.h "depth-map fusion") removes and what it costs: one JSON line per case.

    python tools/fuse_bench.py [--repeats 9] [--warmup 3] [--no-motorcycle]

(a) The 741 x 500 Motorcycle pair, both views of the pair pushed as K = 2 (the right pose is the translation by the baseline that
    cspm_fuse_push derives), min_views = 1, after 1 and 3 PatchMatch iterations, sources RAW and PP (consistent pixels only).  Reported:
    the points of the left view's cloud before (cspm_reproject with the same settings) and after fusion, and the share of the EMITTED
    left-view points with known ground truth whose disparity is off by more than 2 px -- before from the map's disparity, after from
    the fused point (d = f B / z - doffs: view 0's camera frame is the world frame here).
(b) A slanted plane rendered for K in {2, 4, 8} poses at 1242 x 375 as plane fields (cspm_set_planes), pushed with cspm_fuse_push (RAW)
    and fused with cspm_fuse_run_device.  Time: the library's own hipEvent bracket around the call's launches (CSPM_K_MISC,
    cspm_get_timing), --warmup calls, then the median and min - max of --repeats.  Repeated calls on the same views: WARM-CACHE figures.
    Bytes: an upper estimate from the shapes (every other view hit by every pixel) --
        a pass, per reference pixel     depth 8 + used 1 + normal 24 in, S 1 out, and per other view depth 8 + normal 24 in
        the records, per kept pixel     the same reads again + 4 of colour per view, 32 out
        a push, per pixel               the RAW snapshot 24 in 8 out, G's dense pass 24 in 33 out, k_fuse_store 13 in 12 out
The rendering comes from the tests' case table (tests/fuse_cases.py, tests/geom_ref.py)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAL_MC = (3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4)  # the Motorcycle calibration at quarter size (741 wide)
CAL_C3 = (720.0, 620.5, 187.0, 0.54, 0.0)


def _bad(disp, gt):
    m = np.isfinite(gt) & np.isfinite(disp)
    return round(float(np.mean(np.abs(disp[m] - gt[m]) > 2.0)), 5) if m.any() else None, int(m.sum())


def motorcycle(ctx, capi, rd):
    full = rd.load_full()
    if full is None:
        print(json.dumps({"case": "motorcycle", "skipped": "the pair is not in this checkout"}))
        return
    c, l, r, gt = full
    h, w = l.shape[:2]
    f, cx, cy, B, doffs = CAL_MC
    eye, zero = np.eye(3), np.zeros(3)
    for iters in (1, 3):
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        ctx.set_pp_speckle(0)
        ctx.set_pp_median(0)
        ctx.patchmatch(iters)
        for source, name, kw in ((capi.GEOM_RAW, "RAW", {}), (capi.GEOM_PP, "PP", dict(consistent_only=1))):
            disp = ctx.disparity_f64(0) if source == capi.GEOM_RAW else ctx.postprocess_f64()[0]
            before = ctx.reproject(0, CAL_MC, source, dense=False, **kw)
            pix = before["cloud"]["pixel"]
            bad_before, known_before = _bad(disp.ravel()[pix], gt.ravel()[pix])
            ctx.fuse_begin(w, h, 2)
            for v in (0, 1):
                ctx.fuse_push(v, CAL_MC, eye, zero, source, **kw)
            res = ctx.fuse_run(min_views=1, state=False)
            ctx.fuse_end()
            left = res["cloud"][:int(res["view_counts"][0])]
            d_after = f * B / left["z"].astype(np.float64) - doffs
            bad_after, known_after = _bad(d_after, gt.ravel()[left["pixel"]])
            print(json.dumps({"case": "motorcycle", "size": f"{w}x{h}", "iters": iters, "source": name, "points_before_left": int(before["count"]),
                              "points_after_left": int(res["view_counts"][0]), "points_after_right": int(res["view_counts"][1]),
                              "bad2_of_emitted_before": bad_before, "known_before": known_before, "bad2_of_emitted_after": bad_after,
                              "known_after": known_after, "params": "max_reproj 2, max_rel_depth 0.01, min_cos 0, min_views 1, suppress 1"}), flush=True)


def rendered(ctx, capi, args):
    import torch
    import fuse_cases as fc
    import geom_ref as gr
    w, h = 1242, 375
    n = w * h
    nrm, dist = fc.PLANE[0], 20.0
    rng = np.random.default_rng(5)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    for K in (2, 4, 8):
        pairs = (K + 1) // 2
        poses = [(fc.rot(rng.uniform(-2, 2), rng.uniform(-5, 5), rng.uniform(-5, 5)) if k else np.eye(3),
                  np.array([0.8 * k, 0.05 * k, 0.3 * (k % 2)])) for k in range(pairs)]
        ctx.fuse_begin(w, h, K)
        ctx.enable_timing(True)
        push_ms = []
        for k, (R, t) in enumerate(poses):
            ctx.set_images(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            m, hh = R.T @ nrm, dist - nrm @ t
            for v in (0, 1):
                D, A, Bs = gr.render_plane(CAL_C3, v, w, h, m, hh)
                planes = np.zeros((h, w, 6))
                planes[..., 2], planes[..., 3], planes[..., 4], planes[..., 5] = 1.0, A, Bs, D - A * x - Bs * y
                ctx.set_planes(v, planes, np.zeros((h, w)))
            for v in (0, 1):
                if 2 * k + v >= K:
                    break
                ctx.synchronize()
                ctx.reset_timing()
                ctx.fuse_push(v, CAL_C3, R, t, capi.GEOM_RAW)
                ctx.synchronize()
                push_ms.append(ctx.timing()["misc"]["ms"])
        cloud = torch.empty((K * n, 32), dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        vcounts = torch.zeros(K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        times = []
        for i in range(args.warmup + args.repeats):
            ctx.reset_timing()
            ctx.fuse_run_device(d_cloud=cloud.data_ptr(), cloud_cap=K * n, d_count=count.data_ptr(), d_view_counts=vcounts.data_ptr(),
                                min_views=min(2, K - 1))
            ctx.synchronize()
            t = ctx.timing()["misc"]
            assert t["launches"] == 1 and t["evals"] == K * n, t
            if i >= args.warmup:
                times.append(t["ms"])
        ctx.enable_timing(False)
        ctx.fuse_end()
        kept = int(count.item())
        per_eval = 8 + 1 + 24 + 1 + (K - 1) * 32
        moved = K * n * (1 + per_eval) + kept * (per_eval + 4 * K + 32)
        med = statistics.median(times)
        print(json.dumps({"case": "rendered plane", "size": f"{w}x{h}", "views": K, "run_ms_median": round(med, 4), "run_ms_min": round(min(times), 4),
                          "run_ms_max": round(max(times), 4), "repeats": len(times), "launches": K + 4, "kept": kept,
                          "view_counts": [int(t) for t in vcounts.cpu().numpy()], "bytes_moved_upper_estimate": moved,
                          "GBps_at_that_estimate": round(moved / (med * 1e-3) / 1e9, 1), "push_ms_median": round(statistics.median(push_ms), 4),
                          "push_bytes": n * (32 + 57 + 25), "note": "repeated calls on the same views: warm-cache figures"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-motorcycle", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd
    ctx = cs.StereoContext(0)
    if not args.no_motorcycle:
        motorcycle(ctx, capi, rd)
    rendered(ctx, capi, args)
    ctx.close()


if __name__ == "__main__":
    main()
