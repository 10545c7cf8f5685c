"""What cspm_reproject_device (include/cspm.h "reprojection") costs: one JSON line per case.

    python tools/geom_bench.py [--iters 1] [--repeats 9] [--warmup 3] [--fit_radius 5] [--no-motorcycle]

Cases: the C3 geometry (1242 x 375, synthetic) and the 741 x 500 Motorcycle pair, each after --iters PatchMatch iterations, view 0,
source RAW: dense only, cloud only, both, and the same three with a plane fit.  Time: the library's own hipEvent bracket around the
call's launches on the context's stream (CSPM_K_MISC, cspm_get_timing), one call per measurement, after --warmup calls; median and
min - max of --repeats.  Bytes: what the passes of G must move, computed from the shapes and the kept count --
    the disparity snapshot of RAW (k_plane_to_disp_f64)     24 in + 8 out per pixel
    pass 1   D 8 + slopes 16 in;  depth 8 + xyz 24 + normal 24 + keep 1 out when dense
    pass 3   D 8 + slopes 16 + colour 4 in per pixel again;  32 out per kept pixel
(the fit's own traffic, its 8-byte map in and 48 bytes of planes out, is added for the fitted cases; its arithmetic is what it costs) --
and the share of the 8 TB/s HBM peak that time and those bytes amount to.  A call is two to five launches of a few microseconds each:
at these sizes the figure is launch overhead and latency, not bandwidth, and the JSON says so (`launches`)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes per second, the MI355X's specified peak
CAL = (3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4)  # the Motorcycle calibration at quarter size (741 wide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit_radius", type=int, default=5)
    ap.add_argument("--no-motorcycle", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import crossscalepatchmatch_amd as cs
    from crossscalepatchmatch_amd import capi, realdata as rd, synth

    scenes = []
    c, l, r, _, _ = synth.make_config("C3")
    scenes.append(("C3", c, l, r))
    full = None if args.no_motorcycle else rd.load_full()
    if full is not None:
        scenes.append(("motorcycle", full[0], full[1], full[2]))
    ctx = cs.StereoContext(0)
    for name, c, l, r in scenes:
        h, w = l.shape[:2]
        n = w * h
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        ctx.patchmatch(args.iters)
        ctx.synchronize()
        depth = torch.empty((h, w), dtype=torch.float64, device="cuda")
        xyz = torch.empty((3, h, w), dtype=torch.float64, device="cuda")
        normal = torch.empty((3, h, w), dtype=torch.float64, device="cuda")
        keep = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        cloud = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.enable_timing(True)
        for fit in (None, dict(radius=args.fit_radius)):
            for what in ("dense", "cloud", "both"):
                kw = dict(min_cos=0.3)
                if what != "cloud":
                    kw.update(d_depth=depth.data_ptr(), d_xyz=xyz.data_ptr(), d_normal=normal.data_ptr(), d_keep=keep.data_ptr())
                if what != "dense":
                    kw.update(d_cloud=cloud.data_ptr(), cloud_cap=n, d_count=count.data_ptr())
                times = []
                for k in range(args.warmup + args.repeats):
                    ctx.reset_timing()
                    ctx.reproject_device(0, CAL, capi.GEOM_RAW, fit=fit, **kw)
                    ctx.synchronize()
                    t = ctx.timing()["misc"]
                    assert t["launches"] == 1 and t["evals"] == n, t
                    if k >= args.warmup:
                        times.append(t["ms"])
                kept = int(count.item()) if what != "dense" else None
                moved = n * (24 + 8) + n * 24 + (n * 57 if what != "cloud" else 0)
                launches = 2
                if what != "dense":
                    moved += n * 28 + 32 * kept
                    launches += 2
                if fit is not None:
                    moved += n * (8 + 48)
                    launches += 1
                med = statistics.median(times)
                print(json.dumps({"scene": name, "size": f"{w}x{h}", "outputs": what, "fit_radius": args.fit_radius if fit else 0, "ms_median": round(med, 4),
                                  "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "repeats": len(times), "launches": launches,
                                  "bytes_moved": moved, "share_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4), "kept": kept, "pixels": n,
                                  "note": "launch- and latency-bound at this size: the share of peak is what is left of bandwidth, not a roof that was hit"}),
                      flush=True)
        ctx.enable_timing(False)
    ctx.close()


if __name__ == "__main__":
    main()
