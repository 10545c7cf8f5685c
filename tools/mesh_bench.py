"""What cspm_mesh_device (include/cspm.h "triangle meshes") costs and what it connects: one JSON line per case.

    python tools/mesh_bench.py [--iters 1] [--repeats 9] [--warmup 3] [--fit_radius 5] [--no-motorcycle]

Cases: the C3 geometry (1242 x 375, synthetic) and the 741 x 500 Motorcycle pair, each after --iters PatchMatch iterations, view 0,
source RAW, tau in {0.5, 1, 2}: with the field's slopes, with slopes fitted to the map (--fit_radius), and without slopes (the plain
difference test |D_p - D_q| <= tau).  Time: the library's own hipEvent bracket around the call's launches on the context's stream
(CSPM_K_MISC, cspm_get_timing), one call per measurement, after --warmup calls; median and min - max of --repeats.  The context entries
always carry the field's or the fitted slopes, so the row without slopes comes from cspm_mesh_host on the same disparity map: it has
counts and no time.  Counts: vertices, faces, and the share of quads that get both triangles."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAL = (3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4)  # the Motorcycle calibration at quarter size (741 wide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit_radius", type=int, default=5)
    ap.add_argument("--no-motorcycle", action="store_true")
    args = ap.parse_args()
    import numpy as np
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
        n, nq = w * h, (w - 1) * (h - 1)
        ctx.set_images(l, r)
        ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
        ctx.patchmatch(args.iters)
        ctx.synchronize()
        disp = ctx.disparity_f64(0)
        verts = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        faces = torch.empty((2 * nq, 3), dtype=torch.int32, device="cuda")
        quad = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for tau in (0.5, 1.0, 2.0):
            for slopes, fit in (("field", None), ("fitted", dict(radius=args.fit_radius)), ("none", None)):
                row = {"scene": name, "size": f"{w}x{h}", "tau": tau, "slopes": slopes, "fit_radius": args.fit_radius if fit else 0, "pixels": n, "quads": nq}
                if slopes == "none":
                    res = capi.mesh_host(CAL, 0, disp, max_diff=tau, vertices=False, faces=False)
                    nv, nf, q = res["n_vertices"], res["n_faces"], res["quad"]
                    row.update(ms_median=None, note="cspm_mesh_host on the field's disparity map without slope maps: counts only")
                else:
                    ctx.enable_timing(True)
                    times = []
                    for k in range(args.warmup + args.repeats):
                        ctx.reset_timing()
                        ctx.mesh_device(0, CAL, capi.GEOM_RAW, fit=fit, max_diff=tau, d_vertices=verts.data_ptr(), vertex_cap=n, d_faces=faces.data_ptr(),
                                        face_cap=2 * nq, d_quad=quad.data_ptr(), d_n_vertices=counts.data_ptr(), d_n_faces=counts.data_ptr() + 4)
                        ctx.synchronize()
                        t = ctx.timing()["misc"]
                        assert t["launches"] == 1 and t["evals"] == n, t
                        if k >= args.warmup:
                            times.append(t["ms"])
                    ctx.enable_timing(False)
                    nv, nf = (int(t) for t in counts.cpu().numpy())
                    q = quad.cpu().numpy()
                    row.update(ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4), repeats=len(times),
                               launches=8 + (1 if fit else 0),
                               note="launch- and latency-bound at this size: a chain of dependent launches of a few microseconds each")
                row.update(vertices=nv, faces=nf, share_of_quads_with_both_triangles=round(float(np.mean((q[:-1, :-1] & 3) == 3)), 4),
                           share_of_possible_faces=round(nf / (2 * nq), 4))
                print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
