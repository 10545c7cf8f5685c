"""What TSDF fusion (include/cspm.h "TSDF fusion") costs and what its raycast is worth: one JSON line per case.

    python tools/tsdf_bench.py [--repeats 9] [--warmup 3] [--no-motorcycle]

(a) Integration: one exact 1242 x 375 render of the slanted plane (tests/fuse_cases.py) with normals and an image, integrated into a 128^3
    and a 256^3 volume around the plane.  Time: the library's own hipEvent bracket (CSPM_K_MISC, one launch); --warmup calls, then the
    median and min - max of --repeats.  Repeated calls on the same volume: WARM-CACHE figures.  bytes = 24 per voxel (12 read, 12
    written; an upper bound: voxels that leave early write nothing) plus the view's 36 bytes per pixel; the share of the 8 TB/s HBM peak
    follows from them.
(b) Raycast of the 256^3 volume at 1242 x 375 and 741 x 500, and (c) the extraction of its surface points, timed the same way; next to
    it the triangle mesh of the same volume, counts only and with records: the points extraction is the figure the
    mesh is to be compared with (it reads the same two planes about four times over), with the share of vertices no face refers to.
(d) Motorcycle at 741 x 500 after three iterations, both views of the pair integrated (PP source, consistent pixels), raycast at the
    left pose: bad-2.0 of d = f B / z - doffs on the status-1 pixels against the ground truth, next to the post-processed map itself; and
    the mesh of that volume: faces, and whether it has a boundary away from unknown cells (an edge used in one direction only whose two
    vertices' edges are surrounded by known cells)."""
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
HBM_PEAK = 8.0e12


def _timed(ctx, call, args):
    ctx.synchronize()
    ctx.enable_timing(True)
    times = []
    for i in range(args.warmup + args.repeats):
        ctx.reset_timing()
        call()
        t = ctx.timing()["misc"]
        if i >= args.warmup:
            times.append(t["ms"])
    ctx.enable_timing(False)
    return dict(ms_median=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4), launches=int(t["launches"]))


def rendered(ctx, args):
    import fuse_cases as fc
    w, h = 1242, 375
    cam = fc.camera(w, h, 0)
    depth, normal, bgr = fc.render(cam, w, h, [(fc.PLANE[0], fc.PLANE[1], None)])
    ctx.fuse_begin(w, h, 1)
    ctx.fuse_push_maps(depth, cam["f"], cam["cx"], cam["cy"], cam["R"], cam["t"], normal=normal, bgr=bgr)
    for n in (128, 256):
        voxel = 4.8 / n
        ctx.tsdf_begin((-2.4, -2.4, 1.6), voxel, (n, n, n))
        res = _timed(ctx, lambda: ctx.tsdf_integrate(0), args)
        moved = 24 * n ** 3 + 36 * w * h
        res.update(case="integrate", volume=f"{n}^3", view=f"{w}x{h}", bytes=moved, tb_per_s=round(moved / (res["ms_median"] * 1e-3) / 1e12, 3),
                   share_of_hbm_peak=round(moved / (res["ms_median"] * 1e-3) / HBM_PEAK, 4), cache="warm")
        print(json.dumps(res), flush=True)
        if n == 256:
            for rw, rh in ((1242, 375), (741, 500)):
                rc = fc.camera(rw, rh, 0)
                out = {}
                res = _timed(ctx, lambda: out.update(ctx.tsdf_raycast(rc, rw, rh, 0.0, outputs=("status",))), args)
                res.update(case="raycast", volume=f"{n}^3", size=f"{rw}x{rh}", hits=int((out["status"] == 1).sum()), cache="warm",
                           note="the bracket holds the kernel alone; the download of the status map is outside it")
                print(json.dumps(res), flush=True)
            cnt = {}
            res = _timed(ctx, lambda: cnt.update(ctx.tsdf_points(cloud=False)), args)
            res.update(case="extract_count_only", volume=f"{n}^3", points=cnt["count"], cache="warm")
            print(json.dumps(res), flush=True)
            res = _timed(ctx, lambda: cnt.update(ctx.tsdf_points()), args)
            res.update(case="extract", volume=f"{n}^3", points=cnt["count"], cache="warm")
            print(json.dumps(res), flush=True)
            mesh = {}
            res = _timed(ctx, lambda: mesh.update(ctx.tsdf_mesh(vertices=False, faces=False)), args)
            res.update(case="mesh_count_only", volume=f"{n}^3", vertices=mesh["n_vertices"], faces=mesh["n_faces"], cache="warm")
            print(json.dumps(res), flush=True)
            res = _timed(ctx, lambda: mesh.update(ctx.tsdf_mesh()), args)
            used = len(np.unique(mesh["faces"]["v"]))
            res.update(case="mesh", volume=f"{n}^3", vertices=mesh["n_vertices"], faces=mesh["n_faces"],
                       unreferenced_vertex_share=round(1.0 - used / max(mesh["n_vertices"], 1), 5), cache="warm",
                       note="the bracket holds the kernels alone; the downloads of the records are outside it")
            print(json.dumps(res), flush=True)
        ctx.tsdf_end()
    ctx.fuse_end()


def open_edges(faces, n_vertices):
    """-> (directed edges without their reverse, the vertices on them): the boundary of the mesh"""
    v = faces["v"].astype(np.int64)
    a = np.concatenate([v[:, 0], v[:, 1], v[:, 2]])
    b = np.concatenate([v[:, 1], v[:, 2], v[:, 0]])
    fwd, back = a * n_vertices + b, b * n_vertices + a
    alone = ~np.isin(fwd, back)
    return int(alone.sum()), np.unique(np.concatenate([a[alone], b[alone]]))


def _bad(disp, gt):
    m = np.isfinite(gt) & np.isfinite(disp)
    return (round(float(np.mean(np.abs(disp[m] - gt[m]) > 2.0)), 5) if m.any() else None), int(m.sum())


def motorcycle(ctx, capi, rd):
    full = rd.load_full()
    if full is None:
        print(json.dumps({"case": "motorcycle", "skipped": "the pair is not in this checkout"}))
        return
    c, l, r, gt = full
    h, w = l.shape[:2]
    f, cx, cy, B, doffs = CAL_MC
    eye, zero = np.eye(3), np.zeros(3)
    ctx.set_images(l, r)
    ctx.build_cost_grd(c["max_dis"], 35, c["scale_num"], c["reg_lambda"])
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(3)
    pp = ctx.postprocess_f64(valid=True)
    disp = np.where(pp[2] != 0, pp[0], np.nan) if len(pp) > 2 else pp[0]
    bad_pp, known_pp = _bad(disp, gt)
    g = ctx.reproject(0, CAL_MC, capi.GEOM_PP, cloud=False, consistent_only=1)
    z = g["depth"][g["keep"] != 0]
    z0, z1 = np.percentile(z, [1, 99])
    n = 256
    voxel = float(max(z1 * w / f, z1 - z0) * 1.1 / n)
    origin = (-(cx / f) * z1 * 1.05, -(cy / f) * z1 * 1.05, float(z0) - 8 * voxel)
    ctx.fuse_begin(w, h, 2)
    for v in (0, 1):
        ctx.fuse_push(v, CAL_MC, eye, zero, capi.GEOM_PP, consistent_only=1)
    ctx.tsdf_begin(origin, voxel, (n, n, n))
    for v in (0, 1):
        ctx.tsdf_integrate(v)
    ray = ctx.tsdf_raycast(dict(f=f, cx=cx, cy=cy, R=eye, t=zero), w, h, 0.0, outputs=("depth", "status"))
    mesh = ctx.tsdf_mesh()
    W = ctx.tsdf_volume()["W"].reshape(-1)
    ctx.tsdf_end()
    # a boundary edge is "at an unknown cell" when a voxel within one step of either vertex's voxel has W = 0 or lies at the volume's border
    n_open, on_open = open_edges(mesh["faces"], mesh["n_vertices"])
    vox = mesh["vertices"]["pixel"][on_open].astype(np.int64)
    i, j, k = vox % n, (vox // n) % n, vox // (n * n)
    near_unknown = np.zeros(len(vox), bool)
    for dk in (-1, 0, 1, 2):
        for dj in (-1, 0, 1, 2):
            for di in (-1, 0, 1, 2):
                ii, jj, kk = i + di, j + dj, k + dk
                inside = (ii >= 0) & (ii < n) & (jj >= 0) & (jj < n) & (kk >= 0) & (kk < n)
                near_unknown |= ~inside | (W[np.clip((kk * n + jj) * n + ii, 0, n ** 3 - 1)] <= 0.0)
    print(json.dumps({"case": "motorcycle_mesh", "volume": f"{n}^3", "vertices": mesh["n_vertices"], "faces": mesh["n_faces"], "open_edges": n_open,
                      "open_edge_vertices_away_from_unknown_voxels": int((~near_unknown).sum())}), flush=True)
    ctx.fuse_end()
    d = np.where(ray["status"] == 1, f * B / ray["depth"] - doffs, np.nan)
    bad, known = _bad(d, gt)
    print(json.dumps({"case": "motorcycle", "size": f"{w}x{h}", "iters": 3, "source": "PP, consistent pixels", "volume": f"{n}^3", "voxel": round(voxel, 3),
                      "status1_pixels": int((ray["status"] == 1).sum()), "bad2_of_raycast": bad, "known_raycast": known,
                      "bad2_of_consistent_pp_map": bad_pp, "known_pp": known_pp}), flush=True)


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
    rendered(ctx, args)
    if not args.no_motorcycle:
        motorcycle(ctx, capi, rd)
    ctx.close()


if __name__ == "__main__":
    main()
