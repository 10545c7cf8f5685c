"""CPU restatement of the warm-start pipeline (include/cspm.h "warm starts"): a stored plane field re-scored under a cost object,
PatchMatch iterations from it, a field carried up one pyramid level, local-stereo start fields and coarse-to-fine -- on the CPU
oracle (oracle/pyoracle.py) and tests/ca_ref.py only.  tests/test_gpu_warm_oracle.py holds the HIP entries to it bit for bit;
tests/test_warm_ref.py holds it to the oracle's cold run and to tests/pyref.py.  It never imports the GPU package.

A field is (h, w, 6) doubles per view, norm then param, the layout of cspm_get_planes / cspm_set_planes."""
import numpy as np

import ca_ref
from oracle import pyoracle as po


def field_of(pm, v):
    """the (h, w, 6) norm+param field of the oracle's view v (a copy)"""
    P = pm.planes(v)
    return np.concatenate([P[..., 0:3], P[..., 6:9]], -1)


def inject(pm, fields):
    """fields[v] (h, w, 6) -> the oracle's live plane state: norm, point = (x, y, a*x + b*y + c), param.  View propagation and
    refinement recompute the disparity from param, so this is a complete start state; min_cost is left as it is (rescore)."""
    xs = np.arange(pm.w, dtype=np.float64)[None, :]
    ys = np.arange(pm.h, dtype=np.float64)[:, None]
    for v in (0, 1):
        f = np.asarray(fields[v], dtype=np.float64)
        assert f.shape == (pm.h, pm.w, 6), f.shape
        P = pm.planes(v)
        P[..., 0:3] = f[..., 0:3]
        P[..., 3] = xs
        P[..., 4] = ys
        P[..., 5] = f[..., 3] * xs + f[..., 4] * ys + f[..., 5]
        P[..., 6:9] = f[..., 3:6]


def rescore(pm, pc, sum_order=po.SUM_SERIAL):
    """cspm_rescore_planes: min_cost of every stored plane of both views under pc, the planes untouched"""
    for v in (0, 1):
        P, cost = pm.planes(v), pm.min_cost(v)
        for y in range(pm.h):
            for x in range(pm.w):
                cost[y, x] = pc.cost(x, y, P[y, x, 0:3], P[y, x, 6:9], v, sum_order)


def iterate(pm, pc, iters, **opts):
    """iterations 0 .. iters-1 of a cold run from the state that is there: spatial, view, refine"""
    for it in range(iters):
        pm.spatial(it, pc, **opts)
        pm.view(it, pc, **opts)
        pm.refine(it, pc, **opts)


def warm_run(pm, pc, iters, **opts):
    """cspm_patchmatch_warm: the random init replaced by a re-score of the stored field, then the random streams and sweep
    directions of a cold run (opts as for PatchMatch.run: seed, schedule, sum_order, rng_mode, rb_rounds, rb_neighbours)"""
    rescore(pm, pc, opts.get("sum_order", po.SUM_SERIAL))
    iterate(pm, pc, iters, **opts)


def upsample(fields, w, h):
    """cspm_upsample_planes: pixel (x, y) of the w x h field takes the plane at (x>>1, y>>1), normal, a and b as they are, c doubled"""
    out = []
    for f in fields:
        f = np.asarray(f, dtype=np.float64)
        assert f.shape == ((h + 1) // 2, (w + 1) // 2, 6), f.shape
        up = f[np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1].copy()
        up[..., 5] = up[..., 5] * 2.0
        out.append(up)
    return out


def local_stereo_fields(pc, method, max_dis, cs):
    """cspm_local_stereo's plane fields (BOX / GF): ca_ref over the oracle's own level images, raw cells and scale weights"""
    wgts = pc.scale_wgt()
    out = []
    for v in (0, 1):
        bgr = [pc.image(v, s) for s in range(pc.levels)]
        raw = [pc.volume(v, s) for s in range(pc.levels)]
        d, _ = ca_ref.local_stereo_view(method, bgr, raw, wgts, cs, max_dis)
        out.append(ca_ref.planes_of(d))
    return out


def coarse_to_fine(l, r, max_dis, coarse_iters=3, fine_iters=1, cc="GRD", wnd_size=35, scale_num=5, reg_lambda=0.3, dis_scale=4, **opts):
    """capi.coarse_to_fine step by step: a cold run on the full cost object's level-1 images with max_dis (max_dis + 1) // 2 and
    the same cost settings, its field upsampled, then a warm run on the full pair.  Returns (pm, pc) of the full pair."""
    pc = po.PlaneCost(l, r, max_dis, wnd_size, scale_num, reg_lambda, cc)
    if scale_num < 2:  # a single-scale cost has no level 1: a two-level cost provides the pyrDown images
        two = po.PlaneCost(l, r, max_dis, wnd_size, 2, 0.0, "IMG")
        half = [two.image(v, 1).copy() for v in (0, 1)]
    else:
        half = [pc.image(v, 1).copy() for v in (0, 1)]
    cmax = (max_dis + 1) // 2
    cpc = po.PlaneCost(half[0], half[1], cmax, wnd_size, scale_num, reg_lambda, cc)
    cpm = po.PatchMatch(half[0], half[1], cmax, dis_scale)
    cpm.run(coarse_iters, cpc, False, **opts)
    h, w = np.asarray(l).shape[:2]
    pm = po.PatchMatch(l, r, max_dis, dis_scale)
    inject(pm, upsample([field_of(cpm, v) for v in (0, 1)], w, h))
    warm_run(pm, pc, fine_iters, **opts)
    return pm, pc
