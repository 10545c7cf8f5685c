"""CPU restatement of candidate-field merging (include/cspm.h "candidate fields"): a candidate plane per pixel
that wins only where it costs less than the stored plane, the random init as such a challenger (keep-init), and the seeded pipelines
built from them -- on tests/warm_ref.py and the CPU oracle (oracle/pyoracle.py) only.  tests/test_gpu_seed.py holds the HIP entries to
it bit for bit; tests/test_seed_ref.py checks the restatement itself without a GPU.  It never imports the GPU package.

A field is (h, w, 6) doubles per view, norm then param, the layout of cspm_get_planes; a mask is (h, w), 0 = no candidate.  For the
CENGRD cost pc is tests/cengrd_ref.py's plane_cost(): an oracle cost object whose volumes hold the CENGRD cells."""
import numpy as np

import warm_ref
from oracle import pyoracle as po


def has_candidate(field, mask=None):
    """(h, w) bool: the pixels of a candidate field that carry a candidate -- mask != 0 and all six values finite"""
    f = np.asarray(field, dtype=np.float64)
    ok = np.isfinite(f).all(axis=2)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


def merge(pm, pc, fields, masks=(None, None), sum_order=po.SUM_SERIAL):
    """cspm_merge_planes / cspm_merge_planes_host: fields[v] (None: view v is not merged) offered to the oracle's live state.  Every
    pixel on its own: the candidate taken whole, its cost under pc, accepted where cost < min_cost (strict).  The stored costs have to
    belong to pc (warm_ref.rescore otherwise).  Returns the number of accepted candidates."""
    taken = 0
    for v in (0, 1):
        if fields[v] is None:
            continue
        f = np.asarray(fields[v], dtype=np.float64)
        assert f.shape == (pm.h, pm.w, 6), f.shape
        ok = has_candidate(f, masks[v])
        P, cost = pm.planes(v), pm.min_cost(v)
        for y in range(pm.h):
            for x in range(pm.w):
                if not ok[y, x]:
                    continue
                c = pc.cost(x, y, f[y, x, 0:3], f[y, x, 3:6], v, sum_order)
                if c < cost[y, x]:
                    P[y, x, 0:3] = f[y, x, 0:3]
                    P[y, x, 3:6] = (x, y, f[y, x, 3] * x + f[y, x, 4] * y + f[y, x, 5])  # the point warm_ref.inject gives a plane
                    P[y, x, 6:9] = f[y, x, 3:6]
                    cost[y, x] = c
                    taken += 1
    return taken


def init_keep(pm, pc, **opts):
    """cspm_pm_init_keep: the oracle's own InitRandomPlane (seed, rng_mode, sum_order of opts) as the challenger of the state that is
    there; the stored plane stays on a tie.  Returns the number of pixels that took their random plane."""
    old = [(pm.planes(v).copy(), pm.min_cost(v).copy()) for v in (0, 1)]
    pm.init(pc, **opts)
    taken = 0
    for v in (0, 1):
        keep = ~(pm.min_cost(v) < old[v][1])
        pm.planes(v)[keep] = old[v][0][keep]
        pm.min_cost(v)[keep] = old[v][1][keep]
        taken += int((~keep).sum())
    return taken


def seeded_run(pm, pc, iters, seeds=(), **opts):
    """capi.seeded_patchmatch: the random init, every seed (fields, masks) merged in turn, then iterations 0 .. iters-1 of a cold run"""
    pm.init(pc, **opts)
    for fields, masks in seeds:
        merge(pm, pc, fields, masks, opts.get("sum_order", po.SUM_SERIAL))
    warm_ref.iterate(pm, pc, iters, **opts)


def keep_run(pm, pc, iters, **opts):
    """CSPatchMatch::PatchMatchKeep: the stored field re-scored, keep-init, then the iterations"""
    warm_ref.rescore(pm, pc, opts.get("sum_order", po.SUM_SERIAL))
    init_keep(pm, pc, **opts)
    warm_ref.iterate(pm, pc, iters, **opts)


def disparity_planes(disp):
    """(h, w) disparities -> the fronto-parallel planes (0, 0, 1, 0, 0, d)"""
    d = np.asarray(disp, dtype=np.float64)
    f = np.zeros(d.shape + (6,))
    f[..., 2] = 1.0
    f[..., 5] = d
    return f
