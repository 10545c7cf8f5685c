"""CPU restatement of the speckle filter S, written from the specification: plain union-find over the pixels.

S(D, V, max_size, max_diff) -> V'.  Nodes are the pixels with V = 1.  Two nodes are joined when they are 4-neighbours and
|D[p] - D[q]| <= max_diff, compared in f64, false when either value is NaN, pairwise between the two neighbours.  n(p) is the size of
p's connected component, 0 for a non-node.  V'[p] = V[p] && n(p) > max_size.
"""
import numpy as np

import pp_sub_ref as ps


def component_sizes(d, valid, max_diff):
    """n(p) as an (h, w) int32 array"""
    d = np.asarray(d, dtype=np.float64)
    h, w = d.shape
    v = np.ones((h, w), bool) if valid is None else np.asarray(valid) != 0
    thr = np.float64(max_diff)
    with np.errstate(invalid="ignore"):  # inf - inf and NaN operands: the comparison is False, as the specification wants
        right = v[:, :-1] & v[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= thr)
        down = v[:-1, :] & v[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= thr)
    parent = list(range(h * w))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for y, x in zip(*np.nonzero(right)):
        a, b = find(int(y) * w + int(x)), find(int(y) * w + int(x) + 1)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for y, x in zip(*np.nonzero(down)):
        a, b = find(int(y) * w + int(x)), find((int(y) + 1) * w + int(x))
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = np.fromiter((find(i) for i in range(h * w)), np.int64, h * w)
    nodes = v.ravel()
    count = np.bincount(roots[nodes], minlength=h * w)
    return np.where(nodes, count[roots], 0).astype(np.int32).reshape(h, w)


def speckle_filter(d, valid, max_size, max_diff):
    """S: returns (V' as u8, n as int32)"""
    n = component_sizes(d, valid, max_diff)
    v = np.ones(n.shape, bool) if valid is None else np.asarray(valid) != 0
    return (v & (n > max_size)).astype(np.uint8), n


def postprocess_f64_speckle(abc_l, abc_r, img_l, img_r, max_dis, max_size, max_diff):
    """sub-pixel PostProcessing with the filter between the left-right check and the fill: pp_sub_ref's steps as they are, S in between.
    Returns (l, r, l_valid', r_valid', removed): f64 maps, u8 masks after the filter, pixels removed from both masks together."""
    abc = [np.ascontiguousarray(abc_l, dtype=np.float64), np.ascontiguousarray(abc_r, dtype=np.float64)]
    img = [np.asarray(img_l), np.asarray(img_r)]
    d = [ps.plane_disp(abc[0]), ps.plane_disp(abc[1])]
    checked = [ps.lr_check(d, v) for v in (0, 1)]
    if max_size > 0:
        valid = [speckle_filter(d[v], checked[v], max_size, max_diff)[0] != 0 for v in (0, 1)]
    else:
        valid = checked
    removed = int(sum((checked[v] & ~valid[v]).sum() for v in (0, 1)))
    out = []
    for v in (0, 1):
        filled = ps.fill(abc[v], d[v], valid[v], max_dis)
        out.append(ps.weighted_median(img[v], d[v], filled, valid[v]))
    return out[0], out[1], valid[0].astype(np.uint8), valid[1].astype(np.uint8), removed
