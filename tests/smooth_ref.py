"""CPU restatement of the edge-aware global smoother, written from the specification
S(D, C, I, lambda, sigma, T, max_dis) -> O, twice:

  smooth_py     line by line in Python floats (one IEEE f64 operation per operator, nothing contracted)
  smooth        numpy operations across the lines of a pass, serial along each line (numpy does not contract a multiply and an add;
                no reduction is used)

and composed with pp_sub_ref / median_ref for the pipeline (postprocess_f64_smooth).

A pixel is a node when D is finite; c = C at a node, 0.0 elsewhere; N = c * D at a node, 0.0 elsewhere; M = c.  LUT[k] = exp(-k / sigma);
the weight between neighbours is LUT[|dB| + |dG| + |dR|], 1.0 without a guide.  For t = 1 .. T: lambda_t = ((1.5 * 4^(T-t)) / (4^T - 1)) *
lambda, a horizontal pass over every row, then a vertical pass over every column.  A pass solves per line, for F = N and F = M,
    a = -(lambda_t * wl) (0.0 at i = 0), cc = -(lambda_t * wr) (0.0 at i = n-1), b = (1.0 - a) - cc
    r = 1.0 / b, ct[0] = cc * r, ft[0] = F[0] * r;  r = 1.0 / (b - ct[i-1] * a), ct[i] = cc * r, ft[i] = (F[i] - ft[i-1] * a) * r
    U[n-1] = ft[n-1], U[i] = ft[i] - ct[i] * U[i+1]
O = N / M where M > 0 (clamped to [0, max_dis] when max_dis > 0), D's own bits elsewhere.
"""
import math

import numpy as np

import median_ref as mr

PALETTE = np.array([[20, 30, 40], [26, 30, 44], [60, 50, 40], [200, 190, 180]], np.uint8)  # a guide whose weights are neither all 1 nor all negligible
DEFAULTS = dict(lam=100.0, sigma_color=20.0, iterations=3, fill_conf=0.25)


def lut(sigma):
    return np.array([math.exp(-k / sigma) for k in range(766)])


def lambdas(lam, T):
    return [((1.5 * float(4 ** (T - t))) / float(4 ** T - 1)) * lam for t in range(1, T + 1)]


def weights(guide, sigma, shape):
    """(wh, wv): wh[y, x] between (x, y) and (x+1, y), shape (h, w-1); wv[y, x] between (x, y) and (x, y+1), shape (h-1, w)"""
    h, w = shape
    if guide is None:
        return np.ones((h, max(w - 1, 0))), np.ones((max(h - 1, 0), w))
    g = np.asarray(guide).astype(np.int64)
    assert g.shape == (h, w, 3)
    table = lut(sigma)
    return table[np.abs(g[:, 1:] - g[:, :-1]).sum(axis=2)], table[np.abs(g[1:] - g[:-1]).sum(axis=2)]


def init(D, C):
    D = np.ascontiguousarray(D, dtype=np.float64)
    node = np.isfinite(D)
    c = np.where(node, 1.0 if C is None else np.asarray(C, dtype=np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        N = np.where(node, c * np.where(node, D, 0.0), 0.0)
    return D, N, c.copy()


def finish(D, N, M, max_dis):
    out = D.copy()
    q = M > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        z = N[q] / M[q]
    if max_dis > 0:
        z = np.where(z > 0, z, 0.0)
        z = np.where(z < float(max_dis), z, float(max_dis))
    out[q] = z
    return out


# ---- line by line in Python floats -------------------------------------------------------------------------------------------------
def solve_line_py(FN, FM, w, lam_t):
    """one line: FN, FM lists of n floats, w the n-1 weights between neighbours.  Returns (UN, UM)."""
    n = len(FN)
    ct, fn, fm = [0.0] * n, [0.0] * n, [0.0] * n
    for i in range(n):
        a = -(lam_t * w[i - 1]) if i > 0 else 0.0
        cc = -(lam_t * w[i]) if i < n - 1 else 0.0
        b = (1.0 - a) - cc
        if i == 0:
            r = 1.0 / b
            ct[0] = cc * r
            fn[0] = FN[0] * r
            fm[0] = FM[0] * r
        else:
            r = 1.0 / (b - ct[i - 1] * a)
            ct[i] = cc * r
            fn[i] = (FN[i] - fn[i - 1] * a) * r
            fm[i] = (FM[i] - fm[i - 1] * a) * r
    un, um = [0.0] * n, [0.0] * n
    un[n - 1], um[n - 1] = fn[n - 1], fm[n - 1]
    for i in range(n - 2, -1, -1):
        un[i] = fn[i] - ct[i] * un[i + 1]
        um[i] = fm[i] - ct[i] * um[i + 1]
    return un, um


def smooth_py(D, C=None, guide=None, lam=100.0, sigma_color=20.0, iterations=3, max_dis=0):
    D, N, M = init(D, C)
    h, w = D.shape
    wh, wv = weights(guide, sigma_color, (h, w))
    N, M = N.tolist(), M.tolist()
    wh, wv = wh.tolist(), wv.tolist()
    for lam_t in lambdas(float(lam), iterations):
        for y in range(h):
            N[y], M[y] = solve_line_py(N[y], M[y], wh[y], lam_t)
        for x in range(w):
            un, um = solve_line_py([N[y][x] for y in range(h)], [M[y][x] for y in range(h)], [wv[y][x] for y in range(h - 1)], lam_t)
            for y in range(h):
                N[y][x], M[y][x] = un[y], um[y]
    return finish(D, np.array(N, dtype=np.float64).reshape(h, w), np.array(M, dtype=np.float64).reshape(h, w), max_dis)


# ---- numpy across lines, serial along each line ------------------------------------------------------------------------------------
def solve_lines(FN, FM, w, lam_t):
    """every line at once: FN, FM (lines, n), w (lines, n-1); serial in i"""
    lines, n = FN.shape
    ct, fn, fm = np.zeros((lines, n)), np.zeros((lines, n)), np.zeros((lines, n))
    zero = np.zeros(lines)
    for i in range(n):
        a = -(lam_t * w[:, i - 1]) if i > 0 else zero
        cc = -(lam_t * w[:, i]) if i < n - 1 else zero
        b = (1.0 - a) - cc
        if i == 0:
            r = 1.0 / b
            ct[:, 0] = cc * r
            fn[:, 0] = FN[:, 0] * r
            fm[:, 0] = FM[:, 0] * r
        else:
            r = 1.0 / (b - ct[:, i - 1] * a)
            ct[:, i] = cc * r
            fn[:, i] = (FN[:, i] - fn[:, i - 1] * a) * r
            fm[:, i] = (FM[:, i] - fm[:, i - 1] * a) * r
    un, um = np.zeros((lines, n)), np.zeros((lines, n))
    un[:, n - 1], um[:, n - 1] = fn[:, n - 1], fm[:, n - 1]
    for i in range(n - 2, -1, -1):
        un[:, i] = fn[:, i] - ct[:, i] * un[:, i + 1]
        um[:, i] = fm[:, i] - ct[:, i] * um[:, i + 1]
    return un, um


def horizontal_pass(N, M, wh, lam_t):
    return solve_lines(N, M, wh, lam_t)


def vertical_pass(N, M, wv, lam_t):
    un, um = solve_lines(np.ascontiguousarray(N.T), np.ascontiguousarray(M.T), np.ascontiguousarray(wv.T), lam_t)
    return np.ascontiguousarray(un.T), np.ascontiguousarray(um.T)


def smooth(D, C=None, guide=None, lam=100.0, sigma_color=20.0, iterations=3, max_dis=0, with_quotient_mask=False):
    """S; with_quotient_mask: also the mask M > 0 of the pixels whose output came from the quotient"""
    D, N, M = init(D, C)
    wh, wv = weights(guide, sigma_color, D.shape)
    for lam_t in lambdas(float(lam), iterations):
        N, M = horizontal_pass(N, M, wh, lam_t)
        N, M = vertical_pass(N, M, wv, lam_t)
    out = finish(D, N, M, max_dis)
    return (out, M > 0) if with_quotient_mask else out


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def postprocess_f64_smooth(abc_l, abc_r, img_l, img_r, max_dis, median_r=0, params=None):
    """pp_sub_ref.postprocess_f64, then M64 when median_r > 0, then S on both maps when params is given (a dict: lam, sigma_color,
    iterations, fill_conf) with C = 1.0 where the view's mask is 1 and fill_conf elsewhere, I = the view's image, the same max_dis.
    The masks are the unsmoothed run's."""
    l, r, lv, rv = mr.postprocess_f64_median(abc_l, abc_r, img_l, img_r, max_dis, median_r)
    if params is not None:
        p = dict(DEFAULTS, **params)
        if p["lam"] != 0:
            out = []
            for d, v, img in ((l, lv, img_l), (r, rv, img_r)):
                conf = np.where(v != 0, 1.0, float(p["fill_conf"]))
                out.append(smooth(d, conf, img, p["lam"], p["sigma_color"], p["iterations"], max_dis))
            l, r = out
    return l, r, lv, rv
