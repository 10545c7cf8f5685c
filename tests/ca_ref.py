"""numpy restatement of the reference's cost aggregation (CSPM/ca_filter/) and of local stereo over an aggregated cost volume --
the definitions tests/test_gpu_local_stereo.py holds the HIP kernels to.  Every elementwise step is one numpy operation (IEEE f64,
no contraction), in the reference's order; np.add.accumulate sums serially, in the reference's order.

This file is itself held to the reference's own code: tests/test_reference_ca.py compares cumsum, box_filter and aggre_cv with what
ca_filter/*.cpp, compiled unmodified against the test-only OpenCV stand-in, computed (tests/golden/refca_*.npz) -- bit for bit, BF
within rtol 1e-12 (only exp differs; the largest difference seen is 4.3e-16).  One point stays unpinned: `/` is the plain IEEE
quotient here, in the stand-in and in the kernels, while cv::divide of OpenCV 2.4 is believed to share a reciprocal across groups of
elements and may differ in the last place (DESIGN.md sections 2 and 10)."""
import numpy as np

BOX_R, GF_R, GF_EPS = 3, 9, float(np.float32(0.0001))  # BoxCA.cpp:11; GuidedFilter.h:24 (eps is a float promoted to double)
BF_WND, BF_SIG_CLR = 35, 0.03                           # BFCA.cpp:11; BilateralFilter.h:5 (the default, not the .cpp comment's 0.028)
MIN_SIZE = {"BOX": 2 * BOX_R + 1, "GF": 2 * GF_R + 1, "BF": 17}


def cumsum(src, d):
    """CumSum (GuidedFilter.cpp:29-64): d == 1 over y, each row added to the previous one starting from Mat::zeros (0.0 + src[0]);
    d == 2 over x, starting with src[:, 0] itself"""
    src = np.asarray(src, dtype=np.float64)
    if d == 1:
        z = np.concatenate([np.zeros((1,) + src.shape[1:]), src], axis=0)
        return np.add.accumulate(z, axis=0)[1:]
    return np.add.accumulate(src, axis=1)


def box_filter(im, r):
    """BoxFilter (GuidedFilter.cpp:71-122): the unnormalised (2r+1)^2 sum clipped at the borders; needs h, w >= 2r+1"""
    H, W = im.shape
    assert H >= 2 * r + 1 and W >= 2 * r + 1
    dst = np.zeros((H, W))
    cum = cumsum(im, 1)
    dst[:r + 1] = cum[r:2 * r + 1]
    dst[r + 1:H - r] = cum[2 * r + 1:H] - cum[0:H - 2 * r - 1]
    dst[H - r:] = cum[H - 1][None, :] - cum[H - 2 * r - 1:H - r - 1]
    cum = cumsum(dst, 2)
    out = np.zeros((H, W))
    out[:, :r + 1] = cum[:, r:2 * r + 1]
    out[:, r + 1:W - r] = cum[:, 2 * r + 1:W] - cum[:, 0:W - 2 * r - 1]
    out[:, W - r:] = cum[:, W - 1][:, None] - cum[:, W - 2 * r - 1:W - r - 1]
    return out


def guided_filter(I, p, r=GF_R, eps=GF_EPS):
    """GuidedFilter, colour branch with FAST_INV (GuidedFilter.cpp:131-299)"""
    H, W = p.shape
    N = box_filter(np.ones((H, W)), r)
    rgb = [np.ascontiguousarray(I[:, :, c]) for c in range(3)]
    mean_I = [box_filter(rgb[c], r) / N for c in range(3)]
    mean_p = box_filter(p, r) / N
    mean_Ip = [box_filter(rgb[c] * p, r) / N for c in range(3)]
    cov = [mean_Ip[c] - mean_I[c] * mean_p for c in range(3)]
    var = []
    for c in range(3):
        for cp in range(c, 3):
            v = box_filter(rgb[c] * rgb[cp], r) / N
            v = v - mean_I[c] * mean_I[cp]
            var.append(v)
    a11, a12, a13 = var[0] + eps, var[1], var[2]
    a21, a22, a23 = var[1], var[3] + eps, var[4]
    a31, a32, a33 = var[2], var[4], var[5] + eps
    DET = a11 * (a33 * a22 - a32 * a23) - a21 * (a33 * a12 - a32 * a13) + a31 * (a23 * a12 - a22 * a13)
    DET = 1 / DET
    c0, c1, c2 = cov
    a = [DET * (c0 * (a33 * a22 - a32 * a23) + c1 * (a31 * a23 - a33 * a21) + c2 * (a32 * a21 - a31 * a22)),
         DET * (c0 * (a32 * a13 - a33 * a12) + c1 * (a33 * a11 - a31 * a13) + c2 * (a31 * a12 - a32 * a11)),
         DET * (c0 * (a23 * a12 - a22 * a13) + c1 * (a21 * a13 - a23 * a11) + c2 * (a22 * a11 - a21 * a12))]
    b = mean_p.copy()
    for c in range(3):
        b = b - a[c] * mean_I[c]
    q = box_filter(b, r)
    for c in range(3):
        q = q + box_filter(a[c], r) * rgb[c]
    return q / N


def bilateral_filter(I, p, wnd=BF_WND, sig_clr=BF_SIG_CLR):
    """BilateralFilter, colour branch (BilateralFilter.cpp:8-100): sig_sp = wnd / 2.0f, wrap-around borders, taps in raster order.
    p is one slab (h, w) or a stack (n, h, w) filtered slab by slab with the same weights"""
    p = np.asarray(p, dtype=np.float64)
    H, W = p.shape[-2:]
    hw = wnd // 2
    sig_sp = float(np.float32(wnd / 2.0))
    s = np.zeros(p.shape)
    sw = np.zeros((H, W))
    ys, xs = np.arange(H), np.arange(W)
    for wy in range(-hw, hw + 1):
        qy = ys + wy
        qy = np.where(qy < 0, qy + H, qy)
        qy = np.where(qy >= H, qy - H, qy)
        for wx in range(-hw, hw + 1):
            qx = xs + wx
            qx = np.where(qx < 0, qx + W, qx)
            qx = np.where(qx >= W, qx - W, qx)
            Iq = I[qy][:, qx]
            spDis = float(wx * wx + wy * wy)
            clr = np.zeros((H, W))
            for c in range(3):
                clr = clr + np.abs(I[:, :, c] - Iq[:, :, c])
            clr = clr * 0.333333333
            wgt = np.exp(-spDis / (sig_sp * sig_sp) - clr * clr / (sig_clr * sig_clr))
            s = s + wgt * p[..., qy, :][..., qx]
            sw = sw + wgt
    return s / sw


def aggre_cv(method, guide, vol):
    """CAMethod::aggreCV(lImg, rImg, maxDis = len(vol), costVol): slices 1 .. maxDis-1 filtered, slice 0 untouched
    (BoxCA.cpp:8, GFCA.cpp:8, BFCA.cpp:8)"""
    out = np.array(vol, dtype=np.float64, copy=True)
    if method == "BF":
        if len(out) > 1:
            out[1:] = bilateral_filter(guide, out[1:])
        return out
    for d in range(1, len(out)):
        if method == "BOX":
            out[d] = box_filter(out[d], BOX_R)
        elif method == "GF":
            out[d] = guided_filter(guide, out[d])
        else:
            raise ValueError(method)
    return out


def guide_from_bgr(bgr):
    """the local-stereo guide: BGR -> RGB, each 8-bit value times (double)(1.0f/255.0f) (main.cc:77-80, commented out there)"""
    return bgr[:, :, ::-1].astype(np.float64) * float(np.float32(1.0) / np.float32(255.0))


def level_max(agg):
    """max_cost_ of an aggregated level (pre_cs_pc.cc:74-83): starts at -1.0"""
    return max(-1.0, float(np.max(agg)))


def local_costs(agg, maxes, wgts, cs, max_dis, W, H):
    """cost(d) of every level-0 pixel for d = 1 .. max_dis-1 (pre_cs_pc.cc:157-183 / pre_ss_pc.cc:99-111 with a 1x1 window, whose
    weight lookup_exp_[0] is 1.0): agg[s] = aggregated volume (D_s+1, h_s, w_s); returns (max_dis-1, H, W)"""
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((max_dis - 1, H, W))
    for d in range(1, max_dis):
        cost = np.zeros((H, W))
        q = float(d)
        for s in range(len(agg)):
            if s:
                q = q / 2.0
            f = int(q)
            D = agg[s].shape[0] - 1
            if f <= 0 or f >= D:
                c = np.full((H, W), maxes[s])
            else:
                fw = (f + 1) - q
                yy, xx = ys >> s, xs >> s
                c = fw * agg[s][f][yy, xx] + (1 - fw) * agg[s][f + 1][yy, xx]
            if cs:
                sc = 0.0 + 1.0 * c
                cost = cost + sc * wgts[s]
            else:
                cost = cost + 1.0 * c
        out[d - 1] = cost
    return out


def wta(costs):
    """winner-take-all over d = 1 .. : the first d that reaches the minimum (strict < while scanning upward); returns (d*, cost)"""
    best = costs[0].copy()
    bd = np.ones(best.shape, dtype=np.int64)
    for k in range(1, len(costs)):
        better = costs[k] < best
        best = np.where(better, costs[k], best)
        bd = np.where(better, k + 1, bd)
    return bd, best


def local_stereo_view(method, level_bgr, raw, wgts, cs, max_dis):
    """local stereo of one view: level_bgr[s] = the view's level image, raw[s] = its raw cells (D_s+1, h_s, w_s); returns (d*, cost)"""
    agg = [aggre_cv(method, guide_from_bgr(level_bgr[s]), raw[s]) for s in range(len(raw))]
    maxes = [level_max(a) for a in agg]
    H, W = raw[0].shape[1:]
    return wta(local_costs(agg, maxes, wgts, cs, max_dis, W, H))


def planes_of(d):
    """Plane(Vec3d(0,0,1), Point3d(x, y, d)): norm then param, (H, W, 6)"""
    out = np.zeros(d.shape + (6,))
    out[..., 2] = 1.0
    out[..., 3] = -0.0
    out[..., 4] = -0.0
    out[..., 5] = d.astype(np.float64)
    return out
