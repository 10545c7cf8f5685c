"""The CPU restatements of the reprojection G (tests/geom_ref.py; include/cspm.h "reprojection"): they agree with
each other bit for bit, give the exact dyadic answers, keep the specification's identities and borders, build the cloud as specified and
recover a rendered 3-D plane.  Also every CSPM_ERR_ARG the library answers before it opens a device, and the host layer's calibration
reader and PLY writer (tests/helpers/geom_io_check.cc, once more under AddressSanitizer and UBSan as a stand-alone program)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import geom_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL = (300.0, 31.5, 20.25, 0.25, 3.5)


def _random_case(rng, w, h):
    D = rng.uniform(-6.0, 40.0, (h, w))
    D[rng.uniform(size=(h, w)) < 0.05] = np.nan
    D[rng.uniform(size=(h, w)) < 0.03] = np.inf
    D[rng.uniform(size=(h, w)) < 0.03] = -np.inf
    D[rng.uniform(size=(h, w)) < 0.03] = -CAL[4]  # t == 0
    V = (rng.uniform(size=(h, w)) > 0.2).astype(np.uint8)
    A = rng.uniform(-0.6, 0.6, (h, w))
    Bs = rng.uniform(-0.6, 0.6, (h, w))
    A[rng.uniform(size=(h, w)) < 0.05] = np.nan
    Bs[rng.uniform(size=(h, w)) < 0.05] = np.inf
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return D, V, A, Bs, img


@pytest.mark.parametrize("v,left_frame", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("slopes", [False, True])
def test_the_two_restatements_agree_bit_for_bit(v, left_frame, slopes):
    rng = np.random.default_rng(5 + v)
    w, h = 23, 9
    D, V, A, Bs, img = _random_case(rng, w, h)
    kw = dict(z_near=1.0, z_far=60.0, min_cos=0.35, left_frame=left_frame)
    res = gr.reproject(CAL, v, D, V, A if slopes else None, Bs if slopes else None, img, **kw)
    assert 0 < res["count"] < res["ok"].sum() if slopes else res["count"] == res["ok"].sum()
    for y in range(h):
        for x in range(w):
            p = gr.reproject_pixel(CAL, v, x, y, D[y, x], V[y, x], A[y, x] if slopes else None, Bs[y, x] if slopes else None, **kw)
            assert p["ok"] == bool(res["ok"][y, x]) and p["keep"] == bool(res["keep"][y, x])
            want = (p["X"], p["Y"], p["Z"]) if p["ok"] else (gr.NAN,) * 3
            assert gr.same_bits(res["xyz"][:, y, x], np.array(want)), (x, y)
            assert gr.same_bits(res["depth"][y, x], np.float64(want[2]))
            if slopes:
                assert gr.same_bits(res["normal"][:, y, x], np.array(p["N"] if p["ok"] else (gr.NAN,) * 3)), (x, y)
                assert gr.same_bits(res["cos"][y, x], np.float64(p["cos"]))


def test_exact_dyadic_known_answers():
    cal = (256.0, 8.0, 4.0, 0.5, 0.0)
    D = np.full((9, 17), 4.0)
    res = gr.reproject(cal, 0, D, None, np.zeros_like(D), np.zeros_like(D))
    assert np.all(res["depth"] == 32.0)
    assert res["xyz"][0, 4, 8] == 0.0 and res["xyz"][1, 4, 8] == 0.0 and res["xyz"][2, 4, 8] == 32.0
    assert res["xyz"][0, 0, 0] == -1.0 and res["xyz"][1, 0, 0] == -0.5  # (0 - 8) * 32 / 256, (0 - 4) * 32 / 256
    np.testing.assert_array_equal(res["normal"], np.broadcast_to(np.array([0.0, 0.0, -1.0])[:, None, None], (3, 9, 17)))
    p = gr.reproject_pixel(cal, 0, 8, 4, 4.0, 1, 0.0, 0.0)
    assert (p["X"], p["Y"], p["Z"], p["N"], p["cos"]) == (0.0, 0.0, 32.0, (0.0, 0.0, -1.0), 1.0)
    assert gr.reproject(cal, 1, D, left_frame=1)["xyz"][0, 4, 8] == 0.5


def test_cosine_identity_and_sign():
    rng = np.random.default_rng(9)
    w, h = 41, 17
    D = rng.uniform(0.5, 40.0, (h, w))
    A, Bs = rng.uniform(-2, 2, (h, w)), rng.uniform(-2, 2, (h, w))
    res = gr.reproject(CAL, 0, D, None, A, Bs)
    f, cx, cy, _, doffs = CAL
    u, wv = np.arange(w)[None, :] - cx, np.arange(h)[:, None] - cy
    t = D + doffs
    ln = np.sqrt((A * f) ** 2 + (Bs * f) ** 2 + (t - A * u - Bs * wv) ** 2)
    ray = np.sqrt(u * u + wv * wv + f * f)
    np.testing.assert_allclose(res["cos"] * ln * ray, f * t, rtol=8 * np.finfo(float).eps)  # three roundings of cos, two of each root
    assert np.all(res["cos"] > 0.0) and np.all(res["cos"] <= 1.0 + 4 * np.finfo(float).eps)
    np.testing.assert_allclose(np.sqrt((res["normal"] ** 2).sum(0)), 1.0, rtol=4 * np.finfo(float).eps)
    assert np.all((res["normal"] * np.stack([np.broadcast_to(u, D.shape), np.broadcast_to(wv, D.shape), np.full(D.shape, f)])).sum(0) < 0)


def test_range_borders_min_cos_and_left_frame():
    cal = (256.0, 0.0, 0.0, 0.5, 0.0)
    D = np.array([[2.0, 4.0, 8.0, 16.0]])  # Z = 64, 32, 16, 8
    np.testing.assert_array_equal(gr.reproject(cal, 0, D, z_near=16.0, z_far=32.0)["keep"], [[0, 1, 1, 0]])  # both borders inclusive
    np.testing.assert_array_equal(gr.reproject(cal, 0, D, z_near=np.nextafter(16.0, 17), z_far=np.nextafter(32.0, 0))["keep"], [[0, 0, 0, 0]])
    A = np.array([[0.0, 0.005, 0.1, np.nan]])
    res = gr.reproject(cal, 0, D, None, A, np.zeros_like(A), min_cos=0.5)
    assert res["cos"][0, 0] == 1.0 and res["cos"][0, 1] > 0.5 > res["cos"][0, 2] and np.isnan(res["cos"][0, 3])
    np.testing.assert_array_equal(res["keep"], [[1, 1, 0, 0]])  # a NaN cosine fails the test
    np.testing.assert_array_equal(res["ok"], [[1, 1, 1, 1]])     # ... but the pixel stays ok: its dense depth is there
    assert gr.reproject(cal, 0, D, None, A, np.zeros_like(A), min_cos=0.0)["count"] == 4
    at = gr.reproject(cal, 0, D, None, A, np.zeros_like(A), min_cos=float(res["cos"][0, 1]))
    np.testing.assert_array_equal(at["keep"], [[1, 1, 0, 0]])  # cos >= min_cos: equality keeps
    x0 = gr.reproject(cal, 1, D)["xyz"][0]
    np.testing.assert_array_equal(gr.reproject(cal, 1, D, left_frame=1)["xyz"][0], x0 + 0.5)
    np.testing.assert_array_equal(gr.reproject(cal, 0, D, left_frame=1)["xyz"][0], gr.reproject(cal, 0, D)["xyz"][0])


def test_cloud_order_capacity_pixel_colour_and_rounding():
    rng = np.random.default_rng(3)
    w, h = 19, 7
    D, V, A, Bs, img = _random_case(rng, w, h)
    full = gr.reproject(CAL, 0, D, V, A, Bs, img)
    cl = full["cloud"]
    assert full["count"] == len(cl) == full["keep"].sum() > 20
    np.testing.assert_array_equal(cl["pixel"], np.flatnonzero(full["keep"].ravel()))  # raster order, pixel = y*w + x
    assert np.all(np.diff(cl["pixel"].astype(np.int64)) > 0)
    ys, xs = np.divmod(cl["pixel"], w)
    X64 = gr.reproject(CAL, 0, D, None, A, Bs)["xyz"]  # ok without the mask: the kept pixels are a subset
    for k, name in enumerate("xyz"):
        assert gr.same_bits(cl[name], X64[k, ys, xs].astype(np.float32))
    N = full["normal"]
    for k, name in enumerate(("nx", "ny", "nz")):
        assert gr.same_bits(cl[name], N[k, ys, xs].astype(np.float32))
    assert np.isnan(cl["nx"]).any()  # a NaN slope is kept when min_cos == 0 and its normal stays NaN
    np.testing.assert_array_equal(np.stack([cl["b"], cl["g"], cl["r"]], 1), img[ys, xs])
    assert np.all(cl["a"] == 255)
    for cap in (0, 5, len(cl), len(cl) + 9):
        part = gr.reproject(CAL, 0, D, V, A, Bs, img, cap=cap)
        assert part["count"] == len(cl) and gr.same_cloud(part["cloud"], cl[:cap])
    bare = gr.reproject(CAL, 0, D, V)["cloud"]
    assert np.isnan(bare["nx"]).all() and not (bare["b"] | bare["g"] | bare["r"] | bare["a"]).any()
    one = np.float64(1.0) + 2.0 ** -24  # a tie between two floats: round to nearest even
    assert gr.reproject((1.0, 0.0, 0.0, float(one), 0.0), 0, np.array([[1.0]]))["cloud"]["z"][0] == np.float32(1.0)


# ---- the analytic check: a rendered 3-D plane comes back -----------------------------------------------------------------------------
# Measured with this restatement (numpy seed 0, 200 cameras, 130 x 67, f in [300, 4000], depth 5 .. 60 baselines): the largest normal
# error is 3.34e-16 (view 0; 2.23e-16 in view 1) and the largest relative plane residual 8.24e-16 (view 1, in its own frame and moved
# to the left frame; 7.83e-16 in view 0).  The bounds are 100 times the measured values (the margin of DESIGN.md section 17); a
# transcription slip shows at 1e-3 or worse.
NORMAL_BOUND = 100 * 3.34e-16
PLANE_BOUND = 100 * 8.24e-16


def rendered_plane_errors(cameras=200, w=130, h=67, seed=0):
    rng = np.random.default_rng(seed)
    worst = {}
    for _ in range(cameras):
        f = rng.uniform(300.0, 4000.0)
        B = rng.uniform(0.05, 2.0)
        cal = (f, rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, B, rng.uniform(-30.0, 30.0))
        m = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
        m /= np.linalg.norm(m)
        z0 = rng.uniform(5.0, 60.0) * B  # depth of the plane on the optical axis of view 0
        hh = m[2] * z0
        for v, lf in ((0, 0), (1, 0), (1, 1)):
            D, A, Bs = gr.render_plane(cal, v, w, h, m, hh)
            res = gr.reproject(cal, v, D, None, A, Bs, left_frame=lf)
            assert res["ok"].all()
            hv = hh - B * m[0] if (v == 1 and not lf) else hh  # in camera 1's own frame the plane is m . P = hh - B m0
            e_n = np.abs(res["normal"] + m[:, None, None]).max()
            e_p = np.abs((res["xyz"] * m[:, None, None]).sum(0) - hv).max() / abs(hv)
            key = (v, lf)
            worst[key] = (max(worst.get(key, (0, 0))[0], e_n), max(worst.get(key, (0, 0))[1], e_p))
    return worst


def test_rendered_plane_comes_back():
    worst = rendered_plane_errors()
    print("rendered plane, (view, left_frame) -> (normal error, relative plane residual):", worst)
    for key, (e_n, e_p) in worst.items():
        assert e_n <= NORMAL_BOUND, (key, e_n)
        assert e_p <= PLANE_BOUND, (key, e_p)


# ---- argument errors the library answers without a device ----------------------------------------------------------------------------

def _lib():
    from crossscalepatchmatch_amd import capi
    return capi, capi.load_library()


def _host_rc(capi, L, cal=CAL, view=0, w=4, h=3, disp=True, a=False, b=False, normal=False, stride=None, **params):
    n = w * h if w > 0 and h > 0 else 1
    d = np.ones(n)
    sa, sb, nrm = np.zeros(n), np.zeros(n), np.zeros(3 * n)
    img = np.zeros(3 * n, np.uint8)
    k, g = capi.calib_struct(cal), capi.geom_params(**params)
    dp, u8 = capi._dp, capi._u8
    return L.cspm_reproject_host(0, C.byref(k), C.byref(g), view, dp(d) if disp else None, None, dp(sa) if a else None, dp(sb) if b else None,
                                 u8(img) if stride is not None else None, stride or 0, w, h, None, None, dp(nrm) if normal else None, None, None, 0, None)


def test_argument_errors_need_no_device():
    capi, L = _lib()
    ERR_ARG = -1
    nan, inf = math.nan, math.inf
    bad_cal = [(0.0, 1, 1, 1, 0), (-5.0, 1, 1, 1, 0), (300.0, 1, 1, 0.0, 0), (300.0, 1, 1, -1.0, 0), (nan, 1, 1, 1, 0), (300.0, inf, 1, 1, 0),
               (300.0, 1, nan, 1, 0), (300.0, 1, 1, inf, 0), (300.0, 1, 1, 1, nan), (inf, 1, 1, 1, 0)]
    for cal in bad_cal:
        assert not gr.check_args(cal) and _host_rc(capi, L, cal=cal) == ERR_ARG, cal
    bad_params = [dict(z_near=nan), dict(z_near=-1.0), dict(z_near=5.0, z_far=4.0), dict(z_far=nan), dict(min_cos=-0.1), dict(min_cos=1.5),
                  dict(min_cos=nan)]
    for p in bad_params:
        assert not gr.check_args(CAL, **p) and _host_rc(capi, L, **p) == ERR_ARG, p
        assert b"reprojection" in L.cspm_last_error(None)
    for kw in (dict(view=2), dict(view=-1), dict(disp=False), dict(w=0), dict(h=0), dict(w=65536, h=32768), dict(a=True), dict(b=True),
               dict(normal=True), dict(stride=11)):
        assert _host_rc(capi, L, **kw) == ERR_ARG, kw
    g = capi.GeomParams()
    assert L.cspm_geom_default_params(None) == ERR_ARG and L.cspm_geom_default_params(C.byref(g)) == 0
    assert (g.z_near, g.z_far, g.min_cos, g.left_frame, g.consistent_only) == (0.0, inf, 0.0, 0, 0)
    assert gr.check_args(CAL) and gr.check_args(CAL, z_near=0.0, z_far=0.0, min_cos=1.0)
    k = capi.calib_struct(CAL)
    assert L.cspm_reproject(None, 0, 0, C.byref(k), None, None, None, None, None, None, None, 0, None) == ERR_ARG
    assert L.cspm_reproject_device(None, 0, 0, C.byref(k), None, None, None, None, None, None, None, 0, None) == ERR_ARG
    assert capi.Point == gr.POINT and C.sizeof(capi.Calib) == 40 and C.sizeof(capi.GeomParams) == 32


# ---- the host layer's readers and writers ---------------------------------------------------------------------------------------------

def _build_io_check(tmp_path, *flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("geom_io_check" + ("_san" if flags else "")))
    cmd = [cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "crossscalepatchmatch_amd", "host"),
           os.path.join(ROOT, "tests", "helpers", "geom_io_check.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return exe, r


def _run_io_check(exe, tmp_path):
    ply = str(tmp_path / "cloud.ply")
    r = subprocess.run([exe, ply], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "geom_io_check ok" in r.stdout
    return ply


def test_calibration_reader_and_ply_writer(tmp_path):
    exe, r = _build_io_check(tmp_path)
    assert r.returncode == 0, r.stderr
    ply = _run_io_check(exe, tmp_path)
    raw = open(ply, "rb").read()
    head, _, body = raw.partition(b"end_header\n")
    want_head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                 b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n")
    assert head == want_head
    rec = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    assert rec.itemsize == 27 and len(body) == 3 * 27
    pts = np.frombuffer(body, rec)
    # the three records geom_io_check.cc writes: (1, 2, 3) n (0, 0, -1) bgr (10, 20, 30); (-0.5, 0.25, 8) n (0.6, 0, -0.8) bgr (255, 0, 128);
    # (4, 5, 6) with a NaN normal, written as 0 0 0
    np.testing.assert_array_equal(pts["p"], np.array([[1, 2, 3], [-0.5, 0.25, 8], [4, 5, 6]], np.float32))
    np.testing.assert_array_equal(pts["n"], np.array([[0, 0, -1], [0.6, 0, -0.8], [0, 0, 0]], np.float32))
    np.testing.assert_array_equal(pts["rgb"], [[30, 20, 10], [128, 0, 255], [7, 8, 9]])


def test_calibration_reader_and_ply_writer_under_sanitizers(tmp_path):
    exe, r = _build_io_check(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0:
        pytest.skip("the C++ compiler has no AddressSanitizer / UBSan runtime: " + r.stderr.strip().splitlines()[-1][:120])
    _run_io_check(exe, tmp_path)
