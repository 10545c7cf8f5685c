"""The CPU restatements of the mesh specification M (tests/mesh_ref.py; include/cspm.h "triangle meshes"): they
agree with each other bit for bit, give the known answers on a rendered plane, a step, a hole and a diagonal tie, wind every face towards
the camera, index only existing vertices, keep raster order and the capacity rules.  Also every CSPM_ERR_ARG the library answers before
it opens a device, and the host layer's mesh writer (tests/helpers/mesh_io_check.cc, once more under AddressSanitizer and UBSan as a
stand-alone program)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import geom_ref as gr
import mesh_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL = (300.0, 31.5, 20.25, 0.25, 3.5)


def random_case(rng, w, h, holes=True):
    """a slanted surface with a rough half, so that every tau connects some pixels and cuts others; the exact half is dyadic: tau = 0
    connects it"""
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    D = 0.5 * x + 0.25 * y + 8.0
    A, Bs = np.full((h, w), 0.5), np.full((h, w), 0.25)
    rough = rng.uniform(size=(h, w)) < 0.5
    D = np.where(rough, D + rng.uniform(-0.6, 0.6, (h, w)), D)
    A = np.where(rough, A + rng.uniform(-0.3, 0.3, (h, w)), A)
    V = None
    if holes:
        D[rng.uniform(size=(h, w)) < 0.04] = np.nan
        D[rng.uniform(size=(h, w)) < 0.02] = np.inf
        D[rng.uniform(size=(h, w)) < 0.02] = -np.inf
        D[rng.uniform(size=(h, w)) < 0.02] = -CAL[4]  # t == 0
        D[rng.uniform(size=(h, w)) < 0.02] = -30.0    # t < 0
        V = (rng.uniform(size=(h, w)) > 0.1).astype(np.uint8)
        A[rng.uniform(size=(h, w)) < 0.05] = np.nan
        Bs[rng.uniform(size=(h, w)) < 0.05] = np.inf
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return D, V, A, Bs, img


@pytest.mark.parametrize("tau", [0.0, 0.5, math.inf])
@pytest.mark.parametrize("all_vertices", [0, 1])
@pytest.mark.parametrize("v,slopes", [(0, True), (1, True), (0, False)])
def test_the_two_restatements_agree_bit_for_bit(tau, all_vertices, v, slopes):
    rng = np.random.default_rng(11 + v)
    w, h = 19, 9
    D, V, A, Bs, img = random_case(rng, w, h)
    kw = dict(max_diff=tau, all_vertices=all_vertices, z_near=1.0, z_far=60.0, min_cos=0.09, left_frame=v)
    a = mr.mesh(CAL, v, D, V, A if slopes else None, Bs if slopes else None, img, **kw)
    b = mr.mesh_py(CAL, v, D, V, A if slopes else None, Bs if slopes else None, img, **kw)
    assert mr.same_mesh(b, a, "scalar against numpy") is None
    assert np.array_equal(a["vert"], b["vert"])
    assert a["n_vertices"] <= a["keep"].sum() < w * h
    if all_vertices:
        assert a["n_vertices"] == a["keep"].sum() > 0
    if tau == math.inf:  # every triangle whose corners are kept
        assert a["n_faces"] > 50
    elif slopes:
        assert 0 < a["n_faces"] < mr.mesh(CAL, v, D, V, A, Bs, img, **dict(kw, max_diff=math.inf))["n_faces"]


def _edges(faces):
    e = np.sort(np.concatenate([faces["v"][:, [0, 1]], faces["v"][:, [1, 2]], faces["v"][:, [2, 0]]]).astype(np.int64), axis=1)
    return np.unique(e, axis=0)


def _plane(a_sign, v=0, w=23, h=11):
    """a rendered 3-D plane with |a| = 1.5 disparities per pixel"""
    m = np.array([0.6 * a_sign, 0.1, 0.0])
    m[2] = math.sqrt(1.0 - m[0] ** 2 - m[1] ** 2)
    B = CAL[3]
    hh = B * m[0] / (1.5 * a_sign) + v * B * m[0]  # a = B m0 / (hh - v B m0)
    D, A, Bs = gr.render_plane(CAL, v, w, h, m, hh)
    assert abs(abs(A[0, 0]) - 1.5) < 1e-12 and (D + CAL[4] > 0).all()
    return D, A, Bs


@pytest.mark.parametrize("a_sign", [1, -1])
@pytest.mark.parametrize("v", [0, 1])
def test_known_answers_on_a_rendered_plane(a_sign, v):
    w, h = 23, 11
    D, A, Bs = _plane(a_sign, v, w, h)
    res = mr.mesh(CAL, v, D, None, A, Bs, max_diff=1e-6)
    assert res["n_faces"] == 2 * (w - 1) * (h - 1)
    assert res["n_vertices"] == w * h and res["vert"].all()
    assert res["n_vertices"] - len(_edges(res["faces"])) + res["n_faces"] == 1  # a disc
    assert np.all((res["quad"][:-1, :-1] & 3) == 3) and not res["quad"][-1].any() and not res["quad"][:, -1].any()
    # the plain difference test tears the steep surface: every triangle has a horizontal edge, and |a| = 1.5 > tau = 1
    plain = mr.mesh(CAL, v, D, None, None, None, max_diff=1.0)
    assert plain["n_faces"] == 0 and plain["n_vertices"] == 0 and not (plain["quad"] & 3).any()
    assert mr.mesh(CAL, v, D, None, None, None, max_diff=1.0, all_vertices=1)["n_vertices"] == w * h


def test_a_step_is_cut():
    w, h, cut = 17, 7, 9
    D = np.full((h, w), 10.0)
    D[:, cut:] = 13.0
    Z = np.zeros((h, w))
    res = mr.mesh(CAL, 0, D, None, Z, Z, max_diff=1.0)
    side = (res["vertices"]["pixel"] % w >= cut)[res["faces"]["v"].astype(np.int64)]
    assert np.all(side.all(1) | (~side).all(1)), "a face bridges the step"
    assert res["n_faces"] == 2 * (cut - 1) * (h - 1) + 2 * (w - cut - 1) * (h - 1) and res["n_vertices"] == w * h
    assert mr.mesh(CAL, 0, D, None, Z, Z, max_diff=3.0)["n_faces"] == 2 * (w - 1) * (h - 1)  # tau is inclusive


def test_a_hole_removes_four_triangles_and_resplits_its_quads():
    w, h, hx, hy = 9, 7, 4, 3
    D = np.full((h, w), 12.0)
    V = np.ones((h, w), np.uint8)
    V[hy, hx] = 0
    res = mr.mesh(CAL, 0, D, V, max_diff=0.0)
    assert res["n_faces"] == 2 * (w - 1) * (h - 1) - 4 and res["n_vertices"] == w * h - 1
    Q = res["quad"]
    # the hole is p00 of its own quad: only the anti diagonal is kept, T0 holds p00 -> T1 alone; p11 of the quad above left: anti, T0 alone;
    # p10 of the quad on the left: main, T0 = (p00, p01, p11) alone; p01 of the quad above: main, T1 = (p00, p11, p10) alone
    assert (Q[hy, hx], Q[hy - 1, hx - 1], Q[hy, hx - 1], Q[hy - 1, hx]) == (4 | 2, 4 | 1, 1, 2)
    other = np.ones((h, w), bool)
    other[hy - 1:hy + 1, hx - 1:hx + 1] = False
    other[-1], other[:, -1] = False, False
    assert np.all(Q[other] == 3) and res["vmap"][hy, hx] == -1


def test_the_diagonal_tie_takes_main():
    flat = mr.mesh(CAL, 0, np.full((2, 2), 9.0), max_diff=1.0)
    assert flat["quad"][0, 0] == 3 and flat["faces"]["v"].tolist() == [[0, 2, 3], [0, 3, 1]]
    D = np.array([[10.0, 10.25], [10.25, 10.5]])  # |D00 - D11| = 0.5 > |D10 - D01| = 0
    anti = mr.mesh(CAL, 0, D, max_diff=1.0)
    assert anti["quad"][0, 0] == 7 and anti["faces"]["v"].tolist() == [[0, 2, 1], [1, 2, 3]]
    D = np.array([[10.0, 10.5], [10.0, 10.5]])   # |D00 - D11| = |D10 - D01| = 0.5: a tie
    assert mr.mesh(CAL, 0, D, max_diff=1.0)["quad"][0, 0] == 3


def _face_normals(res, v, left_frame):
    """(unit geometric normals, P0 in the view's own camera frame) of every face, from the f64 points"""
    P = res["xyz"].reshape(3, -1).T[res["vertices"]["pixel"].astype(np.int64)][res["faces"]["v"].astype(np.int64)]  # (nf, 3 corners, 3)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    P0 = P[:, 0].copy()
    if left_frame and v == 1:
        P0[:, 0] -= CAL[3]
    return n / np.linalg.norm(n, axis=1)[:, None], P0


@pytest.mark.parametrize("v,left_frame", [(0, 0), (1, 0), (1, 1)])
def test_every_face_is_wound_towards_the_camera(v, left_frame):
    rng = np.random.default_rng(21)
    D, V, A, Bs, img = random_case(rng, 31, 13)
    res = mr.mesh(CAL, v, D, V, A, Bs, img, max_diff=math.inf, left_frame=left_frame)
    n, P0 = _face_normals(res, v, left_frame)
    assert res["n_faces"] > 300 and np.all((n * P0).sum(1) < 0)
    for a_sign in (1, -1):
        D, A, Bs = _plane(a_sign, v)
        n, P0 = _face_normals(mr.mesh(CAL, v, D, None, A, Bs, max_diff=1e-6, left_frame=left_frame), v, left_frame)
        assert np.all((n * P0).sum(1) < 0)


# Measured with this restatement (numpy seed 0, 60 cameras, 33 x 17, f in [300, 4000], depth 5 .. 60 baselines, tau = 1e-6): the largest
# difference between a face's unit geometric normal and G's normal of its first vertex is FACE_NORMAL_MEASURED.  The cross product of two
# one-pixel edges cancels about f / 1 digits of the points, which is why this is far above section 19's vertex normal error.  The bound is
# 100 times the measured value (the margin of DESIGN.md sections 17 and 19); a transcription slip -- a wrong winding, a swapped corner --
# shows at order 1.
FACE_NORMAL_MEASURED = 1.43e-12  # view 0; 1.38e-12 in view 1, in its own frame and in the left one
FACE_NORMAL_BOUND = 100 * FACE_NORMAL_MEASURED


def face_normal_errors(cameras=60, w=33, h=17, seed=0):
    rng = np.random.default_rng(seed)
    worst = {}
    for _ in range(cameras):
        f = rng.uniform(300.0, 4000.0)
        B = rng.uniform(0.05, 2.0)
        cal = (f, rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, B, rng.uniform(-30.0, 30.0))
        m = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.0])
        m /= np.linalg.norm(m)
        hh = m[2] * rng.uniform(5.0, 60.0) * B
        for v, lf in ((0, 0), (1, 0), (1, 1)):
            D, A, Bs = gr.render_plane(cal, v, w, h, m, hh)
            res = mr.mesh(cal, v, D, None, A, Bs, max_diff=1e-6, left_frame=lf)
            assert res["n_faces"] == 2 * (w - 1) * (h - 1)
            P = res["xyz"].reshape(3, -1).T[res["faces"]["v"].astype(np.int64)]  # every pixel is a vertex: vertex number = pixel
            n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
            n /= np.linalg.norm(n, axis=1)[:, None]
            G = res["normal"].reshape(3, -1).T[res["faces"]["v"][:, 0].astype(np.int64)]
            worst[(v, lf)] = max(worst.get((v, lf), 0.0), float(np.abs(n - G).max()))
    return worst


def test_face_normals_equal_the_vertex_normals_on_a_rendered_plane():
    worst = face_normal_errors()
    print("rendered plane, (view, left_frame) -> largest |face normal - G's normal|:", worst)
    for key, e in worst.items():
        assert e <= FACE_NORMAL_BOUND, (key, e)


def test_faces_index_existing_vertices_in_raster_order():
    rng = np.random.default_rng(31)
    w, h = 29, 12
    D, V, A, Bs, img = random_case(rng, w, h)
    for all_vertices in (0, 1):
        res = mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=0.5, all_vertices=all_vertices)
        F, pix = res["faces"]["v"].astype(np.int64), res["vertices"]["pixel"].astype(np.int64)
        assert res["n_faces"] > 50 and F.max() < res["n_vertices"] == len(pix)
        assert np.all(np.diff(pix) > 0)                        # vertices in raster order
        if not all_vertices:
            assert set(np.unique(F)) == set(range(len(pix)))   # every vertex is used, none is missing
            assert res["n_vertices"] < res["keep"].sum()
        corners = pix[F]                                       # the faces' corner pixels
        origin = corners.min(1)                                # main: p00; anti T0: p00; anti T1: p10 = origin + 1
        q = res["quad"].ravel()
        anti_t1 = (q[origin - 1] & 4).astype(bool) & (corners[:, 0] == origin) & (corners[:, 1] == origin + w - 1)
        origin = np.where(anti_t1, origin - 1, origin)
        assert np.all(np.diff(origin) >= 0)                    # faces in raster order of the quad origin
        same = np.flatnonzero(np.diff(origin) == 0)            # both triangles of one quad: T0 first
        d = corners - origin[:, None]
        t0 = (d[:, 0] == 0) & (d[:, 1] == w)
        assert np.all(t0[same]) and not np.any(t0[same + 1])
        assert np.all(np.isin(d, (0, 1, w, w + 1)))
        assert np.bincount(origin, minlength=w * h).tolist() == ((q & 1) + (q >> 1 & 1)).tolist()
    cloud = gr.reproject(CAL, 0, D, V, A, Bs, img)["cloud"]
    assert gr.same_cloud(mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=0.5, all_vertices=1)["vertices"], cloud)  # the vertices ARE the cloud


def test_counts_against_capacities():
    rng = np.random.default_rng(41)
    D, V, A, Bs, img = random_case(rng, 21, 9)
    full = mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=0.5)
    nv, nf = full["n_vertices"], full["n_faces"]
    assert nv > 20 and nf > 20
    for vcap, fcap in ((0, 0), (5, 7), (nv - 1, nf - 1), (nv, nf), (nv + 3, nf + 3)):
        for fn in (mr.mesh, mr.mesh_py):
            part = fn(CAL, 0, D, V, A, Bs, img, max_diff=0.5, vertex_cap=vcap, face_cap=fcap)
            assert (part["n_vertices"], part["n_faces"]) == (nv, nf)
            assert gr.same_cloud(part["vertices"], full["vertices"][:vcap]) and np.array_equal(part["faces"]["v"], full["faces"]["v"][:fcap])
    assert mr.mesh(CAL, 0, D[:1], max_diff=math.inf)["n_faces"] == 0 and mr.mesh(CAL, 0, D[:, :1], max_diff=math.inf)["n_faces"] == 0  # no quads


# ---- argument errors the library answers without a device ----------------------------------------------------------------------------

def _host_rc(capi, L, cal=CAL, view=0, w=4, h=3, disp=True, a=False, b=False, stride=None, geom=None, **mesh):
    n = w * h if w > 0 and h > 0 else 1
    d, sa, sb, img = np.ones(n), np.zeros(n), np.zeros(n), np.zeros(3 * n, np.uint8)
    k, g, m = capi.calib_struct(cal), capi.geom_params(**(geom or {})), capi.mesh_params(**mesh)
    dp, u8 = capi._dp, capi._u8
    return L.cspm_mesh_host(0, C.byref(k), C.byref(g), C.byref(m), view, dp(d) if disp else None, None, dp(sa) if a else None, dp(sb) if b else None,
                            u8(img) if stride is not None else None, stride or 0, w, h, None, 0, None, 0, None, None, None)


def test_argument_errors_need_no_device():
    from crossscalepatchmatch_amd import capi
    L = capi.load_library()
    ERR_ARG = -1
    nan, inf = math.nan, math.inf
    for bad in (dict(max_diff=nan), dict(max_diff=-1.0), dict(max_diff=-inf), dict(max_diff=-1e-300)):
        assert not mr.check_args(**bad) and _host_rc(capi, L, **bad) == ERR_ARG, bad
        assert b"mesh" in L.cspm_last_error(None)
    for cal in ((0.0, 1, 1, 1, 0), (300.0, 1, 1, 0.0, 0), (nan, 1, 1, 1, 0), (300.0, 1, 1, 1, inf)):
        assert _host_rc(capi, L, cal=cal) == ERR_ARG, cal
    for geom in (dict(z_near=-1.0), dict(z_near=5.0, z_far=4.0), dict(min_cos=1.5), dict(min_cos=nan)):
        assert _host_rc(capi, L, geom=geom) == ERR_ARG, geom
    for kw in (dict(view=2), dict(view=-1), dict(disp=False), dict(w=0), dict(h=0), dict(w=65536, h=32768), dict(a=True), dict(b=True), dict(stride=11)):
        assert _host_rc(capi, L, **kw) == ERR_ARG, kw
    m = capi.MeshParams()
    assert L.cspm_mesh_default_params(None) == ERR_ARG and L.cspm_mesh_default_params(C.byref(m)) == 0
    assert (m.max_diff, m.all_vertices) == (1.0, 0)
    assert mr.check_args() and mr.check_args(max_diff=0.0) and mr.check_args(max_diff=inf)
    k = capi.calib_struct(CAL)
    assert L.cspm_mesh(None, 0, 0, C.byref(k), None, None, None, None, 0, None, 0, None, None, None) == ERR_ARG
    assert L.cspm_mesh_device(None, 0, 0, C.byref(k), None, None, None, None, 0, None, 0, None, None, None) == ERR_ARG
    assert capi.Face == mr.FACE and capi.Point == mr.POINT and C.sizeof(capi.MeshParams) == 16


# ---- the host layer's mesh writer -----------------------------------------------------------------------------------------------------

def _build_io_check(tmp_path, *flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("mesh_io_check" + ("_san" if flags else "")))
    cmd = [cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "crossscalepatchmatch_amd", "host"),
           os.path.join(ROOT, "tests", "helpers", "mesh_io_check.cc"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run_io_check(exe, tmp_path):
    ply = str(tmp_path / "mesh.ply")
    r = subprocess.run([exe, ply], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh_io_check ok" in r.stdout
    return ply


def test_mesh_writer(tmp_path):
    exe, r = _build_io_check(tmp_path)
    assert r.returncode == 0, r.stderr
    ply = _run_io_check(exe, tmp_path)
    head, _, body = open(ply, "rb").read().partition(b"end_header\n")
    assert head == (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                    b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                    b"element face 2\nproperty list uchar int vertex_indices\n")
    assert len(body) == 4 * 27 + 2 * 13
    cloud = open(ply + ".cloud", "rb").read().partition(b"end_header\n")[2]
    assert body[:4 * 27] == cloud and len(cloud) == 4 * 27  # the vertex block of WritePLY, byte for byte
    rec = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    pts = np.frombuffer(body[:4 * 27], rec)
    np.testing.assert_array_equal(pts["p"], np.array([[1, 2, 3], [-0.5, 0.25, 8], [4, 5, 6], [7, 8, 9]], np.float32))
    np.testing.assert_array_equal(pts["n"], np.array([[0, 0, -1], [0.6, 0, -0.8], [0, 0, 0], [0, 1, 0]], np.float32))  # a NaN normal is 0 0 0
    np.testing.assert_array_equal(pts["rgb"], [[30, 20, 10], [128, 0, 255], [7, 8, 9], [3, 2, 1]])
    faces = np.frombuffer(body[4 * 27:], np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    assert faces.dtype.itemsize == 13 and faces["n"].tolist() == [3, 3] and faces["v"].tolist() == [[0, 2, 3], [0, 3, 0x01020304]]


def test_mesh_writer_under_sanitizers(tmp_path):
    exe, r = _build_io_check(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0:
        pytest.skip("the C++ compiler has no AddressSanitizer / UBSan runtime: " + r.stderr.strip().splitlines()[-1][:120])
    _run_io_check(exe, tmp_path)
