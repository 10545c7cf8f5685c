"""Triangle meshes on the GPU (include/cspm.h "triangle meshes") held to tests/mesh_ref.py bit for bit (any NaN
equals any NaN): cspm_mesh_host over the wave, workgroup and scan seams, keep patterns, capacities, both views, every optional input and
output; cspm_mesh / cspm_mesh_device on the stored field after a PatchMatch run (RAW, PP, fit); the error returns, the timing counts, the
host layer and cspm_main --l_mesh_ply."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fit_ref
import geom_ref as gr
import mesh_ref as mr
from crossscalepatchmatch_amd import capi
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL = (300.0, 31.5, 20.25, 0.25, 3.5)
SHAPES = [(1, 1), (1, 9), (9, 1),              # no quads
          (2, 2), (7, 5),                      # small quads
          (63, 3), (64, 2), (65, 2),           # a quad whose right neighbour lies in the next wave
          (255, 2), (256, 2), (257, 3),        # the workgroup border, and a row below that lies in another workgroup
          (130, 67),                           # a general odd shape
          (512, 512),                          # exactly one pass of the scan's workgroup (1024 workgroups of 256 pixels)
          (512, 513)]                          # two passes


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the device-variant test needs torch tensors, and
    the host-entry tests of this module would otherwise load the library first"""
    yield


def _maps(w, h, seed, holes=True):
    """a gently slanted surface (every pixel passes a moderate min_cos) with a rough half: some edges hold and some do not"""
    rng = np.random.default_rng(seed)
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    a0, b0 = 0.03125, -0.015625
    D = a0 * (x % 64) + b0 * (y % 64) + 12.0
    A, Bs = np.full((h, w), a0), np.full((h, w), b0)
    rough = rng.uniform(size=(h, w)) < 0.4
    D = np.where(rough, D + rng.uniform(-0.7, 0.7, (h, w)), D)
    A = np.where(rough, A + rng.uniform(-0.4, 0.4, (h, w)), A)
    Bs = np.where(rough, Bs + rng.uniform(-0.4, 0.4, (h, w)), Bs)
    V = None
    if holes:
        D[rng.uniform(size=(h, w)) < 0.03] = np.nan
        D[rng.uniform(size=(h, w)) < 0.01] = np.inf
        D[rng.uniform(size=(h, w)) < 0.01] = -CAL[4]
        D[rng.uniform(size=(h, w)) < 0.01] = -30.0
        V = (rng.uniform(size=(h, w)) > 0.08).astype(np.uint8)
        A[rng.uniform(size=(h, w)) < 0.03] = np.nan
        Bs[rng.uniform(size=(h, w)) < 0.03] = np.inf
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return D, V, A, Bs, img


def _check(cal, v, D, V=None, A=None, Bs=None, img=None, what="", **kw):
    got = capi.mesh_host(cal, v, D, V, A, Bs, img, **kw)
    want = mr.mesh(cal, v, D, V, A, Bs, img, **kw)
    msg = mr.same_mesh(got, want, f"{what} {D.shape[1]}x{D.shape[0]} view {v} {kw}")
    assert msg is None, msg
    return got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_shapes(shape):
    w, h = shape
    D, V, A, Bs, img = _maps(w, h, 70 + w + h)
    got, _ = _check(CAL, 0, D, V, A, Bs, img, max_diff=0.5, min_cos=0.1, z_near=2.0, z_far=40.0)
    if w == 1 or h == 1:
        assert got["n_faces"] == 0 and got["n_vertices"] == 0
    elif w * h >= 64:
        assert 0 < got["n_faces"] < 2 * (w - 1) * (h - 1) and 0 < got["n_vertices"] < w * h
    _check(CAL, 1, D, None, A, Bs, None, max_diff=math.inf, all_vertices=1, left_frame=1)
    _check(CAL, 0, D, V, None, None, img, max_diff=0.0)


def _pattern(name, w, h):
    n = w * h
    k = np.zeros(n, bool)
    if name == "all":
        k[:] = True
    elif name == "alternate":
        k[::2] = True
    elif name == "checkerboard":
        k = ((np.arange(w)[None, :] + np.arange(h)[:, None]) % 2 == 0).ravel()
    elif name == "last":
        k[-1] = True
    elif name == "empty_waves":  # whole waves and a whole workgroup without a kept pixel
        k[:] = True
        k[64:128] = False
        k[256:512] = False
        k[n - 70:n - 6] = False
    elif name == "random":
        k[:] = np.random.default_rng(1).uniform(size=n) > 0.3
    return k.reshape(h, w)


@pytest.mark.parametrize("name", ["all", "none", "alternate", "checkerboard", "last", "empty_waves", "random"])
@pytest.mark.parametrize("all_vertices", [0, 1])
def test_keep_patterns(name, all_vertices):
    w, h = 130, 67
    D, _, A, Bs, img = _maps(w, h, 3, holes=False)
    V = _pattern(name, w, h).astype(np.uint8)
    nq = 2 * (w - 1) * (h - 1)
    out = {"vertex_buffer": np.frombuffer(bytes([0xA5]) * (32 * w * h), capi.Point).copy(),
           "face_buffer": np.frombuffer(bytes([0xA5]) * (12 * nq), capi.Face).copy(), "quad": np.full((h, w), 0xA5, np.uint8)}
    got = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=math.inf, all_vertices=all_vertices, out=out)
    want = mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=math.inf, all_vertices=all_vertices)
    msg = mr.same_mesh(got, want, name)
    assert msg is None, msg
    assert np.all(out["vertex_buffer"][got["n_vertices"]:].view(np.uint8) == 0xA5), "vertex records behind the count were written"
    assert np.all(out["face_buffer"][got["n_faces"]:].view(np.uint8) == 0xA5), "face records behind the count were written"
    if all_vertices:
        assert got["n_vertices"] == V.sum()
    if name == "all":
        assert got["n_faces"] == nq and got["n_vertices"] == w * h
    if name in ("none", "alternate", "checkerboard", "last"):  # checkerboard: every quad has one kept diagonal, none a third kept corner
        assert got["n_faces"] == 0 and len(got["faces"]) == 0 and (all_vertices or got["n_vertices"] == 0)
        assert not (got["quad"] & 3).any()
    if name == "checkerboard":  # ... so the split bit is all that is left: anti where p10 and p01 are the kept pair
        assert np.array_equal(got["quad"][:-1, :-1] == 4, V[:-1, 1:] != 0)
    if name in ("empty_waves", "random"):
        assert 0 < got["n_faces"] < nq


def test_capacities_and_counts_only():
    w, h = 130, 67
    D, V, A, Bs, img = _maps(w, h, 5)
    full = mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=0.5)
    nv, nf = full["n_vertices"], full["n_faces"]
    assert 1000 < nv < w * h and 1000 < nf
    for vcap, fcap in ((0, 0), (1, 1), (63, 64), (257, 255), (nv - 1, nf - 1), (nv, nf), (nv + 1, nf + 1), (nv - 1, nf + 1), (w * h + 100, 2 * w * h + 100)):
        out = {"vertex_buffer": np.frombuffer(bytes([0x5A]) * (32 * max(vcap, 1)), capi.Point).copy(),
               "face_buffer": np.frombuffer(bytes([0x5A]) * (12 * max(fcap, 1)), capi.Face).copy()}
        got = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=0.5, vertex_cap=vcap, face_cap=fcap, quad=False, out=out)
        assert (got["n_vertices"], got["n_faces"]) == (nv, nf), (vcap, fcap)
        assert gr.same_cloud(got["vertices"], full["vertices"][:vcap]) and np.array_equal(got["faces"]["v"], full["faces"]["v"][:fcap]), (vcap, fcap)
        assert np.all(out["vertex_buffer"][min(vcap, nv):].view(np.uint8) == 0x5A) and np.all(out["face_buffer"][min(fcap, nf):].view(np.uint8) == 0x5A)
    only = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=0.5, vertices=False, faces=False, quad=False)  # NULL buffers ask for the counts only
    assert (only["n_vertices"], only["n_faces"]) == (nv, nf) and "vertices" not in only and "faces" not in only
    faces_only = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=0.5, vertices=False, quad=False)  # the faces still carry full vertex numbers
    assert np.array_equal(faces_only["faces"]["v"], full["faces"]["v"])
    blind = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=0.5, counts=False)  # no count pointers
    assert gr.same_cloud(blind["vertices"][:nv], full["vertices"]) and np.array_equal(blind["faces"]["v"][:nf], full["faces"]["v"])


def test_outputs_not_requested_stay_untouched():
    w, h = 65, 9
    D, V, A, Bs, img = _maps(w, h, 23)
    want = mr.mesh(CAL, 0, D, V, A, Bs, img, max_diff=0.5)
    for pick in ("vertices", "faces", "quad", None):
        out = {"vertex_buffer": np.frombuffer(bytes([0x77]) * (32 * w * h), capi.Point).copy(),
               "face_buffer": np.frombuffer(bytes([0x77]) * (12 * 2 * w * h), capi.Face).copy(), "quad": np.full((h, w), 0x77, np.uint8)}
        got = capi.mesh_host(CAL, 0, D, V, A, Bs, img, max_diff=0.5, vertices=pick == "vertices", faces=pick == "faces", quad=pick == "quad", out=dict(out))
        assert (got["n_vertices"], got["n_faces"]) == (want["n_vertices"], want["n_faces"])
        for name, buf in (("vertices", "vertex_buffer"), ("faces", "face_buffer"), ("quad", "quad")):
            if name == pick:
                msg = mr.same_mesh({name: got[name]}, want, name)
                assert msg is None, msg
            else:
                assert np.all(out[buf].view(np.uint8) == 0x77), f"{name} was written although only {pick} was asked for"


@pytest.mark.parametrize("v,lf", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_views_and_optional_inputs(v, lf):
    w, h = 67, 11
    D, V, A, Bs, img = _maps(w, h, 17)
    for tau in (0.0, 0.5, 2.0, math.inf):
        _check(CAL, v, D, V, A, Bs, img, max_diff=tau, left_frame=lf)
    _check(CAL, v, D, V, None, None, img, max_diff=1.0, left_frame=lf, min_cos=0.9)  # no slopes: the plain difference test, NaN normals
    _check(CAL, v, D, None, A, Bs, None, max_diff=1.0, left_frame=lf)                 # no mask, no image: four zero bytes
    _check(CAL, v, D, V, A, Bs, img, max_diff=1.0, left_frame=lf, min_cos=0.6, all_vertices=1)
    _check((3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4), v, D, V, A, Bs, img, max_diff=1.0, left_frame=lf)


# ---- the context entries ---------------------------------------------------------------------------------------------------------------

def _run(ctx, pair, sn=3):
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 9, sn, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(2, seed=5)
    return [ctx.level_image(v, 0) for v in (0, 1)]


def _ctx_same(got, want, what):
    msg = mr.same_mesh(got, want, what)
    assert msg is None, msg


@pytest.mark.parametrize("fixture", ["small_pair", "odd_pair"])
def test_context_raw_pp_and_fit(gpu_ctx, request, fixture):
    pair = request.getfixturevalue(fixture)
    ctx = gpu_ctx
    imgs = _run(ctx, pair)
    kw = dict(min_cos=0.3, z_far=12.0)
    mk = dict(max_diff=2.0)
    fitp = dict(radius=2, max_diff=1.5, min_support=6, use_guide=1)
    try:
        for v in (0, 1):
            planes = ctx.get_planes(v)[0]
            A, Bs = planes[..., 3], planes[..., 4]
            D = ctx.disparity_f64(v)
            first = ctx.mesh(v, CAL, capi.GEOM_RAW, left_frame=v, **mk, **kw)
            print(f"{fixture} RAW view {v}: {first['n_vertices']} vertices, {first['n_faces']} faces")
            assert first["n_faces"] > 0
            _ctx_same(first, mr.mesh(CAL, v, D, None, A, Bs, imgs[v], left_frame=v, **mk, **kw), f"RAW view {v}")
            _ctx_same(ctx.mesh(v, CAL, capi.GEOM_RAW, left_frame=v, **mk, **kw), first, "a second call")
            fitted = fit_ref.fit(D, None, imgs[v], pair["max_dis"], **fitp)[0]
            _ctx_same(ctx.mesh(v, CAL, capi.GEOM_RAW, fit=fitp, **mk, **kw), mr.mesh(CAL, v, D, None, fitted[..., 3], fitted[..., 4], imgs[v], **mk, **kw),
                      f"RAW + fit view {v}")
        for speckle, median in ((0, 0), (12, 1)):
            ctx.set_pp_speckle(speckle, 1.0)
            ctx.set_pp_median(median)
            maps = ctx.postprocess_f64(valid=True)
            for v in (0, 1):
                planes = ctx.get_planes(v)[0]
                Dp, Vp = maps[v], maps[2 + v]
                assert 0 < Vp.sum() < Vp.size
                A = np.where(Vp != 0, planes[..., 3], np.nan)
                Bs = np.where(Vp != 0, planes[..., 4], np.nan)
                _ctx_same(ctx.mesh(v, CAL, capi.GEOM_PP, **mk, **kw), mr.mesh(CAL, v, Dp, None, A, Bs, imgs[v], **mk, **kw), f"PP view {v} {speckle} {median}")
                _ctx_same(ctx.mesh(v, CAL, capi.GEOM_PP, consistent_only=1, **mk, **kw), mr.mesh(CAL, v, Dp, Vp, A, Bs, imgs[v], **mk, **kw),
                          f"PP consistent_only view {v} {speckle} {median}")
                fitted = fit_ref.fit(Dp, Vp, imgs[v], pair["max_dis"], **fitp)[0]
                _ctx_same(ctx.mesh(v, CAL, capi.GEOM_PP, fit=fitp, consistent_only=1, **mk, **kw),
                          mr.mesh(CAL, v, Dp, Vp, fitted[..., 3], fitted[..., 4], imgs[v], **mk, **kw), f"PP + fit view {v} {speckle} {median}")
    finally:
        ctx.set_pp_speckle(0)
        ctx.set_pp_median(0)


def test_all_vertices_are_the_reprojection_cloud(gpu_ctx, odd_pair):
    ctx = gpu_ctx
    _run(ctx, odd_pair)
    for v in (0, 1):
        for source in (capi.GEOM_RAW, capi.GEOM_PP):
            cloud = ctx.reproject(v, CAL, source, dense=False, min_cos=0.5, left_frame=1)
            m = ctx.mesh(v, CAL, source, all_vertices=1, min_cos=0.5, left_frame=1)
            assert m["n_vertices"] == cloud["count"] > 0 and gr.same_cloud(m["vertices"], cloud["cloud"])


def test_device_variant_equals_host_variant(gpu_ctx, odd_pair):
    import torch
    ctx = gpu_ctx
    _run(ctx, odd_pair)
    w, h = odd_pair["w"], odd_pair["h"]
    n, nq = w * h, 2 * (w - 1) * (h - 1)
    kw = dict(min_cos=0.4, left_frame=1, max_diff=0.75)
    for source, fit in ((capi.GEOM_RAW, None), (capi.GEOM_PP, None), (capi.GEOM_RAW, dict(radius=2))):
        want = ctx.mesh(1, CAL, source, fit=fit, **kw)
        verts = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        faces = torch.zeros((nq, 3), dtype=torch.int32, device="cuda")
        quad = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.mesh_device(1, CAL, source, fit=fit, d_vertices=verts.data_ptr(), vertex_cap=n, d_faces=faces.data_ptr(), face_cap=nq, d_quad=quad.data_ptr(),
                        d_n_vertices=counts.data_ptr(), d_n_faces=counts.data_ptr() + 4, **kw)
        ctx.synchronize()
        nv, nf = (int(t) for t in counts.cpu().numpy())
        got = dict(n_vertices=nv, n_faces=nf, quad=quad.cpu().numpy(), vertices=verts.cpu().numpy().view(capi.Point).reshape(-1)[:nv],
                   faces=np.ascontiguousarray(faces.cpu().numpy()).view(np.uint32).view(capi.Face).reshape(-1)[:nf])
        _ctx_same(got, want, f"device variant, source {source}, fit {fit}")
        counts.zero_()
        torch.cuda.synchronize()
        ctx.mesh_device(1, CAL, source, fit=fit, d_n_vertices=counts.data_ptr(), d_n_faces=counts.data_ptr() + 4, **kw)  # the counts alone
        ctx.synchronize()
        assert [int(t) for t in counts.cpu().numpy()] == [want["n_vertices"], want["n_faces"]]


def test_timing_counts_and_scratch(gpu_ctx, small_pair):
    ctx = gpu_ctx
    _run(ctx, small_pair)
    n = small_pair["w"] * small_pair["h"]
    ctx.synchronize()
    ctx.enable_timing(True)
    try:
        ctx.reset_timing()
        ctx.mesh(0, CAL, capi.GEOM_RAW)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 0 and t["init"]["launches"] == 0
        ctx.mesh(1, CAL, capi.GEOM_RAW, fit={}, vertices=False, faces=False, quad=False)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (2, 2 * n)
        ctx.reset_timing()
        ctx.mesh(0, CAL, capi.GEOM_PP)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 1
    finally:
        ctx.enable_timing(False)


def test_error_returns(small_pair):
    ERR_ARG, ERR_STATE = -1, -3
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    k, g, m = capi.calib_struct(CAL), capi.geom_params(), capi.mesh_params()
    nv, nf = C.c_uint(0), C.c_uint(0)

    def rc(view=0, source=capi.GEOM_RAW, cal=k, params=g, fit=None, mesh=m, device=False):
        fn = L.cspm_mesh_device if device else L.cspm_mesh
        ref = lambda s: C.byref(s) if s is not None else None
        return fn(ctx.p, view, source, ref(cal), ref(params), ref(fit), ref(mesh), None, 0, None, 0, None, None if device else C.byref(nv),
                  None if device else C.byref(nf))

    try:
        for dev in (False, True):
            assert rc(device=dev) == ERR_STATE                                  # no images
            assert rc(mesh=capi.mesh_params(max_diff=-1.0), device=dev) == ERR_ARG  # arguments before the state
        ctx.set_images(small_pair["l"], small_pair["r"])
        for dev in (False, True):
            assert rc(device=dev) == ERR_STATE                                  # no plane field
        w, h = small_pair["w"], small_pair["h"]
        ctx.set_planes(0, capi.disparity_planes(np.full((h, w), 4.0)), np.zeros((h, w)))
        ctx.set_planes(1, capi.disparity_planes(np.full((h, w), 4.0)), np.zeros((h, w)))
        for dev in (False, True):
            assert rc(device=dev) == 0                                          # RAW needs no cost object
            assert rc(source=capi.GEOM_PP, device=dev) == ERR_STATE             # PP does
            assert rc(fit=capi.fit_params(), device=dev) == ERR_STATE           # and so does a fit (max_dis)
            assert rc(view=2, device=dev) == ERR_ARG and rc(view=-1, device=dev) == ERR_ARG
            assert rc(source=2, device=dev) == ERR_ARG and rc(source=-1, device=dev) == ERR_ARG
            assert rc(cal=None, device=dev) == ERR_ARG
            assert rc(cal=capi.Calib(0.0, 1, 1, 1, 0), device=dev) == ERR_ARG
            assert rc(params=capi.geom_params(min_cos=1.25), device=dev) == ERR_ARG
            assert rc(mesh=capi.mesh_params(max_diff=math.nan), device=dev) == ERR_ARG
            assert rc(mesh=capi.mesh_params(max_diff=-0.5), device=dev) == ERR_ARG
            assert rc(mesh=capi.mesh_params(max_diff=math.inf), device=dev) == 0
            assert rc(params=None, mesh=None, device=dev) == 0                  # NULL parameters are the defaults
        assert (nv.value, nf.value) == (w * h, 2 * (w - 1) * (h - 1))           # a fronto-parallel field: the whole grid
        ctx.build_cost_grd(small_pair["max_dis"], 9, 0, 0.0)
        for dev in (False, True):
            assert rc(fit=capi.fit_params(radius=0), device=dev) == ERR_ARG
            assert rc(fit=capi.fit_params(), device=dev) == 0
            assert rc(source=capi.GEOM_PP, device=dev) == 0
        dev_rc = lambda verts, faces: L.cspm_mesh_device(ctx.p, 0, 0, C.byref(k), None, None, None, verts, 4, faces, 4, None, None, None)
        assert dev_rc(C.c_void_p(8), None) == ERR_ARG and dev_rc(None, C.c_void_p(2)) == ERR_ARG  # alignment
        ctx.synchronize()
    finally:
        ctx.close()


# ---- the host layer and the command line -----------------------------------------------------------------------------------------------

def test_host_layer_mesh():
    exe = _build_helper("mesh_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mesh_check ok" in r.stdout, r.stdout + r.stderr


def test_cli_mesh_ply(tmp_path):
    """cspm_main --calib --l_mesh_ply --r_mesh_ply on the Motorcycle half-size crop == the C-ABI sequence; the flag conflicts are refused
    before a device is opened"""
    from crossscalepatchmatch_amd import realdata
    cfg, l, r, _ = realdata.load_crop()
    lf, rf, _ = realdata.crop_files()
    h, w = l.shape[:2]
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[3979.911 0 1244.772; 0 3979.911 1019.507; 0 0 1]\ncam1=[3979.911 0 1369.115; 0 3979.911 1019.507; 0 0 1]\n"
                     f"doffs=124.343\nbaseline=193.001\nwidth={2 * w}\nheight={2 * h}\nndisp=270\n")
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    lply, rply = tmp_path / "l_mesh.ply", tmp_path / "r_mesh.ply"
    D, iters, seed = cfg["max_dis"], 1, 3
    base = [main, f"--l_img_file={lf}", f"--r_img_file={rf}", f"--l_dis_file={tmp_path / 'l.png'}", f"--r_dis_file={tmp_path / 'r.png'}", f"--max_dis={D}",
            "--dis_scale=8", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", f"--iters={iters}", f"--seed={seed}", "--quiet=true"]
    mesh = [f"--l_mesh_ply={lply}", f"--r_mesh_ply={rply}", "--mesh_max_diff=0.5", "--geom_min_cos=0.3", "--geom_z_far=5500", "--geom_left_frame=true"]
    for bad in (mesh, mesh + [f"--calib={calib}", f"--batch_list={calib}"], mesh + [f"--calib={calib}", "--mesh_max_diff=-1"]):
        res = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "Error" in res.stdout, res.stdout
    res = subprocess.run(base + mesh + [f"--calib={calib}"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    ctx = capi.StereoContext(0)
    try:
        ctx.set_images(l, r)
        ctx.build_cost_grd(D, 35, 5, 0.3)
        ctx.patchmatch(iters, seed=seed)
        cal = (3979.911 * 0.5, 1244.772 * 0.5, 1019.507 * 0.5, 193.001, 124.343 * 0.5)
        want = [ctx.mesh(v, cal, capi.GEOM_RAW, max_diff=0.5, min_cos=0.3, z_far=5500.0, left_frame=1) for v in (0, 1)]
    finally:
        ctx.close()
    rec = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    for path, res in ((lply, want[0]), (rply, want[1])):
        head, _, body = open(path, "rb").read().partition(b"end_header\n")
        nv, nf = res["n_vertices"], res["n_faces"]
        assert f"element vertex {nv}\n".encode() in head and f"element face {nf}\n".encode() in head
        assert len(body) == 27 * nv + 13 * nf and 1000 < nv < w * h and 1000 < nf
        pts, cl = np.frombuffer(body[:27 * nv], rec), res["vertices"]
        assert gr.same_bits(pts["p"], np.stack([cl["x"], cl["y"], cl["z"]], 1))
        nrm = np.stack([cl["nx"], cl["ny"], cl["nz"]], 1)
        nrm[np.isnan(nrm).any(1)] = 0.0
        assert gr.same_bits(pts["n"], nrm)
        np.testing.assert_array_equal(pts["rgb"], np.stack([cl["r"], cl["g"], cl["b"]], 1))
        faces = np.frombuffer(body[27 * nv:], np.dtype([("n", "u1"), ("v", "<i4", 3)]))
        assert np.all(faces["n"] == 3) and np.array_equal(faces["v"].astype(np.uint32), res["faces"]["v"])
