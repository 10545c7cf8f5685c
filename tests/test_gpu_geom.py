"""Reprojection on the GPU (include/cspm.h "reprojection") held to tests/geom_ref.py bit for bit (NaN positions
included, any NaN payload): cspm_reproject_host over the wave, workgroup and scan seams, keep patterns, capacities, both views, every
optional input and output; cspm_reproject / cspm_reproject_device on the stored field after a PatchMatch run (RAW, PP, fit); the error
returns, the timing counts, the host layer and cspm_main --calib."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fit_ref
import geom_ref as gr
from crossscalepatchmatch_amd import capi
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAL = (300.0, 31.5, 20.25, 0.25, 3.5)
BLOCK, SCAN = 256, 1024  # kGeomBlock, kGeomScanBlock (csrc/cspm_geom.h): one scan pass covers SCAN workgroups of BLOCK pixels
SHAPES = [(1, 1), (7, 5), (63, 3), (64, 4), (65, 5), (255, 1), (256, 1), (257, 1), (130, 67),
          (512, BLOCK * SCAN // 512),       # exactly one pass of the scan's workgroup
          (512, BLOCK * SCAN // 512 + 1)]   # a second pass with a carry
DENSE = ("depth", "xyz", "normal", "keep")


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the device-variant test needs torch tensors, and
    the host-entry tests of this module would otherwise load the library first"""
    yield


def _maps(w, h, seed, holes=True):
    rng = np.random.default_rng(seed)
    D = rng.uniform(1.0, 40.0, (h, w))
    V = None
    if holes:
        D[rng.uniform(size=(h, w)) < 0.04] = np.nan
        D[rng.uniform(size=(h, w)) < 0.02] = np.inf
        D[rng.uniform(size=(h, w)) < 0.02] = -CAL[4]
        D[rng.uniform(size=(h, w)) < 0.02] = -30.0
        V = (rng.uniform(size=(h, w)) > 0.15).astype(np.uint8)
    A = rng.uniform(-0.05, 0.05, (h, w))
    Bs = rng.uniform(-0.05, 0.05, (h, w))
    if holes:
        A[rng.uniform(size=(h, w)) < 0.03] = np.nan
        Bs[rng.uniform(size=(h, w)) < 0.03] = np.inf
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return D, V, A, Bs, img


def _same(got, want, what):
    for name in DENSE:
        if want.get(name) is None:
            assert name not in got, f"{what}: {name} without slopes"
            continue
        assert gr.same_bits(got[name], want[name]), f"{what}: {name} differs in {np.sum(got[name] != want[name])} places"
    assert got["count"] == want["count"], f"{what}: count {got['count']} != {want['count']}"
    assert gr.same_cloud(got["cloud"], want["cloud"]), f"{what}: cloud"


def _check(cal, v, D, V=None, A=None, Bs=None, img=None, cap=None, what="", **params):
    got = capi.reproject_host(cal, v, D, V, A, Bs, img, cloud_cap=cap, **params)
    want = gr.reproject(cal, v, D, V, A, Bs, img, cap=cap, **params)
    _same(got, want, f"{what} {D.shape[1]}x{D.shape[0]} view {v} {params}")
    return got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_shapes(shape):
    w, h = shape
    D, V, A, Bs, img = _maps(w, h, 40 + w + h)
    got, _ = _check(CAL, 0, D, V, A, Bs, img, min_cos=0.6, z_near=2.0, z_far=40.0)
    assert w * h < 64 or 0 < got["count"] < w * h
    _check(CAL, 1, D, None, A, Bs, None, left_frame=1)


def _pattern(name, w, h):
    n = w * h
    k = np.zeros(n, bool)
    if name == "all":
        k[:] = True
    elif name == "alternate":
        k[::2] = True
    elif name == "last":
        k[-1] = True
    elif name == "empty_waves":  # whole waves and a whole workgroup without a kept pixel
        k[:] = True
        k[64:128] = False
        k[256:512] = False
        k[n - 70:n - 6] = False
    elif name == "halves":
        k[:] = np.random.default_rng(1).uniform(size=n) > 0.5
    return k.reshape(h, w)


@pytest.mark.parametrize("name", ["all", "none", "alternate", "last", "empty_waves", "halves"])
def test_keep_patterns(name):
    w, h = 130, 67
    D, _, A, Bs, img = _maps(w, h, 3, holes=False)
    V = _pattern(name, w, h).astype(np.uint8)
    poison = np.frombuffer(bytes([0xA5]) * (32 * w * h), capi.Point).copy()
    got = capi.reproject_host(CAL, 0, D, V, A, Bs, img, out={"cloud_buffer": poison})
    want = gr.reproject(CAL, 0, D, V, A, Bs, img)
    _same(got, want, name)
    assert got["count"] == V.sum()
    assert np.all(poison[got["count"]:].view(np.uint8) == 0xA5), "records behind the count were written"
    if name == "none":
        assert got["count"] == 0 and len(got["cloud"]) == 0


def test_capacity_and_count_only():
    w, h = 130, 67
    D, V, A, Bs, img = _maps(w, h, 5)
    count = gr.reproject(CAL, 0, D, V, A, Bs, img)["count"]
    assert 1000 < count < w * h
    for cap in (0, 1, 63, 64, 257, count - 1, count, count + 1, w * h, w * h + 100):
        poison = np.frombuffer(bytes([0x5A]) * (32 * max(cap, 1)), capi.Point).copy()
        got = capi.reproject_host(CAL, 0, D, V, A, Bs, img, cloud_cap=cap, out={"cloud_buffer": poison}, dense=())
        want = gr.reproject(CAL, 0, D, V, A, Bs, img, cap=cap)
        assert got["count"] == count and gr.same_cloud(got["cloud"], want["cloud"]), cap
        assert np.all(poison[min(cap, count):].view(np.uint8) == 0x5A), cap
    only = capi.reproject_host(CAL, 0, D, V, A, Bs, img, cloud=False, dense=())  # a NULL cloud asks for the count only
    assert only["count"] == count and "cloud" not in only
    nothing = capi.reproject_host(CAL, 0, D, V, A, Bs, img, cloud=False, count=False, dense=("depth",))  # no scan, no cloud pass
    assert gr.same_bits(nothing["depth"], gr.reproject(CAL, 0, D, V)["depth"]) and "count" not in nothing


@pytest.mark.parametrize("v,lf", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_views_optional_inputs_and_ranges(v, lf):
    w, h = 67, 11
    D, V, A, Bs, img = _maps(w, h, 17)
    _check(CAL, v, D, V, A, Bs, img, left_frame=lf)
    _check(CAL, v, D, V, None, None, img, left_frame=lf, min_cos=0.9)       # no slopes: min_cos does not apply, NaN normals in the cloud
    _check(CAL, v, D, None, A, Bs, None, left_frame=lf)                      # no mask, no image: four zero bytes
    _check(CAL, v, D, V, A, Bs, img, left_frame=lf, min_cos=1.0)
    _check(CAL, v, D, V, A, Bs, img, left_frame=lf, min_cos=0.97)
    Z = gr.reproject(CAL, v, D)["depth"]
    zs = np.sort(Z[np.isfinite(Z)])
    _check(CAL, v, D, V, A, Bs, img, left_frame=lf, z_near=float(zs[len(zs) // 4]), z_far=float(zs[3 * len(zs) // 4]))  # borders hit exactly
    _check(CAL, v, D, V, A, Bs, img, left_frame=lf, z_near=float(zs[5]), z_far=float(zs[5]))
    _check((3979.911 / 4, 1244.772 / 4, 1019.507 / 4, 193.001, 124.343 / 4), v, D, V, A, Bs, img, left_frame=lf)          # Middlebury-like numbers


def test_outputs_not_requested_stay_untouched():
    w, h = 65, 9
    D, V, A, Bs, img = _maps(w, h, 23)
    want = gr.reproject(CAL, 0, D, V, A, Bs, img)
    for pick in DENSE + ((),):
        names = (pick,) if pick else ()
        out = {"depth": np.full((h, w), 7.5), "xyz": np.full((3, h, w), 7.5), "normal": np.full((3, h, w), 7.5), "keep": np.full((h, w), 77, np.uint8)}
        got = capi.reproject_host(CAL, 0, D, V, A, Bs, img, dense=names, out=out)
        for name in DENSE:
            if name in names:
                assert gr.same_bits(got[name], want[name]), name
            else:
                assert np.all(out[name] == (77 if name == "keep" else 7.5)), f"{name} was written although only {names} was asked for"
        assert got["count"] == want["count"] and gr.same_cloud(got["cloud"], want["cloud"])


# ---- the context entries ---------------------------------------------------------------------------------------------------------------

def _run(ctx, pair, sn=3):
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 9, sn, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(2, seed=5)
    return [ctx.level_image(v, 0) for v in (0, 1)]


def _ctx_same(got, want, what):
    for name in DENSE:
        assert gr.same_bits(got[name], want[name]), f"{what}: {name}"
    assert got["count"] == want["count"] and gr.same_cloud(got["cloud"], want["cloud"]), what


@pytest.mark.parametrize("fixture", ["small_pair", "odd_pair"])
def test_context_raw_pp_and_fit(gpu_ctx, request, fixture):
    pair = request.getfixturevalue(fixture)
    ctx = gpu_ctx
    imgs = _run(ctx, pair)
    kw = dict(min_cos=0.5, z_far=5.0)
    fitp = dict(radius=2, max_diff=1.5, min_support=6, use_guide=1)
    try:
        for v in (0, 1):
            planes = ctx.get_planes(v)[0]
            A, Bs = planes[..., 3], planes[..., 4]
            D = ctx.disparity_f64(v)
            first = ctx.reproject(v, CAL, capi.GEOM_RAW, left_frame=v, **kw)
            _ctx_same(first, gr.reproject(CAL, v, D, None, A, Bs, imgs[v], left_frame=v, **kw), f"RAW view {v}")
            _ctx_same(ctx.reproject(v, CAL, capi.GEOM_RAW, left_frame=v, **kw), first, "a second call")
            fitted = fit_ref.fit(D, None, imgs[v], pair["max_dis"], **fitp)[0]
            _ctx_same(ctx.reproject(v, CAL, capi.GEOM_RAW, fit=fitp, **kw), gr.reproject(CAL, v, D, None, fitted[..., 3], fitted[..., 4], imgs[v], **kw),
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
                _ctx_same(ctx.reproject(v, CAL, capi.GEOM_PP, **kw), gr.reproject(CAL, v, Dp, None, A, Bs, imgs[v], **kw), f"PP view {v} {speckle} {median}")
                _ctx_same(ctx.reproject(v, CAL, capi.GEOM_PP, consistent_only=1, **kw), gr.reproject(CAL, v, Dp, Vp, A, Bs, imgs[v], **kw),
                          f"PP consistent_only view {v} {speckle} {median}")
                fitted = fit_ref.fit(Dp, Vp, imgs[v], pair["max_dis"], **fitp)[0]
                _ctx_same(ctx.reproject(v, CAL, capi.GEOM_PP, fit=fitp, consistent_only=1, **kw),
                          gr.reproject(CAL, v, Dp, Vp, fitted[..., 3], fitted[..., 4], imgs[v], **kw), f"PP + fit view {v} {speckle} {median}")
    finally:
        ctx.set_pp_speckle(0)
        ctx.set_pp_median(0)


def test_device_variant_equals_host_variant(gpu_ctx, odd_pair):
    import torch
    ctx = gpu_ctx
    _run(ctx, odd_pair)
    w, h = odd_pair["w"], odd_pair["h"]
    n = w * h
    kw = dict(min_cos=0.4, left_frame=1)
    for source, fit in ((capi.GEOM_RAW, None), (capi.GEOM_PP, None), (capi.GEOM_RAW, dict(radius=2))):
        want = ctx.reproject(1, CAL, source, fit=fit, **kw)
        depth = torch.full((h, w), 7.0, dtype=torch.float64, device="cuda")
        xyz = torch.full((3, h, w), 7.0, dtype=torch.float64, device="cuda")
        normal = torch.full((3, h, w), 7.0, dtype=torch.float64, device="cuda")
        keep = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
        cloud = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.reproject_device(1, CAL, source, fit=fit, d_depth=depth.data_ptr(), d_xyz=xyz.data_ptr(), d_normal=normal.data_ptr(), d_keep=keep.data_ptr(),
                             d_cloud=cloud.data_ptr(), cloud_cap=n, d_count=count.data_ptr(), **kw)
        ctx.synchronize()
        got = dict(depth=depth.cpu().numpy(), xyz=xyz.cpu().numpy(), normal=normal.cpu().numpy(), keep=keep.cpu().numpy(), count=int(count.item()))
        got["cloud"] = cloud.cpu().numpy().view(capi.Point).reshape(-1)[:got["count"]]
        _ctx_same(got, want, f"device variant, source {source}, fit {fit}")
        count.zero_()
        torch.cuda.synchronize()
        ctx.reproject_device(1, CAL, source, fit=fit, d_count=count.data_ptr(), **kw)  # the count alone
        ctx.synchronize()
        assert int(count.item()) == want["count"]


def test_timing_counts(gpu_ctx, small_pair):
    ctx = gpu_ctx
    _run(ctx, small_pair)
    n = small_pair["w"] * small_pair["h"]
    ctx.synchronize()
    ctx.enable_timing(True)
    try:
        ctx.reset_timing()
        ctx.reproject(0, CAL, capi.GEOM_RAW)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 0 and t["init"]["launches"] == 0
        ctx.reproject(1, CAL, capi.GEOM_RAW, fit={}, dense=False, cloud=False)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (2, 2 * n)
        ctx.reset_timing()
        ctx.reproject(0, CAL, capi.GEOM_PP)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 1
    finally:
        ctx.enable_timing(False)


def test_error_returns(small_pair):
    ERR_ARG, ERR_STATE = -1, -3
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    k, g = capi.calib_struct(CAL), capi.geom_params()
    cnt = C.c_uint(0)

    def rc(view=0, source=capi.GEOM_RAW, cal=k, params=g, fit=None, device=False):
        fn = L.cspm_reproject_device if device else L.cspm_reproject
        return fn(ctx.p, view, source, C.byref(cal) if cal is not None else None, C.byref(params) if params is not None else None,
                  C.byref(fit) if fit is not None else None, None, None, None, None, None, 0, None if device else C.byref(cnt))

    try:
        for dev in (False, True):
            assert rc(device=dev) == ERR_STATE                                  # no images
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
            assert rc(cal=capi.Calib(300.0, 1, 1, math.nan, 0), device=dev) == ERR_ARG
            assert rc(params=capi.geom_params(z_near=-1.0), device=dev) == ERR_ARG
            assert rc(params=capi.geom_params(z_near=3.0, z_far=2.0), device=dev) == ERR_ARG
            assert rc(params=capi.geom_params(min_cos=1.25), device=dev) == ERR_ARG
            assert rc(params=None, device=dev) == 0                             # NULL parameters are the defaults
        assert cnt.value == w * h
        ctx.build_cost_grd(small_pair["max_dis"], 9, 0, 0.0)
        for dev in (False, True):
            assert rc(fit=capi.fit_params(radius=0), device=dev) == ERR_ARG
            assert rc(fit=capi.fit_params(), device=dev) == 0
            assert rc(source=capi.GEOM_PP, device=dev) == 0
        assert L.cspm_reproject_device(ctx.p, 0, 0, C.byref(k), None, None, None, None, None, None, C.c_void_p(8), 4, None) == ERR_ARG  # alignment
        ctx.synchronize()
    finally:
        ctx.close()


# ---- the host layer and the command line -----------------------------------------------------------------------------------------------

def test_host_layer_reproject(tmp_path):
    exe = _build_helper("geom_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "geom_check ok" in r.stdout, r.stdout + r.stderr


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(t) for t in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_calib_ply_and_depth(tmp_path):
    """cspm_main --calib --l_ply --l_depth_pfm --r_ply on the Motorcycle half-size crop == the C-ABI sequence; the flag conflicts are
    refused before a device is opened"""
    from crossscalepatchmatch_amd import realdata
    cfg, l, r, _ = realdata.load_crop()
    lf, rf, _ = realdata.crop_files()
    h, w = l.shape[:2]
    calib = tmp_path / "calib.txt"
    # the dataset's Motorcycle numbers; width = 2 w makes the reader scale f, cx, cy and doffs by one half
    calib.write_text("cam0=[3979.911 0 1244.772; 0 3979.911 1019.507; 0 0 1]\ncam1=[3979.911 0 1369.115; 0 3979.911 1019.507; 0 0 1]\n"
                     f"doffs=124.343\nbaseline=193.001\nwidth={2 * w}\nheight={2 * h}\nndisp=270\n")
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    lply, rply, pfm = tmp_path / "l.ply", tmp_path / "r.ply", tmp_path / "l_depth.pfm"
    D, iters, seed = cfg["max_dis"], 1, 3
    base = [main, f"--l_img_file={lf}", f"--r_img_file={rf}", f"--l_dis_file={tmp_path / 'l.png'}", f"--r_dis_file={tmp_path / 'r.png'}", f"--max_dis={D}",
            "--dis_scale=8", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", f"--iters={iters}", f"--seed={seed}", "--quiet=true"]
    geom = [f"--l_ply={lply}", f"--r_ply={rply}", f"--l_depth_pfm={pfm}", "--geom_min_cos=0.3", "--geom_z_far=5500", "--geom_left_frame=true"]
    for bad in (geom, geom + [f"--calib={calib}", f"--batch_list={calib}"], geom + [f"--calib={calib}", "--geom_min_cos=2"]):
        res = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "Error" in res.stdout, res.stdout
    res = subprocess.run(base + geom + [f"--calib={calib}"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    ctx = capi.StereoContext(0)
    try:
        ctx.set_images(l, r)
        ctx.build_cost_grd(D, 35, 5, 0.3)
        ctx.patchmatch(iters, seed=seed)
        cal = (3979.911 * 0.5, 1244.772 * 0.5, 1019.507 * 0.5, 193.001, 124.343 * 0.5)
        want = [ctx.reproject(v, cal, capi.GEOM_RAW, min_cos=0.3, z_far=5500.0, left_frame=1) for v in (0, 1)]
    finally:
        ctx.close()
    assert gr.same_bits(_read_pfm(pfm), want[0]["depth"].astype(np.float32))
    rec = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    for path, res in ((lply, want[0]), (rply, want[1])):
        head, _, body = open(path, "rb").read().partition(b"end_header\n")
        assert f"element vertex {res['count']}\n".encode() in head
        pts, cl = np.frombuffer(body, rec), res["cloud"]
        assert len(pts) == len(cl) and 1000 < len(cl) < w * h
        assert gr.same_bits(pts["p"], np.stack([cl["x"], cl["y"], cl["z"]], 1))
        nrm = np.stack([cl["nx"], cl["ny"], cl["nz"]], 1)
        nrm[np.isnan(nrm).any(1)] = 0.0
        assert gr.same_bits(pts["n"], nrm)
        np.testing.assert_array_equal(pts["rgb"], np.stack([cl["r"], cl["g"], cl["b"]], 1))
