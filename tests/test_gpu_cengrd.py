"""-m gpu: the CENGRD matching cost (include/cspm.h) on the device against its CPU restatement
tests/cengrd_ref.py -- an oracle cost object whose volumes hold the cells G + KAPPA * min(H, TAU_CEN) -- bit for bit: the volumes,
max_cost and scale weights of cspm_build_cost_cengrd, cspm_cengrd_build_cv_host, cspm_plane_cost_batch, PatchMatch phase by phase and
as a whole, the 8-bit maps and both post-processings, a warm run, local stereo, the C++ host layer, the command line and streams
of pairs on one context.  tests/test_cengrd_ref.py checks the restatement itself, and that every pair used here exercises both
branches of the min, without a GPU.  Every comparison is assert_array_equal unless it says otherwise."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import cengrd_ref
import pngio
import pp_sub_ref
import warm_ref
from conftest import random_planes
from crossscalepatchmatch_amd import batch, capi
from oracle import pyoracle as po
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crossscalepatchmatch_amd")
DIS_SCALE = 4
RASTER, REDBLACK = po.SCHED_RASTER, po.SCHED_REDBLACK


@functools.lru_cache(maxsize=None)
def _pc(name, sn, lam):
    assert sn in cengrd_ref.SCALES[name], "add the level count to cengrd_ref.SCALES: tests/test_cengrd_ref.py checks the branch fractions for it"
    l, r = cengrd_ref.images(name)
    return cengrd_ref.plane_cost(l, r, cengrd_ref.PAIRS[name].D, 35, sn, lam)


def _build(ctx, name, sn, lam):
    l, r = cengrd_ref.images(name)
    ctx.set_images(l, r)
    ctx.build_cost_cengrd(cengrd_ref.PAIRS[name].D, 35, sn, lam)
    return _pc(name, sn, lam)


def _state(ctx):
    return [ctx.get_planes(v) for v in (0, 1)]


def _assert_state(got, pm, what):
    """got: a context or [(norm_param, min_cost)] per view; pm: the oracle's PatchMatch"""
    got = _state(got) if hasattr(got, "get_planes") else got
    for v in (0, 1):
        P = pm.planes(v)
        np.testing.assert_array_equal(got[v][0][..., :3], P[..., 0:3], err_msg=f"{what}: norm, view {v}")
        np.testing.assert_array_equal(got[v][0][..., 3:], P[..., 6:9], err_msg=f"{what}: param, view {v}")
        np.testing.assert_array_equal(got[v][1], pm.min_cost(v), err_msg=f"{what}: min_cost, view {v}")


def _assert_same_state(a, b, what):
    for v in (0, 1):
        np.testing.assert_array_equal(a[v][0], b[v][0], err_msg=f"{what}: planes, view {v}")
        np.testing.assert_array_equal(a[v][1], b[v][1], err_msg=f"{what}: min_cost, view {v}")


def _assert_maps(ctx, pm, name, what):
    """PlaneToDisp, cspm_postprocess_f64 and cspm_postprocess behind a run == the oracle's / the restatement's"""
    l, r = cengrd_ref.images(name)
    pm.plane_to_disp()
    for v in (0, 1):
        np.testing.assert_array_equal(ctx.disparity_u8(v, DIS_SCALE), pm.dis(v), err_msg=f"{what}: 8-bit map, view {v}")
    abc = [ctx.get_planes(v)[0][..., 3:6] for v in (0, 1)]
    want = pp_sub_ref.postprocess_f64(abc[0], abc[1], l, r, cengrd_ref.PAIRS[name].D)
    for k, (g, w) in enumerate(zip(ctx.postprocess_f64(valid=True), want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: sub-pixel post-processing, output {k}")
    pm.postprocess()
    lo, ro = ctx.postprocess(DIS_SCALE)
    np.testing.assert_array_equal(lo, pm.dis(0), err_msg=f"{what}: post-processed left map")
    np.testing.assert_array_equal(ro, pm.dis(1), err_msg=f"{what}: post-processed right map")


# ---- volumes ---------------------------------------------------------------------------------------------------------------------

VOLUME_CASES = [("small", 0, 0.0), ("small", 5, 0.3), ("odd", 3, 0.3), ("odd", 0, 0.0), ("ragged_63x65", 3, 0.3), ("ragged_64x63", 0, 0.0),
                ("ragged_64x63", 3, 1.0), ("ragged_65x64", 3, 0.0), ("adversarial", 3, 0.3), ("adversarial", 0, 0.0)]


@pytest.mark.parametrize("name,sn,lam", VOLUME_CASES)
def test_volumes_max_cost_and_weights(gpu_ctx, name, sn, lam):
    """every level, both views, through cspm_get_cost_slab; CSPM_OPT_GRD_VOLUMES has no effect on this cost"""
    gpu_ctx.set_option(capi.OPT_GRD_VOLUMES, 0)
    pc = _build(gpu_ctx, name, sn, lam)
    assert gpu_ctx.levels == pc.levels
    np.testing.assert_array_equal(gpu_ctx.scale_weights(), pc.scale_wgt())
    for s in range(pc.levels):
        assert gpu_ctx.level_dims(s) == pc.dims(s)
        for v in (0, 1):
            np.testing.assert_array_equal(gpu_ctx.level_image(v, s), pc.image(v, s))
            np.testing.assert_array_equal(gpu_ctx.cost_volume(v, s), pc.volume(v, s), err_msg=f"level {s}, view {v}")
            assert gpu_ctx.max_cost(v, s) == pc.max_cost_dev(v, s) == pc.max_cost(v, s)
    first = gpu_ctx.cost_volume(1, pc.levels - 1)
    gpu_ctx.set_option(capi.OPT_GRD_VOLUMES, 1)
    _build(gpu_ctx, name, sn, lam)
    np.testing.assert_array_equal(gpu_ctx.cost_volume(1, pc.levels - 1), first)


@pytest.mark.parametrize("name", ["small", "odd", "ragged_65x64"])
def test_build_cv_host_boundary(gpu_ctx, name):
    """CenGrdCC::buildCV / buildRightCV on caller-owned CV_64FC3 RGB buffers == the restatement's single-scale level-0 cells"""
    L = capi.load_library()
    p = cengrd_ref.PAIRS[name]
    l, r = cengrd_ref.images(name)
    pc = _pc(name, 0, 0.0)
    rgb = [np.ascontiguousarray(im[..., ::-1].astype(np.float64)) for im in (l, r)]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for right in (0, 1):
        got = np.zeros((p.D + 1, p.h, p.w))
        assert L.cspm_cengrd_build_cv_host(0, dp(rgb[0]), dp(rgb[1]), p.w, p.h, p.D + 1, right, dp(got)) == 0, L.cspm_last_error(None)
        np.testing.assert_array_equal(got, pc.volume(right, 0))
    assert L.cspm_cengrd_build_cv_host(0, dp(rgb[0]), dp(rgb[1]), p.w, p.h, 0, 0, dp(got)) < 0  # maxDis < 1: an error code, as for the other two entries


# ---- the same field whichever way the cells arrive ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sn,lam", [("small", 3, 0.3), ("ragged_63x65", 0, 0.0)])
def test_uploaded_cells_give_the_same_field(gpu_ctx, name, sn, lam):
    p = cengrd_ref.PAIRS[name]
    pc = _build(gpu_ctx, name, sn, lam)
    gpu_ctx.patchmatch(2, seed=5, schedule=RASTER)
    built = _state(gpu_ctx)
    built_maps = [gpu_ctx.disparity_u8(v, DIS_SCALE) for v in (0, 1)] + list(gpu_ctx.postprocess(DIS_SCALE))
    gpu_ctx.begin_cost(p.D, 35, sn, lam)
    for s in range(pc.levels):
        for v in (0, 1):
            vol = pc.volume(v, s)
            for d in range(vol.shape[0]):
                gpu_ctx.upload_cost_slab(v, s, d, vol[d])
    gpu_ctx.finish_cost()
    for s in range(pc.levels):
        for v in (0, 1):
            assert gpu_ctx.max_cost(v, s) == pc.max_cost(v, s)
    gpu_ctx.patchmatch(2, seed=5, schedule=RASTER)
    _assert_same_state(_state(gpu_ctx), built, "uploaded against built")
    maps = [gpu_ctx.disparity_u8(v, DIS_SCALE) for v in (0, 1)] + list(gpu_ctx.postprocess(DIS_SCALE))
    for a, b in zip(maps, built_maps):
        np.testing.assert_array_equal(a, b)


# ---- cspm_plane_cost_batch ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,sn,lam", [("small", 0, 0.0), ("small", 5, 0.3), ("odd", 3, 0.3)])
def test_plane_cost_batch(gpu_ctx, name, sn, lam):
    """random planes incl. corners, |nz| ~ 0, integer, boundary and out-of-range disparities (conftest.random_planes)"""
    p = cengrd_ref.PAIRS[name]
    pc = _build(gpu_ctx, name, sn, lam)
    rng = np.random.default_rng(77)
    n = 1500
    for view in (0, 1):
        xy, norm, point, param = random_planes(rng, n, p.w, p.h, p.D)
        got = gpu_ctx.plane_cost_batch(view, xy, np.concatenate([norm, param], 1))
        dev = np.array([pc.cost(xy[i, 0], xy[i, 1], norm[i], param[i], view, po.SUM_DEVICE) for i in range(n)])
        np.testing.assert_array_equal(got, dev)  # the device order: bit for bit
        idx = np.arange(300)
        ser = np.array([pc.cost(xy[i, 0], xy[i, 1], norm[i], param[i], view, po.SUM_SERIAL) for i in idx])
        np.testing.assert_allclose(got[idx], ser, rtol=1e-12, atol=0)  # the reference order: rounding only


# ---- the whole pipeline against the oracle with injected volumes ------------------------------------------------------------------

@pytest.mark.parametrize("sched,early_exit", [(RASTER, 1), (RASTER, 0), (REDBLACK, 1), (REDBLACK, 0)])
def test_phase_by_phase(gpu_ctx, sched, early_exit):
    name = "mid"
    p = cengrd_ref.PAIRS[name]
    pc = _build(gpu_ctx, name, 3, 0.3)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    okw = dict(seed=9, schedule=sched, sum_order=po.SUM_DEVICE)
    gkw = dict(seed=9, schedule=sched, early_exit=early_exit)
    pm.init(pc, **okw)
    gpu_ctx.pm_init(**gkw)
    _assert_state(gpu_ctx, pm, "init")
    for it in range(2):
        for phase in ("spatial", "view", "refine"):
            getattr(pm, phase)(it, pc, **okw)
            getattr(gpu_ctx, "pm_" + phase)(it, **gkw)
            _assert_state(gpu_ctx, pm, f"iteration {it}, {phase}")
    _assert_maps(gpu_ctx, pm, name, "phase by phase")


@pytest.mark.parametrize("name,sn,sched,early_exit", [("crop", 5, RASTER, 1), ("crop", 5, REDBLACK, 0), ("mid", 5, REDBLACK, 0), ("mid", 0, RASTER, 0)])
def test_whole_patchmatch_and_maps(gpu_ctx, name, sn, sched, early_exit):
    """a whole 3-iteration cspm_patchmatch, the 8-bit maps, cspm_postprocess and cspm_postprocess_f64"""
    p = cengrd_ref.PAIRS[name]
    pc = _build(gpu_ctx, name, sn, 0.3)
    l, r = cengrd_ref.images(name)
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    pm.run(3, pc, False, seed=31, schedule=sched, sum_order=po.SUM_DEVICE, wavefront=True)
    gpu_ctx.patchmatch(3, seed=31, schedule=sched, early_exit=early_exit)
    _assert_state(gpu_ctx, pm, f"{name}: 3 iterations")
    _assert_maps(gpu_ctx, pm, name, name)


@pytest.mark.parametrize("method,code", [("BOX", capi.CA_BOX), ("GF", capi.CA_GF)])
def test_local_stereo_and_a_warm_run(gpu_ctx, method, code):
    """cspm_local_stereo over the CENGRD volumes == tests/ca_ref.py over the restatement's; from the BOX field one warm iteration"""
    name = "kinds"
    p = cengrd_ref.PAIRS[name]
    pc = _build(gpu_ctx, name, 3, 0.3)
    l, r = cengrd_ref.images(name)
    fields = warm_ref.local_stereo_fields(pc, method, p.D, True)
    gpu_ctx.local_stereo(code)
    for v in (0, 1):
        np.testing.assert_array_equal(gpu_ctx.get_planes(v)[0], fields[v], err_msg=f"local stereo {method}, view {v}")
    if method != "BOX":
        return
    pm = po.PatchMatch(l, r, p.D, DIS_SCALE)
    warm_ref.inject(pm, fields)
    warm_ref.warm_run(pm, pc, 1, seed=3, schedule=RASTER, sum_order=po.SUM_DEVICE)
    gpu_ctx.patchmatch_warm(1, seed=3, schedule=RASTER)
    _assert_state(gpu_ctx, pm, "warm run from the BOX field")


# ---- host layer and command line ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sn", [3, 0])
def test_host_layer_class_and_factory(gpu_ctx, tmp_path, sn):
    """tests/helpers/cengrd_check.cc: PreCSPC / PreSSPC(.., new CenGrdCC, ..) + CSPatchMatch == the C ABI; CenGrdCC::buildCV /
    buildRightCV == the restatement; getCCType("CENGRD") is a CenGrdCC (the helper exits 5 otherwise)"""
    exe = _build_helper("cengrd_check")
    name = "small"
    p = cengrd_ref.PAIRS[name]
    l, r = cengrd_ref.images(name)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<5i", p.w, p.h, p.D, sn, 2))
        f.write(l.tobytes())
        f.write(r.tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stdout.decode() + out.stderr.decode()
    raw = np.fromfile(tmp_path / "out.bin")
    n = p.w * p.h
    assert raw.size == 2 * 7 * n + 2 * (p.D + 1) * n
    _build(gpu_ctx, name, sn, 0.3)
    gpu_ctx.patchmatch(2, seed=12345, schedule=RASTER)
    for v in (0, 1):
        blk = raw[v * 7 * n:(v + 1) * 7 * n]
        npar, cost = gpu_ctx.get_planes(v)
        np.testing.assert_array_equal(blk[:6 * n].reshape(p.h, p.w, 6), npar, err_msg=f"view {v}")
        np.testing.assert_array_equal(blk[6 * n:].reshape(p.h, p.w), cost, err_msg=f"view {v}")
    vols = raw[14 * n:].reshape(2, p.D + 1, p.h, p.w)
    pc = _pc(name, 0, 0.0)
    for right in (0, 1):
        np.testing.assert_array_equal(vols[right], pc.volume(right, 0))


def _cli(args, timeout=300):
    return subprocess.run([os.path.join(PKG, "cspm_main")] + args, capture_output=True, timeout=timeout)


def test_cli(gpu_ctx, tmp_path):
    """cspm_main --cc_name=CENGRD with --use_cs --use_pp, with --ca_name, with --warm_ca and --pp_pfm, and as a --batch_list ==
    the same runs through the C ABI.  The single-pair runs use the Motorcycle crop: the command line's five levels have to hold
    BoxCA's 7-pixel filter on the coarsest one."""
    names = ["crop", "small", "mid", "mid"]
    for k, name in enumerate(names):
        l, r = cengrd_ref.images(name)
        pngio.write_png(str(tmp_path / f"l{k}.png"), l[..., ::-1])
        pngio.write_png(str(tmp_path / f"r{k}.png"), r[..., ::-1])
    flags = ["--dis_scale=4", "--cc_name=CENGRD", "--use_cs=true", "--reg_lambda=0.3", "--seed=777"]
    common = ["--max_dis=32"] + flags
    io = [f"--l_img_file={tmp_path}/l0.png", f"--r_img_file={tmp_path}/r0.png", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png"]

    def maps():
        return pngio.read_png(str(tmp_path / "ld.png")), pngio.read_png(str(tmp_path / "rd.png"))

    p = _cli(io + common + ["--use_pp=true"])
    assert p.returncode == 0 and b"Total Time:" in p.stdout, p.stdout.decode() + p.stderr.decode()
    _build(gpu_ctx, "crop", 5, 0.3)
    gpu_ctx.patchmatch(3, seed=777, schedule=RASTER)
    want = gpu_ctx.postprocess(DIS_SCALE)
    for a, b in zip(maps(), want):
        np.testing.assert_array_equal(a, b)
    # local stereo
    p = _cli(io + common + ["--ca_name=BOX"])
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    _build(gpu_ctx, "crop", 5, 0.3)
    gpu_ctx.local_stereo(capi.CA_BOX)
    for v, a in enumerate(maps()):
        np.testing.assert_array_equal(a, gpu_ctx.disparity_u8(v, DIS_SCALE))
    # warm start + sub-pixel post-processing into the PFM
    p = _cli(io + common + ["--warm_ca=BOX", "--iters=1", "--use_pp=true", "--pp_pfm", f"--l_disp_pfm={tmp_path}/l.pfm"])
    assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
    _build(gpu_ctx, "crop", 5, 0.3)
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.patchmatch_warm(1, seed=777, schedule=RASTER)
    want = gpu_ctx.postprocess(DIS_SCALE)
    for a, b in zip(maps(), want):
        np.testing.assert_array_equal(a, b)
    with open(tmp_path / "l.pfm", "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        pfm = np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]
    np.testing.assert_array_equal(pfm, gpu_ctx.postprocess_f64()[0].astype(np.float32))
    # a batch list: two sizes, buffers reused between pairs
    lines = [" ".join(str(tmp_path / n) for n in (f"l{k}.png", f"r{k}.png", f"bl{k}.png", f"br{k}.png")) for k in (1, 2, 3)]
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    p = _cli([f"--batch_list={tmp_path}/list.txt", "--use_pp=true", "--max_dis=16"] + flags)
    assert p.returncode == 0 and b"Batch: 3 pairs" in p.stdout and b"0 failed" in p.stdout, p.stdout.decode() + p.stderr.decode()
    for k in (1, 2, 3):
        _build(gpu_ctx, names[k], 5, 0.3)
        gpu_ctx.patchmatch(3, seed=777, schedule=RASTER)
        want = gpu_ctx.postprocess(DIS_SCALE)
        np.testing.assert_array_equal(pngio.read_png(str(tmp_path / f"bl{k}.png")), want[0], err_msg=f"batch pair {k}")
        np.testing.assert_array_equal(pngio.read_png(str(tmp_path / f"br{k}.png")), want[1], err_msg=f"batch pair {k}")
    # the names the reference reserves stay unimplemented
    p = _cli(io + ["--max_dis=16", "--dis_scale=4", "--cc_name=CG"])
    assert p.returncode == 1


def test_batch_driver_accepts_the_cost_name(gpu_ctx):
    """batch.run_batch with cc = CENGRD (HipPairFn) == the C ABI pair by pair"""
    import torch
    assert batch.CC_CODES["CENGRD"] not in (batch.CC_CODES["GRD"], batch.CC_CODES["CEN"], batch.CC_CODES["IMG"])
    p = cengrd_ref.PAIRS["small"]
    assert 3 in cengrd_ref.SCALES["small"] and 3 in cengrd_ref.SCALES["small_swapped"]
    imgs = [cengrd_ref.images("small"), cengrd_ref.images("small_swapped")]
    pairs = np.stack([np.stack(im) for im in imgs])
    params = dict(w=p.w, h=p.h, max_dis=p.D, dis_scale=DIS_SCALE, scale_num=3, reg_lambda=0.3, iters=2, seed=9, schedule=0, use_pp=1,
                  cc=batch.CC_CODES["CENGRD"])
    fn = batch.HipPairFn(0, in_flight=2)
    try:
        got = batch.run_batch(pairs, params, fn, device="cuda:0", dist=None).cpu().numpy()
    finally:
        fn.close()
    torch.cuda.synchronize()
    for k, (l, r) in enumerate(imgs):
        gpu_ctx.set_images(l, r)
        gpu_ctx.build_cost_cengrd(p.D, 35, 3, 0.3)
        gpu_ctx.patchmatch(2, seed=9 + k, schedule=RASTER)
        want = gpu_ctx.postprocess(DIS_SCALE)
        np.testing.assert_array_equal(got[k, 0], want[0])
        np.testing.assert_array_equal(got[k, 1], want[1])


# ---- streams of pairs on one context ----------------------------------------------------------------------------------------------

def _fresh(build, l, r, D):
    import crossscalepatchmatch_amd as cs
    ctx = cs.StereoContext(0)
    try:
        ctx.set_images(l, r)
        build(ctx)
        vol = ctx.cost_volume(0, 1)
        ctx.patchmatch(2, seed=4, schedule=RASTER)
        return vol, _state(ctx), ctx.postprocess(DIS_SCALE)
    finally:
        ctx.close()


def test_stream_of_pairs_and_cost_switches(gpu_ctx):
    """two equally sized pairs back to back on one context (buffers reused), then GRD -> CENGRD -> CEN on one context: each result
    equals a fresh context's -- nothing stale is read"""
    import crossscalepatchmatch_amd as cs
    D = 16
    a = cengrd_ref.images("small")
    b = cengrd_ref.images("adversarial")  # the same size
    assert a[0].shape == b[0].shape
    builds = {"GRD": lambda c: c.build_cost_grd(D, 35, 3, 0.3), "CENGRD": lambda c: c.build_cost_cengrd(D, 35, 3, 0.3),
              "CEN": lambda c: c.build_cost_cen(D, 35, 3, 0.3)}
    ctx = cs.StereoContext(0)
    try:
        for what, (l, r), kind in (("pair a", a, "CENGRD"), ("pair b on a's buffers", b, "CENGRD"), ("pair a again", a, "CENGRD"),
                                   ("GRD", a, "GRD"), ("CENGRD after GRD", a, "CENGRD"), ("CEN after CENGRD", a, "CEN"),
                                   ("CENGRD after CEN", b, "CENGRD")):
            ctx.set_images(l, r)
            builds[kind](ctx)
            vol = ctx.cost_volume(0, 1)
            ctx.patchmatch(2, seed=4, schedule=RASTER)
            got = _state(ctx)
            maps = ctx.postprocess(DIS_SCALE)
            want_vol, want, want_maps = _fresh(builds[kind], l, r, D)
            np.testing.assert_array_equal(vol, want_vol, err_msg=what)
            _assert_same_state(got, want, what)
            for x, y in zip(maps, want_maps):
                np.testing.assert_array_equal(x, y, err_msg=what)
    finally:
        ctx.close()


def test_errors(gpu_ctx):
    import crossscalepatchmatch_amd as cs
    l, r = cengrd_ref.images("small")
    gpu_ctx.set_images(l, r)
    with pytest.raises(cs.CspmError):
        gpu_ctx.build_cost_cengrd(0, 35, 0, 0.0)  # max_dis < 1
    gpu_ctx.build_cost_cengrd(16, 35, 0, 0.0)
    with pytest.raises(cs.CspmError):
        gpu_ctx.upload_cost_slab(0, 0, 0, np.zeros((48, 64)))  # not a cspm_begin_cost object
