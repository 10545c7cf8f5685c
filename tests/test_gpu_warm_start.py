"""Warm-started PatchMatch: re-scoring a stored plane field (cspm_rescore_planes), PatchMatch from it (cspm_patchmatch_warm) and
carrying a field up one pyramid level (cspm_upsample_planes), through the C ABI, the C++ host layer and the command line.  This
module holds them to other GPU entries (the random init, the batch engine, the single phases) or to numpy: identities between GPU
paths.  tests/test_gpu_warm_oracle.py holds the same entries to the CPU oracle restarted from the same fields (tests/warm_ref.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import random_planes
from crossscalepatchmatch_amd import capi, realdata as rd
from crossscalepatchmatch_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, D = 128, 96, 24


@pytest.fixture(scope="module")
def pair():
    l, r, _, _ = make_pair(W, H, D, seed=21)
    return l, r


def _new_ctx():
    import crossscalepatchmatch_amd as cs
    return cs.StereoContext(0)


def _build(ctx, kind, max_dis=D):
    if kind == "grd_cs":
        ctx.build_cost_grd(max_dis, 35, 3, 0.3)
    elif kind == "grd_ss":
        ctx.build_cost_grd(max_dis, 35, 0, 0.0)
    elif kind == "grd_cs_volumes":
        ctx.build_cost_grd(max_dis, 35, 3, 0.3, volumes=True)
    elif kind == "grd_ss_no_tables":
        ctx.build_cost_grd(max_dis, 35, 0, 0.0, table_volumes=False)
    elif kind == "cen_cs":
        ctx.build_cost_cen(max_dis, 35, 3, 0.3)
    elif kind == "cen_ss_volumes":
        ctx.build_cost_cen(max_dis, 35, 0, 0.0, volumes=True)
    elif kind == "grdpc":
        ctx.build_cost_img(max_dis, 35, 0, 0.0)
    elif kind == "cspc":
        ctx.build_cost_img(max_dis, 35, 3, 0.3)
    else:
        raise ValueError(kind)


def _planes(ctx):
    return [ctx.get_planes(v) for v in (0, 1)]


def _assert_same(got, want, tag=""):
    for v in (0, 1):
        np.testing.assert_array_equal(got[v][0], want[v][0], err_msg=f"{tag} planes view {v}")
        np.testing.assert_array_equal(got[v][1], want[v][1], err_msg=f"{tag} min_cost view {v}")


KINDS = ["grd_cs", "grd_ss", "grd_cs_volumes", "grd_ss_no_tables", "cen_cs", "cen_ss_volumes", "grdpc", "cspc"]


@pytest.mark.parametrize("kind", KINDS)
def test_rescore_equals_the_init(gpu_ctx, pair, kind):
    gpu_ctx.set_images(*pair)
    _build(gpu_ctx, kind)
    gpu_ctx.pm_init(seed=77)
    init = _planes(gpu_ctx)
    gpu_ctx.rescore_planes()
    _assert_same(_planes(gpu_ctx), init, kind)


def _random_field(rng, w, h, max_dis):
    """a whole field of random planes (random_planes' special cases included), each at its own pixel"""
    xy, norm, _, param = random_planes(rng, w * h, w, h, max_dis)
    npar = np.zeros((h, w, 6))
    npar[xy[:, 1], xy[:, 0]] = np.concatenate([norm, param], 1)  # a pixel drawn twice keeps one of its planes
    empty = ~npar.any(axis=2)
    npar[empty] = np.concatenate([norm, param], 1)[: int(empty.sum())]  # the rest: planes of other pixels
    return npar


@pytest.mark.parametrize("kind", ["grd_cs", "grd_ss", "cen_cs", "cspc", "grd_cs_volumes"])
def test_rescore_equals_the_batch_engine(gpu_ctx, pair, kind):
    rng = np.random.default_rng(5)
    gpu_ctx.set_images(*pair)
    _build(gpu_ctx, kind)
    fields = [_random_field(rng, W, H, D) for _ in (0, 1)]
    for v in (0, 1):
        gpu_ctx.set_planes(v, fields[v], np.full((H, W), -7.0))  # garbage costs
    gpu_ctx.rescore_planes()
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    for v in (0, 1):
        npar, cost = gpu_ctx.get_planes(v)
        np.testing.assert_array_equal(npar, fields[v])  # the planes are not written
        np.testing.assert_array_equal(cost.ravel(), gpu_ctx.plane_cost_batch(v, xy, fields[v].reshape(-1, 6)), err_msg=f"{kind} view {v}")


@pytest.mark.parametrize("schedule", [capi.SCHED_RASTER, capi.SCHED_REDBLACK])
def test_warm_run_from_the_init_field_is_the_cold_run(gpu_ctx, pair, schedule):
    gpu_ctx.set_images(*pair)
    _build(gpu_ctx, "grd_cs")
    gpu_ctx.patchmatch(3, seed=31, schedule=schedule)
    cold = _planes(gpu_ctx)
    gpu_ctx.pm_init(seed=31)
    start = _planes(gpu_ctx)
    warm_ctx = _new_ctx()
    try:
        warm_ctx.set_images(*pair)
        _build(warm_ctx, "grd_cs")
        for v in (0, 1):
            warm_ctx.set_planes(v, start[v][0], np.full((H, W), -1.0))  # below every cost: a skipped re-score would keep every start plane
        warm_ctx.patchmatch_warm(3, seed=31, schedule=schedule)
        _assert_same(_planes(warm_ctx), cold, f"schedule {schedule}")
    finally:
        warm_ctx.close()


def test_warm_run_equals_its_phases(gpu_ctx, pair):
    gpu_ctx.set_images(*pair)
    _build(gpu_ctx, "grd_cs")
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.patchmatch_warm(2, seed=5)
    warm = _planes(gpu_ctx)
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.rescore_planes()
    for it in (0, 1):
        gpu_ctx.pm_spatial(it, seed=5)
        gpu_ctx.pm_view(it, seed=5)
        gpu_ctx.pm_refine(it, seed=5)
    _assert_same(_planes(gpu_ctx), warm)


@pytest.mark.parametrize("kind,method", [("grd_cs", capi.CA_GF), ("cen_ss_volumes", capi.CA_BOX)])
def test_warm_run_only_lowers_costs(gpu_ctx, pair, kind, method):
    gpu_ctx.set_images(*pair)
    _build(gpu_ctx, kind)
    gpu_ctx.local_stereo(method)
    gpu_ctx.rescore_planes()
    start = _planes(gpu_ctx)
    gpu_ctx.patchmatch_warm(1)
    end = _planes(gpu_ctx)
    for v in (0, 1):
        assert np.all(end[v][1] <= start[v][1]), v
        assert np.any(end[v][1] < start[v][1]), v


def test_sweep_timeout_repeats_the_warm_run(pair):
    ctx = _new_ctx()
    try:
        ctx.set_images(*pair)
        _build(ctx, "grd_cs")
        ctx.local_stereo(capi.CA_BOX)
        ctx.patchmatch_warm(2, seed=9, schedule=capi.SCHED_RASTER)
        want = _planes(ctx)
        assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 0
        ctx.local_stereo(capi.CA_BOX)
        ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 0)
        try:
            ctx.patchmatch_warm(2, seed=9, schedule=capi.SCHED_RASTER)
            got = _planes(ctx)  # the getter sees the timeout and repeats the run from its starting field
        finally:
            ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 3000)
        assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 1
        _assert_same(got, want)
    finally:
        ctx.close()


@pytest.mark.parametrize("w,h", [(77, 41), (64, 48)])
def test_upsample_matches_the_formula(gpu_ctx, w, h):
    rng = np.random.default_rng(w + h)
    ws, hs = (w + 1) // 2, (h + 1) // 2
    src = _new_ctx()
    try:
        src.set_images(*make_pair(ws, hs, 8, seed=1)[:2])
        fields = [_random_field(rng, ws, hs, 8) for _ in (0, 1)]
        for v in (0, 1):
            src.set_planes(v, fields[v], rng.random((hs, ws)))
        gpu_ctx.set_images(*make_pair(w, h, 16, seed=2)[:2])
        gpu_ctx.upsample_planes_from(src)
        for v in (0, 1):
            want = fields[v][np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1].copy()
            want[..., 5] *= 2.0
            np.testing.assert_array_equal(gpu_ctx.get_planes(v)[0], want, err_msg=f"{w}x{h} view {v}")
        src.set_images(*make_pair(ws + 1, hs, 8, seed=1)[:2])
        src.set_planes(0, np.zeros((hs, ws + 1, 6)), np.zeros((hs, ws + 1)))
        with pytest.raises(capi.CspmError, match="error -1"):
            gpu_ctx.upsample_planes_from(src)
    finally:
        src.close()


def test_error_codes(pair):
    ctx, other = _new_ctx(), _new_ctx()
    try:
        with pytest.raises(capi.CspmError, match="error -3"):
            ctx.rescore_planes()  # no cost object
        with pytest.raises(capi.CspmError, match="error -3"):
            ctx.patchmatch_warm(1)
        ctx.set_images(*pair)
        _build(ctx, "grd_cs")
        with pytest.raises(capi.CspmError, match="error -3.*no plane field"):
            ctx.patchmatch_warm(1)  # a cost object but nothing to start from
        with pytest.raises(capi.CspmError, match="error -3.*no plane field"):
            ctx.rescore_planes()
        with pytest.raises(capi.CspmError, match="error -3"):
            ctx.upsample_planes_from(other)  # the source has no plane field
        ctx.pm_init()
        for bad in (-1, 16):
            with pytest.raises(capi.CspmError, match="error -1"):
                ctx.patchmatch_warm(bad)
        with pytest.raises(capi.CspmError, match="error -1"):
            ctx.patchmatch_warm(1, rb_neighbours=3)
        with pytest.raises(capi.CspmError, match="error -3"):
            other.upsample_planes_from(ctx)  # the destination has no images
        with pytest.raises(capi.CspmError, match="error -1"):
            ctx.upsample_planes_from(ctx)
        other.set_images(*make_pair(W, H, D, seed=3)[:2])
        with pytest.raises(capi.CspmError, match="error -1.*one pyramid level below"):
            other.upsample_planes_from(ctx)  # same size, not half
        ctx.patchmatch_warm(0)  # zero iterations: only the re-score
        ctx.synchronize()
    finally:
        ctx.close()
        other.close()


def _build_helper(name):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    pkg = os.path.join(ROOT, "crossscalepatchmatch_amd")
    host = os.path.join(pkg, "host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-pthread", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "helpers", name + ".cc"),
                           os.path.join(host, "host_impl.cc"), os.path.join(host, "image_io.cc"), "-L", pkg, "-lcspm_hip", "-lz",
                           "-Wl,-rpath," + pkg])
    return exe


def test_patchmatch_from_equals_the_c_abi(gpu_ctx, pair, tmp_path):
    """CSPatchMatch::LocalStereo + PatchMatchFrom, and SetPlanes + PatchMatchFrom on a second cost object (tests/helpers/
    warm_from_check.cc) == the C ABI sequences; a foreign IPlaneCost is refused"""
    exe = _build_helper("warm_from_check")
    l, r = pair
    iters = 2
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([W, H, D, 3, capi.CA_BOX, iters], np.int32).tobytes())
        f.write(np.ascontiguousarray(l).tobytes())
        f.write(np.ascontiguousarray(r).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert b"foreign refused" in out.stdout
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    n = W * H
    runs = []
    for k in range(2):
        run = []
        for v in (0, 1):
            base = (2 * k + v) * 7 * n
            run.append((raw[base:base + 6 * n].reshape(H, W, 6), raw[base + 6 * n:base + 7 * n].reshape(H, W)))
        runs.append(run)
    gpu_ctx.set_images(l, r)
    gpu_ctx.build_cost_grd(D, 35, 3, 0.3)
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.patchmatch_warm(iters)
    a = _planes(gpu_ctx)
    _assert_same(runs[0], a, "LocalStereo + PatchMatchFrom")
    gpu_ctx.build_cost_grd(D, 35, 3, 0.3)
    for v in (0, 1):
        gpu_ctx.set_planes(v, a[v][0], np.zeros((H, W)))
    gpu_ctx.patchmatch_warm(iters)
    _assert_same(runs[1], _planes(gpu_ctx), "SetPlanes + PatchMatchFrom")


def test_cli_warm_ca_box_equals_the_c_abi(gpu_ctx, tmp_path):
    """cspm_main --warm_ca=BOX --iters=2 --use_pp, alone and in a --batch_list: the 8-bit maps == local_stereo + patchmatch_warm(2) +
    postprocess through the C ABI (160x128: the coarsest of the five levels is 10x8, BOX needs 7)"""
    from PIL import Image
    w, h, d = 160, 128, 24
    l, r, _, _ = make_pair(w, h, d, seed=22)
    lf, rf = tmp_path / "l.png", tmp_path / "r.png"
    Image.fromarray(np.ascontiguousarray(l[..., ::-1])).save(lf)
    Image.fromarray(np.ascontiguousarray(r[..., ::-1])).save(rf)
    cli = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    flags = [f"--max_dis={d}", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--use_pp=true", "--iters=2",
             "--warm_ca=BOX", "--quiet=true"]
    subprocess.check_call([cli, f"--l_img_file={lf}", f"--r_img_file={rf}", f"--l_dis_file={tmp_path}/ld.png",
                           f"--r_dis_file={tmp_path}/rd.png"] + flags, stdout=subprocess.DEVNULL)
    with open(tmp_path / "list.txt", "w") as f:
        for k in range(2):
            f.write(f"{lf} {rf} {tmp_path}/ld{k}.png {tmp_path}/rd{k}.png\n")
    subprocess.check_call([cli, f"--batch_list={tmp_path}/list.txt"] + flags, stdout=subprocess.DEVNULL)
    gpu_ctx.set_images(l, r)
    gpu_ctx.build_cost_grd(d, 35, 5, 0.3)
    gpu_ctx.local_stereo(capi.CA_BOX)
    gpu_ctx.patchmatch_warm(2)
    lo, ro = gpu_ctx.postprocess(4)
    for suffix in ("", "0", "1"):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / f"ld{suffix}.png").convert("L")), lo)
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / f"rd{suffix}.png").convert("L")), ro)
    bad = subprocess.run([cli, f"--l_img_file={lf}", f"--r_img_file={rf}", "--pc_name=IMG"] + flags, capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"--warm_ca needs --pc_name=PRE" in bad.stdout


def test_motorcycle_crop_gf_warm_and_coarse_to_fine(gpu_ctx, record_property):
    """the 200x128 crop (3 levels: GF needs 19 px at the coarsest): GF + 1 warm iteration, and 3 half-size + 1 full-size iterations.
    Only that both finish and never raise a re-scored starting cost; their bad-2.0 is recorded."""
    cfg, l, r, gt = rd.load_crop()
    D_, S, lam, ds = cfg["max_dis"], 3, cfg["reg_lambda"], cfg["dis_scale"]
    rec = {}
    gpu_ctx.set_images(l, r)
    gpu_ctx.build_cost_grd(D_, 35, S, lam)
    gpu_ctx.local_stereo(capi.CA_GF)
    gpu_ctx.rescore_planes()
    start = _planes(gpu_ctx)
    gpu_ctx.patchmatch_warm(1)
    for v in (0, 1):
        assert np.all(gpu_ctx.get_planes(v)[1] <= start[v][1])
    lo, _ = gpu_ctx.postprocess(ds)
    rec["gf_warm1"] = rd.bad_fraction(lo.astype(np.float64) / ds, gt, 2.0)
    # coarse to fine through the helper, then the same steps by hand with the starting costs in between
    full = capi.coarse_to_fine(l, r, D_, 3, 1, "GRD", 35, S, lam)
    try:
        c2f = _planes(full)
        lo, _ = full.postprocess(ds)
        rec["c2f_3_1"] = rd.bad_fraction(lo.astype(np.float64) / ds, gt, 2.0)
    finally:
        full.close()
    coarse = _new_ctx()
    try:
        gpu_ctx.set_images(l, r)
        gpu_ctx.build_cost_grd(D_, 35, S, lam)
        half = [gpu_ctx.level_image(v, 1) for v in (0, 1)]
        coarse.set_images(*half)
        coarse.build_cost_grd((D_ + 1) // 2, 35, S, lam)
        coarse.patchmatch(3)
        gpu_ctx.upsample_planes_from(coarse)
        gpu_ctx.rescore_planes()
        start = _planes(gpu_ctx)
        gpu_ctx.patchmatch_warm(1)
        end = _planes(gpu_ctx)
    finally:
        coarse.close()
    _assert_same(end, c2f, "coarse_to_fine")
    for v in (0, 1):
        assert np.all(end[v][1] <= start[v][1])
    record_property("bad2", {"motorcycle_crop_200x128_D32_GRD_cs3_post_processed": rec})
    print(json.dumps(rec))
