"""-m gpu: the edge-aware global smoother.  cspm_smooth_disparity_host against the CPU restatement
tests/smooth_ref.py bit for bit; the smoother as the last step of the sub-pixel post-processing against the restatement composed with
the existing post-processing restatements, with the median filter off and on, host and device-resident outputs; the switched-off
smoother against a fresh context; the 8-bit entries untouched; cspm_reproject's PP source; setter, getter, argument errors, timing, the
C++ host layer and the CLI.

Shapes are w x h.  The horizontal pass gives a single-wave workgroup 64 rows (kSmRows) and walks x in chunks of 32 columns (kSmChunk);
the vertical pass gives a workgroup 64 columns and takes rows 8 at a time (kSmBatch).  Next to the shapes the issue names, the list
straddles each of these sizes by one: heights 63 / 64 / 65 and 7 / 8 / 9, widths 31 / 32 / 33 and 63 / 64 / 65; 130 x 67 is wider than
four chunks and two column workgroups and taller than one row workgroup.

Before a device result is compared, the restatement alone must show that the case can fail: with lambda = 100, on every map of at
least 25 pixels, it changes at least half of the pixels; in the pipeline tests at least one pixel changes and the masks stay.

tests/conftest.py's gpu_ctx does not reset the smoother: every test that switches it on switches it off again in a finally (smooth_ctx)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geom_ref as gr
import pngio
import smooth_ref as sr
from crossscalepatchmatch_amd import capi
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 9), (63, 5), (65, 17), (130, 67),
          (31, 63), (32, 64), (33, 65), (64, 7), (65, 8), (63, 9)]
# (guide, confidences, T, lambda, max_dis): every value of every axis, and every guide with every kind of confidences
COMBOS = [("none", "none", 1, 100.0, 0), ("palette", "binary", 3, 100.0, 30), ("bw", "random", 1, 100.0, 30), ("palette", "random", 3, 100.0, 0),
          ("bw", "none", 3, 100.0, 0), ("none", "binary", 3, 100.0, 30), ("palette", "none", 1, 0.0, 0), ("bw", "binary", 3, 0.0, 30),
          ("none", "random", 1, 100.0, 0)]
PARAMS = dict(lam=100.0, sigma_color=15.0, iterations=2, fill_conf=0.5)
CAL = (300.0, 31.5, 20.25, 0.25, 3.5)


@pytest.fixture(scope="module", autouse=True)
def _torch_first(_gpu_ctx_session):
    """the host entries need no context, but PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the
    session's context does that, also when this file runs alone"""


@pytest.fixture
def smooth_ctx(gpu_ctx):
    """the session's context; smoothing and the median filter are off again afterwards whatever the test did"""
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_pp_smooth(lam=0)
        gpu_ctx.set_pp_median(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}: {got[diff][0]!r} != {want[diff][0]!r}"


def _case(w, h, guide, conf, seed):
    rng = np.random.default_rng([w, h, seed])
    d = rng.random((h, w)) * 40.0 + 2.0
    bad = rng.random((h, w)) < 0.05
    d[bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    if w > 2 and h > 2:
        d[h // 2, :] = np.nan    # a whole row and a whole column of non-nodes
        d[:, w // 3] = -np.inf
    g = {"none": None, "palette": sr.PALETTE[rng.integers(0, 4, (h, w))], "bw": (rng.integers(0, 2, (h, w, 1)) * 255).astype(np.uint8).repeat(3, axis=2)}[guide]
    c = {"none": None, "binary": (rng.random((h, w)) > 0.3).astype(np.float64), "random": rng.random((h, w))}[conf]
    return d, c, g


# ---- the host entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_host_entry_against_the_restatement(w, h):
    for k, (guide, conf, T, lam, max_dis) in enumerate(COMBOS):
        d, c, g = _case(w, h, guide, conf, k)
        want = sr.smooth(d, c, g, lam, 20.0, T, max_dis)
        if lam > 0 and w * h >= 25:
            changed = float(np.mean(_bits(want) != _bits(d)))
            assert changed >= 0.5, f"{w}x{h} {COMBOS[k]}: the restatement changes only {changed:.3f} of the pixels"
        got = capi.smooth_disparity(0, d, c, g, max_dis=max_dis, lam=lam, sigma_color=20.0, iterations=T)
        _same(got, want, f"{w}x{h} {COMBOS[k]}")


def test_host_entry_properties_on_the_device():
    """what test_smooth_ref.py shows for the restatement, once more for the kernels alone"""
    rng = np.random.default_rng(8)
    d = rng.random((37, 45)) * 30.0 + 1.0
    g = sr.PALETTE[rng.integers(0, 4, (37, 45))]
    _same(capi.smooth_disparity(0, d, None, g, lam=0.0, iterations=3), d, "lambda = 0, C = 1")
    holed = d.copy()
    holed[5, 7] = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    _same(capi.smooth_disparity(0, holed, np.zeros_like(d), g, max_dis=20), holed, "C = 0")
    const = capi.smooth_disparity(0, np.full((33, 17), 37.25), None, rng.integers(0, 256, (33, 17, 3)).astype(np.uint8))
    assert np.abs(const - 37.25).max() <= 100 * 3.6e-14
    holed = d.copy()
    holed[10, :] = np.nan
    out = capi.smooth_disparity(0, holed, None, g)
    assert np.isfinite(out).all() and out.min() >= 1.0 - 1e-9 and out.max() <= 31.0 + 1e-9
    p = capi.smooth_params(sigma_color=7.0, iterations=8)
    assert (p.lambda_, p.sigma_color, p.iterations) == (100.0, 7.0, 8)
    _same(capi.smooth_disparity(0, d, None, g, sigma_color=7.0, iterations=8), sr.smooth(d, None, g, 100.0, 7.0, 8), "sigma 7, T = 8")
    L = capi.load_library()
    o = np.zeros_like(d)
    assert L.cspm_smooth_disparity_host(0, capi._dp(d), None, capi._u8(np.ascontiguousarray(g)), 45, 37, None, 0, capi._dp(o)) == 0  # NULL = the defaults
    _same(o, sr.smooth(d, None, g), "NULL parameters")


# ---- inside the post-processing ----------------------------------------------------------------------------------------------------
def _run(ctx, pair, seed):
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 35, 5, 0.3)
    ctx.patchmatch(1, seed=seed, schedule=capi.SCHED_RASTER)


@pytest.mark.parametrize("median", [0, 2])
def test_f64_pipeline_and_its_device_variant(smooth_ctx, small_pair, median):
    """64 x 48 after one iteration: cspm_postprocess_f64 with smoothing == pp_sub_ref's steps, M64 when on, then S; the masks are the
    unsmoothed run's"""
    import torch
    ctx = smooth_ctx
    l, r, D, w, h = (small_pair[k] for k in ("l", "r", "max_dis", "w", "h"))
    _run(ctx, small_pair, 5)
    abc = [ctx.get_planes(v)[0][..., 3:6] for v in (0, 1)]
    plain = sr.postprocess_f64_smooth(abc[0], abc[1], l, r, D, median, None)
    want = sr.postprocess_f64_smooth(abc[0], abc[1], l, r, D, median, PARAMS)
    changed = np.concatenate([(_bits(p) != _bits(f)).ravel() for p, f in zip(plain[:2], want[:2])])
    assert changed.any() and all(np.array_equal(plain[2 + v], want[2 + v]) and 0 < want[2 + v].sum() < want[2 + v].size for v in (0, 1))
    ctx.set_pp_median(median)
    off = ctx.postprocess_f64(valid=True)
    ctx.set_pp_smooth(**PARAMS)
    got = ctx.postprocess_f64(valid=True)
    outs = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    ctx.postprocess_f64_device(outs[0].data_ptr(), outs[1].data_ptr())
    ctx.synchronize()
    for v in (0, 1):
        _same(off[v], plain[v], f"view {v}, smoothing off")
        _same(got[v], want[v], f"view {v}")
        assert np.array_equal(got[2 + v], want[2 + v]) and np.array_equal(got[2 + v], off[2 + v]), f"view {v}: smoothing changed a mask"
        _same(outs[v].cpu().numpy(), want[v], f"view {v}: device-resident output")
    again = ctx.postprocess_f64()
    for v in (0, 1):
        _same(again[v], want[v], f"view {v}, a second call")


def test_smoothing_off_is_a_fresh_context_and_the_8_bit_entries_never_change(smooth_ctx, small_pair):
    import crossscalepatchmatch_amd as cs
    import torch
    ctx = smooth_ctx
    w, h = small_pair["w"], small_pair["h"]
    fresh = cs.StereoContext(0)
    try:
        _run(fresh, small_pair, 3)
        assert fresh.get_pp_smooth() == dict(lam=0.0, sigma_color=20.0, iterations=3, fill_conf=0.25, on=False)
        want8, want64 = fresh.postprocess(4), fresh.postprocess_f64(valid=True)
    finally:
        fresh.close()
    _run(ctx, small_pair, 3)
    ctx.set_pp_smooth(**PARAMS)
    on8, on64 = ctx.postprocess(4), ctx.postprocess_f64(valid=True)
    dev8 = [torch.zeros((h, w), dtype=torch.uint8, device="cuda:0") for _ in (0, 1)]
    ctx.postprocess_device(4, dev8[0].data_ptr(), dev8[1].data_ptr())
    ctx.synchronize()
    ctx.set_pp_smooth(lam=0)
    got8, got64 = ctx.postprocess(4), ctx.postprocess_f64(valid=True)
    for v in (0, 1):
        assert np.array_equal(on8[v], want8[v]) and np.array_equal(dev8[v].cpu().numpy(), want8[v]), f"view {v}: smoothing changed an 8-bit map"
        assert np.array_equal(got8[v], want8[v])
        _same(got64[v], want64[v], f"view {v}, switched off again")
        assert np.array_equal(got64[2 + v], want64[2 + v]) and np.array_equal(on64[2 + v], want64[2 + v])
    assert any(not np.array_equal(_bits(on64[v]), _bits(want64[v])) for v in (0, 1))


def test_reproject_reads_the_smoothed_maps(smooth_ctx, small_pair):
    ctx = smooth_ctx
    l, r, D = (small_pair[k] for k in ("l", "r", "max_dis"))
    _run(ctx, small_pair, 5)
    imgs = [ctx.level_image(v, 0) for v in (0, 1)]
    planes = [ctx.get_planes(v)[0] for v in (0, 1)]
    plain = sr.postprocess_f64_smooth(planes[0][..., 3:6], planes[1][..., 3:6], l, r, D, 1, None)
    maps = sr.postprocess_f64_smooth(planes[0][..., 3:6], planes[1][..., 3:6], l, r, D, 1, PARAMS)
    ctx.set_pp_median(1)
    ctx.set_pp_smooth(**PARAMS)
    kw = dict(min_cos=0.5, z_far=5.0)
    for v in (0, 1):
        Dp, Vp = maps[v], maps[2 + v]
        assert 0 < Vp.sum() < Vp.size and not np.array_equal(_bits(Dp), _bits(plain[v]))
        A = np.where(Vp != 0, planes[v][..., 3], np.nan)
        Bs = np.where(Vp != 0, planes[v][..., 4], np.nan)
        for extra, V in ((dict(), None), (dict(consistent_only=1), Vp)):
            got, want = ctx.reproject(v, CAL, capi.GEOM_PP, **extra, **kw), gr.reproject(CAL, v, Dp, V, A, Bs, imgs[v], **kw)
            for name in ("depth", "xyz", "normal", "keep"):
                assert gr.same_bits(got[name], want[name]), f"view {v} {extra}: {name}"
            assert got["count"] == want["count"] and gr.same_cloud(got["cloud"], want["cloud"]), f"view {v} {extra}"


def test_setter_getter_and_argument_errors(smooth_ctx):
    ctx, L = smooth_ctx, smooth_ctx.L
    first = ctx.get_pp_smooth()  # the session's context: switched off by whoever used it last, the other values as they left them
    assert first["on"] is False and first["lam"] == 0.0
    ctx.set_pp_smooth()
    assert ctx.get_pp_smooth() == dict(lam=100.0, sigma_color=20.0, iterations=3, fill_conf=0.25, on=True)
    ctx.set_pp_smooth(lam=7.5, sigma_color=3.0, iterations=8, fill_conf=1.0)
    kept = dict(lam=7.5, sigma_color=3.0, iterations=8, fill_conf=1.0, on=True)
    assert ctx.get_pp_smooth() == kept
    for bad in (dict(lam=-1.0), dict(lam=np.nan), dict(lam=np.inf), dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=np.inf),
                dict(sigma_color=np.nan), dict(iterations=0), dict(iterations=9), dict(fill_conf=-0.1), dict(fill_conf=1.1), dict(fill_conf=np.nan)):
        p = capi.smooth_params(**bad)
        assert L.cspm_set_pp_smooth(ctx.p, C.byref(p)) == -1, bad
        assert b"smoothing" in L.cspm_last_error(ctx.p)
    assert ctx.get_pp_smooth() == kept  # a refused call changes nothing
    assert L.cspm_set_pp_smooth(ctx.p, None) == 0 and ctx.get_pp_smooth()["on"] is False
    ctx.set_pp_smooth(lam=5.0)
    ctx.set_pp_smooth(lam=0, sigma_color=-3.0)  # lambda == 0 is off whatever else the structure holds
    assert ctx.get_pp_smooth()["on"] is False
    on = C.c_int(7)
    p = capi.SmoothParams()
    assert L.cspm_get_pp_smooth(ctx.p, None, C.byref(on)) == 0 and on.value == 0 and L.cspm_get_pp_smooth(ctx.p, C.byref(p), None) == 0
    assert L.cspm_set_pp_smooth(None, C.byref(p)) == -1 and L.cspm_get_pp_smooth(None, C.byref(p), C.byref(on)) == -1
    d, o = np.ones((4, 5)), np.zeros((4, 5))
    f = L.cspm_smooth_disparity_host
    q = capi.smooth_params(fill_conf=9.0)  # ignored here
    assert f(0, capi._dp(d), None, None, 5, 4, C.byref(q), 0, capi._dp(o)) == 0 and (o == 1.0).all()
    assert f(0, capi._dp(d), None, None, 5, 4, C.byref(q), 0, capi._dp(d)) == -1 and f(0, None, None, None, 5, 4, C.byref(q), 0, capi._dp(o)) == -1
    assert f(0, capi._dp(d), capi._dp(np.full((4, 5), 1.5)), None, 5, 4, C.byref(q), 0, capi._dp(o)) == -1
    assert f(0, capi._dp(d), None, None, 5, 4, C.byref(capi.smooth_params(iterations=9)), 0, capi._dp(o)) == -1


def test_timing_counts_the_smoother_under_post(smooth_ctx, small_pair):
    ctx = smooth_ctx
    _run(ctx, small_pair, 3)
    k_post = capi.K_NAMES.index("post")

    def launches(fn):
        ctx.L.cspm_enable_timing(ctx.p, 1)
        try:
            ctx.L.cspm_reset_timing(ctx.p)
            fn()
            n, ms = C.c_longlong(), C.c_double()
            assert ctx.L.cspm_get_timing(ctx.p, k_post, C.byref(n), C.byref(ms), None) == 0
            return n.value, ms.value
        finally:
            ctx.L.cspm_enable_timing(ctx.p, 0)

    off8, off64 = launches(lambda: ctx.postprocess(4)), launches(lambda: ctx.postprocess_f64())
    ctx.set_pp_smooth(**PARAMS)
    on8, on64 = launches(lambda: ctx.postprocess(4)), launches(lambda: ctx.postprocess_f64())
    print(f"CSPM_K_POST (brackets, ms): 8-bit off {off8} on {on8}; f64 off {off64} on {on64}")
    assert on64[0] == off64[0] + 1 and on64[1] > 0.0 and on8[0] == off8[0]


# ---- the host layer and the CLI ----------------------------------------------------------------------------------------------------
def test_host_layer_smoothing():
    exe = _build_helper("smooth_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "smooth_check ok" in r.stdout, r.stdout + r.stderr


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_pp_smooth(smooth_ctx, small_pair, tmp_path):
    ctx = smooth_ctx
    flags = ["--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--seed=31", "--iters=1"]
    smooth = ["--pp_smooth_lambda=100", "--pp_smooth_sigma=15", "--pp_smooth_iters=2", "--pp_smooth_fill_conf=0.5"]
    pngio.write_png(str(tmp_path / "l.png"), small_pair["l"][..., ::-1])
    pngio.write_png(str(tmp_path / "r.png"), small_pair["r"][..., ::-1])

    def files(tag):
        return [f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/{tag}ld.png",
                f"--r_dis_file={tmp_path}/{tag}rd.png", f"--l_disp_pfm={tmp_path}/{tag}l.pfm", f"--r_disp_pfm={tmp_path}/{tag}r.pfm"]

    for extra in ([], ["--use_pp"]):
        p = subprocess.run([EXE] + files("e") + flags + smooth + extra, capture_output=True, timeout=120)
        assert p.returncode != 0 and b"--pp_smooth_lambda" in p.stdout and b"--pp_pfm" in p.stdout, extra
    for bad in (["--pp_smooth_lambda=-1"], smooth + ["--pp_smooth_iters=9"], smooth + ["--pp_smooth_sigma=0"], smooth + ["--pp_smooth_fill_conf=1.5"]):
        p = subprocess.run([EXE] + files("e") + flags + ["--use_pp", "--pp_pfm"] + bad, capture_output=True, timeout=120)
        assert p.returncode != 0 and b"--pp_smooth_iters 1 .. 8" in p.stdout, bad
    assert not os.path.exists(tmp_path / "el.pfm") and not os.path.exists(tmp_path / "eld.png")
    subprocess.check_call([EXE] + files("a") + flags + ["--use_pp", "--pp_pfm"] + smooth, stdout=subprocess.DEVNULL, timeout=120)
    (tmp_path / "list.txt").write_text(" ".join(str(tmp_path / n) for n in ("l.png", "r.png", "cld.png", "crd.png", "cl.pfm", "cr.pfm")) + "\n")
    out = subprocess.check_output([EXE, f"--batch_list={tmp_path}/list.txt", "--use_pp", "--pp_pfm"] + smooth + flags, timeout=120).decode()
    assert "0 failed" in out
    ctx.set_images(small_pair["l"], small_pair["r"])
    ctx.build_cost_grd(16, 35, 5, 0.3)
    ctx.patchmatch(1, seed=31, schedule=capi.SCHED_RASTER)
    plain64 = ctx.postprocess_f64()
    ctx.set_pp_smooth(**PARAMS)
    f64, pp8 = ctx.postprocess_f64(), ctx.postprocess(4)
    assert any(not np.array_equal(plain64[v].astype(np.float32), f64[v].astype(np.float32)) for v in (0, 1))
    for v, side in ((0, "l"), (1, "r")):
        for tag in ("a", "c"):
            assert np.array_equal(pngio.read_png(str(tmp_path / f"{tag}{side}d.png")), pp8[v]), (tag, side)
            assert np.array_equal(_read_pfm(str(tmp_path / f"{tag}{side}.pfm")), f64[v].astype(np.float32)), (tag, side)
