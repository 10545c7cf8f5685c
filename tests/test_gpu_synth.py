"""View synthesis on the GPU (include/cspm.h "view synthesis") held to tests/synth_ref.py bit for bit on the image,
the disparity map (NaN positions included, any NaN payload) and the mask: cspm_synthesize_host over the wave and chunk seams and the
widest row the kernel's LDS layout admits, every t / views / fill, ties, empty rows, output memory; cspm_synthesize /
cspm_synthesize_device on the stored field after a PatchMatch run (RAW, PP with filters); the error returns, the timing counts, the host
layer and cspm_main --synth_*."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pngio
import synth_ref as sr
from crossscalepatchmatch_amd import capi
from test_gpu_warm_start import _build_helper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, BLOCK, MAXW = 64, 256, 6784  # the fill's chunk, kSynthBlock, kSynthMaxWidth (csrc/cspm_synth.h): a row is not segmented
assert MAXW == capi.SYNTH_MAX_WIDTH
# the kernel does not segment rows: beyond the issue's shapes, the widest row its LDS layout admits (wider is CSPM_ERR_ARG, tested below),
# and rows around a multiple of the workgroup and of the Middlebury width
SHAPES = sr.SHAPES + [(BLOCK * 4 + 1, 2), (3000, 2), (MAXW, 2)]
SEEN = set()  # mask values met over the module (test_zz_all_mask_values_occurred)


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the device-variant test needs torch tensors, and
    the host-entry tests of this module would otherwise load the library first"""
    yield


def _same(got, want, what):
    for name in ("bgr", "disp", "mask"):
        if name in got:
            assert sr.same_bits(got[name], want[name]), f"{what}: {name} differs in {int(np.sum(got[name] != want[name]))} places"
    if "mask" in got:
        SEEN.update(int(m) for m in np.unique(got["mask"]))


def _check(t, D, V, A, I, what="", **params):
    got = capi.synthesize_host(t, D, I, V, A, **params)
    want = sr.synthesize(t, D, V, A, I, **params)
    _same(got, want, f"{what} t {t} {params}")
    return got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_shapes(shape):
    w, h = shape
    D, V, A, I = sr.shape_case(shape)
    for t in sr.TS:
        for views in (1, 2, 3):
            _, want = _check(t, D, V, A, I, f"{w}x{h}", views=views, fill=1)
            frac = float(np.mean(want["holes"] == 0))
            assert w * h < 64 or 0.02 <= frac <= 0.98, (shape, t, views, frac)  # the reference alone gives a non-trivial answer
            _check(t, D, V, A, I, f"{w}x{h}", views=views, fill=0)


def test_wider_than_the_lds_layout_is_refused():
    """a row is not segmented: MAXW pixels work (test_host_entry_shapes), MAXW + 1 is CSPM_ERR_ARG before a device is opened"""
    w = MAXW + 1
    D = np.ones((1, w))
    I = np.zeros((1, w, 3), np.uint8)
    with pytest.raises(capi.CspmError, match="wider"):
        capi.synthesize_host(0.5, (D, D), (I, I))


@pytest.mark.parametrize("kw", [dict(max_stretch=1.0), dict(max_stretch=math.inf, merge_diff=0.0), dict(merge_diff=math.inf),
                                dict(max_stretch=1.25, merge_diff=3.5), dict(max_stretch=13.0)], ids=str)
def test_parameters_and_optional_inputs(kw):
    w, h = 130, 11
    D, V, A, I = sr.random_case(w, h, 91)
    for t in (0.0, 0.3, 1.0):
        _check(t, D, V, A, I, **kw)
        _check(t, D, (None, None), A, I, **kw)
        _check(t, D, V, (None, None), I, **kw)
        _check(t, D, (V[0], None), (None, A[1]), I, **kw)
    _check(0.6, (D[0], None), (V[0], None), (A[0], None), (I[0], None), views=1, **kw)  # a view `views` does not name may be missing
    _check(0.6, (None, D[1]), (None, V[1]), (None, A[1]), (None, I[1]), views=2, **kw)


def test_ties_are_decided_by_the_smallest_source_x():
    D, A, I = sr.tie_case()
    ties = []
    want = sr.synthesize(1.0, (D, None), (None, None), (A, None), (I, None), views=1, fill=0, ties=ties)
    assert ties[0] >= len(sr.TIE_PLANES)
    for _ in range(3):  # the same answer whatever order the lanes arrive in
        _same(capi.synthesize_host(1.0, (D, None), (I, None), slope_a=(A, None), views=1, fill=0), want, "ties")


def test_shifts_beyond_the_image_and_empty_rows():
    w, h = 70, 5
    D, V, A, I = sr.random_case(w, h, 14)
    far = [np.random.default_rng(v).uniform(w + 1.0, 3.0 * w, (h, w)) for v in (0, 1)]
    for views, t in ((1, 1.0), (2, 0.0)):
        got, _ = _check(t, far, (None, None), (None, None), I, "far", views=views)
        assert np.all(got["mask"] == 0) and np.all(got["bgr"] == 0) and np.all(np.isnan(got["disp"]))
    for v in (0, 1):
        V[v][1, :] = 0                       # a row with no usable pixel
        V[v][3, :] = 0
        V[v][3, 41] = 1                      # a row with a single usable pixel
        D[v][3, 41], A[v][3, 41] = 4.0, 0.1
    for fill in (0, 1):
        got, _ = _check(0.5, D, V, A, I, "rows", fill=fill)
        assert np.all(got["mask"][1] == 0) and np.all(got["bgr"][1] == 0) and np.all(np.isnan(got["disp"][1]))
        assert np.sum((got["mask"][3] != 0) & (got["mask"][3] != 4)) in (1, 2)
        assert fill == 0 or np.all(got["mask"][3] != 0)
    everything = [np.zeros((h, w), np.uint8)] * 2
    got, _ = _check(0.5, D, everything, A, I, "no pixel at all")
    assert np.all(got["mask"] == 0)


def test_known_answers_on_the_device():
    w, h = 67, 9
    rng = np.random.default_rng(5)
    D = rng.uniform(0.0, 40.0, (h, w))
    A = rng.uniform(-0.3, 0.3, (h, w))
    I = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    left = capi.synthesize_host(0.0, (D, None), (I, None), slope_a=(A, None), views=1)
    assert np.array_equal(left["bgr"], I) and sr.same_bits(left["disp"], D) and np.all(left["mask"] == 1)
    right = capi.synthesize_host(1.0, (None, D), (None, I), slope_a=(None, A), views=2)
    assert np.array_equal(right["bgr"], I) and sr.same_bits(right["disp"], D) and np.all(right["mask"] == 2)
    Dc = np.full((h, w), 8.0)
    mid = capi.synthesize_host(0.5, (Dc, None), (I, None), views=1, fill=0)
    assert np.array_equal(mid["bgr"][:, :w - 4], I[:, 4:]) and np.all(mid["mask"][:, w - 4:] == 0)


def test_output_memory():
    """outputs one at a time and all together; unrequested buffers and the bytes between 3 * w and the output stride stay untouched; a
    padded input stride is read correctly"""
    w, h = 65, 9
    D, V, A, I = sr.random_case(w, h, 23)
    want = sr.synthesize(0.5, D, V, A, I)
    pad = 3 * w + 13
    wide = [np.full((h, pad), 0xEE, np.uint8) for _ in (0, 1)]
    Ip = []
    for v in (0, 1):
        wide[v][:, :3 * w] = I[v].reshape(h, 3 * w)
        Ip.append(wide[v][:, :3 * w].reshape(h, w, 3))
        assert Ip[v].strides == (pad, 3, 1)
    for pick in (("bgr",), ("disp",), ("mask",), ("bgr", "disp", "mask"), ()):
        buf = np.full((h, pad + 7), 0xA5, np.uint8)
        out = {"bgr": buf[:, :3 * w].reshape(h, w, 3), "disp": np.full((h, w), 7.5), "mask": np.full((h, w), 77, np.uint8)}
        assert out["bgr"].strides == (pad + 7, 3, 1) and np.shares_memory(out["bgr"], buf)
        keep = dict(out)
        got = capi.synthesize_host(0.5, D, Ip, V, A, outputs=pick, out=out)
        assert set(got) == set(pick)
        _same(got, want, f"outputs {pick}")
        assert np.all(buf[:, 3 * w:] == 0xA5), "bytes beyond 3 * w of an output row were written"
        if "bgr" not in pick:
            assert np.all(buf == 0xA5)
        if "disp" not in pick:
            assert np.all(keep["disp"] == 7.5)
        if "mask" not in pick:
            assert np.all(keep["mask"] == 77)


# ---- the context entries ---------------------------------------------------------------------------------------------------------------

W, H, MAXD = 80, 56, 16


@pytest.fixture(scope="module")
def pair():
    from crossscalepatchmatch_amd import synth
    l, r, _, _ = synth.make_pair(W, H, MAXD, regions=3, seed=21)
    return l, r


def _run(ctx, pair):
    ctx.set_images(pair[0], pair[1])
    ctx.build_cost_grd(MAXD, 9, 3, 0.3)  # cross-scale: three levels
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(2, seed=5)
    return [ctx.level_image(v, 0) for v in (0, 1)]


def _raw_inputs(ctx):
    return [ctx.disparity_f64(v) for v in (0, 1)], [ctx.get_planes(v)[0][..., 3] for v in (0, 1)]


def test_context_raw_and_pp(gpu_ctx, pair):
    ctx = gpu_ctx
    I = _run(ctx, pair)
    try:
        D, A = _raw_inputs(ctx)
        for t in (0.0, 0.5, 1.0):
            for kw in (dict(), dict(views=1, fill=0), dict(views=2, max_stretch=1.5)):
                first = ctx.synthesize(t, capi.GEOM_RAW, **kw)
                _same(first, sr.synthesize(t, D, (None, None), A, I, **kw), f"RAW t {t} {kw}")
                _same(ctx.synthesize(t, capi.GEOM_RAW, **kw), first, "a second call (the scratch is reused)")
        back = ctx.synthesize(0.0, capi.GEOM_RAW, views=1)
        assert np.array_equal(back["bgr"], I[0]) and np.all(back["mask"] == 1), "t = 0 from view 0 alone is the left image"
        for speckle, median in ((0, 0), (12, 1)):
            ctx.set_pp_speckle(speckle, 1.0)
            ctx.set_pp_median(median)
            maps = ctx.postprocess_f64(valid=True)
            Dp, Vp = [maps[0], maps[1]], [maps[2], maps[3]]
            assert all(0 < v.sum() < v.size for v in Vp)
            Ap = [np.where(Vp[v] != 0, A[v], 0.0) for v in (0, 1)]
            for t in (0.25, 1.0):
                for kw in (dict(), dict(views=1, fill=0)):
                    _same(ctx.synthesize(t, capi.GEOM_PP, **kw), sr.synthesize(t, Dp, (None, None), Ap, I, **kw), f"PP {speckle} {median} t {t} {kw}")
    finally:
        ctx.set_pp_speckle(0)
        ctx.set_pp_median(0)


def test_device_variant_equals_host_variant(gpu_ctx, pair):
    import torch
    ctx = gpu_ctx
    _run(ctx, pair)
    stride = 3 * W + 16
    for source in (capi.GEOM_RAW, capi.GEOM_PP):
        want = ctx.synthesize(0.5, source, merge_diff=0.5)
        bgr = torch.full((H, stride), 0xA5, dtype=torch.uint8, device="cuda")
        disp = torch.full((H, W), 7.0, dtype=torch.float64, device="cuda")
        mask = torch.full((H, W), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.synthesize_device(0.5, source, d_bgr=bgr.data_ptr(), out_stride=stride, d_disp=disp.data_ptr(), d_mask=mask.data_ptr(), merge_diff=0.5)
        ctx.synchronize()
        rows = bgr.cpu().numpy()
        got = dict(bgr=rows[:, :3 * W].reshape(H, W, 3), disp=disp.cpu().numpy(), mask=mask.cpu().numpy())
        _same(got, want, f"device variant, source {source}")
        assert np.all(rows[:, 3 * W:] == 0xA5)
        disp.fill_(7.0)
        torch.cuda.synchronize()
        ctx.synthesize_device(0.5, source, d_mask=mask.data_ptr(), merge_diff=0.5)  # the mask alone
        ctx.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want["mask"]) and bool((disp == 7.0).all())


def test_timing_counts(gpu_ctx, pair):
    ctx = gpu_ctx
    _run(ctx, pair)
    n = W * H
    ctx.synchronize()
    ctx.enable_timing(True)
    try:
        ctx.reset_timing()
        ctx.synthesize(0.5, capi.GEOM_RAW)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 0 and t["init"]["launches"] == 0
        ctx.synthesize(0.5, capi.GEOM_RAW, views=1, outputs=("mask",))
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (2, 2 * n)
        ctx.reset_timing()
        ctx.synthesize(0.5, capi.GEOM_PP)
        t = ctx.timing()
        assert (t["misc"]["launches"], t["misc"]["evals"]) == (1, n) and t["post"]["launches"] == 1
    finally:
        ctx.enable_timing(False)


def test_error_returns(small_pair):
    ERR_ARG, ERR_STATE = -1, -3
    L = capi.load_library()
    ctx = capi.StereoContext(0)
    w, h = small_pair["w"], small_pair["h"]
    img = np.zeros((h, w, 3), np.uint8)
    dis = np.zeros((h, w))
    msk = np.zeros((h, w), np.uint8)

    def rc(t=0.5, source=capi.GEOM_RAW, params=capi.synth_params(), device=False, stride=3 * w, want_bgr=True):
        fn = L.cspm_synthesize_device if device else L.cspm_synthesize
        pp = C.byref(params) if params is not None else None
        if device:
            return fn(ctx.p, source, pp, t, None, stride, None, None)  # nothing requested: the checks and the launch, no buffer
        return fn(ctx.p, source, pp, t, capi._u8(img) if want_bgr else None, stride, capi._dp(dis), capi._u8(msk))

    try:
        for dev in (False, True):
            assert rc(device=dev) == ERR_STATE                                  # no images
            assert rc(t=2.0, device=dev) == ERR_ARG                             # the arguments come first
        ctx.set_images(small_pair["l"], small_pair["r"])
        for dev in (False, True):
            assert rc(device=dev) == ERR_STATE                                  # no plane field
        ctx.set_planes(0, capi.disparity_planes(np.full((h, w), 4.0)), np.zeros((h, w)))
        ctx.set_planes(1, capi.disparity_planes(np.full((h, w), 4.0)), np.zeros((h, w)))
        for dev in (False, True):
            assert rc(device=dev) == 0                                          # RAW needs no cost object
            assert rc(source=capi.GEOM_PP, device=dev) == ERR_STATE             # PP does
            assert rc(source=2, device=dev) == ERR_ARG and rc(source=-1, device=dev) == ERR_ARG
            for t in (math.nan, -0.001, 1.001, math.inf):
                assert rc(t=t, device=dev) == ERR_ARG, t
            assert rc(t=0.0, device=dev) == 0 and rc(t=1.0, device=dev) == 0
            for bad in (dict(views=0), dict(views=4), dict(max_stretch=0.99), dict(max_stretch=math.nan), dict(merge_diff=-0.1), dict(merge_diff=math.nan)):
                assert rc(params=capi.synth_params(**bad), device=dev) == ERR_ARG, bad
            assert rc(params=capi.synth_params(max_stretch=math.inf, merge_diff=math.inf), device=dev) == 0
            assert rc(params=None, device=dev) == 0                             # NULL parameters are the defaults
        assert rc(stride=3 * w - 1) == ERR_ARG and rc(stride=3 * w - 1, want_bgr=False) == 0  # the stride matters with an image only
        # two constant fields that agree: at t = 0.5 view 0 lands two columns to the left, view 1 two to the right
        assert np.all(msk[:, :2] == 1) and np.all(msk[:, 2:w - 2] == 3) and np.all(msk[:, w - 2:] == 2) and np.all(dis == 4.0)
        ctx.build_cost_grd(small_pair["max_dis"], 9, 0, 0.0)
        for dev in (False, True):
            assert rc(source=capi.GEOM_PP, device=dev) == 0
        ctx.synchronize()
    finally:
        ctx.close()
    # the host entry (that its arguments are checked before a device is opened is shown where there is none: test_synth_ref.py)
    p = capi.synth_params()
    D = np.ones((h, w))
    view = capi.SynthView(capi._dp(D), None, None, capi._u8(img), 3 * w)
    short = capi.SynthView(capi._dp(D), None, None, capi._u8(img), 3 * w - 1)
    nodisp = capi.SynthView(None, None, None, capi._u8(img), 3 * w)
    noimg = capi.SynthView(capi._dp(D), None, None, None, 3 * w)

    def host(t=0.5, params=p, v0=view, v1=view, ww=w, hh=h, stride=3 * w, bgr=True):
        return L.cspm_synthesize_host(0, C.byref(params) if params is not None else None, t, C.byref(v0) if v0 is not None else None,
                                      C.byref(v1) if v1 is not None else None, ww, hh, capi._u8(img) if bgr else None, stride, None, None)

    assert host() == 0 and host(params=None) == 0
    for t in (math.nan, -0.5, 1.5):
        assert host(t=t) == ERR_ARG
    for bad in (dict(views=0), dict(views=4), dict(max_stretch=0.5), dict(max_stretch=math.nan), dict(merge_diff=-1.0), dict(merge_diff=math.nan)):
        assert host(params=capi.synth_params(**bad)) == ERR_ARG, bad
    assert host(v0=None) == ERR_ARG and host(v1=None) == ERR_ARG and host(v0=nodisp) == ERR_ARG and host(v1=noimg) == ERR_ARG
    assert host(v1=None, params=capi.synth_params(views=1)) == 0  # an unnamed view may be missing
    assert host(v0=nodisp, params=capi.synth_params(views=2)) == 0
    assert host(ww=0) == ERR_ARG and host(hh=0) == ERR_ARG and host(ww=1 << 12, hh=1 << 19) == ERR_ARG
    assert host(ww=MAXW + 1, hh=1, stride=3 * (MAXW + 1)) == ERR_ARG
    assert host(v0=short) == ERR_ARG and host(v1=short) == ERR_ARG and host(stride=3 * w - 1) == ERR_ARG
    assert host(stride=0, bgr=False) == 0
    assert L.cspm_synth_default_params(None) == ERR_ARG
    assert (p.views, p.fill, p.max_stretch, p.merge_diff) == (3, 1, 4.0, 1.0)


# ---- the host layer and the command line -----------------------------------------------------------------------------------------------

def test_host_layer_synthesize():
    exe = _build_helper("synth_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "synth_check ok" in r.stdout, r.stdout + r.stderr


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(t) for t in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_synth_flags(gpu_ctx, small_pair, tmp_path):
    """cspm_main --synth_t --synth_png --synth_dis_pfm (one pair, RAW and --use_pp) and the batch list's columns 7 and 8 == the C-ABI
    sequence; the flag conflicts are refused before a device is opened"""
    exe = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    l, r = small_pair["l"], small_pair["r"]
    pngio.write_png(str(tmp_path / "l.png"), l[..., ::-1])  # files are RGB, imread returns BGR
    pngio.write_png(str(tmp_path / "r.png"), r[..., ::-1])
    match = ["--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--iters=1", "--seed=9", "--quiet=true"]
    base = [exe, f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png"] + match
    png, pfm = tmp_path / "mid.png", tmp_path / "mid.pfm"
    for bad in ([f"--synth_png={png}"], ["--synth_t=0.5"], ["--synth_t=1.5", f"--synth_png={png}"], ["--synth_t=0.5", f"--synth_png={png}", "--synth_views=4"],
                ["--synth_t=0.5", f"--synth_png={png}", "--synth_max_stretch=0.5"], ["--synth_t=0.5", f"--synth_png={png}", f"--batch_list={png}"]):
        res = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "Error" in res.stdout, (bad, res.stdout)
    kw = dict(views=3, max_stretch=2.0, merge_diff=0.5)
    flags = ["--synth_t=0.25", f"--synth_png={png}", f"--synth_dis_pfm={pfm}", "--synth_max_stretch=2", "--synth_merge_diff=0.5"]
    want = {}
    gpu_ctx.set_images(l, r)
    gpu_ctx.build_cost_grd(16, 35, 5, 0.3)
    gpu_ctx.set_pp_speckle(0)
    gpu_ctx.set_pp_median(0)
    gpu_ctx.patchmatch(1, seed=9, schedule=0)
    want[False] = gpu_ctx.synthesize(0.25, capi.GEOM_RAW, **kw)
    want[True] = gpu_ctx.synthesize(0.25, capi.GEOM_PP, **kw)
    want["nofill"] = gpu_ctx.synthesize(0.25, capi.GEOM_RAW, fill=0, views=1)
    for use_pp in (False, True):
        res = subprocess.run(base + flags + [f"--use_pp={'true' if use_pp else 'false'}"], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert np.array_equal(pngio.read_png(str(png))[..., ::-1], want[use_pp]["bgr"]), use_pp
        assert sr.same_bits(_read_pfm(pfm), want[use_pp]["disp"].astype(np.float32)), use_pp
    # per pair under --batch_list: the outputs are the list's columns 7 and 8, `-` skips an optional column
    (tmp_path / "list.txt").write_text(f"{tmp_path}/l.png {tmp_path}/r.png {tmp_path}/bl.png {tmp_path}/br.png - - {tmp_path}/b_mid.png {tmp_path}/b_mid.pfm\n"
                                       f"{tmp_path}/l.png {tmp_path}/r.png {tmp_path}/cl.png {tmp_path}/cr.png - - {tmp_path}/c_mid.ppm\n")
    res = subprocess.run([exe, f"--batch_list={tmp_path}/list.txt", "--synth_t=0.25", "--synth_fill=false", "--synth_views=1"] + match,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "0 failed" in res.stdout, res.stdout + res.stderr
    assert np.array_equal(pngio.read_png(str(tmp_path / "b_mid.png"))[..., ::-1], want["nofill"]["bgr"])
    assert sr.same_bits(_read_pfm(tmp_path / "b_mid.pfm"), want["nofill"]["disp"].astype(np.float32))
    assert np.array_equal(pngio.read_pnm(str(tmp_path / "c_mid.ppm"))[..., ::-1], want["nofill"]["bgr"])
    assert not os.path.exists(tmp_path / "-")
    assert (want["nofill"]["mask"] == 0).any()


def test_zz_all_mask_values_occurred():
    """the module's comparisons covered holes, either view alone, blended and filled pixels (runs last in the file)"""
    assert SEEN == {0, 1, 2, 3, 4}, SEEN
