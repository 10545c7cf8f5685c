"""-m gpu: the median filter.  cspm_median_filter_u8_host against the CPU restatement tests/median_ref.py and,
with no restatement in between, against every recorded output of the reference's own filter (tests/golden/refmedian_*.npz);
cspm_median_filter_f64_host bit for bit; the filter as the last step of all four post-processing entries against the restatement
composed with the existing post-processing restatements; the switched-off filter against a fresh context; setter, getter, argument
errors, timing and the CLI.

Shapes are w x h.  The kernel's tile is 64 x 16: 130 x 67 is wider than two tiles plus one and taller than four.  Before a device
result is compared, the restatement alone must show that the case can fail: on every 6-level map of at least 25 pixels the filter
changes between 5 % and 95 % of the pixels, and in both pipeline tests at least one pixel changes and at least one does not.

tests/conftest.py's gpu_ctx does not reset the filter: every test that switches it on switches it off again in a finally (med_ctx)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import median_ref as mr
import pngio
from crossscalepatchmatch_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
SHAPES = [(1, 1), (3, 9), (70, 1), (1, 70), (63, 5), (65, 17), (130, 67)]
RADII = [1, 2, 3, 7]


@pytest.fixture(scope="module", autouse=True)
def _torch_first(_gpu_ctx_session):
    """the host entries need no context, but PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the
    session's context does that, also when this file runs alone"""


@pytest.fixture
def med_ctx(gpu_ctx):
    """the session's context; the filter is off again afterwards whatever the test did"""
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_pp_median(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _levels(rng, shape):
    """a 6-level map 3k + 100, k in 0 .. 5"""
    return (3 * rng.integers(0, 6, shape) + 100).astype(np.uint8)


def _not_vacuous(src, want, what):
    """asserted on the restatement alone: the filter changes between 5 % and 95 % of a 6-level map of at least 25 pixels"""
    if src.shape[0] * src.shape[1] >= 25:
        changed = float(np.mean(np.asarray(want) != np.asarray(src)))
        assert 0.05 <= changed <= 0.95, f"{what}: the filter changes {changed:.3f} of the pixels"


def _u8_strided(src, r, spad, dpad):
    """cspm_median_filter_u8_host with row strides of w * cn + spad / + dpad bytes; the padding bytes of dst must stay as they were"""
    L = capi.load_library()
    h, w = src.shape[:2]
    cn = src.shape[2] if src.ndim == 3 else 1
    row = w * cn
    sbuf = np.full((h, row + spad), 0xEE, np.uint8)
    sbuf[:, :row] = src.reshape(h, row)
    dbuf = np.full((h, row + dpad), 0x5A, np.uint8)
    rc = L.cspm_median_filter_u8_host(0, capi._u8(sbuf), row + spad, w, h, cn, r, capi._u8(dbuf), row + dpad)
    assert rc == 0, L.cspm_last_error(None)
    assert (dbuf[:, row:] == 0x5A).all(), "the filter wrote into the destination's row padding"
    return dbuf[:, :row].reshape(src.shape)


# ---- the u8 host entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_u8_host_entry_against_the_restatement(w, h, cn):
    rng = np.random.default_rng([w, h, cn])
    src = _levels(rng, (h, w) if cn == 1 else (h, w, cn))
    for r in RADII:
        want = mr.median_u8(src, r)
        _not_vacuous(src, want, f"{w}x{h} r={r} cn={cn}")
        got = capi.median_filter(0, src, r)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"{w}x{h} r={r} cn={cn}: {int((got != want).sum())} bytes differ, first {np.argwhere(got != want)[0]}"
        padded = _u8_strided(src, r, 5, 11)
        assert np.array_equal(padded, want), f"{w}x{h} r={r} cn={cn}, padded strides: {int((padded != want).sum())} bytes differ"


def test_u8_host_entry_every_radius_and_channel_count():
    rng = np.random.default_rng(77)
    for cn in (2, 4):
        src = _levels(rng, (21, 70, cn))
        for r in range(1, capi.MEDIAN_MAX_RADIUS + 1):
            want = mr.median_u8(src, r)
            _not_vacuous(src, want, f"cn={cn} r={r}")
            assert np.array_equal(capi.median_filter(0, src, r), want), (cn, r)


@pytest.mark.parametrize("case", mr.all_cases(), ids=[mr.case_name(*c) for c in mr.all_cases()])
def test_u8_host_entry_against_the_recorded_reference(case):
    """device against reference, no restatement in between"""
    z = np.load(mr.golden_path(mr.case_name(*case)))
    src, out, r = z["src"], z["out"], int(z["r"])
    assert not np.array_equal(src, out)
    got = capi.median_filter(0, src, r)
    assert np.array_equal(got, out), f"{int((got != out).sum())} of {out.size} bytes differ from the reference's output"


# ---- the f64 host entry ------------------------------------------------------------------------------------------------------------
def _f64_compare(d, r, what):
    want = mr.median_f64(d, r)
    got = capi.median_filter(0, d, r)
    diff = _bits(got) != _bits(want)
    assert got.dtype == np.float64 and not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"
    return want


@pytest.mark.parametrize("w,h", SHAPES)
def test_f64_host_entry_bit_for_bit(w, h):
    rng = np.random.default_rng([w, h, 64])
    levels = _levels(rng, (h, w))
    holes = levels.astype(np.float64) + rng.choice([0.0, 0.25, -0.5], (h, w))
    holes[rng.random((h, w)) < 0.10] = np.nan
    if w * h > 1:
        holes[h // 2, w // 2] = np.nan
    for r in RADII:
        want = _f64_compare(levels.astype(np.float64), r, f"6 levels {w}x{h} r={r}")
        _not_vacuous(levels, want, f"{w}x{h} r={r}")
        assert np.array_equal(want, mr.median_u8(levels, r).astype(np.float64))
        want = _f64_compare(holes, r, f"10 % NaNs {w}x{h} r={r}")
        assert np.array_equal(np.isnan(want), np.isnan(holes))


def test_f64_host_entry_hand_cases():
    inf = np.inf
    d = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, np.nan]])
    got = capi.median_filter(0, d, 1)
    assert got[1, 1] == 4.0 and got[0, 0] == 2.0 and got[1, 2] == 5.0 and np.isnan(got[2, 2])  # NaN taps do not vote; the lower median
    _f64_compare(d, 1, "3x3 with a NaN")
    d = np.full((5, 5), 2.5)
    payload = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF], np.uint64).view(np.float64)
    d[1, 1], d[2, 3], d[4, 4] = payload
    got = capi.median_filter(0, d, 2)
    assert np.array_equal(_bits(got)[[1, 2, 4], [1, 3, 4]], payload.view(np.uint64)) and (got[~np.isnan(d)] == 2.5).all()  # a NaN centre stays, bit-equal
    alone = np.full((3, 3), np.nan)
    assert np.array_equal(_bits(capi.median_filter(0, alone, 1)), _bits(alone))
    got = capi.median_filter(0, np.array([[-0.0, 0.0, -0.0]]), 1)
    assert np.array_equal(_bits(got), _bits(np.array([[-0.0, -0.0, -0.0]])))
    got = capi.median_filter(0, np.array([[0.0, -0.0, 0.0]]), 1)
    assert np.array_equal(_bits(got), _bits(np.array([[0.0, 0.0, 0.0]])))
    got = capi.median_filter(0, np.array([[-inf, inf, -inf, 3.0, -inf]]), 1)
    assert np.array_equal(got, np.array([[-inf, -inf, 3.0, -inf, -inf]]))
    rng = np.random.default_rng(9)
    wild = rng.integers(0, 1 << 63, (33, 70), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (33, 70), dtype=np.uint64)  # every bit pattern, NaNs and subnormals among them
    for r in (1, 2, 5):
        _f64_compare(wild.view(np.float64), r, f"random bit patterns r={r}")


# ---- inside the post-processing ----------------------------------------------------------------------------------------------------
def _run(ctx, pair, seed):
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 35, 5, 0.3)
    ctx.patchmatch(1, seed=seed, schedule=capi.SCHED_RASTER)


def _changed_and_kept(plain, filtered, what):
    """asserted on the restatement alone"""
    diff = np.concatenate([(_bits(p) != _bits(f)).ravel() for p, f in zip(plain, filtered)])
    assert diff.any() and not diff.all(), f"{what}: the filter changes {int(diff.sum())} of {diff.size} pixels"


def test_f64_pipeline_and_its_device_variant(med_ctx, small_pair):
    """64 x 48 after one iteration: cspm_postprocess_f64 with r = 2 == pp_sub_ref's steps, then M64; the masks are those of r = 0"""
    import torch
    l, r, D, w, h = (small_pair[k] for k in ("l", "r", "max_dis", "w", "h"))
    _run(med_ctx, small_pair, 5)
    abc = [med_ctx.get_planes(v)[0][..., 3:6] for v in (0, 1)]
    plain = mr.postprocess_f64_median(abc[0], abc[1], l, r, D, 0)
    want = mr.postprocess_f64_median(abc[0], abc[1], l, r, D, 2)
    _changed_and_kept(plain[:2], want[:2], "f64 pipeline")
    off = med_ctx.postprocess_f64(valid=True)
    med_ctx.set_pp_median(2)
    got = med_ctx.postprocess_f64(valid=True)
    outs = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    med_ctx.postprocess_f64_device(outs[0].data_ptr(), outs[1].data_ptr())
    med_ctx.synchronize()
    for v in (0, 1):
        diff = _bits(got[v]) != _bits(want[v])
        assert not diff.any(), f"view {v}: {int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"
        assert np.array_equal(got[2 + v], want[2 + v]) and np.array_equal(got[2 + v], off[2 + v]), f"view {v}: the filter changed a mask"
        assert np.array_equal(_bits(off[v]), _bits(plain[v]))
        assert np.array_equal(_bits(outs[v].cpu().numpy()), _bits(want[v])), f"view {v}: device-resident output"


def test_8_bit_pipeline_and_its_device_variant(med_ctx, small_pair):
    """cspm_postprocess with r = 2 == the oracle's PostProcessing on the oracle's own run, then M8"""
    import torch
    l, r, D, w, h = (small_pair[k] for k in ("l", "r", "max_dis", "w", "h"))
    _run(med_ctx, small_pair, 5)
    pc = po.PlaneCost(l, r, D, 35, 5, 0.3)
    pm = po.PatchMatch(l, r, D, 4)
    pm.run(1, pc, False, seed=5, schedule=po.SCHED_RASTER, sum_order=po.SUM_DEVICE)
    plain = mr.postprocess_u8_median(pm, 0)
    want = mr.postprocess_u8_median(pm, 2)
    diff = np.concatenate([(p != f).ravel() for p, f in zip(plain, want)])
    assert diff.any() and not diff.all(), f"8-bit pipeline: the filter changes {int(diff.sum())} of {diff.size} pixels"
    off = med_ctx.postprocess(4)
    med_ctx.set_pp_median(2)
    got = med_ctx.postprocess(4)
    outs = [torch.zeros((h, w), dtype=torch.uint8, device="cuda:0") for _ in (0, 1)]
    med_ctx.postprocess_device(4, outs[0].data_ptr(), outs[1].data_ptr())
    med_ctx.synchronize()
    for v in (0, 1):
        assert np.array_equal(off[v], plain[v])
        assert np.array_equal(got[v], want[v]), f"view {v}: {int((got[v] != want[v]).sum())} pixels differ"
        assert np.array_equal(outs[v].cpu().numpy(), want[v]), f"view {v}: device-resident output"
    again = med_ctx.postprocess(4)  # the second buffers and the maps have changed places twice by now
    assert all(np.array_equal(again[v], want[v]) for v in (0, 1))


def test_filter_off_is_a_fresh_context(med_ctx, small_pair):
    import crossscalepatchmatch_amd as cs
    fresh = cs.StereoContext(0)
    try:
        _run(fresh, small_pair, 3)
        assert fresh.get_pp_median() == 0
        want8, want64 = fresh.postprocess(4), fresh.postprocess_f64(valid=True)
    finally:
        fresh.close()
    _run(med_ctx, small_pair, 3)
    med_ctx.set_pp_median(2)
    on8, on64 = med_ctx.postprocess(4), med_ctx.postprocess_f64(valid=True)
    med_ctx.set_pp_median(0)
    got8, got64 = med_ctx.postprocess(4), med_ctx.postprocess_f64(valid=True)
    for v in (0, 1):
        assert np.array_equal(got8[v], want8[v])
        assert np.array_equal(_bits(got64[v]), _bits(want64[v])) and np.array_equal(got64[2 + v], want64[2 + v])
    assert any(not np.array_equal(on8[v], want8[v]) for v in (0, 1)) and any(not np.array_equal(_bits(on64[v]), _bits(want64[v])) for v in (0, 1))


def test_setter_getter_and_argument_errors(med_ctx):
    ctx, L = med_ctx, med_ctx.L
    assert ctx.get_pp_median() == 0
    for r in range(0, capi.MEDIAN_MAX_RADIUS + 1):
        ctx.set_pp_median(r)
        assert ctx.get_pp_median() == r
    for r in (-1, capi.MEDIAN_MAX_RADIUS + 1, 1 << 20):
        assert L.cspm_set_pp_median(ctx.p, r) == -1, r
    assert ctx.get_pp_median() == capi.MEDIAN_MAX_RADIUS
    ctx.set_pp_median(0)
    value = C.c_int(5)
    assert L.cspm_set_pp_median(None, 1) == -1 and L.cspm_get_pp_median(None, C.byref(value)) == -1 and L.cspm_get_pp_median(ctx.p, None) == -1
    src = np.full((6, 8 * 3), 7, np.uint8)
    dst = np.zeros_like(src)
    sp, dp = capi._u8(src), capi._u8(dst)
    u8 = L.cspm_median_filter_u8_host
    assert u8(0, sp, 24, 8, 6, 3, 2, dp, 24) == 0 and (dst == 7).all()
    for r in (0, -1, capi.MEDIAN_MAX_RADIUS + 1):
        assert u8(0, sp, 24, 8, 6, 3, r, dp, 24) == -1, r
    for cn in (0, 5, -1):
        assert u8(0, sp, 24, 8, 6, cn, 2, dp, 24) == -1, cn
    assert u8(0, None, 24, 8, 6, 3, 2, dp, 24) == -1 and u8(0, sp, 24, 8, 6, 3, 2, None, 24) == -1
    assert u8(0, sp, 23, 8, 6, 3, 2, dp, 24) == -1 and u8(0, sp, 24, 8, 6, 3, 2, dp, 23) == -1
    assert b"stride" in L.cspm_last_error(None)
    assert u8(0, sp, 24, 8, 6, 3, 2, sp, 24) == -1                                                       # src == dst
    assert u8(0, sp, 24, 0, 6, 3, 2, dp, 24) == -1 and u8(0, sp, 24, 8, 0, 3, 2, dp, 24) == -1
    d = np.zeros((4, 4))
    o = np.ones((4, 4))
    f64 = L.cspm_median_filter_f64_host
    assert f64(0, capi._dp(d), 4, 4, 1, capi._dp(o)) == 0 and not o.any()
    for r in (0, -1, capi.MEDIAN_MAX_RADIUS + 1):
        assert f64(0, capi._dp(d), 4, 4, r, capi._dp(o)) == -1, r
    assert f64(0, None, 4, 4, 1, capi._dp(o)) == -1 and f64(0, capi._dp(d), 4, 4, 1, None) == -1 and f64(0, capi._dp(d), 4, 4, 1, capi._dp(d)) == -1
    assert f64(0, capi._dp(d), 0, 4, 1, capi._dp(o)) == -1
    with pytest.raises(TypeError):
        capi.median_filter(0, np.zeros((4, 4), np.float32), 1)


def test_timing_counts_the_filter_under_post(med_ctx, small_pair):
    _run(med_ctx, small_pair, 3)
    k_post = capi.K_NAMES.index("post")

    def launches(fn):
        med_ctx.L.cspm_enable_timing(med_ctx.p, 1)
        try:
            med_ctx.L.cspm_reset_timing(med_ctx.p)
            fn()
            n, ms = C.c_longlong(), C.c_double()
            assert med_ctx.L.cspm_get_timing(med_ctx.p, k_post, C.byref(n), C.byref(ms), None) == 0
            return n.value, ms.value
        finally:
            med_ctx.L.cspm_enable_timing(med_ctx.p, 0)

    off8, off64 = launches(lambda: med_ctx.postprocess(4)), launches(lambda: med_ctx.postprocess_f64())
    med_ctx.set_pp_median(2)
    on8, on64 = launches(lambda: med_ctx.postprocess(4)), launches(lambda: med_ctx.postprocess_f64())
    print(f"CSPM_K_POST (launches, ms): 8-bit off {off8} on {on8}; f64 off {off64} on {on64}")
    assert on8[0] == off8[0] + 1 and on64[0] == off64[0] + 1 and on8[1] > 0.0 and on64[1] > 0.0


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_pp_median(med_ctx, small_pair, tmp_path):
    flags = ["--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--seed=31", "--iters=1"]
    pngio.write_png(str(tmp_path / "l.png"), small_pair["l"][..., ::-1])
    pngio.write_png(str(tmp_path / "r.png"), small_pair["r"][..., ::-1])

    def files(tag):
        return [f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/{tag}ld.png",
                f"--r_dis_file={tmp_path}/{tag}rd.png", f"--l_disp_pfm={tmp_path}/{tag}l.pfm", f"--r_disp_pfm={tmp_path}/{tag}r.pfm"]

    p = subprocess.run([EXE] + files("e") + flags + ["--pp_median=2"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--pp_median" in p.stdout and b"--use_pp" in p.stdout
    p = subprocess.run([EXE] + files("e") + flags + ["--use_pp", "--pp_median=8"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--pp_median" in p.stdout and b"0 .. 7" in p.stdout
    assert not os.path.exists(tmp_path / "el.pfm") and not os.path.exists(tmp_path / "eld.png")
    subprocess.check_call([EXE] + files("a") + flags + ["--use_pp", "--pp_median=2", "--pp_pfm"], stdout=subprocess.DEVNULL, timeout=120)
    subprocess.check_call([EXE] + files("b") + flags + ["--use_pp", "--pp_median=2"], stdout=subprocess.DEVNULL, timeout=120)
    (tmp_path / "list.txt").write_text(" ".join(str(tmp_path / n) for n in ("l.png", "r.png", "cld.png", "crd.png", "cl.pfm", "cr.pfm")) + "\n")
    out = subprocess.check_output([EXE, f"--batch_list={tmp_path}/list.txt", "--use_pp", "--pp_median=2", "--pp_pfm"] + flags, timeout=120).decode()
    assert "0 failed" in out
    med_ctx.set_images(small_pair["l"], small_pair["r"])
    med_ctx.build_cost_grd(16, 35, 5, 0.3)
    med_ctx.patchmatch(1, seed=31, schedule=capi.SCHED_RASTER)
    plain8 = med_ctx.postprocess(4)
    med_ctx.set_pp_median(2)
    f64, pp8 = med_ctx.postprocess_f64(), med_ctx.postprocess(4)
    assert any(not np.array_equal(plain8[v], pp8[v]) for v in (0, 1))
    for v, side in ((0, "l"), (1, "r")):
        for tag in ("a", "b", "c"):
            assert np.array_equal(pngio.read_png(str(tmp_path / f"{tag}{side}d.png")), pp8[v]), (tag, side)
        for tag in ("a", "c"):  # --pp_pfm: the PFM maps are the filtered sub-pixel maps
            assert np.array_equal(_read_pfm(str(tmp_path / f"{tag}{side}.pfm")), f64[v].astype(np.float32)), (tag, side)
        assert np.array_equal(_read_pfm(str(tmp_path / f"b{side}.pfm")), med_ctx.disparity_f64(v).astype(np.float32))  # without it: the raw plane disparities
