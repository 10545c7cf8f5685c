"""-m gpu: the speckle filter.  cspm_filter_speckles_host against the CPU restatement tests/speckle_ref.py
(masks and sizes with array_equal), the filter inside all four post-processing entries against the restatement composed with
pp_sub_ref's steps (bit for bit), the switched-off filter against a fresh context, argument errors and the CLI.

Shapes are w x h.  Two preconditions are asserted on the restatement alone before a random map is compared: between 5 % and 95 % of the
valid pixels are removed, and a component straddles the boundary between columns 63 and 64.  The first cannot hold for the one-pixel
image and the second needs w > 64, so they are asserted for every shape on which they can hold; the comparison runs on all six."""
import os
import subprocess

import numpy as np
import pytest

import pngio
import pp_sub_ref as ps
import speckle_ref as sr
from crossscalepatchmatch_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
SHAPES = [(1, 1), (70, 1), (1, 70), (63, 5), (65, 17), (130, 67)]  # w x h: wave (64 lanes), tile (64 x 16) and launch (256) borders
INF = float("inf")


@pytest.fixture
def spk_ctx(gpu_ctx):
    """the session's context; the filter is off again afterwards whatever the test did"""
    yield gpu_ctx
    gpu_ctx.set_pp_speckle(0, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _compare(d, valid, max_size, max_diff, what):
    want = sr.speckle_filter(d, valid, max_size, max_diff)
    got = capi.filter_speckles(0, d, valid, max_size, max_diff)
    assert np.array_equal(got[1], want[1]), f"{what}: sizes differ at {int((got[1] != want[1]).sum())} pixels, first {np.argwhere(got[1] != want[1])[0]}"
    assert np.array_equal(got[0], want[0]), f"{what}: masks differ at {int((got[0] != want[0]).sum())} pixels"
    return want


# ---- the filter alone --------------------------------------------------------------------------------------------------------------
# (levels, max_size, max_diff, seed) per shape: integer levels 0 .. levels-1; max_diff 0.5 joins equal values only, 1.0 also adjacent ones
RANDOM = {(1, 1): (2, 1, 0.5, 0), (70, 1): (2, 2, 0.5, 3), (1, 70): (2, 2, 0.5, 1), (63, 5): (3, 3, 0.5, 2), (65, 17): (3, 4, 0.5, 3),
          (130, 67): (3, 6, 0.5, 4)}


def _random_case(w, h, with_valid):
    levels, max_size, max_diff, seed = RANDOM[(w, h)]
    rng = np.random.default_rng(1000 * seed + w + 7 * h + int(with_valid))
    d = rng.integers(0, levels, (h, w)).astype(np.float64)
    valid = (rng.random((h, w)) < 0.85).astype(np.uint8) if with_valid else None
    if w > 64:  # the seam between the first two tile columns carries at least one link, whatever the draw
        d[h // 2, 63:65] = d[h // 2, 63]
        if valid is not None:
            valid[h // 2, 63:65] = 1
    return d, valid, max_size, max_diff


def random_preconditions(w, h, d, valid, max_size, max_diff):
    """asserted on the restatement alone"""
    out, n = sr.speckle_filter(d, valid, max_size, max_diff)
    nodes = n > 0
    if w * h > 1:
        removed = (nodes & (out == 0)).sum() / nodes.sum()
        assert 0.05 <= removed <= 0.95, f"{w}x{h}: {removed:.3f} of the valid pixels removed"
    if w > 64:
        seam = nodes[:, 63] & nodes[:, 64] & (np.abs(d[:, 63] - d[:, 64]) <= max_diff)
        assert seam.any(), f"{w}x{h}: no component straddles columns 63 | 64"


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("w,h", SHAPES)
def test_random_quantised_maps(w, h, with_valid):
    d, valid, max_size, max_diff = _random_case(w, h, with_valid)
    random_preconditions(w, h, d, valid, max_size, max_diff)
    _compare(d, valid, max_size, max_diff, f"random {w}x{h} valid={with_valid}")


@pytest.mark.parametrize("w,h", SHAPES)
def test_checkerboard_constant_and_nan_maps(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    checker = ((xs + ys) % 2 * 10).astype(np.float64)
    _, n = _compare(checker, None, 1, 1.0, f"checkerboard {w}x{h}")
    assert (n == 1).all()
    _, n = _compare(np.full((h, w), 3.25), None, w * h - 1, 0.0, f"constant {w}x{h}")
    assert (n == w * h).all()
    out, _ = _compare(np.full((h, w), 3.25), None, w * h, 0.0, f"constant {w}x{h}, removed")
    assert not out.any()
    rng = np.random.default_rng(w * 131 + h)
    d = rng.integers(0, 2, (h, w)).astype(np.float64)
    d[rng.random((h, w)) < 0.15] = np.nan
    d[h // 2, w // 2] = np.nan
    valid = (rng.random((h, w)) < 0.9).astype(np.uint8)
    valid[h // 2, w // 2] = 1
    for mask in (None, valid):
        _, n = _compare(d, mask, 2, INF, f"NaNs {w}x{h}")
        assert (n[np.isnan(d) & (n > 0)] == 1).all() and n[h // 2, w // 2] == 1
    _compare(d, valid, 0, 1.0, f"NaNs {w}x{h}, max_size 0")


@pytest.mark.parametrize("along_rows", [True, False])
def test_serpentine_through_the_whole_image(along_rows):
    """a one-pixel-wide path through all of 130 x 67 (every other line, joined at alternating ends): one component, and every one of
    its tile pieces hangs on the next through a single border link -- the longest merge chains the image can hold"""
    w, h = 130, 67
    valid = np.zeros((h, w) if along_rows else (w, h), np.uint8)
    valid[0::2, :] = 1
    valid[1::4, -1] = 1
    valid[3::4, 0] = 1
    if not along_rows:
        valid = np.ascontiguousarray(valid.T)
    d = np.full((h, w), 7.5)
    size = int(valid.sum())
    _, n = _compare(d, valid, size - 1, 0.0, "serpentine")
    assert (n[valid == 1] == size).all()
    out, _ = _compare(d, valid, size, 0.0, "serpentine, removed")
    assert not out.any()
    d2 = np.where((np.mgrid[0:h, 0:w][0 if along_rows else 1] // 2) % 2 == 0, 7.5, 8.25)  # neighbouring lines 0.75 apart: one component at 1.0 only
    _, n = _compare(d2, valid, 10, 1.0, "serpentine, two levels joined")
    assert (n[valid == 1] == size).all()
    _, n = _compare(d2, valid, 10, 0.5, "serpentine, two levels apart")
    assert n.max() < size


def test_infinite_max_diff_labels_the_mask_alone():
    rng = np.random.default_rng(5)
    mask = (rng.random((67, 130)) < 0.6).astype(np.uint8)
    a = _compare(rng.normal(0.0, 1e6, (67, 130)), mask, 9, INF, "inf, random values")
    b = _compare(np.zeros((67, 130)), mask, 9, 0.0, "inf, constant values")
    assert np.array_equal(a[1], b[1])


def test_argument_errors(spk_ctx):
    ctx, L = spk_ctx, spk_ctx.L
    for size, diff in ((-1, 1.0), (5, -0.5), (5, float("nan")), (5, INF), (5, -INF)):
        assert L.cspm_set_pp_speckle(ctx.p, size, diff) == -1, (size, diff)
    assert ctx.get_pp_speckle() == (0, 1.0)
    ctx.set_pp_speckle(7, 0.0)
    assert ctx.get_pp_speckle() == (7, 0.0)
    assert L.cspm_set_pp_speckle(None, 1, 1.0) == -1 and L.cspm_get_pp_speckle(None, None, None) == -1
    d = np.zeros((4, 4))
    out = np.zeros((4, 4), np.uint8)
    dp, op = capi._dp(d), capi._u8(out)
    assert L.cspm_filter_speckles_host(0, dp, None, 1 << 16, 1 << 15, 1, 1.0, op, None) == -1  # w * h == 2^31
    assert b"2^31" in L.cspm_last_error(None)
    assert L.cspm_filter_speckles_host(0, dp, None, 4, 4, -1, 1.0, op, None) == -1
    assert L.cspm_filter_speckles_host(0, dp, None, 4, 4, 1, -1.0, op, None) == -1
    assert L.cspm_filter_speckles_host(0, dp, None, 4, 4, 1, float("nan"), op, None) == -1
    assert L.cspm_filter_speckles_host(0, None, None, 4, 4, 1, 1.0, op, None) == -1
    assert L.cspm_filter_speckles_host(0, dp, None, 4, 4, 1, 1.0, None, None) == -1
    assert L.cspm_filter_speckles_host(0, dp, None, 4, 4, 1, 1.0, op, None) == 0 and out.all()  # size_out may be NULL


# ---- inside the post-processing ----------------------------------------------------------------------------------------------------
def _abc(ctx):
    return [ctx.get_planes(v)[0][..., 3:6] for v in (0, 1)]


def _inject(ctx, l, r, D, disp):
    """images, a single-scale cost object and fronto-parallel fields of the given disparities"""
    ctx.set_images(l, r)
    ctx.build_cost_grd(D, 35, 0, 0.0)
    h, w = l.shape[:2]
    for v in (0, 1):
        npar = np.zeros((h, w, 6))
        npar[..., 2] = 1.0
        npar[..., 5] = disp[v]
        ctx.set_planes(v, npar, np.zeros((h, w)))


BLOB_SIZES = [40, 1, 2, 5, 13, 20, 21, 27, 33, 39, 8, 16, 24, 30, 36, 3]


def blob_fields(w, h, rng, integer):
    """both views' disparity maps: background 4, and in each 24 x 16 cell one 4-connected blob of 1 .. 40 pixels whose disparity
    (8 .. 11, with a quarter-pixel fraction unless integer) the other view confirms.  Returns (d_left, d_right, blob sizes)."""
    dl, dr = np.full((h, w), 4.0), np.full((h, w), 4.0)
    sizes = []
    cells = [(cx, cy) for cy in range(0, h - 15, 16) for cx in range(0, w - 23, 24)]
    for k, (cx, cy) in enumerate(cells):
        size = BLOB_SIZES[k % len(BLOB_SIZES)]
        box = np.zeros((6, 8), bool)  # the blob grows inside columns 14 .. 21, rows 5 .. 10 of its cell
        box[rng.integers(0, 6), rng.integers(0, 8)] = True
        while box.sum() < size:
            grown = np.zeros_like(box)
            grown[1:] |= box[:-1]; grown[:-1] |= box[1:]; grown[:, 1:] |= box[:, :-1]; grown[:, :-1] |= box[:, 1:]
            ys, xs = np.nonzero(grown & ~box)
            j = rng.integers(0, len(ys))
            box[ys[j], xs[j]] = True
        shift = 8 + k % 4
        value = float(shift) if integer else shift + 0.25 * (k % 2)
        ys, xs = np.nonzero(box)
        dl[cy + 5 + ys, cx + 14 + xs] = value
        dr[cy + 5 + ys, cx + 14 + xs - shift] = value
        sizes.append(size)
    return dl, dr, sizes


def _check_f64(ctx, l, r, D, max_size, max_diff, what):
    """postprocess_f64 with the filter == the restatement on the context's own planes: maps, masks, removed count"""
    ctx.set_pp_speckle(max_size, max_diff)
    got = ctx.postprocess_f64(valid=True)
    removed = ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED)
    abc = _abc(ctx)
    want = sr.postprocess_f64_speckle(abc[0], abc[1], l, r, D, max_size, max_diff)
    print(f"{what}: removed {want[4]} pixels (device {removed}), inconsistent afterwards {int((want[2] == 0).sum())} + {int((want[3] == 0).sum())}")
    for v in (0, 1):
        assert np.array_equal(got[2 + v], want[2 + v]), f"{what}: mask of view {v}: {int((got[2 + v] != want[2 + v]).sum())} pixels differ"
        diff = _bits(got[v]) != _bits(want[v])
        assert not diff.any(), f"{what}: view {v}: {diff.sum()} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"
    assert removed == want[4]
    return got, want


def test_f64_pipeline_after_patchmatch(spk_ctx):
    """80 x 56, D = 16, cross-scale, one iteration: what PatchMatch leaves behind, speckles included"""
    import torch
    w, h, D = 80, 56, 16
    l, r, _, _ = synth.make_pair(w, h, D, regions=3, seed=21)
    spk_ctx.set_images(l, r)
    spk_ctx.build_cost_grd(D, 35, 5, 0.3)
    spk_ctx.patchmatch(1, seed=5, schedule=capi.SCHED_RASTER)
    got, want = _check_f64(spk_ctx, l, r, D, 30, 1.0, "80x56 after one iteration")
    assert want[4] > 0, "nothing removed: the case checks nothing"
    outs = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
    spk_ctx.postprocess_f64_device(outs[0].data_ptr(), outs[1].data_ptr())
    spk_ctx.synchronize()
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) == want[4]
    for v in (0, 1):
        assert np.array_equal(_bits(outs[v].cpu().numpy()), _bits(got[v]))


def test_f64_pipeline_on_consistent_blobs(spk_ctx):
    w, h, D = 96, 64, 16
    l, r, _, _ = synth.make_pair(w, h, D, regions=3, seed=33)
    dl, dr, sizes = blob_fields(w, h, np.random.default_rng(8), integer=False)
    assert min(sizes) == 1 and max(sizes) == 40 and len(sizes) == 16
    _inject(spk_ctx, l, r, D, [dl, dr])
    plain = spk_ctx.postprocess_f64(valid=True)
    assert plain[2][dl > 4.0].all() and plain[3][dr > 4.0].all(), "the blobs pass the left-right check"
    got, want = _check_f64(spk_ctx, l, r, D, 20, 1.0, "blobs")
    small = sum(s for s in sizes if s <= 20)
    assert want[4] >= 2 * small
    for v, d in ((0, dl), (1, dr)):
        assert (got[2 + v][d > 4.0] == 0).sum() == small  # the small blobs left the mask, the large ones stayed
        assert (got[v][d > 4.0] != d[d > 4.0]).sum() >= 1   # and were filled or medianed away


def test_8_bit_pipeline_on_integer_blobs(spk_ctx):
    """integer fronto-parallel fields, dis_scale 1: the f64 restatement's values are the 8-bit path's"""
    import torch
    w, h, D = 96, 64, 16
    l, r, _, _ = synth.make_pair(w, h, D, regions=3, seed=34)
    dl, dr, sizes = blob_fields(w, h, np.random.default_rng(9), integer=True)
    _inject(spk_ctx, l, r, D, [dl, dr])
    spk_ctx.set_pp_speckle(20, 1.0)
    got = spk_ctx.postprocess(1)
    removed = spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED)
    want = sr.postprocess_f64_speckle(ps.fronto_field(dl), ps.fronto_field(dr), l, r, D, 20, 1.0)
    assert want[4] >= 2 * sum(s for s in sizes if s <= 20) and removed == want[4]
    outs = [torch.zeros((h, w), dtype=torch.uint8, device="cuda:0") for _ in (0, 1)]
    spk_ctx.postprocess_device(1, outs[0].data_ptr(), outs[1].data_ptr())
    spk_ctx.synchronize()
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) == want[4]
    for v in (0, 1):
        assert np.array_equal(got[v].astype(np.float64), want[v]), f"view {v}: {int((got[v] != want[v]).sum())} pixels differ"
        assert np.array_equal(outs[v].cpu().numpy(), got[v])
    spk_ctx.set_pp_speckle(0, 1.0)
    off = spk_ctx.postprocess(1)
    assert any(not np.array_equal(off[v], got[v]) for v in (0, 1)), "the filter changed nothing: the case checks nothing"


def test_filter_off_is_a_fresh_context(spk_ctx, small_pair):
    import crossscalepatchmatch_amd as cs
    l, r, D = small_pair["l"], small_pair["r"], small_pair["max_dis"]

    def run(ctx):
        ctx.set_images(l, r)
        ctx.build_cost_grd(D, 35, 5, 0.3)
        ctx.patchmatch(1, seed=3, schedule=capi.SCHED_RASTER)

    fresh = cs.StereoContext(0)
    try:
        run(fresh)
        want8, want64 = fresh.postprocess(4), fresh.postprocess_f64(valid=True)
        assert fresh.get_option(capi.OPT_PP_SPECKLE_REMOVED) == 0 and fresh.get_pp_speckle() == (0, 1.0)
    finally:
        fresh.close()
    run(spk_ctx)
    spk_ctx.set_pp_speckle(40, 2.0)
    on8, on64 = spk_ctx.postprocess(4), spk_ctx.postprocess_f64(valid=True)
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) > 0
    spk_ctx.set_pp_speckle(0, 2.5)
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) == 0
    got8, got64 = spk_ctx.postprocess(4), spk_ctx.postprocess_f64(valid=True)
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) == 0
    for v in (0, 1):
        assert np.array_equal(got8[v], want8[v])
        assert np.array_equal(_bits(got64[v]), _bits(want64[v])) and np.array_equal(got64[2 + v], want64[2 + v])
    assert any(not np.array_equal(on64[2 + v], want64[2 + v]) for v in (0, 1)) and any(not np.array_equal(on8[v], want8[v]) for v in (0, 1))


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def test_cli_speckle_flags(spk_ctx, small_pair, tmp_path):
    flags = ["--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--use_cs=true", "--reg_lambda=0.3", "--seed=31", "--iters=1"]
    speckle = ["--pp_speckle_size=25", "--pp_speckle_diff=1.5"]
    pngio.write_png(str(tmp_path / "l.png"), small_pair["l"][..., ::-1])
    pngio.write_png(str(tmp_path / "r.png"), small_pair["r"][..., ::-1])
    files = [f"--l_img_file={tmp_path}/l.png", f"--r_img_file={tmp_path}/r.png", f"--l_dis_file={tmp_path}/ld.png", f"--r_dis_file={tmp_path}/rd.png",
             f"--l_disp_pfm={tmp_path}/l.pfm", f"--r_disp_pfm={tmp_path}/r.pfm"]
    p = subprocess.run([EXE] + files + flags + speckle, capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--pp_speckle_size" in p.stdout and b"--use_pp" in p.stdout
    assert not os.path.exists(tmp_path / "l.pfm")
    subprocess.check_call([EXE] + files + flags + speckle + ["--use_pp", "--pp_pfm"], stdout=subprocess.DEVNULL, timeout=120)
    (tmp_path / "list.txt").write_text(" ".join(str(tmp_path / n) for n in ("l.png", "r.png", "bl.png", "br.png", "bl.pfm", "br.pfm")) + "\n")
    out = subprocess.check_output([EXE, f"--batch_list={tmp_path}/list.txt", "--use_pp"] + flags + speckle, timeout=120).decode()
    assert "0 failed" in out
    spk_ctx.set_images(small_pair["l"], small_pair["r"])
    spk_ctx.build_cost_grd(16, 35, 5, 0.3)
    spk_ctx.patchmatch(1, seed=31, schedule=capi.SCHED_RASTER)
    plain = spk_ctx.postprocess_f64()
    spk_ctx.set_pp_speckle(25, 1.5)
    f64, pp8 = spk_ctx.postprocess_f64(), spk_ctx.postprocess(4)
    assert spk_ctx.get_option(capi.OPT_PP_SPECKLE_REMOVED) > 0 and any(not np.array_equal(plain[v], f64[v]) for v in (0, 1))
    for v, side in ((0, "l"), (1, "r")):
        assert np.array_equal(_read_pfm(str(tmp_path / f"{side}.pfm")), f64[v].astype(np.float32))
        assert np.array_equal(pngio.read_png(str(tmp_path / f"{side}d.png")), pp8[v])
        assert np.array_equal(pngio.read_png(str(tmp_path / f"b{side}.png")), pp8[v])  # batch mode, without --pp_pfm: the 8-bit maps are filtered
        assert np.array_equal(_read_pfm(str(tmp_path / f"b{side}.pfm")), spk_ctx.disparity_f64(v).astype(np.float32))
