"""Rectification on the GPU (include/cspm.h "rectification") held to tests/rectify_ref.py bit for bit:
cspm_rectify_host (maps, valid bytes, image bytes) on random raw bytes over the wave and workgroup seams, strides, output sizes, half-pixel
ties, partly invalid rigs and rays behind a camera; the context path (cspm_set_rectification, cspm_set_images_raw(_device),
cspm_get_rect_map) down to the planes of a PatchMatch iteration; the error returns."""
import ctypes as C

import numpy as np
import pytest

import crossscalepatchmatch_amd as cs
import rectify_ref as rr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _torch_first(_gpu_ctx_session):
    """PyTorch's HIP runtime has to initialise before the library's (tests/conftest.py): the device-variant test needs torch tensors"""
    yield


def _same_f64(got, want):
    """bit for bit; NaN positions must agree, any NaN payload"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _raw(rig, seed):
    return np.random.default_rng(seed).integers(0, 256, (rig["raw_h"], rig["raw_w"], 3), dtype=np.uint8)


def _check_host(rig, rect, raw, what, **kw):
    """both views of cspm_rectify_host against the restatement; returns the restatement's valid fractions"""
    crig, crect = rr.capi_rig(rig), rr.capi_rect(rect)
    fractions = []
    for v in (0, 1):
        bgr, sx, sy, valid = rr.rectify(rig, rect, v, raw)
        got = capi.rectify_host(crig, crect, v, raw, **kw)
        assert _same_f64(got["map"][0], sx) and _same_f64(got["map"][1], sy), f"{what}, view {v}: the map differs"
        assert np.array_equal(got["valid"], valid), f"{what}, view {v}: {np.sum(got['valid'] != valid)} valid bytes differ"
        assert np.array_equal(got["bgr"], bgr), f"{what}, view {v}: {np.sum(got['bgr'] != bgr)} image bytes differ"
        assert not got["bgr"][valid == 0].any()
        fractions.append(float(valid.mean()))
    return fractions


def test_same_size_with_padded_rows():
    """raw 67 x 45 -> 67 x 45, raw and output rows longer than 3*w; the padding of the output rows stays untouched"""
    rig = rr.random_rig(np.random.default_rng(11))
    rect, _ = rr.compute(rig)
    raw = _raw(rig, 1)
    crig, crect = rr.capi_rig(rig), rr.capi_rect(rect)
    padded = np.full((45, 3 * 67 + 13), 0x5A, np.uint8)
    padded[:, :3 * 67] = raw.reshape(45, -1)
    for v in (0, 1):
        bgr, sx, sy, valid = rr.rectify(rig, rect, v, raw)
        got = capi.rectify_host(crig, crect, v, padded, raw_stride=padded.shape[1], out_stride=3 * 67 + 7)
        assert np.array_equal(got["bgr"], bgr) and np.array_equal(got["valid"], valid)
        assert _same_f64(got["map"][0], sx) and _same_f64(got["map"][1], sy)
        assert np.all(got["bgr_rows"][:, 3 * 67:] == 0xA5)
        assert 0 < valid.sum() < valid.size


@pytest.mark.parametrize("w,h", [(130, 37), (1, 1), (64, 4), (65, 3), (257, 2)])
def test_output_size_differs_from_the_raw_size(w, h):
    """sizes off (and on) the 64-lane and 256-lane boundaries of the two kernels"""
    rig = rr.random_rig(np.random.default_rng(12))
    rect, _ = rr.compute(rig, w=w, h=h)
    assert (rect["w"], rect["h"]) == (w, h)
    _check_host(rig, rect, _raw(rig, 2), f"{w}x{h}")


def test_each_output_is_optional():
    rig = rr.random_rig(np.random.default_rng(13))
    rect, _ = rr.compute(rig)
    crig, crect = rr.capi_rig(rig), rr.capi_rect(rect)
    raw = _raw(rig, 3)
    bgr, sx, sy, valid = rr.rectify(rig, rect, 1, raw)
    got = capi.rectify_host(crig, crect, 1, None, outputs=("map",))
    assert set(got) == {"map"} and _same_f64(got["map"][0], sx) and _same_f64(got["map"][1], sy)
    got = capi.rectify_host(crig, crect, 1, None, outputs=("valid",))
    assert np.array_equal(got["valid"], valid)
    got = capi.rectify_host(crig, crect, 1, raw, outputs=("bgr",))
    assert np.array_equal(got["bgr"], bgr)


def test_half_pixel_shift_rounds_ties_to_even():
    """the identity rig with cx = 24.0: sx = x - 0.5 exactly, so tx = 0.5 and every odd sum of two neighbours is a tie"""
    rig = rr.identity_rig()
    rect, _ = rr.compute(rig, cx=24.0)
    sx, sy, _, valid = rr.rect_map(rig, rect, 0)
    assert np.array_equal(sx[0], np.arange(48) - 0.5) and not valid[:, 0].any() and valid[:, 1:].all()
    raw = _raw(rig, 4)
    want = rr.remap(raw, sx, sy, valid)
    s = raw[:, :-1].astype(int) + raw[:, 1:].astype(int)
    ties = s % 2 == 1
    assert ties.sum() > 1000
    assert np.array_equal(want[:, 1:][ties], ((s[ties] + 1) // 4 * 2).astype(np.uint8))  # the even neighbour of s / 2
    _check_host(rig, rect, raw, "half-pixel shift")


def test_partly_invalid_rigs():
    rng = np.random.default_rng(14)
    for k in range(3):
        rig = rr.random_rig(rng)
        rect, _ = rr.compute(rig)
        for fr in _check_host(rig, rect, _raw(rig, 5 + k), f"rig {k}"):
            assert 0.05 <= fr <= 0.95, fr


def test_rays_behind_a_camera():
    rig = rr.behind_rig()
    rect, _ = rr.compute(rig)
    front = rr.rect_map(rig, rect, 1)[2]
    assert (~front).sum() >= 1
    _check_host(rig, rect, _raw(rig, 8), "camera 1 yawed 100 degrees")


def test_host_entry_argument_errors():
    L = capi.load_library()
    rig = rr.identity_rig()
    rect, _ = rr.compute(rig)
    crig, crect = rr.capi_rig(rig), rr.capi_rect(rect)
    raw = _raw(rig, 9)
    out = np.zeros((36, 48, 3), np.uint8)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
    call = lambda r, q, v, rawp, rs, o, os_: L.cspm_rectify_host(0, r, q, v, rawp, rs, o, os_, None, None)  # noqa: E731
    assert call(None, C.byref(crect), 0, u8(raw), 144, u8(out), 144) == -1
    assert call(C.byref(crig), None, 0, u8(raw), 144, u8(out), 144) == -1
    assert call(C.byref(crig), C.byref(crect), 2, u8(raw), 144, u8(out), 144) == -1
    assert call(C.byref(crig), C.byref(crect), 0, None, 144, u8(out), 144) == -1
    assert call(C.byref(crig), C.byref(crect), 0, u8(raw), 143, u8(out), 144) == -1
    assert call(C.byref(crig), C.byref(crect), 0, u8(raw), 144, u8(out), 143) == -1
    bad = rr.capi_rect(rect)
    bad.f = 0.0
    assert call(C.byref(crig), C.byref(bad), 0, u8(raw), 144, u8(out), 144) == -1
    assert L.cspm_last_error(None).decode().startswith("rectification")
    assert call(C.byref(crig), C.byref(crect), 0, u8(raw), 144, u8(out), 144) == 0 and np.array_equal(out, raw)


# ---- the context path, 96 x 64, max_dis = 16 ----
W, H, D = 96, 64, 16


@pytest.fixture(scope="module")
def ctx_case(mid_pair):
    """one rig with a raw size of 96 x 64, two raw pairs (a textured one and random bytes) and the restatement's rectified bytes of both"""
    rig = rr.random_rig(np.random.default_rng(21), raw_w=W, raw_h=H, f=90.0, max_deg=3.0)
    rect, calib = rr.compute(rig)
    pairs = [(mid_pair["l"], mid_pair["r"]), (_raw(rig, 31), _raw(rig, 32))]
    maps = [rr.rect_map(rig, rect, v) for v in (0, 1)]
    want = [[rr.remap(p[v], maps[v][0], maps[v][1], maps[v][3]) for v in (0, 1)] for p in pairs]
    return dict(rig=rig, rect=rect, calib=calib, pairs=pairs, maps=maps, want=want)


def _map_equals(ctx, case):
    for v in (0, 1):
        sx, sy, valid = ctx.rect_map(v)
        m = case["maps"][v]
        if not (_same_f64(sx, m[0]) and _same_f64(sy, m[1]) and np.array_equal(valid, m[3].astype(np.uint8))):
            return False
    return True


def test_context_raw_pairs_match_the_restatement_down_to_the_planes(ctx_case):
    case = ctx_case
    a, b = cs.StereoContext(0), cs.StereoContext(0)
    try:
        rect, calib = a.set_rectification(rr.capi_rig(case["rig"]))
        assert (rect.w, rect.h) == (W, H) and (calib.f, calib.cx, calib.cy, calib.baseline, calib.doffs) == case["calib"]
        assert _map_equals(a, case)
        a.enable_timing(True)
        a.reset_timing()
        a.set_images_raw(*case["pairs"][0])
        assert a.timing()["misc"]["launches"] == 3  # the remap of both views as one bracket, then the two of cspm_set_images_device's path
        a.enable_timing(False)
        assert (a.w, a.h) == (W, H)
        b.set_images(*case["want"][0])
        for c in (a, b):
            c.build_cost_grd(D, 35, 5, 0.3)  # cspm_get_level_image reads the cost object's level images
        for v in (0, 1):
            assert np.array_equal(a.level_image(v, 0), case["want"][0][v]), v
        for c in (a, b):
            c.patchmatch(1, seed=7)
        for v in (0, 1):
            for got, want in zip(a.get_planes(v), b.get_planes(v)):
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), v
        # a second raw pair reuses the maps
        a.set_images_raw(*case["pairs"][1])
        a.build_cost_grd(D, 35, 5, 0.3)
        assert _map_equals(a, case)
        for v in (0, 1):
            assert np.array_equal(a.level_image(v, 0), case["want"][1][v]), v
        # the same rig again launches nothing and keeps the maps
        a.enable_timing(True)
        a.reset_timing()
        a.set_rectification(rr.capi_rig(case["rig"]), rr.capi_rect(case["rect"]))
        assert a.timing()["misc"]["launches"] == 0 and _map_equals(a, case)
        a.enable_timing(False)
    finally:
        a.close()
        b.close()


def test_device_variant_with_torch_buffers(ctx_case):
    import torch
    case = ctx_case
    ctx = cs.StereoContext(0)
    try:
        ctx.set_rectification(rr.capi_rig(case["rig"]), rr.capi_rect(case["rect"]))
        stride = 3 * W + 9
        bufs = []
        for img in case["pairs"][1]:
            rows = np.full((H, stride), 0x77, np.uint8)
            rows[:, :3 * W] = img.reshape(H, -1)
            bufs.append(torch.from_numpy(rows).cuda())
        torch.cuda.synchronize()
        ctx.set_images_raw_device(bufs[0].data_ptr(), bufs[1].data_ptr(), stride)
        ctx.build_cost_grd(D, 35, 0, 0.0)
        ctx.synchronize()
        for v in (0, 1):
            assert np.array_equal(ctx.level_image(v, 0), case["want"][1][v]), v
    finally:
        ctx.close()


def test_state_and_argument_errors(ctx_case):
    case = ctx_case
    L = capi.load_library()
    ctx = cs.StereoContext(0)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731
    try:
        l, r = (np.ascontiguousarray(p) for p in case["pairs"][0])
        assert L.cspm_set_images_raw(ctx.p, u8(l), u8(r), 3 * W) == -3  # CSPM_ERR_STATE: no rectification yet
        assert "rectification" in L.cspm_last_error(ctx.p).decode()
        assert L.cspm_set_images_raw_device(ctx.p, None, None, 3 * W) == -3
        assert L.cspm_get_rect_map(ctx.p, 0, None, None) == -3
        with pytest.raises(cs.CspmError, match="-3"):
            ctx.set_images_raw(l, r)
        with pytest.raises(cs.CspmError, match="-3"):
            ctx.rect_map(0)
        crig, crect = rr.capi_rig(case["rig"]), rr.capi_rect(case["rect"])
        assert L.cspm_set_rectification(ctx.p, C.byref(crig), None) == -1
        bad = rr.capi_rig(case["rig"])
        bad.raw_w = 0
        assert L.cspm_set_rectification(ctx.p, C.byref(bad), C.byref(crect)) == -1
        ctx.set_rectification(crig, crect)
        # a wrong raw size: rows shorter than the rig's (the C entry takes the size from the rig), and images of another shape
        assert L.cspm_set_images_raw(ctx.p, u8(l), u8(r), 3 * W - 1) == -1
        assert L.cspm_set_images_raw(ctx.p, u8(l), None, 3 * W) == -1
        assert L.cspm_get_rect_map(ctx.p, 2, None, None) == -1
        with pytest.raises(cs.CspmError, match="-1"):
            ctx.set_images_raw(l[:, :-1], r[:, :-1])
        with pytest.raises(cs.CspmError, match="-1"):
            ctx.set_images_raw(l[:-1], r[:-1])
        ctx.set_images_raw(l, r)
        # dropped: the plain entry still works, the raw one is a state error again
        assert ctx.set_rectification(None) is None
        assert L.cspm_set_images_raw(ctx.p, u8(l), u8(r), 3 * W) == -3
        ctx.set_images(l, r)
        ctx.build_cost_grd(D, 35, 0, 0.0)
        for v, img in enumerate((l, r)):
            assert np.array_equal(ctx.level_image(v, 0), img)
        ctx.patchmatch(1, seed=3)
        assert ctx.disparity_u8(0, 4).shape == (H, W)
    finally:
        ctx.close()


def test_a_new_rectification_of_another_size_replaces_the_old(ctx_case):
    case = ctx_case
    ctx = cs.StereoContext(0)
    try:
        ctx.set_rectification(rr.capi_rig(case["rig"]), rr.capi_rect(case["rect"]))
        ctx.set_images_raw(*case["pairs"][0])
        rect2, _ = rr.compute(case["rig"], f=70.0, w=130, h=37)
        ctx.set_rectification(rr.capi_rig(case["rig"]), rr.capi_rect(rect2))
        ctx.set_images_raw(*case["pairs"][1])
        ctx.build_cost_grd(D, 35, 0, 0.0)
        assert (ctx.w, ctx.h) == (130, 37)
        for v in (0, 1):
            want = rr.rectify(case["rig"], rect2, v, case["pairs"][1][v])[0]
            assert np.array_equal(ctx.level_image(v, 0), want), v
    finally:
        ctx.close()


def test_host_layer_rectification():
    """RectifyPair, DeviceSlot::SetRectification, DevicePlaneCost::LevelImages, the CSPatchMatch constructor for raw pairs and the rig
    reader (tests/helpers/rect_check.cc)"""
    import subprocess
    from test_gpu_warm_start import _build_helper
    exe = _build_helper("rect_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rect_check ok" in r.stdout, r.stdout + r.stderr
