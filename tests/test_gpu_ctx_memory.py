"""What a context holds on the device (DESIGN.md "Context memory"), read through CSPM_OPT_DEVICE_BYTES on contexts of this module's own:
0 for a fresh one and the two image buffers after set_images; one pass over every lazily allocating entry, then the same pass twice more
without a byte's difference and with the same planes and maps bit for bit; a geometry change that leaves the new images alone; optional
volumes whose first, middle or last allocation fails and leave exactly what a build without them holds; and the rectification's maps
and raw-pair buffers, allocated once and gone with set_rectification(None).  Pairs: 64 x 48 D = 16 and 77 x 41 D = 21, three levels."""
import numpy as np
import pytest

import rectify_ref as rr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

CAL = (300.0, 31.5, 20.25, 0.25, 3.5)
WND, LEVELS, LAMBDA = 9, 3, 0.3


def _images_bytes(w, h):
    return 2 * 4 * w * h + 2 * 3 * w * h  # the packed words of both views, the host pair's staging bytes


def _bytes(ctx):
    return ctx.get_option(capi.OPT_DEVICE_BYTES)


@pytest.fixture
def ctx(_gpu_ctx_session):
    c = capi.StereoContext(0)
    yield c
    c.close()


def _full_pass(c, pair):
    """every entry that allocates on first use, once; the planes and maps it produced"""
    w, h, D = pair["w"], pair["h"], pair["max_dis"]
    out = {}
    c.set_pp_speckle(20, 1.0)
    c.set_pp_median(1)
    c.set_pp_smooth(lam=100.0)
    c.set_images(pair["l"], pair["r"])
    c.build_cost_grd(D, WND, LEVELS, LAMBDA)
    c.patchmatch(1, seed=5)
    c.patchmatch(1, seed=5, schedule=capi.SCHED_DIFFUSE, rb_neighbours=4)
    c.patchmatch_warm(1, seed=5)
    c.set_option(capi.OPT_SWEEP_FLOW, 1)
    c.pm_spatial(0, seed=5)
    c.set_option(capi.OPT_SWEEP_FLOW, 0)
    for v in (0, 1):
        out[f"pm_planes{v}"], out[f"pm_cost{v}"] = c.get_planes(v)
    out["pp_l"], out["pp_r"] = c.postprocess(4)
    out["pp64_l"], out["pp64_r"], out["pp64_lv"], out["pp64_rv"] = c.postprocess_f64(valid=True)
    rng = np.random.default_rng(3)
    c.merge_planes(1, capi.disparity_planes(rng.uniform(1.0, D - 1.0, (h, w))), rng.uniform(size=(h, w)) < 0.6)
    c.fit_planes(merge=True, radius=2)
    c.segment_planes(merge=True, step=8)
    for v in (0, 1):
        out[f"cand_planes{v}"], out[f"cand_cost{v}"] = c.get_planes(v)
    geo = c.reproject(0, CAL, fit=dict(radius=2), min_cos=0.3, z_far=12.0)
    out["geo_depth"], out["geo_cloud"] = geo["depth"], geo["cloud"]
    out["geo_pp_keep"] = c.reproject(1, CAL, source=capi.GEOM_PP, cloud=False)["keep"]
    mesh = c.mesh(0, CAL, max_diff=2.0)
    out["mesh_vertices"], out["mesh_faces"] = mesh["vertices"], mesh["faces"]
    out["synth_bgr"] = c.synthesize(0.5)["bgr"]
    c.local_stereo(capi.CA_BOX)
    for v in (0, 1):
        out[f"ls_planes{v}"], out[f"ls_cost{v}"] = c.get_planes(v)
    return out


def test_fresh_context_holds_nothing_then_the_images(ctx, small_pair, odd_pair):
    assert _bytes(ctx) == 0
    for pair in (small_pair, odd_pair, small_pair):
        ctx.set_images(pair["l"], pair["r"])
        assert _bytes(ctx) == _images_bytes(pair["w"], pair["h"])


@pytest.mark.parametrize("first", ["small_pair", "odd_pair"])
def test_steady_state_and_geometry_change(ctx, request, first, small_pair, odd_pair):
    pair = request.getfixturevalue(first)
    other = odd_pair if pair is small_pair else small_pair
    one = _full_pass(ctx, pair)
    held = _bytes(ctx)
    print(f"{pair['w']} x {pair['h']}: {held} bytes after one pass, {_images_bytes(pair['w'], pair['h'])} of them images")
    assert held > _images_bytes(pair["w"], pair["h"])
    _full_pass(ctx, pair)
    assert _bytes(ctx) == held, "the second pass allocated or freed"
    three = _full_pass(ctx, pair)
    assert _bytes(ctx) == held, "the third pass allocated or freed"
    assert ctx.get_option(capi.OPT_SWEEP_FALLBACKS) == 0 and ctx.get_option(capi.OPT_VOLUME_FALLBACKS) == 0
    for name in one:
        assert one[name].shape == three[name].shape and one[name].tobytes() == three[name].tobytes(), name
    assert one["geo_cloud"].size > 0 and one["mesh_faces"].size > 0 and np.isfinite(one["ls_cost0"]).any()
    # the other size: cost object, field and local-stereo scratch are all gone, the new images are all there is
    ctx.set_images(other["l"], other["r"])
    assert _bytes(ctx) == _images_bytes(other["w"], other["h"])


def _build(c, pair, **kw):
    c.set_images(pair["l"], pair["r"])
    c.build_cost_grd(pair["max_dis"], WND, LEVELS, LAMBDA, **kw)
    return _bytes(c)


@pytest.mark.parametrize("nth,sweep_pairs", [(1, False), (4, False), (6, False), (4, True)])
def test_failed_optional_volume_leaves_what_a_build_without_holds(ctx, small_pair, nth, sweep_pairs):
    plain = capi.StereoContext(0)
    try:
        without = _build(plain, small_pair, table_volumes=False, sweep_pairs=False)
    finally:
        plain.close()
    ctx.set_option(capi.OPT_FAULT_VOLUME_ALLOC, nth)
    before = ctx.get_option(capi.OPT_VOLUME_FALLBACKS)
    held = _build(ctx, small_pair, table_volumes=True, sweep_pairs=sweep_pairs)
    assert ctx.get_option(capi.OPT_VOLUME_FALLBACKS) == before + 1
    assert ctx.get_option(capi.OPT_TABLE_VOLUMES_ACTIVE) == 0 and ctx.get_option(capi.OPT_SWEEP_PAIRS_ACTIVE) == 0
    assert held == without
    ctx.patchmatch(1, seed=5)  # and it runs without them
    ctx.synchronize()


def test_optional_volumes_are_counted(ctx, small_pair):
    without = _build(ctx, small_pair, table_volumes=False, sweep_pairs=False)
    w, h, D, vols = small_pair["w"], small_pair["h"], small_pair["max_dis"], 0
    for s in range(LEVELS):
        if s:
            w, h, D = (w + 1) // 2, (h + 1) // 2, D // 2
        vols += 2 * 8 * ((D + 1) * h * (w + 2 * (WND // 2 + 2)) + 64)  # cspm_api.hip alloc_cost: both views' cells, padded columns, the slack
    held = _build(ctx, small_pair, table_volumes=True, sweep_pairs=False)
    assert ctx.get_option(capi.OPT_TABLE_VOLUMES_ACTIVE) == 1 and ctx.get_option(capi.OPT_VOLUME_FALLBACKS) == 0
    assert held == without + vols


def test_rectification_buffers(ctx):
    w, h = 77, 41
    rig = rr.random_rig(np.random.default_rng(31))
    rw, rh = rig["raw_w"], rig["raw_h"]
    rect, _ = rr.compute(rig, w=w, h=h)
    before = _bytes(ctx)
    assert before == 0
    ctx.set_rectification(rr.capi_rig(rig), rr.capi_rect(rect))
    maps = 2 * (2 * 8 + 1) * w * h
    assert _bytes(ctx) == before + maps
    ctx.set_rectification(rr.capi_rig(rig), rr.capi_rect(rect))  # the same rig again: nothing
    assert _bytes(ctx) == before + maps
    rng = np.random.default_rng(32)
    raw_buffers = 2 * 4 * rw * rh + 2 * 3 * w * h + 2 * 3 * rw * rh  # packed raw words, the rectified pair, the host pair's staging bytes
    images = 2 * 4 * w * h  # the rectified pair arrives on the device: no staging bytes
    for _ in range(2):
        ctx.set_images_raw(rng.integers(0, 256, (rh, rw, 3), dtype=np.uint8), rng.integers(0, 256, (rh, rw, 3), dtype=np.uint8))
        assert _bytes(ctx) == before + maps + raw_buffers + images
    ctx.set_rectification(None)
    assert _bytes(ctx) == before + images
