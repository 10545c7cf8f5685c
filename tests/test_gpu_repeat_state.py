"""When a run may be repeated after a sweep timeout: the transition table of the repeat record (cspm_api.hip `Repeat`).

A persistent raster sweep that gives up waiting is repeated with per-diagonal launches by the next synchronising call -- when exactly
one whole run is unchecked and nothing tainted it.  Which entry taints, and for how long, is what these cases pin: a taint "that
stays" (cspm_pm_init, cspm_set_planes, cspm_rescore_planes, the single phases) outlives the call when no sweep is pending and blocks
the repeat of the NEXT run; a taint "of an unchecked run" (new images, a new cost object, cspm_local_stereo, the merges,
cspm_pm_init_keep) only counts behind a run that has not been checked yet.

Every case: its own context, the 96 x 64 pair, fused GRD cells, the raster schedule, two iterations, and the library's bounded
give-up hook CSPM_OPT_SWEEP_TIMEOUT_MS = 0 armed once.  The pair has five cross-scale levels except where cspm_local_stereo takes
part: its BOX filter needs 7 pixels on every level, and the pair's fifth level is 6 x 4, so those cases run three levels.
"""
import contextlib

import numpy as np
import pytest

# gpu_ctx: the session's context is opened (after PyTorch has initialised its HIP runtime) before any context of this module
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_ctx")]

ITERS = 2
KW = dict(seed=9, schedule=0)  # capi.SCHED_RASTER


def _open(pair, scale_num=5):
    import crossscalepatchmatch_amd as cs
    ctx = cs.StereoContext(0)
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 35, scale_num, 0.3)
    return ctx


@contextlib.contextmanager
def _armed(ctx):
    """every wait of a persistent sweep enqueued in here gives up at once"""
    from crossscalepatchmatch_amd import capi
    ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 0)
    try:
        yield
    finally:
        ctx.set_option(capi.OPT_SWEEP_TIMEOUT_MS, 3000)


def _fallbacks(ctx):
    from crossscalepatchmatch_amd import capi
    return ctx.get_option(capi.OPT_SWEEP_FALLBACKS)


def _planes(ctx):
    out = [ctx.get_planes(v) for v in (0, 1)]
    for npar, cost in out:
        npar.setflags(write=False)
        cost.setflags(write=False)
    return out


def _assert_planes(ctx, want):
    for v in (0, 1):
        npar, cost = ctx.get_planes(v)
        np.testing.assert_array_equal(npar, want[v][0])
        np.testing.assert_array_equal(cost, want[v][1])


@pytest.fixture(scope="module")
def cold_ref(mid_pair):
    """planes and costs of an untimed cspm_patchmatch(2, seed 9), by the number of cross-scale levels"""
    ref = {}
    for scale_num in (5, 3):
        ctx = _open(mid_pair, scale_num)
        try:
            ctx.patchmatch(ITERS, **KW)
            ref[scale_num] = _planes(ctx)
            assert _fallbacks(ctx) == 0
        finally:
            ctx.close()
    return ref


def _assert_refused(ctx, check):
    """the synchronising call reports the timeout and repeats nothing"""
    import crossscalepatchmatch_amd as cs
    with pytest.raises(cs.CspmError, match="timed out"):
        check()
    assert _fallbacks(ctx) == 0


def _assert_usable(ctx, want):
    """the refusal reset the record: with the timeout back at its default the next run is an ordinary one"""
    ctx.patchmatch(ITERS, **KW)
    _assert_planes(ctx, want)
    assert _fallbacks(ctx) == 0


def test_pm_init_before_a_run_blocks_its_repeat(mid_pair, cold_ref):
    """the known limit: cspm_pm_init taints while nothing is pending, and the taint waits for the next check"""
    ctx = _open(mid_pair)
    try:
        ctx.pm_init(seed=9)
        with _armed(ctx):
            ctx.patchmatch(ITERS, **KW)
            _assert_refused(ctx, lambda: ctx.get_planes(0))
        _assert_usable(ctx, cold_ref[5])
    finally:
        ctx.close()


def test_a_check_between_pm_init_and_the_run_clears_the_taint(mid_pair, cold_ref):
    ctx = _open(mid_pair)
    try:
        ctx.pm_init(seed=9)
        ctx.patchmatch(ITERS, **KW)
        ctx.get_planes(0)  # untimed: the sweep is checked, the record reset
        with _armed(ctx):
            ctx.patchmatch(ITERS, **KW)
            _assert_planes(ctx, cold_ref[5])
        assert _fallbacks(ctx) == 1
    finally:
        ctx.close()


def test_set_planes_before_a_warm_run_blocks_its_repeat(mid_pair, cold_ref):
    ctx = _open(mid_pair)
    try:
        for v in (0, 1):
            ctx.set_planes(v, *cold_ref[5][v])
        with _armed(ctx):
            ctx.patchmatch_warm(ITERS, **KW)
            _assert_refused(ctx, ctx.synchronize)
        _assert_usable(ctx, cold_ref[5])
    finally:
        ctx.close()


def test_local_stereo_and_pm_init_keep_before_a_warm_run_do_not(mid_pair):
    from crossscalepatchmatch_amd import capi
    ctx = _open(mid_pair, 3)
    try:
        def start():
            ctx.local_stereo(capi.CA_BOX)
            ctx.pm_init_keep(seed=9)
        start()
        ctx.patchmatch_warm(ITERS, **KW)
        want = _planes(ctx)
        assert _fallbacks(ctx) == 0
        start()
        with _armed(ctx):
            ctx.patchmatch_warm(ITERS, **KW)
            _assert_planes(ctx, want)
        assert _fallbacks(ctx) == 1
    finally:
        ctx.close()


def _merge_host(ctx, pair, scale_num):
    ctx.merge_disparity(0, np.full((pair["h"], pair["w"]), 3.0))


def _local_stereo(ctx, pair, scale_num):
    from crossscalepatchmatch_amd import capi
    ctx.local_stereo(capi.CA_BOX)


def _same_images(ctx, pair, scale_num):
    ctx.set_images(pair["l"], pair["r"])


def _same_cost(ctx, pair, scale_num):
    ctx.build_cost_grd(pair["max_dis"], 35, scale_num, 0.3)


def _rescore(ctx, pair, scale_num):
    ctx.rescore_planes()


@pytest.mark.parametrize("behind, scale_num", [(_merge_host, 5), (_local_stereo, 3), (_same_images, 5), (_same_cost, 5), (_rescore, 5)],
                         ids=["merge_planes_host", "local_stereo", "set_images", "build_cost_grd", "rescore_planes"])
def test_a_call_behind_an_unchecked_run_blocks_its_repeat(mid_pair, cold_ref, behind, scale_num):
    """the run's planes, images or cost object are no longer what it started from"""
    ctx = _open(mid_pair, scale_num)
    try:
        with _armed(ctx):
            ctx.patchmatch(ITERS, **KW)
            behind(ctx, mid_pair, scale_num)
            _assert_refused(ctx, lambda: ctx.get_planes(0))
        if behind is _same_images:  # new images leave the context without a cost object
            _same_cost(ctx, mid_pair, scale_num)
        _assert_usable(ctx, cold_ref[scale_num])
    finally:
        ctx.close()


def test_device_outputs_behind_a_repeated_warm_run(mid_pair):
    """both kinds of map enqueued behind the run are written again from the repeated run's planes"""
    import torch
    h, w = mid_pair["h"], mid_pair["w"]
    ctx = _open(mid_pair)
    try:
        ctx.patchmatch(1, **KW)
        ctx.patchmatch_warm(ITERS, **KW)
        want_pp = ctx.postprocess_f64()
        want_u8 = ctx.disparity_u8(1, 4)
        assert _fallbacks(ctx) == 0
        pp = [torch.zeros((h, w), dtype=torch.float64, device="cuda:0") for _ in (0, 1)]
        u8 = torch.zeros((h, w), dtype=torch.uint8, device="cuda:0")
        ctx.patchmatch(1, **KW)
        ctx.synchronize()
        with _armed(ctx):
            ctx.patchmatch_warm(ITERS, **KW)
            ctx.postprocess_f64_device(pp[0].data_ptr(), pp[1].data_ptr())
            ctx.disparity_u8_device(1, 4, u8.data_ptr())
            ctx.synchronize()
        assert _fallbacks(ctx) == 1
        for v in (0, 1):
            np.testing.assert_array_equal(pp[v].cpu().numpy().view(np.uint64), want_pp[v].view(np.uint64))
        np.testing.assert_array_equal(u8.cpu().numpy(), want_u8)
    finally:
        ctx.close()
