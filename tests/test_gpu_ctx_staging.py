"""The context entries that move data between caller memory and the device (crossscalepatchmatch_amd/csrc/cspm_api.hip, DESIGN.md
section 16), called through the ctypes handle on odd_pair (77 x 41: ragged wave tails, a kept-pixel count that is neither 0 nor w * h):
every optional output alone and none at all against the all-outputs call bit for bit, with poisoned buffers that must stay poisoned where
nothing was asked for; record capacities around the count; the same calls on a caller's stream; and the three users of the candidate
buffer (merge_planes, fit_planes(merge), segment_planes(merge)) one behind the other.  The error paths of these entries (a HIP call that
fails mid-entry) are not exercised: that would take a device failure."""
import ctypes as C

import numpy as np
import pytest

import rectify_ref as rr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

CAL = (300.0, 31.5, 20.25, 0.25, 3.5)
GEOM = dict(min_cos=0.3, z_far=12.0)
POISON = 0xA7


def _poisoned(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = POISON
    return a


def _is_poison(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == POISON))


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _start(ctx, pair):
    ctx.set_images(pair["l"], pair["r"])
    ctx.build_cost_grd(pair["max_dis"], 9, 3, 0.3)
    ctx.set_pp_speckle(0)
    ctx.set_pp_median(0)
    ctx.patchmatch(1, seed=5)


@pytest.fixture(scope="module")
def ctx(_gpu_ctx_session, odd_pair):
    """a context of this module's own with one finished run on odd_pair"""
    c = capi.StereoContext(0)
    _start(c, odd_pair)
    yield c
    c.close()


def _call(ctx, fn, *args):
    rc = fn(ctx.p, *args)
    assert rc == 0, ctx.L.cspm_last_error(ctx.p).decode()


def _reproject(ctx, names, cap=None, view=0):
    """cspm_reproject with the outputs in `names` (of depth, xyz, normal, keep, cloud, count) and NULL for the rest; every buffer comes
    back, poisoned where the library did not write"""
    w, h = ctx.w, ctx.h
    cap = w * h if cap is None else cap
    b = dict(depth=_poisoned((h, w), np.float64), xyz=_poisoned((3, h, w), np.float64), normal=_poisoned((3, h, w), np.float64),
             keep=_poisoned((h, w), np.uint8), cloud=_poisoned(w * h + 8, capi.Point), count=_poisoned(1, np.uint32))
    k, g = capi.calib_struct(CAL), capi.geom_params(**GEOM)
    arg = lambda name, conv: conv(b[name]) if name in names else None
    _call(ctx, ctx.L.cspm_reproject, view, capi.GEOM_RAW, C.byref(k), C.byref(g), None, arg("depth", capi._dp), arg("xyz", capi._dp),
          arg("normal", capi._dp), arg("keep", capi._u8), arg("cloud", capi._vp), cap, arg("count", lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))))
    return b


def _mesh(ctx, names, vcap=None, fcap=None, view=0):
    """cspm_mesh with the outputs in `names` (of vertices, faces, quad, n_vertices, n_faces) and NULL for the rest"""
    w, h = ctx.w, ctx.h
    vcap = w * h if vcap is None else vcap
    fcap = 2 * w * h if fcap is None else fcap
    b = dict(vertices=_poisoned(w * h + 8, capi.Point), faces=_poisoned(2 * w * h + 8, capi.Face), quad=_poisoned((h, w), np.uint8),
             n_vertices=_poisoned(1, np.uint32), n_faces=_poisoned(1, np.uint32))
    k, g, m = capi.calib_struct(CAL), capi.geom_params(**GEOM), capi.mesh_params(max_diff=2.0)
    arg = lambda name, conv: conv(b[name]) if name in names else None
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))
    _call(ctx, ctx.L.cspm_mesh, view, capi.GEOM_RAW, C.byref(k), C.byref(g), None, C.byref(m), arg("vertices", capi._vp), vcap, arg("faces", capi._vp),
          fcap, arg("quad", capi._u8), arg("n_vertices", up), arg("n_faces", up))
    return b


def _alone_and_none(call, names, full):
    """every output of `names` requested alone, and none of them: what was asked for equals `full`, the rest is still poison"""
    for pick in list(names) + [None]:
        got = call([pick] if pick else [])
        for name in names:
            if name == pick:
                assert _same(got[name], full[name]), f"{name} alone differs from the all-outputs call"
            else:
                assert _is_poison(got[name]), f"{name} was written although only {pick} was asked for"


@pytest.fixture(scope="module")
def full_reproject(ctx):
    return _reproject(ctx, ("depth", "xyz", "normal", "keep", "cloud", "count"))


@pytest.fixture(scope="module")
def full_mesh(ctx):
    return _mesh(ctx, ("vertices", "faces", "quad", "n_vertices", "n_faces"))


def test_reproject_outputs_alone_and_none(ctx, full_reproject):
    full, n = full_reproject, ctx.w * ctx.h
    count = int(full["count"][0])
    print(f"reproject: {count} of {n} pixels kept")
    assert 0 < count < n
    assert not _is_poison(full["cloud"][:count]) and _is_poison(full["cloud"][count:])
    _alone_and_none(lambda names: _reproject(ctx, names), ("depth", "xyz", "normal", "keep", "cloud", "count"), full)


def test_reproject_capacities(ctx, full_reproject):
    full, n = full_reproject, ctx.w * ctx.h
    count = int(full["count"][0])
    for cap in (0, 1, count - 1, count, count + 1, n):
        got = _reproject(ctx, ("cloud", "count"), cap)
        wrote = min(count, cap)
        assert int(got["count"][0]) == count, cap
        assert _same(got["cloud"][:wrote], full["cloud"][:wrote]) and _is_poison(got["cloud"][wrote:]), cap


def test_mesh_outputs_alone_and_none(ctx, full_mesh):
    full, n = full_mesh, ctx.w * ctx.h
    nv, nf = int(full["n_vertices"][0]), int(full["n_faces"][0])
    print(f"mesh: {nv} vertices, {nf} faces of {n} pixels")
    assert 0 < nv < n and 0 < nf < 2 * n
    assert _is_poison(full["vertices"][nv:]) and _is_poison(full["faces"][nf:])
    _alone_and_none(lambda names: _mesh(ctx, names), ("vertices", "faces", "quad", "n_vertices", "n_faces"), full)


def test_mesh_capacities(ctx, full_mesh):
    full, n = full_mesh, ctx.w * ctx.h
    nv, nf = int(full["n_vertices"][0]), int(full["n_faces"][0])
    for vcap, fcap in ((0, 0), (1, 1), (nv - 1, nf - 1), (nv, nf), (nv + 1, nf + 1), (n, n)):
        got = _mesh(ctx, ("vertices", "faces", "n_vertices", "n_faces"), vcap, fcap)
        wv, wf = min(nv, vcap), min(nf, fcap)
        assert (int(got["n_vertices"][0]), int(got["n_faces"][0])) == (nv, nf), (vcap, fcap)
        assert _same(got["vertices"][:wv], full["vertices"][:wv]) and _is_poison(got["vertices"][wv:]), vcap
        assert _same(got["faces"][:wf], full["faces"][:wf]) and _is_poison(got["faces"][wf:]), fcap


def test_reproject_and_mesh_on_a_caller_stream(ctx, full_reproject, full_mesh):
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    own = ctx.stream_ptr()
    ctx.set_stream(stream.cuda_stream)
    try:
        assert ctx.stream_ptr() == stream.cuda_stream
        count, nv, nf = int(full_reproject["count"][0]), int(full_mesh["n_vertices"][0]), int(full_mesh["n_faces"][0])
        got = _reproject(ctx, ("depth", "xyz", "normal", "keep", "cloud", "count"))
        for name in got:
            assert _same(got[name], full_reproject[name]), name
        got = _reproject(ctx, ("cloud", "count"), count - 1)
        assert int(got["count"][0]) == count and _same(got["cloud"][:count - 1], full_reproject["cloud"][:count - 1]) and _is_poison(got["cloud"][count - 1:])
        got = _mesh(ctx, ("vertices", "faces", "quad", "n_vertices", "n_faces"))
        for name in got:
            assert _same(got[name], full_mesh[name]), name
        got = _mesh(ctx, ("vertices", "faces", "n_vertices", "n_faces"), nv - 1, nf - 1)
        assert (int(got["n_vertices"][0]), int(got["n_faces"][0])) == (nv, nf)
        assert _same(got["vertices"][:nv - 1], full_mesh["vertices"][:nv - 1]) and _is_poison(got["vertices"][nv - 1:])
        assert _same(got["faces"][:nf - 1], full_mesh["faces"][:nf - 1]) and _is_poison(got["faces"][nf - 1:])
    finally:
        ctx.set_stream(0)
    assert ctx.stream_ptr() == own


def test_synthesize_outputs_alone_and_none(ctx):
    w, h = ctx.w, ctx.h
    p = capi.synth_params()

    def call(names):
        b = dict(bgr=_poisoned((h, w * 3 + 5), np.uint8), disp=_poisoned((h, w), np.float64), mask=_poisoned((h, w), np.uint8))
        arg = lambda name, conv: conv(b[name]) if name in names else None
        _call(ctx, ctx.L.cspm_synthesize, capi.GEOM_RAW, C.byref(p), 0.5, arg("bgr", capi._u8), w * 3 + 5, arg("disp", capi._dp), arg("mask", capi._u8))
        return b

    full = call(("bgr", "disp", "mask"))
    assert not _is_poison(full["bgr"][:, :w * 3]) and _is_poison(full["bgr"][:, w * 3:]), "the padding of the image rows was written"
    assert 0 < np.count_nonzero(full["mask"]) and not _is_poison(full["disp"])
    _alone_and_none(call, ("bgr", "disp", "mask"), full)


def test_postprocess_f64_outputs_alone_and_none(ctx):
    w, h = ctx.w, ctx.h

    def call(names):
        b = dict(l=_poisoned((h, w), np.float64), r=_poisoned((h, w), np.float64), l_valid=_poisoned((h, w), np.uint8), r_valid=_poisoned((h, w), np.uint8))
        arg = lambda name: capi._u8(b[name]) if name in names else None
        _call(ctx, ctx.L.cspm_postprocess_f64, capi._dp(b["l"]), capi._dp(b["r"]), arg("l_valid"), arg("r_valid"))
        return b

    full = call(("l_valid", "r_valid"))
    for v in ("l_valid", "r_valid"):
        assert set(np.unique(full[v])) == {0, 1}, "the left-right check is expected to pass some pixels of odd_pair and to fail some"
    for pick in ("l_valid", "r_valid", None):
        got = call([pick] if pick else [])
        assert _same(got["l"], full["l"]) and _same(got["r"], full["r"])
        for name in ("l_valid", "r_valid"):
            assert _same(got[name], full[name]) if name == pick else _is_poison(got[name]), (name, pick)


def test_rect_map_outputs_alone_and_none(_gpu_ctx_session):
    w, h = 77, 41
    rig = rr.random_rig(np.random.default_rng(31))
    rect, _ = rr.compute(rig, w=w, h=h)
    c = capi.StereoContext(0)
    try:
        c.set_rectification(rr.capi_rig(rig), rr.capi_rect(rect))

        def call(names):
            b = dict(xy=_poisoned((2, h, w), np.float64), valid=_poisoned((h, w), np.uint8))
            _call(c, c.L.cspm_get_rect_map, 1, capi._dp(b["xy"]) if "xy" in names else None, capi._u8(b["valid"]) if "valid" in names else None)
            return b

        full = call(("xy", "valid"))
        sx, sy, valid = c.rect_map(1)
        assert _same(full["xy"][0], sx) and _same(full["xy"][1], sy) and _same(full["valid"], valid) and 0 < np.count_nonzero(valid)
        _alone_and_none(call, ("xy", "valid"), full)
    finally:
        c.close()


def _candidate_chain(c, pair, steps, sync):
    """merge_planes with a mask over a field that has NaN planes, fit_planes(merge) and segment_planes(merge) on one context; the field
    after each of the first `steps` steps (planes and costs of both views), read back only where `sync` says so"""
    w, h = pair["w"], pair["h"]
    rng = np.random.default_rng(3)
    field = capi.disparity_planes(rng.uniform(1.0, pair["max_dis"] - 1.0, (h, w)))
    field[rng.uniform(size=(h, w)) < 0.2] = np.nan  # no candidates, in and outside the mask
    mask = rng.uniform(size=(h, w)) < 0.6
    todo = [lambda: c.merge_planes(1, field, mask), lambda: c.fit_planes(merge=True, radius=2), lambda: c.segment_planes(merge=True, step=8)][:steps]
    states = []
    for k, step in enumerate(todo):
        step()
        if sync or k == steps - 1:
            states.append([c.get_planes(v) for v in (0, 1)])
    return states


def test_candidate_buffer_users_follow_one_another(ctx, odd_pair):
    chain = _candidate_chain(ctx, odd_pair, 3, sync=True)  # every step's field is read back before the next step
    start = None
    for k in (1, 2, 3):
        other = capi.StereoContext(0)
        try:
            _start(other, odd_pair)
            if start is None:
                start = [other.get_planes(v) for v in (0, 1)]
            last = _candidate_chain(other, odd_pair, k, sync=False)[-1]  # the steps before it enqueued back to back, then step k
        finally:
            other.close()
        for v in (0, 1):
            assert _same(last[v][0], chain[k - 1][v][0]) and _same(last[v][1], chain[k - 1][v][1]), f"step {k}, view {v}"
    # every step changed the field it found, and lowered no pixel's cost
    before = start
    for k, state in enumerate(chain):
        changed = sum(int(np.count_nonzero(state[v][1] != before[v][1])) for v in (0, 1))
        print(f"step {k + 1}: {changed} pixels took a candidate")
        assert changed > 0 and not any(np.any(state[v][1] > before[v][1]) for v in (0, 1)), f"step {k + 1}"
        before = state
