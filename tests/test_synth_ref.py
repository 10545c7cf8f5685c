"""The CPU restatement of specification N (tests/synth_ref.py) against itself and against answers known in closed
form.  No device: the GPU tests (test_gpu_synth.py) hold the library to this restatement bit for bit, and the random cases they use
are checked here first to be non-trivial."""
import math

import numpy as np
import pytest

import synth_ref as sr


def _img(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the two restatements agree bit for bit --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (63, 3), (65, 5), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_loop_and_vectorised_restatements_agree(shape):
    w, h = shape
    D, V, A, I = sr.random_case(w, h, 50 + w)
    for t in sr.TS:
        for views in (1, 2, 3):
            for fill in (0, 1):
                a = sr.synthesize(t, D, V, A, I, views=views, fill=fill)
                b = sr.synthesize_loop(t, D, V, A, I, views=views, fill=fill)
                what = f"{w}x{h} t {t} views {views} fill {fill}"
                assert sr.same_result(a, b), what
                assert sr.same_bits(a["holes"], b["holes"]) and sr.same_bits(a["colour"], b["colour"]), what
    for kw in (dict(max_stretch=1.0), dict(max_stretch=math.inf, merge_diff=0.0), dict(merge_diff=math.inf), dict(max_stretch=1.25, merge_diff=3.5)):
        assert sr.same_result(sr.synthesize(0.5, D, V, A, I, **kw), sr.synthesize_loop(0.5, D, V, A, I, **kw)), kw


def test_ties_go_to_the_smallest_source_x():
    """In exact arithmetic two pixels of one view cannot tie.  In f64 they do: on one plane with a non-dyadic slope the footprints of two
    neighbouring pixels can both claim the target pixel on their common border, with bit-equal d'.  sr.TIE_PLANES were found by search;
    the test asserts that they do tie and that the restatement which keeps a running best (greatest key, then smallest x, whatever
    came first) agrees with the one that sorts."""
    D, A, I = sr.tie_case()
    ties = []
    a = sr.synthesize(1.0, (D, None), (None, None), (A, None), (I, None), views=1, fill=0, ties=ties)
    assert ties[0] >= len(sr.TIE_PLANES), ties
    b = sr.synthesize_loop(1.0, (D, None), (None, None), (A, None), (I, None), views=1, fill=0)
    assert sr.same_result(a, b) and sr.same_bits(a["colour"], b["colour"])


# ---- known answers -----------------------------------------------------------------------------------------------------------------

def test_t0_gives_the_left_image_and_t1_the_right_one():
    w, h = 67, 9
    rng = np.random.default_rng(5)
    D = rng.uniform(0.0, 40.0, (h, w))
    A = rng.uniform(-0.3, 0.3, (h, w))
    I = _img(w, h, 6)
    for fn in (sr.synthesize, sr.synthesize_loop):
        left = fn(0.0, (D, None), (None, None), (A, None), (I, None), views=1)
        assert np.array_equal(left["bgr"], I) and sr.same_bits(left["disp"], D) and np.all(left["mask"] == 1)
        right = fn(1.0, (None, D), (None, None), (None, A), (None, I), views=2)
        assert np.array_equal(right["bgr"], I) and sr.same_bits(right["disp"], D) and np.all(right["mask"] == 2)
    # both views at t = 0: a constant integer disparity puts view 1's warp exactly on view 0's disparity (within merge_diff)
    d = 6
    Dc = np.full((h, w), float(d))
    I1 = _img(w, h, 7)
    both = sr.synthesize(0.0, (Dc, Dc), (None, None), (None, None), (I, I1), views=3)
    assert np.array_equal(both["bgr"], I) and sr.same_bits(both["disp"], Dc) and np.all(both["mask"] != 0) and np.all(both["mask"] != 4)
    assert np.all(both["mask"][:, :d] == 1) and np.all(both["mask"][:, d:] == 3)
    both = sr.synthesize(1.0, (Dc, Dc), (None, None), (None, None), (I1, I), views=3)
    assert np.array_equal(both["bgr"], I) and sr.same_bits(both["disp"], Dc)
    assert np.all(both["mask"][:, w - d:] == 2) and np.all(both["mask"][:, :w - d] == 3)


@pytest.mark.parametrize("d", [2, 8, 20])
def test_constant_even_disparity_shifts_by_half_at_the_middle(d):
    w, h = 50, 4
    D = np.full((h, w), float(d))
    I = _img(w, h, d)
    s = d // 2
    for fn in (sr.synthesize, sr.synthesize_loop):
        res = fn(0.5, (D, None), (None, None), (None, None), (I, None), views=1, fill=0)
        assert np.array_equal(res["bgr"][:, :w - s], I[:, s:]) and np.all(res["mask"][:, :w - s] == 1)
        assert np.all(res["mask"][:, w - s:] == 0) and np.all(res["bgr"][:, w - s:] == 0) and np.all(np.isnan(res["disp"][:, w - s:]))
        assert np.all(res["disp"][:, :w - s] == d)
        res = fn(0.5, (D, None), (None, None), (None, None), (I, None), views=1, fill=1)
        assert np.array_equal(res["bgr"][:, :w - s], I[:, s:])
        assert np.all(res["mask"][:, w - s:] == 4) and np.all(res["disp"] == d)
        assert np.array_equal(res["bgr"][:, w - s:], np.repeat(I[:, w - 1:w], s, axis=1))  # the nearest covered pixel: the last column


def test_two_layers_occlusion_and_background_fill():
    """a near layer (disparity 8, columns 20 .. 39) over a far one (disparity 2), rendered at t = 1 from view 0: the near layer hides
    the far one where both land, the hole it opens (columns 32 .. 37) is filled from the far side, and the mask is 4 exactly there and
    on the two columns nothing reaches at the right border"""
    w, h = 60, 3
    D = np.full((h, w), 2.0)
    D[:, 20:40] = 8.0
    I = _img(w, h, 9)
    for fn in (sr.synthesize, sr.synthesize_loop):
        raw = fn(1.0, (D, None), (None, None), (None, None), (I, None), views=1, fill=0)
        assert np.all(raw["disp"][:, 12:32] == 8.0) and np.array_equal(raw["bgr"][:, 12:32], I[:, 20:40])  # columns 12 .. 17: both layers land
        assert np.all(raw["disp"][:, :12] == 2.0) and np.array_equal(raw["bgr"][:, :12], I[:, 2:14])
        assert np.all(raw["disp"][:, 38:58] == 2.0) and np.array_equal(raw["bgr"][:, 38:58], I[:, 40:60])
        hole = np.zeros((h, w), bool)
        hole[:, 32:38] = True
        hole[:, 58:] = True
        assert np.array_equal(raw["mask"] == 0, hole)
        res = fn(1.0, (D, None), (None, None), (None, None), (I, None), views=1, fill=1)
        assert np.array_equal(res["mask"] == 4, hole) and np.array_equal(res["mask"] == 1, ~hole)
        assert np.all(res["disp"][:, 32:38] == 2.0), "the disocclusion takes the background's disparity"
        assert np.array_equal(res["bgr"][:, 32:38], np.repeat(res["bgr"][:, 38:39], 6, axis=1))
        assert np.array_equal(res["bgr"][:, 58:], np.repeat(res["bgr"][:, 57:58], 2, axis=1))
        assert np.array_equal(res["bgr"][~hole], raw["bgr"][~hole])


# one slanted plane over a ramp.  (t, view, a, b, c): D = a x + b y + c stays >= 0 over the image; g = 1 + sigma a
PLANES = [(0.0, 1, 3.0, 0.125, 0.0),       # g = 4: the cap itself
          (0.0, 1, 0.5, 0.25, 1.0),        # g = 1.5
          (1.0, 0, -0.5, 0.125, 60.0),     # g = 1.5, from view 0
          (0.25, 0, 0.3, -0.0625, 9.0),    # g = 0.925: compressed
          (0.5, 1, 1.7, 0.03125, 0.4),     # g = 1.85
          (0.75, 0, -2.0, 0.5, 200.0)]     # g = 2.5
# The ramp is I = k x with k = 1, 2, 1 per channel (w = 100 keeps 2 x below 256: every value is an integer, so bilinear taps are exact).
# The largest |colour - k xs| measured over PLANES on the CPU (IEEE f64; the test prints it) is 2.85e-14, an ulp of the colour (up to
# 198); the bound asserted is 100 times that.
RAMP_MEASURED, RAMP_BOUND = 2.85e-14, 2.85e-12


@pytest.mark.parametrize("case", PLANES, ids=lambda c: f"t{c[0]}v{c[1]}a{c[2]}")
def test_slanted_plane_over_a_ramp(case):
    t, v, a, b, c = case
    w, h = 100, 5
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    D = a * x + b * y + c
    assert np.all(D >= 0.0)
    A = np.full((h, w), a)
    I = np.zeros((h, w, 3), np.uint8)
    I[..., 0] = np.arange(w)
    I[..., 1] = 2 * np.arange(w)
    I[..., 2] = np.arange(w)
    k = np.array([1.0, 2.0, 1.0])
    sigma = sr.sigmas(t)[v]
    g = 1.0 + sigma * a
    pick = lambda m: (m, None) if v == 0 else (None, m)
    worst = 0.0
    for fn in (sr.synthesize, sr.synthesize_loop):
        res = fn(t, pick(D), (None, None), pick(A), pick(I), views=1 << v, fill=0)
        xs = (x - sigma * (b * y + c)) / g                      # the closed form, x = the target column
        lo, hi = sigma * (b * y + c) - 0.5 * g, (w - 1) * g + sigma * (b * y + c) + 0.5 * g
        covered = (x >= lo + 1e-9) & (x < hi - 1e-9)           # the image of [-0.5, w - 0.5) under the plane's warp
        assert covered.sum() > 20
        assert np.all(res["mask"][covered] == 1 << v), "a crack inside the plane's footprint"
        inside = covered & (xs >= 0.0) & (xs <= w - 1.0)        # where neither bilinear tap is clamped
        err = np.abs(res["colour"] - k * xs[..., None])[inside]
        worst = max(worst, float(err.max()))
        assert err.max() <= RAMP_BOUND, err.max()
        want = k * xs[..., None]
        frac = np.abs(want - np.floor(want) - 0.5)
        sure = inside[..., None] & (frac > RAMP_BOUND)
        assert np.array_equal(res["bgr"][sure], np.rint(want)[sure].astype(np.uint8))
        assert np.all(np.abs(res["disp"] - (a * xs + b * y + c))[inside] <= 1e-11)
    print(f"slanted plane {case}: worst |colour - k xs| = {worst:.3e}")
    dropped = sr.synthesize(t, pick(D), (None, None), (None, None), pick(I), views=1 << v, fill=0)
    holes = int(np.sum(dropped["mask"][covered] == 0))
    if g > 1.0:
        assert holes > 0, "without the slopes a stretched plane must crack: the point of the feature"


def test_unusable_pixels_contribute_nothing():
    w, h = 40, 6
    D, V, A, I = sr.random_case(w, h, 77)
    rng = np.random.default_rng(8)
    for v in (0, 1):
        D[v] = np.where(np.isfinite(D[v]) & (D[v] >= 0), D[v], 5.0)
        A[v] = np.where(np.isfinite(A[v]), np.clip(A[v], -0.3, 0.3), 0.1)
        V[v][:] = 1
    base = dict(max_stretch=2.0)
    t = 0.5
    want = sr.synthesize(t, D, V, A, I, **base)
    bad = rng.random((h, w)) < 0.3
    # every way of being unusable equals V = 0
    Vz = [np.where(bad, 0, V[v]).astype(np.uint8) for v in (0, 1)]
    ref = sr.synthesize(t, D, Vz, A, I, **base)
    assert not sr.same_result(ref, want)
    for value in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
        Db = [np.where(bad, value, D[v]) for v in (0, 1)]
        for fn in (sr.synthesize, sr.synthesize_loop):
            assert sr.same_result(fn(t, Db, V, A, I, **base), ref), value
    # g <= 0 (seen from behind) and g > max_stretch: sigma = -0.5 and +0.5 at t = 0.5
    for a0, a1 in ((2.0, -2.0), (2.5, -7.0), (-2.0 - 1e-9, 2.0 + 1e-9), (-30.0, 30.0)):
        Ab = [np.where(bad, a0, A[0]), np.where(bad, a1, A[1])]
        for fn in (sr.synthesize, sr.synthesize_loop):
            assert sr.same_result(fn(t, D, V, Ab, I, **base), ref), (a0, a1)
    # g = max_stretch exactly is still used
    Ab = [np.where(bad, -2.0, A[0]), np.where(bad, 2.0, A[1])]
    assert not sr.same_result(sr.synthesize(t, D, V, Ab, I, **base), ref)
    # a non-finite slope acts as 0
    Az = [np.where(bad, 0.0, A[v]) for v in (0, 1)]
    for value in (np.nan, np.inf, -np.inf):
        An = [np.where(bad, value, A[v]) for v in (0, 1)]
        for fn in (sr.synthesize, sr.synthesize_loop):
            assert sr.same_result(fn(t, D, V, An, I, **base), fn(t, D, V, Az, I, **base)), value
    assert sr.same_result(sr.synthesize(t, D, (None, None), (None, None), I), sr.synthesize(t, D, V, [np.zeros((h, w))] * 2, I))


def test_a_row_without_a_pixel_stays_a_hole_and_shifts_beyond_the_image_land_nowhere():
    w, h = 33, 4
    D, V, A, I = sr.random_case(w, h, 4)
    for v in (0, 1):
        V[v][1, :] = 0                 # a row with no usable pixel
        V[v][2, :] = 0
        V[v][2, 17] = 1                # a row with a single usable pixel
        D[v][2, 17], A[v][2, 17] = 3.0, 0.0
    for fn in (sr.synthesize, sr.synthesize_loop):
        res = fn(0.5, D, V, A, I)
        assert np.all(res["mask"][1] == 0) and np.all(res["bgr"][1] == 0) and np.all(np.isnan(res["disp"][1]))
        assert set(np.unique(res["mask"][2])) <= {1, 2, 3, 4} and np.sum(res["mask"][2] != 4) in (1, 2)
    far = [np.random.default_rng(1).uniform(w + 1.0, 3.0 * w, (h, w)) for _ in (0, 1)]
    res = sr.synthesize(1.0, far, (None, None), (None, None), I, views=1)
    assert np.all(res["mask"] == 0)
    res = sr.synthesize(0.0, far, (None, None), (None, None), I, views=2)
    assert np.all(res["mask"] == 0)


def test_argument_rules():
    ok = dict(t=0.5, w=8, h=4)
    assert sr.check_args(**ok)
    for bad in (dict(t=math.nan), dict(t=-0.01), dict(t=1.01), dict(views=0), dict(views=4), dict(max_stretch=0.99), dict(max_stretch=math.nan),
                dict(merge_diff=-0.5), dict(merge_diff=math.nan), dict(w=0), dict(h=0), dict(w=1 << 16, h=1 << 15), dict(strides=(24, 23))):
        assert not sr.check_args(**{**ok, **bad}), bad
    assert sr.check_args(**{**ok, "max_stretch": math.inf, "merge_diff": math.inf, "strides": (24, 100)})
    assert sr.check_args(t=0.0, w=8, h=4) and sr.check_args(t=1.0, w=8, h=4)


def test_argument_errors_need_no_device():
    """cspm_synthesize_host checks its arguments before it opens a device: on a machine without one every bad call is CSPM_ERR_ARG
    (a good call fails later, with another code, or succeeds where there is a device)"""
    import ctypes as C
    from crossscalepatchmatch_amd import capi
    L = capi.load_library()
    ERR_ARG = -1
    w, h = 8, 4
    D = np.ones((h, w))
    img = np.zeros((h, w, 3), np.uint8)
    p = capi.synth_params()
    assert (p.views, p.fill, p.max_stretch, p.merge_diff) == (sr.DEFAULTS["views"], sr.DEFAULTS["fill"], sr.DEFAULTS["max_stretch"], sr.DEFAULTS["merge_diff"])
    view = capi.SynthView(capi._dp(D), None, None, capi._u8(img), 3 * w)
    short = capi.SynthView(capi._dp(D), None, None, capi._u8(img), 3 * w - 1)
    nodisp = capi.SynthView(None, None, None, capi._u8(img), 3 * w)
    noimg = capi.SynthView(capi._dp(D), None, None, None, 3 * w)

    def host(t=0.5, params=p, v0=view, v1=view, ww=w, hh=h, stride=3 * w, bgr=True):
        return L.cspm_synthesize_host(0, C.byref(params) if params is not None else None, t, C.byref(v0) if v0 is not None else None,
                                      C.byref(v1) if v1 is not None else None, ww, hh, capi._u8(img) if bgr else None, stride, None, None)

    for t in (math.nan, -0.5, 1.5, math.inf):
        assert host(t=t) == ERR_ARG and not sr.check_args(t, w, h)
        assert b"view synthesis" in L.cspm_last_error(None)
    for bad in (dict(views=0), dict(views=4), dict(max_stretch=0.5), dict(max_stretch=math.nan), dict(merge_diff=-1.0), dict(merge_diff=math.nan)):
        assert host(params=capi.synth_params(**bad)) == ERR_ARG and not sr.check_args(0.5, w, h, **bad), bad
    assert host(v0=None) == ERR_ARG and host(v1=None) == ERR_ARG and host(v0=nodisp) == ERR_ARG and host(v1=noimg) == ERR_ARG
    assert host(ww=0) == ERR_ARG and host(hh=0) == ERR_ARG and host(ww=1 << 12, hh=1 << 19) == ERR_ARG
    assert host(ww=capi.SYNTH_MAX_WIDTH + 1, hh=1, stride=3 * (capi.SYNTH_MAX_WIDTH + 1)) == ERR_ARG
    assert host(v0=short) == ERR_ARG and host(v1=short) == ERR_ARG and host(stride=3 * w - 1) == ERR_ARG
    assert L.cspm_synth_default_params(None) == ERR_ARG
    assert L.cspm_synthesize(None, 0, None, 0.5, None, 0, None, None) == ERR_ARG
    assert L.cspm_synthesize_device(None, 0, None, 0.5, None, 0, None, None) == ERR_ARG
    assert C.sizeof(capi.SynthParams) == 24 and C.sizeof(capi.SynthView) == 40


# ---- the GPU tests' random cases are non-trivial -------------------------------------------------------------------------------------

def test_the_shared_random_cases_are_not_trivial():
    seen = set()
    for shape in sr.SHAPES:
        w, h = shape
        D, V, A, I = sr.shape_case(shape)
        for t in sr.TS:
            for views in (1, 2, 3):
                res = sr.synthesize(t, D, V, A, I, views=views, fill=1)
                frac = float(np.mean(res["holes"] == 0))
                assert w * h < 64 or 0.02 <= frac <= 0.98, (shape, t, views, frac)
                seen |= set(np.unique(res["mask"])) | set(np.unique(res["holes"]))
    assert seen == {0, 1, 2, 3, 4}
