"""The aggregation kernels (csrc/cspm_ca.h) against what the reference's OWN filters computed, and the batched paths of aggregation
and local stereo, which run only above 128 slices.

1. cspm_aggregate_cv_host on every recorded aggreCV case of tests/test_reference_ca.py against the record itself
   (tests/golden/refca_*.npz: output of ca_filter/*.cpp compiled unmodified): BOX and GF bit for bit, BF within rtol 1e-12 (only exp
   differs, see tests/test_reference_ca.py); the largest BF difference is printed (-s) and kept in DESIGN.md section 10.
2. The walks have one lane per column / row in workgroups of 64: W and H at 63 / 64 / 65, against tests/ca_ref.py.
3. k_ca_bf filters register blocks of 8 slices: 8, 9, 16, 17 filtered slices.
4. cspm_aggregate_cv_host's batch loop: 130 and 257 filtered slices are two and three trips (ca_batch is 128 for small slabs).
5. Local stereo over several level-0 batches (max_dis 176: d = 1..127 | 128..175; max_dis 320: 1..127 | 128..254 | 255..319, and a
   level 1 of 160 filtered slices assembled from two filter calls): planes and min_cost exact against ca_ref.  The cost cells are
   uniform random slabs uploaded through cspm_begin_cost / cspm_upload_cost_slab / cspm_finish_cost, so that the winners spread
   over all d: the test asserts on the ca_ref expectation alone that in each view at least 10 % of the pixels win on each side of
   every batch boundary.  One constructed tie: equal minimum costs on both sides of a boundary, the smaller d must win.
6. BF through two level-0 batches at its smallest legal size.

Reads tests/golden/ only."""
import numpy as np
import pytest

import ca_ref
import test_reference_ca as rca
from crossscalepatchmatch_amd import capi
from crossscalepatchmatch_amd.synth import make_pair
from test_gpu_local_stereo import METHODS, _check, _expected, _expected_bf

pytestmark = pytest.mark.gpu

BATCH = 128  # ca_batch() of any slab below ~630 K pixels (cspm_api.hip)


@pytest.mark.parametrize("name,op,dims,slabs,guide", [c for c in rca.CASES if c[1] in METHODS], ids=[c[0] for c in rca.CASES if c[1] in METHODS])
def test_aggregate_cv_host_equals_the_reference_record(gpu_ctx, name, op, dims, slabs, guide):
    g, vol, want = rca.load_record(name)
    got = capi.aggregate_cv_host(0, METHODS[op], g, vol)
    np.testing.assert_array_equal(got[0], vol[0], err_msg=f"{name}: slice 0 untouched")
    if op == "BF":
        if len(vol) > 1:
            print(f"{name}: kernel vs record, largest relative difference {rca.max_rel_diff(got[1:], want[1:]):.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"{name}: k_ca_bf against the reference's BilateralFilter")
    else:
        np.testing.assert_array_equal(got, want, err_msg=f"{name}: the kernels against the reference's own {op} filter")


@pytest.mark.parametrize("method", ["BOX", "GF"])
@pytest.mark.parametrize("w,h", [(63, 20), (64, 20), (65, 20), (20, 63), (20, 64), (20, 65), (129, 65)])
def test_walks_at_workgroup_edges(gpu_ctx, method, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    guide = rng.random((h, w, 3))
    vol = rng.normal(0.0, 5.0, (3, h, w))
    np.testing.assert_array_equal(capi.aggregate_cv_host(0, METHODS[method], guide, vol), ca_ref.aggre_cv(method, guide, vol))


@pytest.mark.parametrize("filtered", [8, 9, 16, 17])
def test_bf_register_blocks(gpu_ctx, filtered):
    w, h = 20, 17
    rng = np.random.default_rng(filtered)
    guide = rng.random((h, w, 3))
    vol = rng.uniform(0.5, 10.0, (filtered + 1, h, w))  # every slice different
    got = capi.aggregate_cv_host(0, capi.CA_BF, guide, vol)
    want = ca_ref.aggre_cv("BF", guide, vol)
    print(f"BF {filtered} slices: kernel vs ca_ref, largest relative difference {rca.max_rel_diff(got[1:], want[1:]):.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    for d in range(1, filtered + 1):  # no slice left as it came or filled from a neighbour
        assert not np.array_equal(got[d], vol[d]) and not np.array_equal(got[d], got[d - 1])


@pytest.mark.parametrize("method", ["BOX", "GF"])
@pytest.mark.parametrize("n", [131, 258])  # 130 = 128 + 2 and 257 = 128 + 128 + 1 filtered slices
def test_host_batch_loop(gpu_ctx, method, n):
    w, h = 24, 21
    assert -(-(n - 1) // BATCH) == {131: 2, 258: 3}[n]
    rng = np.random.default_rng(n)
    guide = rng.random((h, w, 3))
    vol = rng.normal(0.0, 5.0, (n, h, w))
    np.testing.assert_array_equal(capi.aggregate_cv_host(0, METHODS[method], guide, vol), ca_ref.aggre_cv(method, guide, vol))


def _boundaries(max_dis):
    """the first d of every level-0 batch after the first: batch k folds d = 1 + 127 k .. min(127 (k + 1), max_dis - 1) (ca_local_view)"""
    return list(range(BATCH, max_dis, BATCH - 1))


def _upload(ctx, w, h, max_dis, scale_num, lam, seed, slab_of):
    """a noise pair (the guides) and cost cells slab_of(rng, v, s, d, h_s, w_s) uploaded for every view, level and d"""
    l, r, _, _ = make_pair(w, h, 8, seed=seed)
    ctx.set_images(l, r)
    ctx.begin_cost(max_dis, 35, scale_num, lam)
    rng = np.random.default_rng(seed)
    for v in range(2):
        for s in range(ctx.levels):
            ws, hs, D = ctx.level_dims(s)
            for d in range(D + 1):
                ctx.upload_cost_slab(v, s, d, slab_of(rng, v, s, d, hs, ws))
    ctx.finish_cost()


def _uniform(rng, v, s, d, h, w):
    return rng.uniform(0.5, 10.0, (h, w))


def _assert_both_sides(exp, max_dis, tag):
    bounds = _boundaries(max_dis)
    for v in range(2):
        d = exp[v][0]
        for b in bounds:
            below, above = float(np.mean(d < b)), float(np.mean(d >= b))
            print(f"{tag} view {v}: d* < {b} at {below:.3f} of the pixels, d* >= {b} at {above:.3f}")
            assert below >= 0.10 and above >= 0.10, (tag, v, b, below, above)
    return bounds


# GF needs 19 at every level: 40x38 -> 20x19; BOX needs 7: 36x30 -> 18x15
@pytest.mark.parametrize("method,w,h,max_dis,scale_num", [("BOX", 36, 30, 176, 0), ("BOX", 36, 30, 176, 2), ("BOX", 36, 30, 320, 0), ("BOX", 36, 30, 320, 2),
                                                          ("GF", 40, 38, 176, 0), ("GF", 40, 38, 176, 2), ("GF", 40, 38, 320, 0), ("GF", 40, 38, 320, 2)])
def test_local_stereo_over_several_batches(gpu_ctx, method, w, h, max_dis, scale_num):
    tag = f"{method}/{w}x{h}/D{max_dis}/s{scale_num}"
    _upload(gpu_ctx, w, h, max_dis, scale_num, 0.3 if scale_num else 0.0, max_dis + scale_num, _uniform)
    for s in range(gpu_ctx.levels):
        ws, hs, _ = gpu_ctx.level_dims(s)
        assert min(ws, hs) >= ca_ref.MIN_SIZE[method]
    assert gpu_ctx.level_dims(0)[2] == max_dis
    if max_dis == 320 and scale_num:
        assert gpu_ctx.level_dims(1)[2] > BATCH  # level 1 is assembled from two filter calls
    exp = _expected(gpu_ctx, method, max_dis, scale_num)
    assert len(_assert_both_sides(exp, max_dis, tag)) == (1 if max_dis == 176 else 2)
    gpu_ctx.local_stereo(METHODS[method])
    _check(gpu_ctx, method, exp, tag)


def test_local_stereo_tie_across_a_batch_boundary(gpu_ctx):
    """BOX over small integers and halves: every sum is exact.  Left third: slabs 127 and 128 are the equal minimum (the last d of
    batch 0 and the first of batch 1) -> 127 wins.  Middle third: 254 and 255 likewise -> 254.  Right third: 128 is strictly lower
    than 127 -> 128, a winner that only the second batch sees."""
    w, h, max_dis = 24, 14, 258
    third = w // 3

    def slab_of(rng, v, s, d, hs, ws):
        slab = rng.integers(5, 20, (hs, ws)).astype(np.float64)
        if d in (127, 128):
            slab[:, :third] = 1.0
            slab[:, 2 * third:] = 1.0 if d == 127 else 0.5
        if d in (254, 255):
            slab[:, third:2 * third] = 1.0
        return slab

    _upload(gpu_ctx, w, h, max_dis, 0, 0.0, 77, slab_of)
    assert _boundaries(max_dis) == [128, 255]
    exp = _expected(gpu_ctx, "BOX", max_dis, 0)
    for v in range(2):
        agg = ca_ref.aggre_cv("BOX", np.zeros((h, w, 3)), gpu_ctx.cost_volume(v, 0))
        costs = ca_ref.local_costs([agg], [ca_ref.level_max(agg)], [1.0], False, max_dis, w, h)  # costs[d - 1]
        best = costs.min(axis=0)
        for lo, want_d, x in ((127, 127, 0), (254, 254, third + third // 2)):
            tie = (costs[lo - 1] == best) & (costs[lo] == best)
            assert tie[:, x].all(), f"view {v}: the constructed tie of d = {lo}, {lo + 1} is not the minimum at column {x}"
            assert (exp[v][0][tie] == want_d).all()
        assert (exp[v][0][:, w - 1] == 128).all() and (costs[127][:, w - 1] < costs[126][:, w - 1]).all()
    gpu_ctx.local_stereo(capi.CA_BOX)
    _check(gpu_ctx, "BOX", exp, "tie")


def test_local_stereo_bf_over_two_batches(gpu_ctx):
    w, h, max_dis = 17, 17, 176  # BF's smallest size; d = 1..127 | 128..175
    _upload(gpu_ctx, w, h, max_dis, 0, 0.0, 5, _uniform)
    exp = _expected_bf(gpu_ctx, max_dis, 0)
    assert _assert_both_sides(exp, max_dis, "BF") == [128]
    gpu_ctx.local_stereo(capi.CA_BF)
    for v in range(2):
        print(f"BF two batches view {v}: min_cost vs ca_ref, largest relative difference {rca.max_rel_diff(gpu_ctx.get_planes(v)[1], exp[v][1]):.3e}")
    _check(gpu_ctx, "BF", exp, "BF/two batches")
