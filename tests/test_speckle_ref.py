"""-m "not gpu": the CPU restatement of the speckle filter (tests/speckle_ref.py) on hand cases, and against an
independent labelling of the mask where max_diff = inf makes the disparities irrelevant."""
import numpy as np
import pytest

import speckle_ref as sr

INF = float("inf")


def _blob(h, w, cells, value=5.0, background=50.0):
    d = np.full((h, w), background)
    for y, x in cells:
        d[y, x] = value
    return d


def test_a_component_of_exactly_max_size_is_removed_and_one_more_pixel_keeps_it():
    d = np.full((9, 12), 50.0)
    d[1, 1:6] = 5.0            # 5 pixels
    d[4:6, 2:5] = 9.0          # 6 pixels
    valid = np.zeros((9, 12), np.uint8)
    valid[1, 1:6] = valid[4:6, 2:5] = 1
    out, n = sr.speckle_filter(d, valid, 5, 1.0)
    assert (n[1, 1:6] == 5).all() and (n[4:6, 2:5] == 6).all() and n.sum() == 5 * 5 + 6 * 6
    assert not out[1, 1:6].any() and out[4:6, 2:5].all() and out.sum() == 6
    out, _ = sr.speckle_filter(d, valid, 6, 1.0)
    assert not out.any()
    out, _ = sr.speckle_filter(d, valid, 4, 1.0)
    assert np.array_equal(out, valid)


def test_diagonal_neighbours_are_not_joined():
    d = _blob(6, 6, [(1, 1), (2, 2), (3, 3), (3, 4)])
    _, n = sr.speckle_filter(d, None, 1, 1.0)
    assert n[1, 1] == 1 and n[2, 2] == 1 and n[3, 3] == 2 and n[3, 4] == 2
    assert n[0, 0] == 36 - 4  # the background flows round the staircase through the 4-neighbourhood


def test_a_ramp_is_one_component_although_its_ends_differ_by_far_more_than_max_diff():
    d = np.arange(40, dtype=np.float64)[None, :] * 0.75  # steps of 0.75 <= 1, ends 29.25 apart
    out, n = sr.speckle_filter(d, None, 39, 1.0)
    assert (n == 40).all() and out.all()
    out, n = sr.speckle_filter(d, None, 39, 0.5)      # steps above the threshold: forty components of one pixel
    assert (n == 1).all() and not out.any()
    d2 = d.copy()
    d2[0, 20:] += 0.5                                  # one step of 1.25 cuts the ramp in two
    _, n = sr.speckle_filter(d2, None, 0, 1.0)
    assert (n == 20).all()


def test_an_invalid_column_splits_a_region():
    d = np.full((5, 9), 7.0)
    valid = np.ones((5, 9), np.uint8)
    valid[:, 3] = 0
    out, n = sr.speckle_filter(d, valid, 15, 1.0)
    assert (n[:, :3] == 15).all() and (n[:, 3] == 0).all() and (n[:, 4:] == 25).all()
    assert not out[:, :4].any() and out[:, 4:].all()
    valid[2, 3] = 1                                     # one valid pixel in the column bridges the two sides
    _, n = sr.speckle_filter(d, valid, 15, 1.0)
    assert (n[valid == 1] == 41).all()


def test_a_nan_pixel_is_a_component_of_its_own():
    d = np.full((4, 7), 3.0)
    d[:, 3] = np.nan                                    # a NaN column: every pixel of it alone, and the sides apart
    out, n = sr.speckle_filter(d, None, 1, INF)
    assert (n[:, 3] == 1).all() and (n[:, :3] == 12).all() and (n[:, 4:] == 12).all()
    assert not out[:, 3].any() and out[:, :3].all() and out[:, 4:].all()


def test_max_size_zero_is_the_identity():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 3, (13, 17)).astype(np.float64)
    d[rng.random((13, 17)) < 0.1] = np.nan
    valid = (rng.random((13, 17)) < 0.7).astype(np.uint8)
    out, n = sr.speckle_filter(d, valid, 0, 1.0)
    assert np.array_equal(out, valid)
    assert ((n > 0) == (valid == 1)).all()
    out, _ = sr.speckle_filter(d, None, 0, 0.0)
    assert out.all()


def test_the_comparison_is_pairwise_not_against_a_seed():
    d = np.array([[0.0, 1.0, 2.0, 1.0, 0.0, 5.0]])
    _, n = sr.speckle_filter(d, None, 0, 1.0)
    assert n.tolist() == [[5, 5, 5, 5, 5, 1]]


def _flood_sizes(mask):
    """a second, differently written labelling: breadth-first flood fill from every unvisited pixel of the mask"""
    h, w = mask.shape
    n = np.zeros((h, w), np.int32)
    seen = np.zeros((h, w), bool)
    for y0 in range(h):
        for x0 in range(w):
            if not mask[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            todo, k = [(y0, x0)], 0
            while k < len(todo):
                y, x = todo[k]
                k += 1
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not seen[yy, xx]:
                        seen[yy, xx] = True
                        todo.append((yy, xx))
            for y, x in todo:
                n[y, x] = len(todo)
    return n


@pytest.mark.parametrize("shape,density,seed", [((1, 1), 1.0, 0), ((1, 40), 0.7, 1), ((40, 1), 0.7, 2), ((33, 47), 0.6, 3), ((70, 131), 0.55, 4),
                                                ((20, 20), 1.0, 5)])
def test_with_an_infinite_max_diff_the_filter_labels_the_mask_alone(shape, density, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < density
    d = rng.normal(0.0, 1e6, shape)  # finite, and irrelevant
    out, n = sr.speckle_filter(d, mask, 7, INF)
    try:
        from scipy import ndimage
    except ImportError:
        want = _flood_sizes(mask)
    else:
        lab, k = ndimage.label(mask)  # the default structure is the 4-neighbourhood
        want = np.where(mask, np.bincount(lab.ravel(), minlength=k + 1)[lab], 0).astype(np.int32)
        assert np.array_equal(want, _flood_sizes(mask))
    assert np.array_equal(n, want)
    assert np.array_equal(out, (mask & (want > 7)).astype(np.uint8))


def test_postprocess_with_max_size_zero_is_pp_sub_ref():
    import pp_sub_ref as ps
    rng = np.random.default_rng(9)
    h, w = 12, 40
    d = rng.choice([3.0, 4.0], (h, w))
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    abc = [ps.fronto_field(d), ps.fronto_field(d)]
    a = ps.postprocess_f64(abc[0], abc[1], img, img, 16)
    b = sr.postprocess_f64_speckle(abc[0], abc[1], img, img, 16, 0, 1.0)
    assert b[4] == 0
    for x, y in zip(a, b[:4]):
        assert np.array_equal(x, y)
    c = sr.postprocess_f64_speckle(abc[0], abc[1], img, img, 16, 3, 0.0)  # speckles of the two-valued noise leave the masks
    assert c[4] > 0 and c[4] == int((a[2] != c[2]).sum() + (a[3] != c[3]).sum())
    assert not (c[2] & ~a[2]).any()


# ---- the public surface (host logic only: no device needed) ----------------------------------------------------------------------
def test_new_symbols_are_exported_bound_and_check_their_arguments():
    import ctypes as C
    from crossscalepatchmatch_amd import capi
    L = capi.load_library()
    for name in ("cspm_set_pp_speckle", "cspm_get_pp_speckle", "cspm_filter_speckles_host"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert capi.OPT_PP_SPECKLE_REMOVED == 21
    assert callable(capi.StereoContext.set_pp_speckle) and callable(capi.StereoContext.get_pp_speckle) and callable(capi.filter_speckles)
    assert L.cspm_set_pp_speckle(None, 5, 1.0) == -1 and L.cspm_get_pp_speckle(None, None, None) == -1  # CSPM_ERR_ARG without a context
    d = np.zeros((2, 2))
    out = np.zeros((2, 2), np.uint8)
    dp, op = d.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.cspm_filter_speckles_host(0, dp, None, 1 << 16, 1 << 15, 1, 1.0, op, None) == -1  # w * h == 2^31, refused before any device call
    assert b"2^31" in L.cspm_last_error(None)
    for size, diff in ((-1, 1.0), (1, -1.0), (1, float("nan"))):
        assert L.cspm_filter_speckles_host(0, dp, None, 2, 2, size, diff, op, None) == -1


def test_cli_refuses_a_speckle_size_without_use_pp(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(exe), "build the host layer: python -c 'import __graft_entry__ as g; g.build()'"
    common = [exe, f"--l_img_file={tmp_path}/none.png", f"--r_img_file={tmp_path}/none.png", "--max_dis=16", "--dis_scale=4", "--cc_name=GRD",
              f"--l_disp_pfm={tmp_path}/l.pfm"]
    p = subprocess.run(common + ["--pp_speckle_size=50", "--pp_speckle_diff=2"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--pp_speckle_size" in p.stdout and b"--use_pp" in p.stdout
    p = subprocess.run(common + ["--use_pp", "--pp_speckle_size=-3"], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"--pp_speckle_size must be >= 0" in p.stdout
    assert not os.path.exists(tmp_path / "l.pfm")
