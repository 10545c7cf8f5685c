"""The one-shot host entries run on the device they name: the same call on device 0 and on device 1 gives the
same bits, and the caller's current device is as it was.  Five entries that between them use every member of the staging helper: plain
and strided uploads and downloads, the packed guide image, optional buffers, the plane transposition, the count-then-copy download and
the batch loop.  Needs two devices; with one it skips."""
import ctypes as C

import numpy as np
import pytest

import geom_ref as gr
from crossscalepatchmatch_amd import capi

pytestmark = pytest.mark.gpu

CAL = (300.0, 4.0, 4.0, 0.25, 3.5)


def _median_f64(dev):
    src = np.random.default_rng(1).uniform(0.0, 40.0, (5, 7))
    src[2, 3] = np.nan
    return [capi.median_filter(dev, src, 1)]


def _median_u8_padded(dev):
    L = capi.load_library()
    w, h, cn, s_src, s_dst = 7, 5, 3, 7 * 3 + 5, 7 * 3 + 2  # rows of 21 bytes in strides of 26 and 23
    src = np.random.default_rng(2).integers(0, 256, (h, s_src), dtype=np.uint8)
    dst = np.full((h, s_dst), 0xAB, np.uint8)
    rc = L.cspm_median_filter_u8_host(dev, capi._u8(src), s_src, w, h, cn, 2, capi._u8(dst), s_dst)
    assert rc == 0, L.cspm_last_error(None)
    assert (dst[:, w * cn:] == 0xAB).all()  # the padding is not written
    return [dst]


def _fit_guided(dev):
    rng = np.random.default_rng(3)
    disp = rng.uniform(1.0, 30.0, (9, 9))
    disp[4, 4] = np.nan
    valid = (rng.uniform(size=(9, 9)) > 0.1).astype(np.uint8)
    guide = rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)
    return list(capi.fit_planes_host(disp, valid, guide, max_dis=32, device=dev, radius=2, min_support=3))


def _reproject_cloud(dev):
    rng = np.random.default_rng(4)
    disp = rng.uniform(1.0, 40.0, (9, 9))
    disp[1, 2] = np.nan
    a, b = rng.uniform(-0.05, 0.05, (2, 9, 9))
    img = rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)
    got = capi.reproject_host(CAL, 0, disp, None, a, b, img, device=dev)
    assert 0 < got["count"] == len(got["cloud"]) <= 81
    return [got[k] for k in ("depth", "xyz", "normal", "keep")] + [np.array([got["count"]]), got["cloud"]]


def _aggregate(dev):
    """BOX on a 7 x 7 guide and GF on a 19 x 19 one, 3 slices each: GF's own check takes nothing below 19 x 19 (2 * 9 + 1)"""
    res = []
    for method, s in ((capi.CA_BOX, 7), (capi.CA_GF, 19)):
        rng = np.random.default_rng(5 + s)
        guide = rng.uniform(0.0, 1.0, (s, s, 3))
        vol = rng.uniform(0.0, 10.0, (3, s, s))
        res.append(capi.aggregate_cv_host(dev, method, guide, vol))
    return res


def _same(a, b):
    if a.dtype.names:
        return a.shape == b.shape and all(gr.same_bits(a[n], b[n]) for n in a.dtype.names)
    return gr.same_bits(a, b)


@pytest.mark.parametrize("entry", [_median_f64, _median_u8_padded, _fit_guided, _reproject_cloud, _aggregate], ids=lambda f: f.__name__.strip("_"))
def test_device_1_gives_what_device_0_gives(_gpu_ctx_session, entry):
    import torch
    if capi.load_library().cspm_device_count() < 2:
        pytest.skip("one device")
    res = []
    for dev in (0, 1):
        before = torch.cuda.current_device()
        res.append(entry(dev))
        assert torch.cuda.current_device() == before
    assert len(res[0]) == len(res[1]) and res[0]
    for k, (a, b) in enumerate(zip(*res)):
        assert _same(a, b), f"output {k} differs between device 0 and device 1"
