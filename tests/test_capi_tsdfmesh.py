"""-m "not gpu": the TSDF mesh entries are in the library and declared by the ctypes view, the one-shot entry checks its arguments before
a device is opened (with cspm_tsdf_depth_maps' messages) and refuses to compute without one, the context entries refuse a NULL context,
and the command line refuses --tsdf_mesh_ply without what it needs before any pair runs.  --tsdf_mesh_ply is a file name: it adds no
flag parser (the triples it needs are parsed by the parsers tests/helpers/tsdf_flags_check.cc already drives under ASan and UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crossscalepatchmatch_amd as cs
from crossscalepatchmatch_amd import capi
from test_capi_tsdf import H, PARAM_BAD, VOL, W, _view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cspm_tsdf_mesh", "cspm_tsdf_mesh_device", "cspm_tsdf_set_volume", "cspm_tsdf_mesh_depth_maps")


def test_symbols_are_present_and_declared():
    L = cs.load_library()
    header = open(os.path.join(ROOT, "include", "cspm.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(L, name).argtypes is not None, name
        assert f"int {name}(" in header, name
    for name in ("tsdf_mesh", "tsdf_mesh_device", "tsdf_set_volume"):
        assert callable(getattr(capi.StereoContext, name))
    assert callable(capi.tsdf_mesh_depth_maps)
    assert capi.Face.itemsize == 12 and capi.Point.itemsize == 32


def _call(views, w=W, h=H, null_params=False, null_views=False, **over):
    """-> (rc, message, untouched): every output pre-filled"""
    vol = dict(VOL, **{k: over.pop(k) for k in ("origin", "voxel", "dims") if k in over})
    pts = np.frombuffer(bytes([0xAB]) * (32 * 16), capi.Point).copy()
    tri = np.frombuffer(bytes([0x5A]) * (12 * 16), capi.Face).copy()
    p = capi.tsdf_params(vol["origin"], vol["voxel"], vol["dims"], **over)
    arr = (capi.FuseView * max(len(views), 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, img = capi._fuse_maps(v["depth"], v.get("normal"), v.get("bgr"), w, h)
        R, t = capi._pose(v["R"], v["t"])
        keep.append((d, n, img))
        arr[k] = capi.FuseView(capi._dp(d), capi._opt(capi._dp, n), capi._opt(capi._u8, img), 3 * w, float(v["f"]), float(v["cx"]), float(v["cy"]),
                               (C.c_double * 9)(*R), (C.c_double * 3)(*t))
    nv, nf = C.c_uint(0xABABABAB), C.c_uint(0xCDCDCDCD)
    L = cs.load_library()
    rc = L.cspm_tsdf_mesh_depth_maps(0, None if null_params else C.byref(p), None if null_views else arr, len(views), w, h, capi._vp(pts), len(pts),
                                     capi._vp(tri), len(tri), C.byref(nv), C.byref(nf))
    msg = L.cspm_last_error(None).decode() if rc else ""
    untouched = nv.value == 0xABABABAB and nf.value == 0xCDCDCDCD and np.all(pts.view(np.uint8) == 0xAB) and np.all(tri.view(np.uint8) == 0x5A)
    return rc, msg, untouched


VIEW_BAD = [
    ("too many views", lambda: _call([_view()] * 65), "fusion: the number of views must be in 1 .. 64"),
    ("no view", lambda: _call([]), "fusion: the number of views must be in 1 .. 64"),
    ("NULL views", lambda: _call([_view()], null_views=True), "fusion: no views"),
    ("NULL parameters", lambda: _call([_view()], null_params=True), "tsdf: no parameters"),
    ("f = 0", lambda: _call([_view(), _view(f=0.0)]), "fusion: f must be positive"),
    ("R scaled", lambda: _call([_view(R=np.eye(3) * 1.00001)]), "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"),
    ("normals in some views", lambda: _call([_view(normal=np.zeros((3, H, W))), _view()]), "fusion: normals in some views but not all"),
    ("w = 0", lambda: _call([_view(depth=np.zeros((H, 0)))], w=0), "fusion: w and h must be at least 1"),
]
BAD = [(what, (lambda over=over: _call([_view()], **over)), msg) for what, over, msg in PARAM_BAD] + VIEW_BAD


@pytest.mark.parametrize("what,call,msg", BAD, ids=[b[0] for b in BAD])
def test_arguments_are_checked_before_the_device(what, call, msg):
    rc, got, untouched = call()
    assert rc == -1 and got == msg  # CSPM_ERR_ARG, whether there is a device or not
    assert untouched


def test_a_null_context_is_refused():
    L = cs.load_library()
    assert L.cspm_tsdf_mesh(None, None, 0, None, 0, None, None) == -1
    assert L.cspm_tsdf_mesh_device(None, None, 0, None, 0, None, None) == -1
    assert L.cspm_tsdf_set_volume(None, None, None, None) == -1


def test_without_a_device_the_entry_refuses():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg, untouched = _call([_view(), _view(t=np.array([0.1, 0.0, 0.0]))])
    assert rc == -2 and msg.startswith("no HIP device")  # CSPM_ERR_HIP: no CPU fallback
    assert untouched


def test_cli_refuses_the_mesh_flag_without_what_it_needs(tmp_path):
    """--tsdf_mesh_ply needs what --tsdf_ply needs; it may stand for --tsdf_ply; refusals are made before any pair runs"""
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(main), "build() makes cspm_main"
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[90 0 47.5; 0 90 31.5; 0 0 1]\ncam1=[90 0 47.5; 0 90 31.5; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\nndisp=16\n")
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"l{k}.png r{k}.png ld{k}.png rd{k}.png" for k in range(3)) + "\n")
    poses = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")
    base = [main, "--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--quiet=true"]
    fuse = [f"--fuse_poses={poses}", f"--fuse_ply={tmp_path / 'f.ply'}", f"--batch_list={lst}", f"--calib={calib}"]
    mesh = f"--tsdf_mesh_ply={tmp_path / 'm.ply'}"
    vol = ["--tsdf_origin=-2,-2,1", "--tsdf_dims=32,32,32", "--tsdf_voxel=0.125"]
    needs = "the TSDF flags need --tsdf_ply, --tsdf_origin, --tsdf_dims, --tsdf_voxel and the fusion"
    ranges = "--tsdf_origin must be finite, --tsdf_voxel > 0"
    for flags, msg in ((fuse + [mesh], needs), (fuse + [mesh, vol[0], vol[2]], needs), (fuse + [mesh, vol[1], vol[2]], needs), ([mesh, f"--batch_list={lst}"] + vol, needs),
                       (fuse + [mesh, vol[0], vol[1]], ranges), (fuse + [mesh, "--tsdf_origin=1,2", vol[1], vol[2]], "--tsdf_origin must be x,y,z and --tsdf_dims nx,ny,nz"),
                       (fuse + [mesh] + vol + ["--tsdf_register=true"], "--tsdf_register changes what --fuse_register registers")):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error" in r.stdout and msg in r.stdout, (flags, r.stdout + r.stderr)
        assert not (tmp_path / "m.ply").exists()
    # with everything it needs and no --tsdf_ply the flags are accepted: the run then fails on the list's missing images, not on a flag
    r = subprocess.run(base + fuse + [mesh] + vol, capture_output=True, text=True, timeout=120)
    assert "the TSDF flags need" not in r.stdout and "--tsdf_origin must" not in r.stdout, r.stdout + r.stderr
