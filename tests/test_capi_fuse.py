"""-m "not gpu": the one-shot fusion entry checks its arguments before a device is opened and refuses to compute without one (the two
properties tests/test_capi_symbols.py asserts for the cspm_*_host entries), capi.FuseParams mirrors the library's defaults, and the
host layer's poses-file reader (tests/helpers/pose_check.cc, once more under AddressSanitizer and UBSan as a stand-alone program)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossscalepatchmatch_amd as cs
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3, 2
EYE = np.eye(3)


def _view(**over):
    v = dict(depth=np.full((H, W), 2.0), normal=None, bgr=None, f=4.0, cx=1.0, cy=0.5, R=EYE, t=np.zeros(3))
    v.update(over)
    return {k: x for k, x in v.items() if x is not None}


def _call(views, w=W, h=H, **params):
    """-> (rc, message, outputs): every output pre-filled with the byte 0xAB"""
    out = dict(cloud_buffer=np.frombuffer(bytes([0xAB]) * (32 * 70 * W * H), capi.Point).copy(), state=np.full((70, H, W), 0xAB, np.uint8),
               view_counts=np.full(70, 0xABABABAB, np.uint32))
    try:
        capi.fuse_depth_maps(views, w, h, cloud_cap=len(out["cloud_buffer"]), out=out, **params)
        rc, msg = 0, ""
    except capi.CspmError as e:
        rc, msg = str(e)[len("cspm error "):].split(": ", 1)
    return int(rc), msg, out


BAD = [
    ("too many views", lambda: _call([_view()] * 65), "fusion: the number of views must be in 1 .. 64"),
    ("no view", lambda: _call([]), "fusion: the number of views must be in 1 .. 64"),
    ("f = 0", lambda: _call([_view(), _view(f=0.0)]), "fusion: f must be positive"),
    ("cx = inf", lambda: _call([_view(cx=math.inf)]), "fusion: the camera and its pose must be finite"),
    ("t NaN", lambda: _call([_view(t=np.array([0.0, 0.0, math.nan]))]), "fusion: the camera and its pose must be finite"),
    ("R scaled", lambda: _call([_view(R=EYE * 1.00001)]), "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"),
    ("R sheared", lambda: _call([_view(R=np.array([[1.0, 1e-5, 0], [0, 1, 0], [0, 0, 1]]))]), "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"),
    ("max_reproj < 0", lambda: _call([_view()], max_reproj=-1.0), "fusion: max_reproj must be >= 0"),
    ("max_reproj NaN", lambda: _call([_view()], max_reproj=math.nan), "fusion: max_reproj must be >= 0"),
    ("max_rel_depth < 0", lambda: _call([_view()], max_rel_depth=-1e-3), "fusion: max_rel_depth must be >= 0"),
    ("max_rel_depth NaN", lambda: _call([_view()], max_rel_depth=math.nan), "fusion: max_rel_depth must be >= 0"),
    ("min_cos > 1", lambda: _call([_view()], min_cos=1.01), "fusion: min_cos must be in [0, 1]"),
    ("min_cos < 0", lambda: _call([_view()], min_cos=-0.01), "fusion: min_cos must be in [0, 1]"),
    ("min_views < 0", lambda: _call([_view()], min_views=-1), "fusion: min_views must be in 0 .. 63"),
    ("min_views > 63", lambda: _call([_view()], min_views=64), "fusion: min_views must be in 0 .. 63"),
    ("normals in some views", lambda: _call([_view(normal=np.zeros((3, H, W))), _view()]), "fusion: normals in some views but not all"),
    ("w = 0", lambda: _call([_view(depth=np.zeros((H, 0)))], w=0), "fusion: w and h must be at least 1"),
]


@pytest.mark.parametrize("what,call,msg", BAD, ids=[b[0] for b in BAD])
def test_arguments_are_checked_before_the_device(what, call, msg):
    rc, got, out = call()
    assert rc == -1 and got == msg  # CSPM_ERR_ARG, whether there is a device or not
    assert all(np.all(a.view(np.uint8) == 0xAB) for a in out.values())


def test_stride_and_null_arguments_are_checked_before_the_device():
    L = cs.load_library()
    depth = np.full((H, W), 2.0)
    img = np.zeros((H, W, 3), np.uint8)
    cnt = C.c_uint(0xABABABAB)

    def call(view, n=1):
        return L.cspm_fuse_depth_maps(0, None, C.byref(view) if view is not None else None, n, W, H, None, 0, C.byref(cnt), None, None)

    eye, zero = (C.c_double * 9)(*EYE.ravel()), (C.c_double * 3)()
    ok = dict(depth=capi._dp(depth), normal=None, bgr=capi._u8(img), bgr_stride=3 * W, f=4.0, cx=1.0, cy=0.5, R=eye, t=zero)
    for over, msg in ((dict(bgr_stride=3 * W - 1), "fusion: bgr_stride is below 3 * w"), (dict(depth=None), "fusion: no depth map")):
        assert call(capi.FuseView(**dict(ok, **over))) == -1 and L.cspm_last_error(None).decode() == msg
    assert call(None) == -1 and L.cspm_last_error(None).decode() == "fusion: no views"
    assert L.cspm_fuse_depth_maps(0, None, C.byref(capi.FuseView(**ok)), 1, 65536, 32768, None, 0, C.byref(cnt), None, None) == -1
    assert L.cspm_last_error(None).decode() == "w * h must be below 2^31: cloud records hold 32-bit pixel indices"
    assert cnt.value == 0xABABABAB


def test_without_a_device_the_entry_refuses():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg, out = _call([_view(), _view(t=np.array([0.1, 0.0, 0.0]))], min_views=1)
    assert rc == -2 and msg.startswith("no HIP device")  # CSPM_ERR_HIP: no CPU fallback
    assert all(np.all(a.view(np.uint8) == 0xAB) for a in out.values())
    with pytest.raises(cs.CspmError, match="no HIP device"):
        cs.StereoContext(0)


def test_params_defaults_mirror_the_library():
    p = capi.fuse_params()
    assert (p.max_reproj, p.max_rel_depth, p.min_cos, p.min_views, p.suppress) == (2.0, 0.01, 0.0, 2, 1)
    assert C.sizeof(capi.FuseParams) == 32 and C.sizeof(capi.FuseView) == 4 * 8 + 15 * 8
    import fuse_ref
    assert fuse_ref.DEFAULTS == dict(max_reproj=2.0, max_rel_depth=0.01, min_cos=0.0, min_views=2, suppress=1)
    with pytest.raises(TypeError):
        capi.fuse_params(no_such_field=1)
    assert cs.load_library().cspm_fuse_default_params(None) == -1


# ---- the poses-file reader ---------------------------------------------------------------------------------------------------------
def _build(tmp_path, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("pose_check" + ("_san" if flags else "")))
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "crossscalepatchmatch_amd", "host"),
           os.path.join(ROOT, "tests", "helpers", "pose_check.cc"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _check_reader(exe, tmp_path):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "pose_check ok" in r.stdout, r.stdout + r.stderr
    golden = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")
    r = subprocess.run([exe, golden], capture_output=True, text=True)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and lines[0] == "ok 3", r.stdout + r.stderr
    got = np.array([[float(t) for t in ln.split()] for ln in lines[1:]])
    want = [[float(t) for t in ln.split("#")[0].split()] for ln in open(golden) if ln.split("#")[0].strip()]
    assert np.array_equal(got, np.array(want)) and got.shape == (3, 12)
    for k in range(3):  # the fixture holds rotations the library accepts
        R = got[k].reshape(3, 4)[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6
    bad = tmp_path / "bad.txt"
    bad.write_text("1 0 0 0 0 1 0 0 0 0 1 0\n\n# fine so far\n1 0 0 0 0 1 0 0 0 0 1\n")
    r = subprocess.run([exe, str(bad)], capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout.strip() == "bad 4"
    r = subprocess.run([exe, str(tmp_path / "missing.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout.strip() == "bad 0"
    empty = tmp_path / "empty.txt"
    empty.write_text("# nothing\n\n")
    r = subprocess.run([exe, str(empty)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 0"


def test_pose_reader(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    _check_reader(exe, tmp_path)


def test_pose_reader_under_sanitizers(tmp_path):
    exe, r = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    _check_reader(exe, tmp_path)


def test_cli_refuses_bad_fusion_flags_before_a_device(tmp_path):
    """a pose count that differs from the pair count, a malformed poses file and flag conflicts are errors before any pair runs"""
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(main), "build() makes cspm_main"
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[90 0 47.5; 0 90 31.5; 0 0 1]\ncam1=[90 0 47.5; 0 90 31.5; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\nndisp=16\n")
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"l{k}.png r{k}.png ld{k}.png rd{k}.png" for k in range(2)) + "\n")
    poses = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")  # three poses, two pairs
    malformed = tmp_path / "poses_bad.txt"
    malformed.write_text("1 0 0 0 0 1 0 0 0 0 1\n")
    base = [main, "--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--quiet=true"]
    fuse = [f"--fuse_poses={poses}", f"--fuse_ply={tmp_path / 'f.ply'}"]
    for flags, msg in ((fuse + [f"--batch_list={lst}", f"--calib={calib}"], "holds 3 poses, the batch list 2 pairs"),
                       ([f"--fuse_poses={malformed}", fuse[1], f"--batch_list={lst}", f"--calib={calib}"], "as a poses file"),
                       (fuse + [f"--batch_list={lst}"], "the fusion needs --fuse_poses, --fuse_ply, --batch_list and --calib or --rig"),
                       (fuse + [f"--calib={calib}"], "the fusion needs --fuse_poses, --fuse_ply, --batch_list and --calib or --rig"),
                       ([fuse[0], f"--batch_list={lst}", f"--calib={calib}"], "the fusion needs --fuse_poses, --fuse_ply, --batch_list and --calib or --rig"),
                       (fuse + [f"--batch_list={lst}", f"--calib={calib}", "--fuse_source=median"], "--fuse_source must be raw or pp"),
                       (fuse + [f"--batch_list={lst}", f"--calib={calib}", "--fuse_min_views=64"], "--fuse_min_views 0 .. 63")):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error" in r.stdout and msg in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "f.ply") and not os.path.exists(tmp_path / "ld0.png")
