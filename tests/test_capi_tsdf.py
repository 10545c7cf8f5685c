"""-m "not gpu": the one-shot TSDF entry checks its arguments before a device is opened and refuses to compute without one (the two
properties tests/test_capi_symbols.py asserts for the cspm_*_host entries), capi.TsdfParams mirrors the library's defaults and its
argument rules are those of tests/tsdf_ref.py; the host layer's TSDF flag parsers (tests/helpers/tsdf_flags_check.cc, once more under
AddressSanitizer and UBSan as a stand-alone program) and the command line's refusal of bad TSDF flags before any pair runs."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossscalepatchmatch_amd as cs
import tsdf_ref as tr
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3, 2
EYE = np.eye(3)
VOL = dict(origin=(-1.0, -1.0, 1.0), voxel=0.5, dims=(4, 4, 4))


def _view(**over):
    v = dict(depth=np.full((H, W), 2.0), normal=None, bgr=None, f=4.0, cx=1.0, cy=0.5, R=EYE, t=np.zeros(3))
    v.update(over)
    return {k: x for k, x in v.items() if x is not None}


def _call(views, w=W, h=H, **over):
    """-> (rc, message, outputs): every output pre-filled with the byte 0xAB"""
    vol = dict(VOL, **{k: over.pop(k) for k in ("origin", "voxel", "dims") if k in over})
    out = dict(cloud_buffer=np.frombuffer(bytes([0xAB]) * (32 * 3 * 64), capi.Point).copy(), D=np.full((4, 4, 4), np.nan, np.float32),
               W=np.full((4, 4, 4), np.nan, np.float32), C=np.full((4, 4, 4, 4), 0xAB, np.uint8))
    before = {k: a.tobytes() for k, a in out.items()}
    p = capi.tsdf_params(vol["origin"], vol["voxel"], vol["dims"], **over)
    arr = (capi.FuseView * max(len(views), 1))()
    keep = []
    for k, v in enumerate(views):
        d, n, img = capi._fuse_maps(v["depth"], v.get("normal"), v.get("bgr"), w, h)
        R, t = capi._pose(v["R"], v["t"])
        keep.append((d, n, img))
        arr[k] = capi.FuseView(capi._dp(d), capi._opt(capi._dp, n), capi._opt(capi._u8, img), 3 * w, float(v["f"]), float(v["cx"]), float(v["cy"]),
                               (C.c_double * 9)(*R), (C.c_double * 3)(*t))
    cnt = C.c_uint(0xABABABAB)
    fp = C.POINTER(C.c_float)
    L = cs.load_library()
    rc = L.cspm_tsdf_depth_maps(0, C.byref(p), arr, len(views), w, h, capi._vp(out["cloud_buffer"]), len(out["cloud_buffer"]), C.byref(cnt),
                                out["D"].ctypes.data_as(fp), out["W"].ctypes.data_as(fp), capi._u8(out["C"]))
    msg = L.cspm_last_error(None).decode() if rc else ""
    untouched = cnt.value == 0xABABABAB and all(a.tobytes() == before[k] for k, a in out.items())
    return rc, msg, untouched


PARAM_BAD = [
    ("voxel = 0", dict(voxel=0.0), "tsdf: the origin must be finite and voxel finite and > 0"),
    ("voxel NaN", dict(voxel=math.nan), "tsdf: the origin must be finite and voxel finite and > 0"),
    ("origin inf", dict(origin=(0.0, math.inf, 0.0)), "tsdf: the origin must be finite and voxel finite and > 0"),
    ("nx = 0", dict(dims=(0, 4, 4)), "tsdf: nx, ny and nz must be at least 1"),
    ("nz < 0", dict(dims=(4, 4, -1)), "tsdf: nx, ny and nz must be at least 1"),
    ("2^31 voxels", dict(dims=(2048, 2048, 512)), "tsdf: nx * ny * nz must be below 2^31"),
    ("trunc < 0", dict(trunc=-0.1), "tsdf: trunc must be finite and > 0 (0 = 4 * voxel)"),
    ("trunc inf", dict(trunc=math.inf), "tsdf: trunc must be finite and > 0 (0 = 4 * voxel)"),
    ("max_weight < 1", dict(max_weight=0.5), "tsdf: max_weight must be in [1, 16777216]"),
    ("max_weight NaN", dict(max_weight=math.nan), "tsdf: max_weight must be in [1, 16777216]"),
    ("max_weight 2^25", dict(max_weight=2.0 ** 25), "tsdf: max_weight must be in [1, 16777216]"),
    ("min_cos > 1", dict(min_cos=1.01), "tsdf: min_cos must be in [0, 1]"),
    ("min_cos < 0", dict(min_cos=-0.01), "tsdf: min_cos must be in [0, 1]"),
    ("step_rel = 0", dict(step_rel=0.0), "tsdf: step_rel must be in (0, 1]"),
    ("step_rel > 1", dict(step_rel=1.5), "tsdf: step_rel must be in (0, 1]"),
]
VIEW_BAD = [
    ("too many views", lambda: _call([_view()] * 65), "fusion: the number of views must be in 1 .. 64"),
    ("no view", lambda: _call([]), "fusion: the number of views must be in 1 .. 64"),
    ("f = 0", lambda: _call([_view(), _view(f=0.0)]), "fusion: f must be positive"),
    ("t NaN", lambda: _call([_view(t=np.array([0.0, 0.0, math.nan]))]), "fusion: the camera and its pose must be finite"),
    ("R scaled", lambda: _call([_view(R=EYE * 1.00001)]), "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"),
    ("normals in some views", lambda: _call([_view(normal=np.zeros((3, H, W))), _view()]), "fusion: normals in some views but not all"),
    ("w = 0", lambda: _call([_view(depth=np.zeros((H, 0)))], w=0), "fusion: w and h must be at least 1"),
]
BAD = [(what, (lambda over=over: _call([_view()], **over)), msg) for what, over, msg in PARAM_BAD] + VIEW_BAD


@pytest.mark.parametrize("what,call,msg", BAD, ids=[b[0] for b in BAD])
def test_arguments_are_checked_before_the_device(what, call, msg):
    rc, got, untouched = call()
    assert rc == -1 and got == msg  # CSPM_ERR_ARG, whether there is a device or not
    assert untouched


@pytest.mark.parametrize("what,over,msg", PARAM_BAD, ids=[b[0] for b in PARAM_BAD])
def test_the_restatement_refuses_the_same_parameters(what, over, msg):
    assert tr.check_params(**VOL) and not tr.check_params(**dict(VOL, **over))


def test_null_arguments_are_checked_before_the_device():
    L = cs.load_library()
    depth = np.full((H, W), 2.0)
    img = np.zeros((H, W, 3), np.uint8)
    cnt = C.c_uint(0xABABABAB)
    p = capi.tsdf_params(**VOL)
    eye, zero = (C.c_double * 9)(*EYE.ravel()), (C.c_double * 3)()
    ok = dict(depth=capi._dp(depth), normal=None, bgr=capi._u8(img), bgr_stride=3 * W, f=4.0, cx=1.0, cy=0.5, R=eye, t=zero)

    def call(params, view, n=1, w=W, h=H):
        return L.cspm_tsdf_depth_maps(0, C.byref(params) if params is not None else None, C.byref(view) if view is not None else None, n, w, h, None, 0,
                                      C.byref(cnt), None, None, None)

    assert call(None, capi.FuseView(**ok)) == -1 and L.cspm_last_error(None).decode() == "tsdf: no parameters"
    for over, msg in ((dict(bgr_stride=3 * W - 1), "fusion: bgr_stride is below 3 * w"), (dict(depth=None), "fusion: no depth map")):
        assert call(p, capi.FuseView(**dict(ok, **over))) == -1 and L.cspm_last_error(None).decode() == msg
    assert call(p, None) == -1 and L.cspm_last_error(None).decode() == "fusion: no views"
    assert call(p, capi.FuseView(**ok), w=65536, h=32768) == -1
    assert L.cspm_last_error(None).decode() == "w * h must be below 2^31: cloud records hold 32-bit pixel indices"
    assert cnt.value == 0xABABABAB
    assert L.cspm_tsdf_begin(None, C.byref(p)) == -1 and L.cspm_tsdf_clear(None) == -1 and L.cspm_tsdf_end(None) == -1  # a NULL context


def test_without_a_device_the_entry_refuses():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg, untouched = _call([_view(), _view(t=np.array([0.1, 0.0, 0.0]))])
    assert rc == -2 and msg.startswith("no HIP device")  # CSPM_ERR_HIP: no CPU fallback
    assert untouched


def test_params_defaults_mirror_the_library():
    p = capi.TsdfParams()
    assert cs.load_library().cspm_tsdf_default_params(C.byref(p)) == 0
    assert (list(p.origin), p.voxel, p.nx, p.ny, p.nz) == ([0.0, 0.0, 0.0], 0.0, 0, 0, 0)
    assert (p.trunc, p.max_weight, p.min_cos, p.step_rel) == (0.0, 64.0, 0.0, 0.5)
    assert tr.DEFAULTS == dict(trunc=0.0, max_weight=64.0, min_cos=0.0, step_rel=0.5)
    assert C.sizeof(capi.TsdfParams) == 4 * 8 + 16 + 4 * 8 and C.sizeof(capi.TsdfCamera) == 15 * 8
    q = capi.tsdf_params((1.0, 2.0, 3.0), 0.25, (5, 6, 7), trunc=0.75, max_weight=3, min_cos=0.5, step_rel=1.0)
    assert (list(q.origin), q.voxel, q.nx, q.ny, q.nz, q.trunc, q.max_weight, q.min_cos, q.step_rel) == ([1.0, 2.0, 3.0], 0.25, 5, 6, 7, 0.75, 3.0, 0.5, 1.0)
    with pytest.raises(TypeError):
        capi.tsdf_params((0, 0, 0), 1.0, (1, 1, 1), no_such_field=1)
    assert cs.load_library().cspm_tsdf_default_params(None) == -1


# ---- the flag parsers of the host layer ------------------------------------------------------------------------------------------------
def _build(tmp_path, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("tsdf_flags_check" + ("_san" if flags else "")))
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "crossscalepatchmatch_amd", "host"),
           os.path.join(ROOT, "tests", "helpers", "tsdf_flags_check.cc"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _check_parsers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tsdf_flags_check ok" in r.stdout, r.stdout + r.stderr
    for kind, text, want in (("triple", "-2.4,-2.4,2.3", "ok -2.3999999999999999 -2.3999999999999999 2.2999999999999998"), ("triple", "1,2", "bad"),
                             ("triple", "1,2,3 4", "bad"), ("triple", "x" * 5000, "bad"), ("triple", "1," * 3000, "bad"), ("dims", "96,96,64", "ok 96 96 64"),
                             ("dims", "96,96", "bad"), ("dims", "9999999999,1,1", "bad"), ("dims", "1,1,0.5", "bad")):
        r = subprocess.run([exe, kind, text], capture_output=True, text=True)
        assert r.stdout.strip() == want and r.returncode == (0 if want.startswith("ok") else 2), (kind, text[:20], r.stdout + r.stderr)


def test_flag_parsers(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    _check_parsers(exe)


def test_flag_parsers_under_sanitizers(tmp_path):
    exe, r = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    if r.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-200:])
    _check_parsers(exe)


def test_cli_refuses_bad_tsdf_flags_before_a_device(tmp_path):
    """missing flags, malformed triples, values out of range and --tsdf_register without --fuse_register are errors before any pair runs"""
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(main), "build() makes cspm_main"
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[90 0 47.5; 0 90 31.5; 0 0 1]\ncam1=[90 0 47.5; 0 90 31.5; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\nndisp=16\n")
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"l{k}.png r{k}.png ld{k}.png rd{k}.png" for k in range(3)) + "\n")
    poses = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")
    base = [main, "--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--quiet=true"]
    fuse = [f"--fuse_poses={poses}", f"--fuse_ply={tmp_path / 'f.ply'}", f"--batch_list={lst}", f"--calib={calib}"]
    vol = [f"--tsdf_ply={tmp_path / 't.ply'}", "--tsdf_origin=-2,-2,1", "--tsdf_dims=32,32,32", "--tsdf_voxel=0.125"]
    needs = "the TSDF flags need --tsdf_ply, --tsdf_origin, --tsdf_dims, --tsdf_voxel and the fusion"
    ranges = "--tsdf_origin must be finite, --tsdf_voxel > 0"
    for flags, msg in ((fuse + vol[1:], needs), (fuse + [vol[0], vol[2], vol[3]], needs), (fuse + ["--tsdf_trunc=0.5"], needs), (vol + [f"--batch_list={lst}"], needs),
                       (fuse + ["--tsdf_register=true"], needs), (fuse + vol + ["--tsdf_register=true"], "--tsdf_register changes what --fuse_register registers"),
                       (fuse + [vol[0], "--tsdf_origin=-2,-2", vol[2], vol[3]], "--tsdf_origin must be x,y,z and --tsdf_dims nx,ny,nz"),
                       (fuse + [vol[0], vol[1], "--tsdf_dims=32,32,3.5", vol[3]], "--tsdf_origin must be x,y,z and --tsdf_dims nx,ny,nz"),
                       (fuse + vol[:3], ranges), (fuse + vol[:3] + ["--tsdf_voxel=-1"], ranges), (fuse + [vol[0], vol[1], "--tsdf_dims=32,0,32", vol[3]], ranges),
                       (fuse + [vol[0], vol[1], "--tsdf_dims=2048,2048,512", vol[3]], ranges), (fuse + vol + ["--tsdf_trunc=-0.5"], ranges),
                       (fuse + vol + ["--tsdf_max_weight=0"], ranges), (fuse + vol + ["--tsdf_min_cos=1.5"], ranges),
                       (fuse + [vol[0], "--tsdf_origin=nan,0,0", vol[2], vol[3]], ranges)):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error" in r.stdout and msg in r.stdout, (flags, r.stdout + r.stderr)
    assert not os.path.exists(tmp_path / "t.ply") and not os.path.exists(tmp_path / "f.ply") and not os.path.exists(tmp_path / "ld0.png")
