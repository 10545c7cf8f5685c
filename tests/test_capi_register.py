"""-m "not gpu": the one-shot registration entry checks its arguments before a device is opened, leaves its outputs alone when it refuses
and does not compute without a device; capi.RegParams mirrors the library's defaults; cspm_main refuses bad registration flags before
any pair runs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import crossscalepatchmatch_amd as cs
import register_ref as rr
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3, 2
EYE = np.eye(3)
NORMAL = np.broadcast_to(np.array([0.0, 0.0, -1.0])[:, None, None], (3, H, W)).copy()


def _view(**over):
    v = dict(depth=np.full((H, W), 2.0), normal=NORMAL, f=4.0, cx=1.0, cy=0.5, R=EYE, t=np.zeros(3))
    v.update(over)
    return {k: x for k, x in v.items() if x is not None}


def _poison():
    return dict(R=np.frombuffer(bytes([0xAB]) * 72, np.float64).copy(), t=np.frombuffer(bytes([0xAB]) * 24, np.float64).copy(),
                iters=np.full(40 * 70, 0xAB, np.uint8).view(capi.REG_ITER))  # a view: a copy of padded records drops the padding


def _call(views, src=1, targets=0b01, w=W, h=H, **params):
    """-> (rc, message, outputs): every output pre-filled with the byte 0xAB"""
    out = _poison()
    try:
        capi.register_depth_maps(views, w, h, src, targets, out=out, **params)
        rc, msg = 0, ""
    except capi.CspmError as e:
        rc, msg = str(e)[len("cspm error "):].split(": ", 1)
    return int(rc), msg, out


TWO = [_view(), _view(t=np.array([0.1, 0.0, 0.0]))]
MASK = "registration: the targets must be other views that exist, at least one"
BAD = [
    ("too many views", lambda: _call([_view()] * 65), "fusion: the number of views must be in 1 .. 64"),
    ("no view", lambda: _call([]), "fusion: the number of views must be in 1 .. 64"),
    ("src = -1", lambda: _call(TWO, src=-1), "registration: no such source view"),
    ("src = K", lambda: _call(TWO, src=2), "registration: no such source view"),
    ("no target", lambda: _call(TWO, targets=0), MASK),
    ("the source a target", lambda: _call(TWO, targets=0b11), MASK),
    ("a target that is no view", lambda: _call(TWO, targets=0b101), MASK),
    ("bit 63", lambda: _call(TWO, targets=(1 << 63) | 1), MASK),
    ("iters = 0", lambda: _call(TWO, iters=0), "registration: iters must be in 1 .. 64"),
    ("iters = 65", lambda: _call(TWO, iters=65), "registration: iters must be in 1 .. 64"),
    ("stride = 0", lambda: _call(TWO, stride=0), "registration: stride must be at least 1"),
    ("max_dist < 0", lambda: _call(TWO, max_dist=-1.0), "registration: max_dist must be >= 0"),
    ("max_dist NaN", lambda: _call(TWO, max_dist=math.nan), "registration: max_dist must be >= 0"),
    ("huber < 0", lambda: _call(TWO, huber=-0.01), "registration: huber must be >= 0"),
    ("huber NaN", lambda: _call(TWO, huber=math.nan), "registration: huber must be >= 0"),
    ("min_cos > 1", lambda: _call(TWO, min_cos=1.01), "registration: min_cos must be in [0, 1]"),
    ("min_cos NaN", lambda: _call(TWO, min_cos=math.nan), "registration: min_cos must be in [0, 1]"),
    ("min_pairs < 0", lambda: _call(TWO, min_pairs=-1), "registration: min_pairs must be >= 0"),
    ("pivot_rel = 1", lambda: _call(TWO, pivot_rel=1.0), "registration: pivot_rel must be in [0, 1)"),
    ("pivot_rel < 0", lambda: _call(TWO, pivot_rel=-1e-12), "registration: pivot_rel must be in [0, 1)"),
    ("f = 0", lambda: _call([_view(), _view(f=0.0)]), "fusion: f must be positive"),
    ("a start pose that is no rotation", lambda: _call([_view(), _view(R=EYE * 1.00001)]), "fusion: R is not a rotation (max |R R^T - I| > 1e-6)"),
    ("t NaN", lambda: _call([_view(t=np.array([0.0, 0.0, math.nan])), _view()]), "fusion: the camera and its pose must be finite"),
    ("a view without normals", lambda: _call([_view(), _view(normal=None)]), "registration: the views carry no normals"),
    ("w = 0", lambda: _call([_view(depth=np.zeros((H, 0)), normal=np.zeros((3, H, 0)))] * 2, w=0), "fusion: w and h must be at least 1"),
]


@pytest.mark.parametrize("what,call,msg", BAD, ids=[b[0] for b in BAD])
def test_arguments_are_checked_before_the_device(what, call, msg):
    rc, got, out = call()
    assert rc == -1 and got == msg  # CSPM_ERR_ARG, whether there is a device or not
    ref = _poison()
    assert all(out[k].tobytes() == ref[k].tobytes() for k in ref)


def test_null_arguments_are_checked_before_the_device():
    L = cs.load_library()
    depth = np.full((H, W), 2.0)
    eye, zero = (C.c_double * 9)(*EYE.ravel()), (C.c_double * 3)()
    ok = dict(depth=capi._dp(depth), normal=capi._dp(NORMAL), bgr=None, bgr_stride=0, f=4.0, cx=1.0, cy=0.5, R=eye, t=zero)
    two = (capi.FuseView * 2)(capi.FuseView(**ok), capi.FuseView(**ok))
    assert L.cspm_register_depth_maps(0, None, None, 2, W, H, 1, 1, None, None, None) == -1 and L.cspm_last_error(None).decode() == "fusion: no views"
    two[0] = capi.FuseView(**dict(ok, depth=None))
    assert L.cspm_register_depth_maps(0, None, two, 2, W, H, 1, 1, None, None, None) == -1 and L.cspm_last_error(None).decode() == "fusion: no depth map"
    assert L.cspm_reg_default_params(None) == -1


def test_without_a_device_the_entry_refuses():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg, out = _call(TWO, min_pairs=1)
    assert rc == -2 and msg.startswith("no HIP device")  # CSPM_ERR_HIP: no CPU fallback
    ref = _poison()
    assert all(out[k].tobytes() == ref[k].tobytes() for k in ref)


def test_params_defaults_mirror_the_library():
    p = capi.reg_params()
    assert {k: getattr(p, k) for k, _ in capi.RegParams._fields_} == rr.DEFAULTS
    assert rr.DEFAULTS == dict(iters=8, stride=1, max_dist=0.5, huber=0.05, min_cos=0.0, min_pairs=100, pivot_rel=1e-8)
    assert C.sizeof(capi.RegParams) == 48 and C.sizeof(capi.RegIter) == 40 == capi.REG_ITER.itemsize
    assert [capi.REG_ITER.fields[k][1] for k, _ in capi.RegIter._fields_] == [getattr(capi.RegIter, k).offset for k, _ in capi.RegIter._fields_]
    with pytest.raises(TypeError):
        capi.reg_params(no_such_field=1)
    assert capi._mask([0, 2, 3]).value == 0b1101 == capi._mask(0b1101).value


def test_the_new_names_are_bound_and_none_is_a_one_shot_host_entry():
    new = ["cspm_reg_default_params", "cspm_fuse_register", "cspm_fuse_get_pose", "cspm_fuse_set_pose", "cspm_register_depth_maps"]
    L = cs.load_library()
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read()
    for name in new:
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr and not name.endswith("_host")


def test_cli_refuses_bad_registration_flags_before_a_device(tmp_path):
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(main), "build() makes cspm_main"
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[90 0 47.5; 0 90 31.5; 0 0 1]\ncam1=[90 0 47.5; 0 90 31.5; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\nndisp=16\n")
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"l{k}.png r{k}.png ld{k}.png rd{k}.png" for k in range(2)) + "\n")
    poses = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")  # three poses, two pairs
    base = [main, "--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--quiet=true"]
    ply, blist, cal = f"--fuse_ply={tmp_path / 'f.ply'}", f"--batch_list={lst}", f"--calib={calib}"
    needs = "--fuse_register needs --fuse_ply, --batch_list and --calib or --rig"
    values = "--fuse_reg_iters must be 1 .. 64, --fuse_reg_stride >= 1, --fuse_reg_max_dist and --fuse_reg_huber >= 0 and --fuse_register_window 1 .. 63"
    for flags, msg in ((["--fuse_register", blist, cal], needs), (["--fuse_register", ply, cal], needs), (["--fuse_register", ply, blist], needs),
                       (["--fuse_register", ply, blist, cal, "--fuse_reg_iters=0"], values), (["--fuse_register", ply, blist, cal, "--fuse_reg_iters=65"], values),
                       (["--fuse_register", ply, blist, cal, "--fuse_reg_stride=0"], values), (["--fuse_register", ply, blist, cal, "--fuse_reg_max_dist=-1"], values),
                       (["--fuse_register", ply, blist, cal, "--fuse_reg_huber=-0.5"], values), (["--fuse_register", ply, blist, cal, "--fuse_register_window=0"], values),
                       (["--fuse_register", ply, blist, cal, f"--fuse_poses={poses}"], "holds 3 poses, the batch list 2 pairs"),
                       ([ply, blist, cal, f"--fuse_poses_out={tmp_path / 'out.txt'}", f"--fuse_poses={poses}"], "--fuse_poses_out writes the poses of --fuse_register"),
                       ([ply, blist, cal], "the fusion needs --fuse_poses, --fuse_ply, --batch_list and --calib or --rig")):  # as before
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error" in r.stdout and msg in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "f.ply") and not os.path.exists(tmp_path / "ld0.png") and not os.path.exists(tmp_path / "out.txt")
