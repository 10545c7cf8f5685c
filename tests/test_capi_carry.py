"""-m "not gpu": the one-shot carry entry checks its arguments before a device is opened, leaves its outputs alone when it refuses and
does not compute without a device; capi.CarryParams mirrors the library's defaults; the pose helper is pure host code; cspm_main refuses
bad carry flags before any pair runs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import carry_ref as cr
import crossscalepatchmatch_amd as cs
import fuse_cases as fc
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3, 2
EYE = np.eye(3)
CAL = (4.0, 1.0, 0.5, 0.2, 0.0)
FIELD = np.zeros((H, W, 6))
FIELD[..., 2] = 1.0
FIELD[..., 5] = 2.0


def _poison(w=W, h=H):
    n = max(w, 0) * max(h, 0)
    return dict(planes=np.frombuffer(bytes([0xAB]) * (48 * n), np.float64).reshape(max(h, 0), max(w, 0), 6).copy(),
                state=np.full((max(h, 0), max(w, 0)), 0xAB, np.uint8), source=np.full((max(h, 0), max(w, 0)), 0x2B2B2B2B, np.int32))


def _call(field=FIELD, src_calib=CAL, src_view=0, dst_calib=CAL, dst_view=0, w_t=W, h_t=H, max_dis=8, R=EYE, t=np.zeros(3), **params):
    """-> (rc, message, outputs): every output pre-filled"""
    out = _poison(w_t, h_t)
    try:
        capi.carry_plane_field(field, src_calib, src_view, dst_calib, dst_view, w_t, h_t, max_dis, R, t, out=out, **params)
        rc, msg = 0, ""
    except capi.CspmError as e:
        rc, msg = str(e)[len("cspm error "):].split(": ", 1)
    return int(rc), msg, out


def _cal(**over):
    d = dict(f=CAL[0], cx=CAL[1], cy=CAL[2], baseline=CAL[3], doffs=CAL[4])
    d.update(over)
    return tuple(d[k] for k in ("f", "cx", "cy", "baseline", "doffs"))


FINITE, POSITIVE = "carry: the calibration must be finite", "carry: f and baseline must be positive"
ROT = "carry: R is not a rotation (max |R R^T - I| > 1e-6)"
SIZE = "carry: w and h must be at least 1"
BAD = [
    ("source f NaN", lambda: _call(src_calib=_cal(f=math.nan)), FINITE),
    ("source doffs infinite", lambda: _call(src_calib=_cal(doffs=math.inf)), FINITE),
    ("target cy NaN", lambda: _call(dst_calib=_cal(cy=math.nan)), FINITE),
    ("source f = 0", lambda: _call(src_calib=_cal(f=0.0)), POSITIVE),
    ("target baseline < 0", lambda: _call(dst_calib=_cal(baseline=-0.2)), POSITIVE),
    ("source view 2", lambda: _call(src_view=2), "carry: view must be 0 or 1"),
    ("target view -1", lambda: _call(dst_view=-1), "carry: view must be 0 or 1"),
    ("R scaled", lambda: _call(R=EYE * 1.00001), ROT),
    ("R sheared", lambda: _call(R=np.array([[1.0, 1e-5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])), ROT),
    ("R NaN", lambda: _call(R=np.where(EYE == 0, math.nan, EYE)), "carry: the motion must be finite"),
    ("t infinite", lambda: _call(t=np.array([0.0, math.inf, 0.0])), "carry: the motion must be finite"),
    ("max_dis < 0", lambda: _call(max_dis=-1), "carry: max_dis must be >= 0"),
    ("target w = 0", lambda: _call(w_t=0), SIZE),
    ("target h < 0", lambda: _call(h_t=-3), SIZE),
    ("source w = 0", lambda: _call(field=np.zeros((H, 0, 6))), SIZE),
    ("target of 2^31 pixels", lambda: _call_big(), "carry: w * h must be below 2^31: winners are 32-bit pixel indices"),
    ("fill = 2", lambda: _call(fill=2), "carry: fill must be 0 or 1"),
    ("fill = -1", lambda: _call(fill=-1), "carry: fill must be 0 or 1"),
]


def _call_big():
    """the size check comes before any output is touched: NULL outputs, sizes straight into the entry"""
    L = cs.load_library()
    ks, p = capi.calib_struct(CAL), capi.carry_params()
    R, t = capi._pose(EYE, np.zeros(3))
    rc = L.cspm_carry_plane_field(0, capi._dp(FIELD), None, C.byref(ks), 0, W, H, C.byref(ks), 0, 65536, 32768, 8, capi._dp(R), capi._dp(t), C.byref(p),
                                  None, None, None)
    return rc, L.cspm_last_error(None).decode(), {}


@pytest.mark.parametrize("what,call,msg", BAD, ids=[b[0] for b in BAD])
def test_arguments_are_checked_before_the_device(what, call, msg):
    rc, got, out = call()
    assert rc == -1 and got == msg  # CSPM_ERR_ARG, whether there is a device or not
    if out:
        ref = _poison(*out["state"].shape[::-1])
        assert all(out[k].tobytes() == ref[k].tobytes() for k in ref)


def test_null_arguments_are_checked_before_the_device():
    L = cs.load_library()
    ks, p = capi.calib_struct(CAL), capi.carry_params()
    R, t = capi._pose(EYE, np.zeros(3))
    args = lambda **o: [o.get("dev", 0), o.get("field", capi._dp(FIELD)), None, o.get("ks", C.byref(ks)), 0, W, H, o.get("kt", C.byref(ks)), 0, W, H, 8,
                        o.get("R", capi._dp(R)), o.get("t", capi._dp(t)), C.byref(p), None, None, None]
    for over, msg in ((dict(field=None), "carry: no source plane field"), (dict(ks=None), "carry: no calibration"), (dict(kt=None), "carry: no calibration"),
                      (dict(R=None), "carry: no motion"), (dict(t=None), "carry: no motion")):
        assert L.cspm_carry_plane_field(*args(**over)) == -1 and L.cspm_last_error(None).decode() == msg
    assert L.cspm_carry_default_params(None) == -1
    assert L.cspm_carry_relative_pose(None, None, None, None, None, None) == -1 and L.cspm_last_error(None).decode() == "carry: a pose is missing"
    assert L.cspm_carry_planes(None, None, None, None, None, None, None, 1) == -1


def test_without_a_device_the_entry_refuses():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg, out = _call()
    assert rc == -2 and msg.startswith("no HIP device")  # CSPM_ERR_HIP: no CPU fallback
    ref = _poison()
    assert all(out[k].tobytes() == ref[k].tobytes() for k in ref)


def test_params_defaults_mirror_the_library():
    p = capi.carry_params()
    assert {k: getattr(p, k) for k, _ in capi.CarryParams._fields_} == cr.DEFAULTS == dict(fill=1)
    assert C.sizeof(capi.CarryParams) == 4
    assert capi.carry_params(fill=0).fill == 0
    with pytest.raises(TypeError):
        capi.carry_params(no_such_field=1)


def test_relative_pose_is_host_code_and_equals_the_restatement():
    Rs, ts = fc.rot(3.0, -7.0, 11.0), np.array([0.3, -0.2, 0.7])
    Rt, tt = fc.rot(-2.0, 5.0, 1.0), np.array([-0.1, 0.4, 0.2])
    R, t = capi.carry_relative_pose(Rs, ts, Rt, tt)
    Rw, tw = cr.relative_pose(Rs, ts, Rt, tt)
    assert R.tobytes() == Rw.tobytes() and t.tobytes() == tw.tobytes()  # bit for bit: the association is part of the interface
    L = cs.load_library()  # an output may be an input
    a, b = np.ascontiguousarray(Rs).reshape(9).copy(), ts.copy()
    Rt9, tt3 = capi._pose(Rt, tt)
    assert L.cspm_carry_relative_pose(capi._dp(a), capi._dp(b), capi._dp(Rt9), capi._dp(tt3), capi._dp(a), capi._dp(b)) == 0
    assert a.tobytes() == Rw.tobytes() and b.tobytes() == tw.tobytes()


def test_the_new_names_are_bound_and_none_is_a_one_shot_host_entry():
    new = ["cspm_carry_default_params", "cspm_carry_relative_pose", "cspm_carry_plane_field", "cspm_carry_planes"]
    L = cs.load_library()
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read()
    for name in new:
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr and not name.endswith("_host")
    assert hasattr(capi.StereoContext, "carry_planes_from")


def test_cli_refuses_bad_carry_flags_before_a_device(tmp_path):
    main = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
    assert os.path.exists(main), "build() makes cspm_main"
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[90 0 47.5; 0 90 31.5; 0 0 1]\ncam1=[90 0 47.5; 0 90 31.5; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\nndisp=16\n")
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(f"l{k}.png r{k}.png ld{k}.png rd{k}.png" for k in range(2)) + "\n")
    poses = os.path.join(ROOT, "tests", "golden", "fuse", "poses.txt")  # three poses, two pairs
    two = tmp_path / "two.txt"
    two.write_text("1 0 0 0 1 0 0 0 1 0 0 0\n1 0 0 0 1 0 0 0 1 0.05 0 0\n")
    base = [main, "--max_dis=16", "--dis_scale=4", "--cc_name=GRD", "--quiet=true"]
    blist, cal, cp = f"--batch_list={lst}", f"--calib={calib}", f"--carry_poses={two}"
    needs = "--carry_poses needs --batch_list and --calib or --rig"
    for flags, msg in (([cp, cal], needs), ([cp, blist], needs),
                       ([cp, blist, cal, "--carry_iters=-1"], "--carry_iters must be 0 .. 15"), ([cp, blist, cal, "--carry_iters=16"], "--carry_iters must be 0 .. 15"),
                       ([f"--carry_poses={poses}", blist, cal], "holds 3 poses, the batch list 2 pairs"),
                       ([blist, cal, "--carry_iters=2"], "--carry_iters and --carry_no_fill need --carry_poses"),
                       ([blist, cal, "--carry_no_fill"], "--carry_iters and --carry_no_fill need --carry_poses"),
                       ([f"--carry_poses={tmp_path / 'missing.txt'}", blist, cal], "missing.txt")):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error" in r.stdout and msg in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "ld0.png")
