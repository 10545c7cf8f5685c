"""cspm_main --rig (include/cspm.h "rectification", INTEGRATION.md "rig files") on the small committed rig and raw pair under
tests/golden/rectify/ (tests/golden/make_rectify.py): the rectified images it writes equal the restatement tests/rectify_ref.py, the
derived calibration serves --l_ply without --calib, one rig serves a --batch_list; and -- without a GPU -- a malformed rig file, a rig
that cannot be rectified and --rig together with --calib are refused before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import pngio
import rectify_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
DATA = os.path.join(ROOT, "tests", "golden", "rectify")
RIG, L_RAW, R_RAW = (os.path.join(DATA, n) for n in ("rig.txt", "l_raw.png", "r_raw.png"))


def _parse_rig(path):
    """the rig file read by the test itself: float() of the file's tokens, the doubles the host reader's strtod gives"""
    kv = dict(line.strip().split("=", 1) for line in open(path) if "=" in line and not line.startswith("#"))
    nums = {k: [float(t) for t in re.findall(r"[-+0-9.eE]+", v)] for k, v in kv.items()}
    cams = []
    for v in (0, 1):
        m, d = nums[f"cam{v}"], nums[f"dist{v}"]
        cams.append(rr.camera(m[0], m[4], m[2], m[5], m[1], *d))
    return rr.make_rig(cams[0], cams[1], np.array(nums["R"]).reshape(3, 3), nums["T"], int(nums["width"][0]), int(nums["height"][0]))


def _base(tmp_path, l=L_RAW, r=R_RAW):
    return [MAIN, f"--l_img_file={l}", f"--r_img_file={r}", f"--l_dis_file={tmp_path / 'l.png'}", f"--r_dis_file={tmp_path / 'r.png'}", "--max_dis=16",
            "--dis_scale=8", "--cc_name=GRD", "--iters=1", "--seed=3"]


def _ply_vertices(path):
    head = open(path, "rb").read(400)
    return int(re.search(rb"element vertex (\d+)", head).group(1))


@pytest.mark.gpu
def test_cli_rig_rectified_images_ply_and_batch(tmp_path):
    rig = _parse_rig(RIG)
    raws = [np.ascontiguousarray(pngio.read_png(p)[..., ::-1]) for p in (L_RAW, R_RAW)]  # the file's RGB -> BGR
    lrect, rrect, ply = tmp_path / "l_rect.png", tmp_path / "r_rect.png", tmp_path / "l.ply"
    res = subprocess.run(_base(tmp_path) + [f"--rig={RIG}", f"--l_rect_file={lrect}", f"--r_rect_file={rrect}", f"--l_ply={ply}"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "Rectification: 96 x 64 raw -> 96 x 64" in res.stdout
    rect, _ = rr.compute(rig)
    for v, path in enumerate((lrect, rrect)):
        want = rr.rectify(rig, rect, v, raws[v])[0]
        assert 0.5 < (want.any(axis=2)).mean() < 1.0  # the data has a black border and is mostly valid
        assert np.array_equal(pngio.read_png(str(path))[..., ::-1], want), v
    assert pngio.read_png(str(tmp_path / "l.png")).shape == (64, 96)
    assert 0 < _ply_vertices(ply) <= 96 * 64
    # another projection: the maps and every output follow --rect_f / --rect_w / --rect_h
    res = subprocess.run(_base(tmp_path) + [f"--rig={RIG}", f"--l_rect_file={lrect}", "--rect_f=70", "--rect_w=130", "--rect_h=37", "--quiet=true"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    rect2, _ = rr.compute(rig, f=70.0, w=130, h=37)
    assert np.array_equal(pngio.read_png(str(lrect))[..., ::-1], rr.rectify(rig, rect2, 0, raws[0])[0])
    assert pngio.read_png(str(tmp_path / "l.png")).shape == (37, 130)
    # one rig, a two-line batch: both pairs equal the single run of the same raw pair (the second swaps nothing but the output names)
    single = [pngio.read_png(str(tmp_path / n)) for n in ("l.png", "r.png")]
    blist = tmp_path / "batch.txt"
    blist.write_text("".join(f"{L_RAW} {R_RAW} {tmp_path / f'bl{k}.png'} {tmp_path / f'br{k}.png'}\n" for k in (0, 1)))
    res = subprocess.run(_base(tmp_path) + [f"--rig={RIG}", "--rect_f=70", "--rect_w=130", "--rect_h=37", f"--batch_list={blist}", "--in_flight=1"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "2 pairs" in res.stdout and "0 failed" in res.stdout, res.stdout + res.stderr
    for k in (0, 1):
        for n, want in zip((f"bl{k}.png", f"br{k}.png"), single):
            assert np.array_equal(pngio.read_png(str(tmp_path / n)), want), n
    # a raw pair of another size is that pair's error
    small = tmp_path / "small.png"
    pngio.write_png(str(small), raws[0][:40, :50, ::-1])
    res = subprocess.run(_base(tmp_path, small, small) + [f"--rig={RIG}"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "rig's size" in res.stdout, res.stdout


def test_cli_refuses_a_bad_rig_before_a_device_is_opened(tmp_path):
    text = open(RIG).read()
    cases = {
        "truncated matrix": text.replace("; 0 0 1]\ndist0", "]\ndist0", 1),
        "missing key": "\n".join(line for line in text.splitlines() if not line.startswith("T=")) + "\n",
        "not a number": text.replace("width=96", "width=wide"),
        "not a camera matrix": re.sub(r"cam1=\[([^;]*); 0 ", r"cam1=[\1; 0.5 ", text, count=1),
        "empty": "",
        "a key given twice": text + "T=[-0.2 0.0 0.0]\n",
    }
    for name, body in cases.items():
        bad = tmp_path / "bad_rig.txt"
        bad.write_text(body)
        res = subprocess.run(_base(tmp_path) + [f"--rig={bad}"], capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "can not read" in res.stdout and "rig file" in res.stdout, (name, res.stdout)
        assert "HIP" not in res.stdout and not (tmp_path / "l.png").exists(), name
    # well-formed, but camera 1 is on the left: the derivation's message, still before any device
    swapped = tmp_path / "swapped.txt"
    swapped.write_text(re.sub(r"T=\[-", "T=[", text, count=1))
    res = subprocess.run(_base(tmp_path) + [f"--rig={swapped}"], capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "camera 1 must be to the right" in res.stdout, res.stdout
    missing = subprocess.run(_base(tmp_path) + [f"--rig={tmp_path / 'nowhere.txt'}"], capture_output=True, text=True, timeout=60)
    assert missing.returncode != 0 and "can not read" in missing.stdout


def test_cli_refuses_rig_with_calib_and_rect_flags_without_rig(tmp_path):
    calib = tmp_path / "calib.txt"
    calib.write_text("cam0=[300 0 48; 0 300 32; 0 0 1]\ncam1=[300 0 48; 0 300 32; 0 0 1]\ndoffs=0\nbaseline=0.2\nwidth=96\nheight=64\n")
    res = subprocess.run(_base(tmp_path) + [f"--rig={RIG}", f"--calib={calib}"], capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "not with --calib" in res.stdout, res.stdout
    assert "HIP" not in res.stdout and not (tmp_path / "l.png").exists()
    for flags in (["--rect_f=70"], [f"--l_rect_file={tmp_path / 'x.png'}"]):
        res = subprocess.run(_base(tmp_path) + flags, capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "need --rig" in res.stdout, res.stdout
    res = subprocess.run(_base(tmp_path) + [f"--rig={RIG}", f"--l_rect_file={tmp_path / 'x.png'}", f"--batch_list={calib}"], capture_output=True, text=True,
                         timeout=60)
    assert res.returncode != 0 and "not with --batch_list" in res.stdout, res.stdout
