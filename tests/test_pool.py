"""DevPool (crossscalepatchmatch_amd/csrc/cspm_pool.h, DESIGN.md "Context memory"), the owner of everything a context keeps on the device,
over a fake allocator that counts live blocks and fails the k-th call: tests/helpers/pool_check.cc, a stand-alone program that includes the
header alone, built and run plain and once more under AddressSanitizer and UBSan.  Its cases: get on a set slot allocates nothing; a failing
k-th get hands the status back, leaves its slot null and the earlier entries owned, and the sequence repeated allocates exactly the missing
ones; release frees every base once and nulls every slot, also after two slots' contents were swapped and with a lead in front of the slot's
pointer; rewind and drop free only their entries; bytes() follows every step; no elements means one; the destructor releases; nothing is
live at the end of any case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, *flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("pool_check" + ("_san" if flags else "")))
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "crossscalepatchmatch_amd", "csrc"),
           os.path.join(ROOT, "tests", "helpers", "pool_check.cc"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pool_check ok" in r.stdout


def test_pool_header_includes_no_hip_header():
    src = open(os.path.join(ROOT, "crossscalepatchmatch_amd", "csrc", "cspm_pool.h")).read()
    assert "#include <hip" not in src and "#include \"cspm_" not in src


def test_pool_owns_every_allocation(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    _run(exe)


def test_pool_owns_every_allocation_under_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0:
        pytest.skip("the C++ compiler has no AddressSanitizer / UBSan runtime: " + r.stderr.strip().splitlines()[-1][:120])
    _run(exe)
