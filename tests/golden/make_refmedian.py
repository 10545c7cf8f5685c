#!/usr/bin/env python
"""Records tests/golden/refmedian_<case>.npz: what the reference's own median filter (ctmf.c of the reference checkout, compiled in
place into a temporary directory with one `gcc -O2 -shared` call and loaded with ctypes) computes on every case of
tests/median_ref.py -- the input image, r, cn, memsize and the output.  Only these data files are committed; nothing of the
reference's text, and nothing compiled from it, enters the repository.

Run from the repo root where the reference checkout is readable:  python tests/golden/make_refmedian.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import build_ref  # noqa: E402
import median_ref as mr  # noqa: E402


def load_reference_filter(tmp):
    """the reference's ctmf() as a ctypes function, or None when the checkout or gcc is missing"""
    ref = build_ref.reference_dir()
    src = os.path.join(ref, "ctmf.c") if ref else None
    if not src or not os.path.exists(src):
        return None
    so = os.path.join(tmp, "libctmf.so")
    try:
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-o", so, src])
    except (OSError, subprocess.CalledProcessError):
        return None
    fn = C.CDLL(so).ctmf
    u8p = C.POINTER(C.c_uint8)
    fn.restype, fn.argtypes = None, [u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulong]
    return fn


def run_reference(fn, img, r, cn, memsize):
    src = np.ascontiguousarray(img)
    h, w = src.shape[:2]
    dst = np.zeros_like(src)
    u8p = C.POINTER(C.c_uint8)
    fn(src.ctypes.data_as(u8p), dst.ctypes.data_as(u8p), w, h, w * cn, w * cn, r, cn, memsize)
    return dst


def main():
    total = 0
    with tempfile.TemporaryDirectory() as tmp:
        fn = load_reference_filter(tmp)
        if fn is None:
            raise SystemExit("the reference checkout's ctmf.c or gcc is missing")
        for case in mr.all_cases():
            w, h, r, cn, memsize, kind = case
            assert memsize // 544 > 2 * r, "the reference's stripe arithmetic needs memsize / 544 > 2r"
            img = mr.case_input(*case)
            out = run_reference(fn, img, r, cn, memsize)
            path = mr.golden_path(mr.case_name(*case))
            np.savez_compressed(path, src=img, r=r, cn=cn, memsize=memsize, out=out)
            total += os.path.getsize(path)
            print(mr.case_name(*case), os.path.getsize(path), "bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
