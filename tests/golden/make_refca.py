#!/usr/bin/env python
"""Records tests/golden/refca_<case>.npz: what the reference's own cost-aggregation filters (oracle/_ref/cacheck, built by build()
through oracle/build_ref.py where the reference checkout is readable) compute on every case of tests/test_reference_ca.py -- the
inputs (guide, stack of slabs) and the output stack.

Run from the repo root after build():  python tests/golden/make_refca.py
"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import build_ref  # noqa: E402
import test_reference_ca as t  # noqa: E402


def main():
    if not os.path.exists(build_ref.CACHECK):
        raise SystemExit(f"{build_ref.CACHECK} is missing: run build() where the reference checkout is readable")
    total = 0
    for name, op, dims, slabs, guide in t.CASES:
        g, vol = t.case_inputs(name, dims, slabs, guide)
        with tempfile.TemporaryDirectory() as tmp:
            out = t.run_reference(build_ref.CACHECK, Path(tmp), op, g, vol)
        np.savez_compressed(t.golden_path(name), guide=g, vol=vol, out=out)
        total += os.path.getsize(t.golden_path(name))
        print(name, os.path.getsize(t.golden_path(name)), "bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
