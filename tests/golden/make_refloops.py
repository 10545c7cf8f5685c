#!/usr/bin/env python
"""Records tests/golden/refloops_<case>.npz: what the reference's own loops (oracle/_ref/refcheck, built by build() through
oracle/build_ref.py where the reference checkout is readable) compute on every case of tests/test_reference_loops.py -- the inputs
(pair, GetPlaneCost queries) and the outputs (the queries' costs, both views' plane records [h, w, 10] and 8-bit maps).

Run from the repo root after build():  python tests/golden/make_refloops.py
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
import test_reference_loops as t  # noqa: E402


def main():
    if not os.path.exists(build_ref.REFCHECK):
        raise SystemExit(f"{build_ref.REFCHECK} is missing: run build() where the reference checkout is readable")
    for case in t.CASES:
        name, kind, dims = case[:3]
        with tempfile.TemporaryDirectory() as tmp:
            qcost, views = t.run_case(build_ref.REFCHECK, Path(tmp), *case)
        l, r, (xyv, npnt) = t.case_inputs(name, kind, dims)
        np.savez_compressed(t.golden_path(name), l=l, r=r, xyv=xyv, npnt=npnt, qcost=qcost,
                            planes0=views[0][0], dis0=views[0][1], planes1=views[1][0], dis1=views[1][1])
        print(name, os.path.getsize(t.golden_path(name)), "bytes")


if __name__ == "__main__":
    main()
