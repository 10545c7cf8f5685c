"""Builds the three reference-derived checkers into oracle/_ref/ (kept out of git) when the reference checkout is readable.

- oracle/_ref/refcheck: the reference's own CSPatchMatch / PreSSPC / PreCSPC / GrdCC / CenCC / GrdPC / CSPC, compiled UNMODIFIED
  against the test-only stand-ins for <opencv2/opencv.hpp> and <gflags/gflags.h> (tests/helpers/refcheck/) and driven by
  tests/helpers/refcheck_main.cc.  tests/golden/make_refloops.py records its outputs under tests/golden/; tests/test_reference_loops.py
  holds the oracle against those records and, where this binary exists, the binary against them.
- oracle/_ref/cacheck: the reference's own cost-aggregation filters (ca_filter/GuidedFilter.cpp, BilateralFilter.cpp, BoxCA.cpp, GFCA.cpp,
  BFCA.cpp), compiled UNMODIFIED against the same stand-in and driven by tests/helpers/cacheck_main.cc.  tests/golden/make_refca.py
  records its outputs; tests/test_reference_ca.py holds tests/ca_ref.py against those records and, where this binary exists, the binary
  against them; tests/test_gpu_ca_reference.py holds the HIP kernels against the records.
- oracle/_ref/cspm_ref_main: the reference's main.cc, unchanged, compiled and linked against crossscalepatchmatch_amd/host/
  (tests/test_host_layer.py runs it).

The reference checkout is found at $CSPM_REFERENCE_DIR, else at BASELINE.json's "reference_path".  Without it nothing is built and
the tests that need these binaries say so.  A compile that fails leaves <name>.failed with the compiler's output instead of the
binary, for the test to report.  Nothing of the reference is copied into the repository: main.cc is compiled from a temporary copy.

    python oracle/build_ref.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref")
HOST = os.path.join(ROOT, "crossscalepatchmatch_amd", "host")
HELP = os.path.join(ROOT, "tests", "helpers")
LOOP_SOURCES = ["cs_patchmatch.cc", "plane_cost/pre_ss_pc.cc", "plane_cost/pre_cs_pc.cc", "cc/grd_cc.cpp", "cc/cen_cc.cc", "plane_cost/grd_pc.cc",
                "plane_cost/cspc.cc"]
CA_SOURCES = ["ca_filter/GuidedFilter.cpp", "ca_filter/BilateralFilter.cpp", "ca_filter/BoxCA.cpp", "ca_filter/GFCA.cpp", "ca_filter/BFCA.cpp"]
REFCHECK = os.path.join(OUT, "refcheck")
CACHECK = os.path.join(OUT, "cacheck")
REF_MAIN = os.path.join(OUT, "cspm_ref_main")


def reference_dir():
    """the reference's CSPM/ source directory, or None when it is not readable here"""
    base = os.environ.get("CSPM_REFERENCE_DIR")
    if not base:
        try:
            with open(os.path.join(ROOT, "BASELINE.json")) as f:
                base = json.load(f).get("reference_path")
        except (OSError, ValueError):
            base = None
    if not base:
        return None
    d = os.path.join(base, "CSPM")
    need = LOOP_SOURCES + CA_SOURCES + ["main.cc"]
    return d if all(os.access(os.path.join(d, s), os.R_OK) for s in need) else None


def failure(exe):
    """the compiler output of a failed build of `exe`, or None"""
    p = exe + ".failed"
    if os.path.exists(p):
        with open(p, errors="replace") as f:
            return f.read()
    return None


def _compile(exe, cmd):
    for p in (exe, exe + ".failed"):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        with open(exe + ".failed", "w") as f:
            f.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        print(f"oracle/build_ref.py: building {os.path.relpath(exe, ROOT)} failed (see {os.path.relpath(exe, ROOT)}.failed)", file=sys.stderr)


def build():
    """needs oracle/libcspm_oracle.so and crossscalepatchmatch_amd/libcspm_hip.so (build() makes both first); returns the reference
    directory it compiled from, or None"""
    ref = reference_dir()
    if ref is None:
        return None
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        # the reference spells its includes with backslashes (cs_patchmatch.h:12, cc/grd_cc.h:2-3): forwarding headers whose NAMES
        # contain the backslash let GCC resolve them
        fwd = os.path.join(tmp, "fwd")
        subprocess.check_call(["sh", os.path.join(HOST, "make_forwarding_headers.sh"), fwd])
        for hname in ("commfunc.h", "cc_method.h"):  # cc/grd_cc.h:2-3: #include "..\commfunc.h"
            with open(os.path.join(fwd, "..\\" + hname), "w") as f:
                f.write(f'#pragma once\n#include "{hname}"\n')
        # ca_filter/*.h: #include "..\\CommFunc.h" and "..\\CAMethod.h", while the files are commfunc.h and ca_method.h
        for wname, hname in (("CommFunc.h", "commfunc.h"), ("CAMethod.h", "ca_method.h")):
            with open(os.path.join(fwd, "..\\" + wname), "w") as f:
                f.write(f'#pragma once\n#include "{hname}"\n')
        # no -fopenmp: the rows run in order, so the n-th cv::RNG is the n-th row (stand-in header)
        _compile(REFCHECK, ["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-w", "-I", fwd, "-I", os.path.join(HELP, "refcheck"), "-I", ref,
                            "-o", REFCHECK, os.path.join(HELP, "refcheck_main.cc")] + [os.path.join(ref, s) for s in LOOP_SOURCES] +
                 ["-L", os.path.join(ROOT, "oracle"), "-lcspm_oracle", "-Wl,-rpath,$ORIGIN/.."])
        _compile(CACHECK, ["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-w", "-I", fwd, "-I", os.path.join(HELP, "refcheck"), "-I", ref,
                           "-o", CACHECK, os.path.join(HELP, "cacheck_main.cc")] + [os.path.join(ref, s) for s in CA_SOURCES] +
                 ["-L", os.path.join(ROOT, "oracle"), "-lcspm_oracle", "-Wl,-rpath,$ORIGIN/.."])
        # main.cc from a copy: next to the reference's own headers its quoted includes would not reach host/
        src = os.path.join(tmp, "main.cc")
        shutil.copyfile(os.path.join(ref, "main.cc"), src)
        pkg = os.path.join(ROOT, "crossscalepatchmatch_amd")
        _compile(REF_MAIN, ["g++", "-O1", "-std=c++14", "-I", fwd, "-I", HOST, "-o", REF_MAIN, src, os.path.join(HOST, "host_impl.cc"),
                            os.path.join(HOST, "image_io.cc"), "-L", pkg, "-lcspm_hip", "-lz", "-Wl,-rpath,$ORIGIN/../../crossscalepatchmatch_amd"])
    return ref


if __name__ == "__main__":
    print(build() or "no reference checkout: nothing built")
