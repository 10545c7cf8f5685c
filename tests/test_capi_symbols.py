"""-m "not gpu": libcspm_hip.so builds (hipcc cross-compiles gfx950 without a GPU), loads, exports every
symbol include/cspm.h declares, and refuses to compute without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

import crossscalepatchmatch_amd as cs
from crossscalepatchmatch_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "cspm.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cspm_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree():
    assert _declared() == sorted(capi.SYMBOLS)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(cs.library_path()):
        cs.build_library()
    lib = C.CDLL(cs.library_path())
    for name in _declared():
        assert hasattr(lib, name), name


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = cs.load_library()
    assert L.cspm_device_count() == 0
    with pytest.raises(cs.CspmError, match="no HIP device"):
        cs.StereoContext(0)
    p = capi.PmParams()
    assert L.cspm_pm_default_params(C.byref(p)) == 0 and p.early_exit == 1  # pure host logic still answers


def _one_shot_call(name, bad):
    """One call of a one-shot host entry on 2 x 2 inputs, every output pre-filled with the byte 0xAB.  Returns (rc, outputs, the
    message its argument check gives).  With `bad`, one argument is invalid, taken from the entry's own check."""
    import numpy as np
    L = cs.load_library()
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    outs = []

    def out(nbytes):
        outs.append(np.full(nbytes, 0xAB, np.uint8))
        return outs[-1]

    f64 = lambda n: out(8 * n).ctypes.data_as(dp)
    u8 = lambda n: out(n).ctypes.data_as(u8p)
    i32 = lambda n: out(4 * n).ctypes.data_as(i32p)
    u32 = lambda n: out(4 * n).ctypes.data_as(C.POINTER(C.c_uint))
    raw = lambda n: out(n).ctypes.data_as(C.c_void_p)
    w = h = 2
    n = w * h
    disp = np.ones((h, w))
    bgr = np.arange(3 * n, dtype=np.uint8).reshape(h, w, 3)
    rgb = bgr.astype(np.float64)
    calib = capi.Calib(100.0, 0.5, 0.5, 0.1, 0.0)
    keep = [disp, bgr, rgb]  # inputs stay alive over the call
    if name in ("cspm_grd_build_cv_host", "cspm_cen_build_cv_host", "cspm_cengrd_build_cv_host"):
        rc = getattr(L, name)(0, capi._dp(rgb), capi._dp(rgb), w, h, 0 if bad else 2, 0, f64(2 * n))
        msg = "bad arguments"
    elif name == "cspm_aggregate_cv_host":
        # 7 x 7: the smallest slabs BOX takes (its own check refuses 2 x 2 before the device), and two slices, since one is no work
        guide = np.zeros((7, 7, 3))
        keep.append(guide)
        rc = L.cspm_aggregate_cv_host(0, 99 if bad else capi.CA_BOX, capi._dp(guide), 7, 7, 2, f64(2 * 49))
        msg = "unknown aggregation method (CSPM_CA_BOX / GF / BF)"
    elif name == "cspm_filter_speckles_host":
        rc = L.cspm_filter_speckles_host(0, capi._dp(disp), None, w, h, -1 if bad else 1, 1.0, u8(n), i32(n))
        msg = "bad arguments"
    elif name == "cspm_fit_planes_host":
        rc = L.cspm_fit_planes_host(0, capi._dp(disp), None, None, 0, w, h, -1 if bad else 4, None, f64(6 * n), u8(n))
        msg = "bad arguments"
    elif name == "cspm_segment_host":
        K = L.cspm_segment_count(w, h, 16)
        assert K == 1
        rc = L.cspm_segment_host(0, capi._u8(bgr), 5 if bad else 6, w, h, None, i32(n), i32(5 * K), i32(K))
        msg = "bad arguments"
    elif name == "cspm_segment_planes_host":
        labels = np.zeros(n, np.int32)
        keep.append(labels)
        rc = L.cspm_segment_planes_host(0, capi._dp(disp), None, capi._i32(labels), w, h, -1 if bad else 4, None, f64(3), i32(1), f64(6 * n), u8(n))
        msg = "bad arguments"
    elif name == "cspm_median_filter_u8_host":
        src = np.arange(n, dtype=np.uint8)
        keep.append(src)
        rc = L.cspm_median_filter_u8_host(0, capi._u8(src), w, w, h, 1, 0 if bad else 1, u8(n), w)
        msg = "bad arguments"
    elif name == "cspm_median_filter_f64_host":
        rc = L.cspm_median_filter_f64_host(0, capi._dp(disp), w, h, 0 if bad else 1, f64(n))
        msg = "bad arguments"
    elif name == "cspm_smooth_disparity_host":
        rc = L.cspm_smooth_disparity_host(0, capi._dp(disp), None, None, w, h, None, -1 if bad else 4, f64(n))
        msg = "bad arguments"
    elif name == "cspm_reproject_host":
        rc = L.cspm_reproject_host(0, C.byref(calib), None, 2 if bad else 0, capi._dp(disp), None, None, None, None, 0, w, h, f64(n), f64(3 * n), None,
                                   u8(n), raw(32 * n), n, u32(1))
        msg = "reprojection: view must be 0 or 1"
    elif name == "cspm_mesh_host":
        rc = L.cspm_mesh_host(0, C.byref(calib), None, None, 2 if bad else 0, capi._dp(disp), None, None, None, None, 0, w, h, raw(32 * n), n, raw(12 * 2), 2,
                              u8(n), u32(1), u32(1))
        msg = "reprojection: view must be 0 or 1"
    elif name == "cspm_synthesize_host":
        view = capi.SynthView(capi._dp(disp), None, None, capi._u8(bgr), 3 * w)
        rc = L.cspm_synthesize_host(0, None, 2.0 if bad else 0.5, C.byref(view), C.byref(view), w, h, u8(3 * n), 3 * w, f64(n), u8(n))
        msg = "view synthesis: t must be in [0, 1]"
    elif name == "cspm_rectify_host":
        cam = capi.Camera(2.0, 2.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
        rig = capi.Rig((capi.Camera * 2)(cam, cam), eye, (C.c_double * 3)(-1.0, 0.0, 0.0), w, h)
        rect = capi.Rectification()
        assert L.cspm_rectify_compute(C.byref(rig), None, C.byref(rect), None) == 0, L.cspm_last_error(None)
        m = rect.w * rect.h
        rc = L.cspm_rectify_host(0, C.byref(rig), C.byref(rect), 2 if bad else 0, capi._u8(bgr), 3 * w, u8(3 * m), 3 * rect.w, f64(2 * m), u8(m))
        msg = "rectification: view must be 0 or 1"
    else:
        raise AssertionError(name)
    del keep
    return rc, outs, msg


ONE_SHOT_ENTRIES = sorted(s for s in capi.SYMBOLS if s.endswith("_host") and s != "cspm_merge_planes_host")  # that one works on a context


def test_there_are_fifteen_one_shot_entries():
    assert len(ONE_SHOT_ENTRIES) == 15


@pytest.mark.parametrize("name", ONE_SHOT_ENTRIES)
def test_one_shot_entry_without_a_device(name):
    """valid arguments and no device: the HIP error code, cspm_create's message in the thread's creation error, no output written"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, outs, _ = _one_shot_call(name, bad=False)
    assert rc == -2  # CSPM_ERR_HIP
    assert cs.load_library().cspm_last_error(None).decode().startswith("no HIP device")
    assert outs and all((o == 0xAB).all() for o in outs)


@pytest.mark.parametrize("name", ONE_SHOT_ENTRIES)
def test_one_shot_entry_checks_its_arguments_before_the_device(name):
    """one invalid argument: CSPM_ERR_ARG and the check's own message, whether there is a device or not; no output written"""
    rc, outs, msg = _one_shot_call(name, bad=True)
    assert rc == -1  # CSPM_ERR_ARG
    assert cs.load_library().cspm_last_error(None).decode() == msg and msg
    assert outs and all((o == 0xAB).all() for o in outs)


def test_product_does_not_reference_the_oracle():
    """The oracle is test infrastructure: nothing under crossscalepatchmatch_amd/ (the product) or tools/ (profiling and build
    helpers) may import, link or load it -- only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do."""
    for top in ("crossscalepatchmatch_amd", "tools", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".sh", ".h", ".hip", ".cc", ".cpp", ".c", "Makefile")):
                    txt = open(os.path.join(dirpath, f), errors="ignore").read()
                    assert "pyoracle" not in txt and "cspm_oracle" not in txt and "libcspm_oracle" not in txt, os.path.join(dirpath, f)


def test_bench_fails_loudly_without_a_gpu():
    """bench.py has no CPU path either: without a visible GPU it must exit non-zero with a message, for any --gpus."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in ([], ["--gpus", "2"]):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0"] + extra, capture_output=True, timeout=600)
        assert p.returncode != 0
        assert b"needs a GPU" in p.stderr + p.stdout


def test_kernel_source_hash_ignores_comments_but_not_code(tmp_path, monkeypatch):
    """bench.py quotes the committed rocprofv3 counters (profiles/refine_pmc.json) only while kernel_source_hash() equals the hash
    the file was stamped with: editing a comment must not invalidate a measurement, editing code must."""
    import bench
    d = tmp_path / "crossscalepatchmatch_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "a.h").write_text("// header\nint f(int x) { return x + 1; }  /* plus one */\n")
    (d / "b.hip").write_text("__global__ void k() {}\n")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    h0 = bench.kernel_source_hash()
    (d / "a.h").write_text("// another header comment\n\nint f(int x) {\n  return x + 1;   /* still plus one */\n}\n")
    assert bench.kernel_source_hash() == h0
    (d / "a.h").write_text("// header\nint f(int x) { return x + 2; }\n")
    assert bench.kernel_source_hash() != h0


def test_effective_cpus_is_bounded_by_what_the_container_may_use():
    from oracle import pyoracle as po
    n = po.effective_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    try:
        assert n <= len(os.sched_getaffinity(0))
    except AttributeError:
        pass


def test_header_is_plain_c_and_links_from_c(tmp_path):
    """include/cspm.h is the boundary a cgo / JNI / ctypes binding is written against: it must compile as pedantic C99 (no C++
    in the signatures) and a C program must link against the shared library and get a status code -- not an exception -- back."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "crossscalepatchmatch_amd")
    src = tmp_path / "bind.c"
    src.write_text('#include <stdio.h>\n#include "cspm.h"\n'
                   "int main(void) {\n"
                   "  cspm_ctx *ctx = NULL;\n"
                   "  int rc = cspm_create(&ctx, 1 << 20);  /* no such device anywhere: an error code either way */\n"
                   '  printf("%d|%s\\n", rc, cspm_last_error(NULL));\n'
                   "  if (ctx) cspm_destroy(ctx);\n"
                   "  return rc == CSPM_OK;\n"
                   "}\n")
    exe = tmp_path / "bind"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lcspm_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rc, msg = out.stdout.strip().split("|", 1)
    assert int(rc) < 0 and msg  # a negative status and a message


def test_python_constants_mirror_the_header():
    """capi.py repeats the option keys, kernel classes and phase codes of include/cspm.h by hand: they must not drift apart."""
    import re
    from crossscalepatchmatch_amd import capi
    hdr = open(os.path.join(ROOT, "include", "cspm.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(CSPM_[A-Z0-9_]+)\s+(-?\d+)\s*(?:/\*.*)?$", hdr, re.M)}
    opts = {k: v for k, v in defs.items() if k.startswith("CSPM_OPT_")}
    assert len(set(opts.values())) == len(opts), "two options share a key"
    for name, value in opts.items():
        py = name[len("CSPM_"):]
        assert getattr(capi, py) == value, name
    for k, name in enumerate(capi.K_NAMES):
        assert defs["CSPM_K_" + {"grd": "GRD", "init": "INIT", "spatial": "SPATIAL", "view": "VIEW", "refine": "REFINE", "misc": "MISC", "post": "POST"}[name]] == k
    assert defs["CSPM_K_COUNT"] == len(capi.K_NAMES)
