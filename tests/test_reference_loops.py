"""The reference's OWN loops next to the oracle (round-4 review, item 7).

cs_patchmatch.cc, plane_cost/pre_ss_pc.cc, pre_cs_pc.cc, grd_pc.cc, cspc.cc, cc/grd_cc.cpp and cc/cen_cc.cc are compiled UNMODIFIED
against test-only stand-ins for <opencv2/opencv.hpp> and <gflags/gflags.h> (tests/helpers/refcheck/): every OpenCV call is delegated to
the oracle's restated contracts and cv::RNG is the specified counter-based generator in its ROW_SHARED mode (the reference builds
with USE_OMP and re-seeds every row, cs_patchmatch.cc:129-131).  THIS PINS NOTHING -- a build against stand-ins is not a reference
build -- but it is the one available check that the oracle's TRANSCRIPTION of the reference-owned code
(loop structure, traversal orders, strict-`<` accept rules, indexing, the order of the random draws, post-processing) has no slip:
planes, stored costs, 8-bit maps and sampled GetPlaneCost values must be identical to the oracle's reference order, bit for bit.

What that binary computed on every case below is recorded under tests/golden/refloops_<case>.npz (inputs and outputs,
tests/golden/make_refloops.py), so the oracle is held against it on any checkout.  Where build() could compile the binary
(oracle/build_ref.py -> oracle/_ref/refcheck: the reference checkout was readable), it is also run here and must reproduce the
record.  Nothing of the reference enters the repository."""
import os
import struct
import subprocess

import numpy as np
import pytest

from crossscalepatchmatch_amd import synth
from oracle import build_ref
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIS_SCALE, SEED = 16, 4321


def golden_path(name):
    return os.path.join(GOLDEN, f"refloops_{name}.npz")


def _run_reference(exe, tmp_path, l, r, max_dis, dis_scale, scale_num, lam, iters, use_pp, wnd, seed, queries, kind=0):
    h, w = l.shape[:2]
    xyv, npnt = queries
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<9i", w, h, max_dis, dis_scale, scale_num, iters, int(use_pp), wnd, kind))
        f.write(struct.pack("<dQ", lam, seed))
        f.write(np.ascontiguousarray(l, np.uint8).tobytes())
        f.write(np.ascontiguousarray(r, np.uint8).tobytes())
        f.write(struct.pack("<i", len(xyv)))
        f.write(np.ascontiguousarray(xyv, np.int32).tobytes())
        f.write(np.ascontiguousarray(npnt, np.float64).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=900)
    raw = open(tmp_path / "out.bin", "rb").read()
    nq = len(xyv)
    qcost = np.frombuffer(raw, np.float64, nq)
    off = nq * 8
    views = []
    for v in (0, 1):
        rec = np.frombuffer(raw, np.float64, w * h * 10, off).reshape(h, w, 10)
        off += w * h * 80
        dis = np.frombuffer(raw, np.uint8, w * h, off).reshape(h, w)
        off += w * h
        views.append((rec, dis))
    assert off == len(raw)
    return qcost, views


def _queries(rng, n, w, h, max_dis):
    xyv = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 2, n)], 1).astype(np.int32)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[0] = [0.0, 0.0, 1.0]
    nrm[1] = [0.6, 0.8, 1e-9]   # |nz| < kDoubleEps
    nrm[2] = [0.0, 0.0, -1.0]
    z = rng.uniform(-0.3 * max_dis, 1.3 * max_dis, n)
    z[0] = 5.0
    pnt = np.stack([xyv[:, 0], xyv[:, 1], z], 1).astype(np.float64)
    return xyv, np.concatenate([nrm, pnt], 1)


CASES = [
    # name, pair, (w, h, max_dis), scale_num, lambda, iters, use_pp, wnd, cost ("GRD" / "CEN": CCMethod + PreSSPC / PreCSPC; "IMG": GrdPC / CSPC)
    ("ss_noise", "noise", (40, 26, 10), 0, 0.0, 2, True, 9, "GRD"),
    ("cs_noise", "noise", (44, 30, 12), 3, 0.3, 2, True, 9, "GRD"),
    ("cs5_lambda0", "noise", (48, 34, 16), 5, 0.0, 1, False, 7, "GRD"),
    ("cs_blocks", "blocks", (40, 28, 10), 3, 0.3, 2, True, 9, "GRD"),
    ("ss_black", "black", (36, 24, 8), 0, 0.0, 2, True, 9, "GRD"),
    ("cs_dup_rows_odd_iters", "dup_rows", (41, 27, 10), 2, 1.0, 3, True, 7, "GRD"),
    ("census_cs", "noise", (42, 28, 10), 3, 0.3, 2, True, 9, "CEN"),
    ("census_ss_blocks", "blocks", (40, 26, 8), 0, 0.0, 2, True, 9, "CEN"),
    ("grdpc", "noise", (40, 26, 10), 0, 0.0, 2, True, 9, "IMG"),
    ("cspc", "noise", (44, 30, 12), 3, 0.3, 2, True, 9, "IMG"),
    ("cspc_periodic", "periodic", (40, 26, 10), 2, 0.3, 2, True, 7, "IMG"),
]


def case_inputs(name, kind, dims):
    """the pair and the GetPlaneCost queries of one case (what the record was made from)"""
    w, h, max_dis = dims
    if kind == "noise":
        l, r = synth.make_pair(w, h, max_dis, regions=2, seed=len(name))[:2]
    else:
        l, r = synth.make_adversarial(kind, w, h, max_dis, seed=3)
    rng = np.random.default_rng(7)
    return l, r, _queries(rng, 60, w, h, max_dis)


def run_case(exe, tmp_path, name, kind, dims, scale_num, lam, iters, use_pp, wnd, cc):
    """the reference binary on one case: (GetPlaneCost of the queries, [(plane records [h, w, 10], 8-bit map)] per view)"""
    l, r, queries = case_inputs(name, kind, dims)
    return _run_reference(exe, tmp_path, l, r, dims[2], DIS_SCALE, scale_num, lam, iters, use_pp, wnd, SEED, queries,
                          kind={"GRD": 0, "CEN": 1, "IMG": 2}[cc])


@pytest.mark.parametrize("name,kind,dims,scale_num,lam,iters,use_pp,wnd,cc", CASES, ids=[c[0] for c in CASES])
def test_reference_loops_equal_the_oracle(tmp_path, name, kind, dims, scale_num, lam, iters, use_pp, wnd, cc):
    w, h, max_dis = dims
    dis_scale, seed = DIS_SCALE, SEED
    l, r, queries = case_inputs(name, kind, dims)
    with np.load(golden_path(name)) as g:
        rec_in = {k: g[k] for k in ("l", "r", "xyv", "npnt")}
        qcost = g["qcost"]
        views = [(g["planes0"], g["dis0"]), (g["planes1"], g["dis1"])]
    # the record is of exactly these inputs
    for key, want in (("l", l), ("r", r), ("xyv", queries[0]), ("npnt", queries[1])):
        np.testing.assert_array_equal(rec_in[key], want, err_msg=f"{name}: recorded input {key} (tests/golden/make_refloops.py)")
    # the reference's loops themselves, where build() could compile them: they reproduce the record
    failed = build_ref.failure(build_ref.REFCHECK)
    if failed is not None:
        pytest.fail("oracle/_ref/refcheck did not build:\n" + failed)
    if os.path.exists(build_ref.REFCHECK):
        live_q, live_views = run_case(build_ref.REFCHECK, tmp_path, name, kind, dims, scale_num, lam, iters, use_pp, wnd, cc)
        np.testing.assert_array_equal(live_q, qcost, err_msg=f"{name}: the reference binary's GetPlaneCost against its record")
        for v in (0, 1):
            np.testing.assert_array_equal(live_views[v][0], views[v][0], err_msg=f"{name}: the reference binary's planes against its record, view {v}")
            np.testing.assert_array_equal(live_views[v][1], views[v][1], err_msg=f"{name}: the reference binary's 8-bit map against its record, view {v}")
    # the oracle: reference order (serial sweep, serial window sum), one thread, the row-shared random streams of the reference's USE_OMP build
    pc = po.PlaneCost(l, r, max_dis, wnd, scale_num, lam, cc=cc)
    xyv, npnt = queries
    want = np.array([pc.cost(xyv[i, 0], xyv[i, 1], npnt[i, :3], po.plane_param(npnt[i, :3], npnt[i, 3:]), xyv[i, 2], po.SUM_SERIAL)
                     for i in range(len(xyv))])
    np.testing.assert_array_equal(qcost, want, err_msg="GetPlaneCost (pre_ss_pc.cc:74-118 / pre_cs_pc.cc:133-188 / grd_pc.cc:72-176 / cspc.cc:107-183)")
    pm = po.PatchMatch(l, r, max_dis, dis_scale)
    pm.run(iters, pc, use_pp, seed=seed, schedule=po.SCHED_RASTER, sum_order=po.SUM_SERIAL, rng_mode=po.RNG_ROW_SHARED, threads=1)
    for v in (0, 1):
        rec, dis = views[v]
        P = pm.planes(v)
        np.testing.assert_array_equal(rec[..., 0:3], P[..., 0:3], err_msg=f"{name}: normals, view {v}")
        np.testing.assert_array_equal(rec[..., 3:6], P[..., 3:6], err_msg=f"{name}: points, view {v}")
        np.testing.assert_array_equal(rec[..., 6:9], P[..., 6:9], err_msg=f"{name}: plane parameters, view {v}")
        np.testing.assert_array_equal(rec[..., 9], pm.min_cost(v), err_msg=f"{name}: stored costs, view {v}")
        np.testing.assert_array_equal(dis, pm.dis(v), err_msg=f"{name}: 8-bit map{' after post-processing' if use_pp else ''}, view {v}")
