"""tests/seed_ref.py, the CPU restatement of candidate-field merging, checked on its own: the merge is a per-pixel minimum, idempotent
and inert on its own field; keep-init and an all-masked seeded run are the oracle's cold run.  Also what needs no device of the new
public surface: the three C ABI names and the cspm_main flags with their conflicts."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cengrd_ref
import seed_ref
import warm_ref
from crossscalepatchmatch_amd import capi
from crossscalepatchmatch_amd.synth import make_pair
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "crossscalepatchmatch_amd", "cspm_main")
W, H, D = 40, 28, 8
KW = dict(seed=5, schedule=po.SCHED_RASTER, sum_order=po.SUM_DEVICE)


@functools.lru_cache(maxsize=None)
def _images():
    l, r, _, _ = make_pair(W, H, D, regions=3, seed=31)
    return l, r


@functools.lru_cache(maxsize=None)
def _pc(cc):
    l, r = _images()
    if cc == "CENGRD":
        return cengrd_ref.plane_cost(l, r, D, 35, 2, 0.3)
    return po.PlaneCost(l, r, D, 35, 2, 0.3, cc)


def _pm():
    return po.PatchMatch(*_images(), D, 4)


def _state(pm):
    return [(warm_ref.field_of(pm, v), pm.planes(v)[..., 3:6].copy(), pm.min_cost(v).copy()) for v in (0, 1)]


def _assert_same(a, b, what):
    for v in (0, 1):
        for k, name in enumerate(("planes", "points", "min_cost")):
            np.testing.assert_array_equal(a[v][k], b[v][k], err_msg=f"{what}: {name}, view {v}")


def _init_field(seed, pc):
    pm = _pm()
    pm.init(pc, seed=seed, sum_order=po.SUM_DEVICE)
    return [warm_ref.field_of(pm, v) for v in (0, 1)]


@pytest.mark.parametrize("cc", ["GRD", "CENGRD"])
def test_merge_is_the_per_pixel_minimum(cc):
    pc = _pc(cc)
    pm = _pm()
    pm.init(pc, **{k: KW[k] for k in ("seed", "sum_order")})
    before = _state(pm)
    cand = _init_field(77, pc)
    mask = [None, (np.indices((H, W)).sum(0) % 2).astype(np.uint8)]
    cand[0][3, 4, 1] = np.nan
    cand[0][5, 6, 5] = np.inf
    taken = seed_ref.merge(pm, pc, cand, mask, po.SUM_DEVICE)
    assert 0 < taken < 2 * W * H
    for v in (0, 1):
        has = seed_ref.has_candidate(cand[v], mask[v])
        for y in range(H):
            for x in range(W):
                old_c = before[v][2][y, x]
                c = pc.cost(x, y, cand[v][y, x, :3], cand[v][y, x, 3:], v, po.SUM_DEVICE) if has[y, x] else np.inf
                assert pm.min_cost(v)[y, x] == min(old_c, c)
                want = cand[v][y, x] if c < old_c else before[v][0][y, x]
                np.testing.assert_array_equal(warm_ref.field_of(pm, v)[y, x], want)
    has0 = seed_ref.has_candidate(cand[0], mask[0])
    assert not has0[3, 4] and not has0[5, 6] and has0[3, 5]  # a NaN or an inf anywhere in the six values: no candidate
    once = _state(pm)
    assert seed_ref.merge(pm, pc, cand, mask, po.SUM_DEVICE) == 0  # merging twice gives what merging once gives
    _assert_same(_state(pm), once, "second merge")


def test_merging_a_field_into_itself_changes_nothing():
    pc = _pc("GRD")
    pm = _pm()
    pm.run(1, pc, False, **KW)
    before = _state(pm)
    assert seed_ref.merge(pm, pc, [warm_ref.field_of(pm, v) for v in (0, 1)], (None, None), po.SUM_DEVICE) == 0
    _assert_same(_state(pm), before, "self merge")


def test_init_keep_on_the_init_field_and_masked_seeded_run_are_the_cold_run():
    pc = _pc("GRD")
    pm = _pm()
    pm.init(pc, seed=5, sum_order=po.SUM_DEVICE)
    before = _state(pm)
    assert seed_ref.init_keep(pm, pc, seed=5, sum_order=po.SUM_DEVICE) == 0
    _assert_same(_state(pm), before, "keep-init on its own init field")
    assert seed_ref.init_keep(pm, pc, seed=6, sum_order=po.SUM_DEVICE) > 0  # another seed's planes do win somewhere
    assert all(np.all(pm.min_cost(v) <= before[v][2]) for v in (0, 1))
    cold = _pm()
    cold.run(2, pc, False, **KW)
    seeded = _pm()
    zeros = [np.zeros((H, W), np.uint8)] * 2
    seed_ref.seeded_run(seeded, pc, 2, [(_init_field(77, pc), zeros)], **KW)
    _assert_same(_state(seeded), _state(cold), "all-masked seeded run")


def test_capi_symbols_and_methods():
    for name in ("cspm_merge_planes", "cspm_merge_planes_host", "cspm_pm_init_keep"):
        assert name in capi.SYMBOLS
    for name in ("merge_planes_from", "merge_planes", "merge_disparity", "pm_init_keep"):
        assert callable(getattr(capi.StereoContext, name))
    assert callable(capi.seeded_patchmatch)
    d = np.array([[1.5, np.nan]])
    np.testing.assert_array_equal(capi.disparity_planes(d), seed_ref.disparity_planes(d))
    header = open(os.path.join(ROOT, "include", "cspm.h")).read()
    for name in ("cspm_merge_planes(", "cspm_merge_planes_host(", "cspm_pm_init_keep("):
        assert "int " + name in header


def _cli(*args):
    return subprocess.run([CLI, "--quiet=true"] + list(args), capture_output=True, timeout=60)


def test_cli_seed_flags_parse():
    """every check below fires before a device is opened: --pp_pfm without --use_pp is refused AFTER the flags were parsed"""
    p = _cli("--seed_ca=BOX", "--l_seed_pfm=l.pfm", "--r_seed_pfm=r.pfm", "--pp_pfm=true")
    assert p.returncode != 0
    assert b"unknown command line flag" not in p.stdout + p.stderr
    assert b"--pp_pfm" in p.stdout


@pytest.mark.parametrize("args", [("--seed_ca=BOX", "--warm_ca=BOX"), ("--seed_ca=GF", "--ca_name=BOX"), ("--seed_ca=BOX", "--pc_name=IMG"),
                                  ("--seed_ca=MEDIAN",), ("--seed_ca=BOX", "--pc_name=PLUGIN"), ("--l_seed_pfm=l.pfm", "--pc_name=PLUGIN"),
                                  ("--r_seed_pfm=r.pfm", "--warm_ca=BOX"), ("--l_seed_pfm=l.pfm", "--ca_name=GF")])
def test_cli_seed_flag_conflicts(args):
    p = _cli(*args)
    assert p.returncode != 0
    assert b"unknown command line flag" not in p.stdout + p.stderr
    assert b"seed" in p.stdout  # the message names the seeded start
