"""bench.py with N > 1 on the 1-GPU box: two ranks sharing GPU 0, gloo as the control plane (CSPM_BENCH_BACKEND=gloo -- the driver's
8-GPU runs use one rank per GPU and RCCL).  Covers the launcher bench.py becomes without torchrun, the barrier / MAX-over-ranks
timing and the whole-job `value`, for the sharded default (every rank times its own pairs) and for C4 (rank 0 holds the batch,
batch.run_batch dispatches it)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, backend="gloo", **extra_env):
    env = dict(os.environ, CSPM_BENCH_BACKEND=backend, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], check=True, env=env, timeout=900, capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout  # rank 0 prints ONE line and nothing else reaches stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("config,pixels", [("C1", 450 * 375), ("C4", 1242 * 375)])
def test_two_ranks_one_line(config, pixels):
    steps = 2
    one = _bench("--gpus", "1", "--config", config, "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline")
    two = _bench("--gpus", "2", "--config", config, "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline")
    for line, n in ((one, 1), (two, 2)):
        assert line["n_gpus"] == n and line["steps"] == steps and line["warmup"] == 1
        assert line["scaling"] == "weak" and line["higher_is_better"] is True and line["vs_baseline"] is None
        assert config in line["config"]["workload"]
        # whole-job throughput: every rank's pairs over the slowest rank's time
        want = pixels * steps * n / (line["ms_per_step"] * steps / 1e3) / 1e6
        assert abs(line["value"] - want) <= 1e-6 * want
    assert "cpu_baseline" not in two or two["cpu_baseline"] is None  # the CPU leg runs at N = 1 only


def test_rccl_process_group_and_a_clean_stdout():
    """CSPM_BENCH_FORCE_DIST=1: bench.py creates an RCCL process group (backend nccl) even at one GPU, the barrier / MAX reduction run
    as RCCL collectives and C4 goes through run_batch's broadcast / scatter / gather -- the code path of the driver's 8-GPU runs, on
    the one GPU a test box has.  RCCL writes a version banner to file descriptor 1: the result line must still be the ONLY thing
    on stdout."""
    line = _bench("--gpus", "1", "--config", "C4", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", backend="nccl", CSPM_BENCH_FORCE_DIST="1")
    assert line["n_gpus"] == 1 and "batch.run_batch" in line["config"]["dispatch"]
    want = 1242 * 375 * 3 / (line["ms_per_step"] * 3 / 1e3) / 1e6
    assert abs(line["value"] - want) <= 1e-6 * want


def test_eight_ranks_share_the_gpu_one_line():
    """The driver's SCALE run is `bench.py --gpus 8` on an 8-GPU node; this box has one GPU.  Rehearsal: 8 ranks sharing GPU 0, gloo as the
    control plane -- launcher, rank -> device mapping, barrier, MAX reduction of the times, SUM reduction of the fallback counters and the
    stdout discipline run at world size 8 here first: one JSON line, n_gpus 8, pixels = 8 x 3 x 450 x 375."""
    steps = 3
    line = _bench("--gpus", "8", "--config", "C1", "--steps", str(steps), "--warmup", "1", "--in-flight", "1", "--no-cpu-baseline")
    assert line["n_gpus"] == 8 and line["steps"] == steps and line["scaling"] == "weak"
    want = 8 * steps * 450 * 375 / (line["ms_per_step"] * steps / 1e3) / 1e6
    assert abs(line["value"] - want) <= 1e-6 * want
    assert line["sweep_fallbacks"] == 0 and line["volume_fallbacks"] == 0
    assert "real_pair_bad2" not in line  # N = 1 only, like the CPU leg


def test_bench_line_says_what_happened_in_the_timed_region():
    """round-5 review, Weak 9 / 11: the line carries the fallback counters of the timed region and whether the DMA-table volumes were
    active; the overlapping hipEvent brackets are labelled as such; the accuracy on the real Middlebury pair rides along."""
    line = _bench("--gpus", "1", "--config", "C3", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full")
    assert line["sweep_fallbacks"] == 0 and line["volume_fallbacks"] == 0 and line["table_volumes_active"] is True
    assert "kernel_ms_per_step" not in line and "kernel_bracket_ms_per_pair_overlapping" in line  # 3 pairs in flight
    rp = line["real_pair_bad2"]
    assert 0.05 < rp["crop_200x128_D32"]["post_processed"] < 0.25
    if rp["full_741x500_D64"] is not None:
        assert 0.03 < rp["full_741x500_D64"]["post_processed"] < 0.15 and 0.07 < rp["half_370x250_D32"]["raw"] < 0.15
    one = _bench("--gpus", "1", "--config", "C1", "--steps", "2", "--warmup", "1", "--in-flight", "1", "--no-cpu-baseline", "--no-real-pair", "--full")
    assert "kernel_ms_per_step" in one and "real_pair_bad2" not in one
