"""BASELINE.json configs[4] (C5) AS STATED, as a parity case: the 26 Criteo-1TB tables at their full vocabularies (largest
40,000,000 rows; 204 M rows, 157 GB of bf16 tables + fp32 Adagrad accumulators in all) MOD row-sharded over EIGHT ranks,
power-law ids, ml_perf bag lengths, global batch 65,536 (8,192 per rank), tables under 2,048 rows replicated as the
reference's model does below its embedding_threshold (examples/ml_perf/main.py:135-141, configs/v6e_8.py:15-179).

The eight ranks run one per GPU and the collectives go over gloo, staged through the host (a functional rig -- every
kernel, every routing decision and every exchange block is the 8-way one; only the links are not xGMI).  With fewer than
eight GPUs the test skips: eight ranks on one GPU are more processes than a shared GPU takes at once.  The
run is bench.py's own N = 8 path, whose `parity` object checks one forward + one fused Adagrad update of the timed layer on
a slice against an unsharded recompute: pooled outputs bit for bit against per-owner fp32 pooling, updated rows within one
bf16 ulp of acc += g^2; w -= lr g / sqrt(acc) with g = the row's GLOBAL lookup count over all eight batches times the
step's gradient, no lookup dropped by the static exchange."""

import json
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout=900):
    detail = os.path.join(tempfile.mkdtemp(prefix="krs_c5_"), "bench_detail.json")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--dist-backend", "gloo", "--criteo-vocab", "40000000",
           "--id-skew", "4", "--steps", "1", "--warmup", "1", "--sustained-steps", "0", "--probe-steps", "0", "--no-cpu-baseline",
           "--detail", detail] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096
    line = json.loads(last)
    with open(detail) as f:
        return line, json.load(f), r.stderr


def test_c5_criteo_vocabularies_sharded_eight_ways_parity():
    import gc

    import torch

    # one GPU per rank: eight ranks (plus this process and the launcher) are more processes than one shared GPU takes at once
    if torch.cuda.device_count() < 8:
        pytest.skip(f"needs 8 GPUs (one rank per GPU), found {torch.cuda.device_count()}")
    # the eight ranks are processes of their own and need ~160 GB between them: hand back what this process's caching
    # allocator still holds from earlier tests of the session
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(0)
    if total < 200 * 2 ** 30:
        pytest.skip("C5 needs ~160 GB of HBM for the tables and their accumulators")
    assert free > 170 * 2 ** 30, f"only {free >> 30} GiB of HBM are free: an earlier test of this session still holds device memory"
    line, full, _ = _run(["--replicate-below", "2048"])
    assert line["n_gpus"] == 8 and full["ranks"] == 8 and "Criteo-1TB scale" in full["config"]["workload"]
    assert "204184588 rows" in full["config"]["workload"] and "power-law" in full["config"]["workload"]
    assert "MOD row-sharded over 8 GPUs" in full["config"]["parallelism"]
    par = full["parity"]
    assert par["checked"] and par["ok"], par
    assert par["fwd_max_ulp"] == 0.0 and par["fwd_bit_equal_fraction"] == 1.0          # bit for bit vs the per-owner recompute
    assert par["update_max_ulp"] <= 1.001 and par["accumulator_max_rel_err"] <= 1e-6 and par["rows_moved"]
    assert par["max_lookups_of_a_checked_row"] > 1000        # power-law ids: hot rows, contributions from all eight batches
    assert par["checked_rows"] >= 64 * 150
    assert full["overflow_steps"] == 0 and "invalid" not in full and "invalid" not in line
    assert line["parity"]["ok"] is True and line["overflow_steps"] == 0
    ex = full["exchange"]
    assert ex["mode"] == "static" and ex["need"][0] <= ex["capacity"][0] and ex["need"][1] <= ex["capacity"][1]
    assert ex["bytes_at_need"] <= ex["bytes_at_capacity"]
