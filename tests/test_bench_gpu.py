"""bench.py on one GPU at a small shape: a plain run sets up, warms up, times its steps, writes --dump-outputs and prints the
line, and runs none of the legs that --full adds; a --full run adds them BEHIND the timed steps, so the two runs time the same
steps and dump the same bits."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_step", "roofline_dominant", "roofline_dominant_kernel", "embed_fwd_lookups_per_s", "also",
             "also_c2", "sustained", "cpu_baseline")


def _run(tmp, name, extra):
    detail = os.path.join(tmp, name + "_detail.json")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4096",
           "--vocab", "50000", "--detail", detail, "--dump-outputs", os.path.join(tmp, name)] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("{") and len(last) < 4096
    with open(detail) as f:
        return json.loads(last), json.load(f)


def test_plain_run_times_only_its_steps_and_full_adds_its_legs_behind_them(tmp_path):
    tmp = str(tmp_path)
    line, rec = _run(tmp, "plain", [])
    assert line["metric"].startswith("embedding lookups/sec") and line["unit"] == "lookups/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(4096 * 214 / (line["ms_per_step"] * 1e-3), rel=1e-4)
    assert rec["step_stats"]["median_ms"] > 0 and len(rec["step_stats"]["each_ms"]) == 3
    for key in FULL_ONLY:
        assert key not in rec and key not in line, key
    assert set(rec["wall_seconds"]) == {"setup_build_model", "primary_leg", "total_since_import"}

    # (C2 and the host-CPU leg left out to keep the test short: they run in the benchmark's own --full run)
    line_f, rec_f = _run(tmp, "full", ["--full", "--no-c2", "--no-cpu-baseline", "--sustained-steps", "20"])
    assert line_f["roofline"]["bound"] == "hbm" and line_f["roofline"]["frac"] > 0 and rec_f["roofline_step"]
    assert rec_f["also"]["value"] > 0 and "L = 1" in rec_f["also"]["workload"] and rec_f["sustained"]["steps"] == 20
    assert "secondary_leg" in rec_f["wall_seconds"]
    names = sorted(os.listdir(os.path.join(tmp, "plain")))
    assert "xl.npy" in names and "inter.npy" in names and "table_cat_0.npy" in names
    assert names == sorted(os.listdir(os.path.join(tmp, "full")))
    for n in names:
        np.testing.assert_array_equal(np.load(os.path.join(tmp, "plain", n)), np.load(os.path.join(tmp, "full", n)), err_msg=n)
