"""bench.py's N > 1 path end to end on the test box's one GPU: two ranks launched as the driver launches them
(torch.distributed.run), sharing cuda:0, collectives over gloo staged through the host (--dist-backend gloo is the
debugging switch for exactly this; production uses nccl = RCCL).  Checks that the run completes and that rank 0
prints the contract's JSON line for the sharded + data-parallel configuration."""

import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _detail_path():
    import tempfile

    return os.path.join(tempfile.mkdtemp(prefix="krs_bench_"), "bench_detail.json")


def test_two_rank_bench_run_over_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
           "--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--batch", "4096", "--vocab", "50000", "--sustained-steps", "4", "--detail", _detail_path()]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["unit"] == "lookups/s" and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert "row-sharded over 2 GPUs" in d["config"]["parallelism"] and d["config"]["global_batch"] == 4096
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1.5
    # the N > 1 line checks ITSELF (round-4 review, next #1a): one step against an unsharded recompute of a slice, rows read
    # back from their owners over the job's own collectives -- two ranks, real kernels on both
    par = d["parity"]
    assert par["checked"] and par["ok"] and "invalid" not in d, par
    assert par["fwd_max_ulp"] == 0.0 and par["update_max_ulp"] <= 1.001 and par["rows_moved"] and par["checked_rows"] > 1000
    assert d["sustained"]["steps"] == 4 and d["sustained"]["median_ms"] > 0


def test_the_self_check_of_the_sharded_line_has_teeth():
    """One table row moved behind the layer's back (KRS_BENCH_PARITY_SABOTAGE) before the checked step: `parity.ok` is false
    and the line is marked invalid."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["KRS_BENCH_PARITY_SABOTAGE"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-sharded", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--batch", "2048", "--vocab", "20000", "--sustained-steps", "0", "--probe-steps", "0", "--detail", _detail_path()]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["parity"]["checked"] and not d["parity"]["ok"] and d["parity"]["fwd_max_ulp"] > 1.0
    assert "self-check" in d["invalid"]


def _json_line(stdout):
    """The LAST stdout line (the driver's: below 4 KB, contract keys present) merged over the side file it names, which holds
    the deep members (`phases`, `graph_leg`, `exchange`, per-step times)."""
    last = stdout.strip().splitlines()[-1]
    assert last.startswith("{") and len(last) < 4096, len(last)
    line = json.loads(last)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "detail"):
        assert key in line, key
    with open(line["detail"]) as f:
        full = json.load(f)
    for key in ("value", "ms_per_step", "n_gpus"):
        assert abs(full[key] - line[key]) <= 1e-5 * abs(full[key]), key
    if "parity" in full:
        assert line["parity"]["ok"] == full["parity"]["ok"]
    if "invalid" in full:
        assert "invalid" in line
    return dict(line, **full)


def test_bare_bench_command_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it (RANK unset) starts its two ranks itself; with more ranks
    than GPUs and the default backend it falls back to gloo and says so in the line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--batch", "4096", "--vocab", "50000", "--sustained-steps", "0", "--detail", _detail_path()]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["value"] > 0
    import torch

    if torch.cuda.device_count() < 2:
        assert "gloo" in d["backend"] and "NOT a measurement" in d["backend"]
    else:
        assert "RCCL" in d["backend"]
    assert d["a2a_bytes_per_step"] > 0 and d["exchange"]["mode"] == "static"
    assert d["step_stats"]["median_ms"] > 0 and "roofline_step" in d
    # the N > 1 line attributes its time (round-3 review, item 5): per-phase event times with min / max over the ranks,
    # bytes per link and the achieved rate of every all-to-all, the wait for the dense all-reduce, dropped lookups
    ph = d["phases"]
    for name in ("route", "a2a_ids", "unpack", "pool", "a2a_partials", "combine", "gather_grads", "a2a_grads", "k2",
                 "allreduce_wait", "dense_and_rest"):
        assert name in ph and ph[name]["ms_per_step"] >= 0 or name == "dense_and_rest", name
    for name in ("a2a_ids", "a2a_partials", "a2a_grads"):
        e = ph[name]
        assert e["min_ms"] <= e["max_ms"] and e["bytes_off_rank_per_step"] > 0 and e["bytes_per_link_per_step"] > 0
        assert e["GB_per_s_per_rank"] > 0
    assert d["overflow_steps"] == 0 and "invalid" not in d


def test_sharded_step_through_a_one_rank_rccl_communicator():
    """--force-sharded --rccl-self: the sharded layer's collectives (all_to_all_single of the packed blocks, of the
    partials and of the gradients) run through RCCL itself on a one-rank communicator -- the call path the multi-GPU
    run takes, on the one GPU of the test box."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    for exchange in ("static", "exact"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-sharded", "--rccl-self", "--exchange", exchange,
               "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--batch", "8192", "--vocab", "100000",
               "--sustained-steps", "0", "--detail", _detail_path()]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _json_line(r.stdout)
        assert d["backend"] == "nccl (RCCL)" and d["exchange"]["mode"] == exchange and d["a2a_bytes_per_step"] > 0
        assert "one-rank RCCL communicator" in d["config"]["parallelism"]
        # the self-check ran over the RCCL communicator too, and -- static exchange -- the step was captured into a HIP graph
        # WITH its collectives and replayed behind the eager legs; the faster leg is `value`, both are in the line
        assert d["parity"]["ok"] and d["parity"]["fwd_max_ulp"] == 0.0
        if exchange == "static":
            gl = d["graph_leg"]
            assert gl["attempted"] and gl["ok"], gl
            assert gl["ms_per_step"] > 0 and gl["host_enqueue_ms_per_step"] < gl["ms_per_step"]
            assert ("eager_leg" in d) == bool(gl.get("promoted_to_value"))
        else:
            assert "graph_leg" not in d


def test_virtual_world_runs_rank_zero_of_an_n_way_job_with_n_way_shapes():
    """`--force-sharded --virtual-world N` (round 5): one process, rank 0's 1/N shard and batch / N samples, ids routed to N
    owners, N blocks per exchange, loopback copies for the links -- the per-rank KERNEL time of an N-way job, a projection
    that the line labels as such (no parity: the other ranks' shards do not exist)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--force-sharded", "--virtual-world", "4", "--steps", "3",
           "--warmup", "2",
           "--no-cpu-baseline", "--batch", "8192", "--vocab", "100000", "--sustained-steps", "0", "--detail", _detail_path()]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["virtual_world"] == 4 and "4-way job on ONE GPU" in d["config"]["parallelism"] and "projection" in d["config"]["parallelism"]
    assert d["parity"] == {"checked": False, "ok": True, "reason": d["parity"]["reason"]} and "graph_leg" not in d
    ex = d["exchange"]
    # batch / 4 samples per rank, every bag split over up to 4 owners: more segments than bags, four blocks per exchange
    bags = (8192 // 4) * 26
    assert ex["mode"] == "static" and ex["received"][1] > bags and ex["need"][0] <= ex["capacity"][0]
    assert d["overflow_steps"] == 0 and "invalid" not in d and d["phases"]["combine"]["ms_per_step"] > 0
    import torch

    from keras_rs_amd import _lib as L
    import keras_rs_amd.layers as kl
    from keras_rs_amd.sharded import ShardedDistributedEmbedding

    tc = kl.TableConfig("t", 1000, 16, optimizer=kl.Adagrad(0.1, 0.1), combiner="sum", placement="sparsecore")
    layer = ShardedDistributedEmbedding({"f": kl.FeatureConfig("f", tc, (64, 3), (64, 16))}, virtual_world=4, exchange="static")
    out = layer({"f": torch.randint(0, 1000, (64, 3), device="cuda:0", dtype=torch.int32)})["f"]
    assert out.shape == (64, 16) and layer.shard.shape[0] == 250 and layer.world == 4 and layer.virtual
    with pytest.raises(L.KrsError):
        layer.get_embedding_tables()
