"""K13 in-batch softmax retrieval loss: forward + backward of three implementations of the same loss in one process,
device events, warm-up first (development aid):
  fused   retrieval_ops.retrieval_xent(path="fused"): the K13 kernels, scores never stored;
  slab    retrieval_ops.retrieval_xent(path="slab"): krs_gemm + K11 on slabs of query rows, in fp32;
  stored  retrieval_task_loss of examples/two_tower_retrieval.py without hard-negative mining: the stored-matrix head
          (scores = q c^T, labels = eye, the two correction layers, CategoricalCrossentropy).
bf16, D = 128, B = N in {1024, 8192, 32768, 65536} and B = 256 against N = 2^20.  One JSON line per shape with the
time and the peak memory of each (or why it did not run); --out FILE also writes them there.

The fused path is reported against 10 B N D flops -- five products of 2 B N D each: the forward's scores, the scores
recomputed by each of the backward's two sweeps, and the two gradient products -- over the 2.5 PF/s bf16 matrix peak,
as `fused_tflops` and `fused_of_peak`."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import retrieval_ops

SHAPES = [(1024, 1024), (8192, 8192), (32768, 32768), (65536, 65536), (256, 2**20)]
D = 128
PEAK_FLOPS = 2.5e15


def _example():
    spec = importlib.util.spec_from_file_location("two_tower_retrieval",
                                                  os.path.join(ROOT, "examples", "two_tower_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(fn, steps, warm):
    """(microseconds per call, peak bytes above what was allocated before), or (None, reason) when it cannot run."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    try:
        us = timed(fn, steps, warm)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None, "cannot allocate"
    return round(us, 1), torch.cuda.max_memory_allocated() - m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", default="fused,slab,stored")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    head = _example().retrieval_task_loss
    paths = args.paths.split(",")
    lines = []
    for b, n in SHAPES:
        q = (torch.randn((b, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16).requires_grad_(True)
        c = (torch.randn((n, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16).requires_grad_(True)
        ids = torch.randint(0, n, (n,), device=dev, generator=gen, dtype=torch.int32)
        prob = torch.rand(n, device=dev, generator=gen)
        bias = -torch.log(torch.clamp(prob, 1e-6, 1.0))

        def op(path):
            def run():
                q.grad = c.grad = None
                retrieval_ops.retrieval_xent(q, c, cand_bias=bias, cand_ids=ids, path=path,
                                             reduction="sum_over_batch_size").backward()
            return run

        def stored():
            q.grad = c.grad = None
            head(q, c, cand_ids=ids, cand_prob=prob, num_hard_negatives=None).backward()

        rec = {"B": b, "N": n, "D": D, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
               "score_matrix_fp32_bytes": b * n * 4}
        for name, fn in (("fused", op("fused")), ("slab", op("slab")), ("stored", stored)):
            if name in paths:
                rec[f"{name}_us"], rec[f"{name}_peak_bytes"] = measure(fn, args.steps, args.warmup)
        if rec.get("fused_us"):
            flops = 10.0 * b * n * D
            rec["fused_tflops"] = round(flops / rec["fused_us"] / 1e6, 1)
            rec["fused_of_peak"] = round(flops / (rec["fused_us"] * 1e-6) / PEAK_FLOPS, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, c, ids, prob, bias
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
