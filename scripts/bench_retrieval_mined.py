"""K14 in-batch softmax retrieval loss with hard-negative mining: forward + backward of two implementations of the same
loss in one process, device events, warm-up first (development aid):
  mined   retrieval_ops.retrieval_xent(num_hard_negatives=32, path="fused"): krs_retrieval_mine, K11 on the
          [B, 33] logits, K1 / K2 for the gradients; the scores are never stored;
  stored  retrieval_task_loss(num_hard_negatives=32) of examples/two_tower_retrieval.py: the stored-matrix head
          (scores = q c^T, labels = eye, the two correction layers, HardNegativeMining, CategoricalCrossentropy).
bf16, D = 128, B = N in {1024, 8192, 32768}.  One JSON line per shape with the time and the peak memory of each (or why
it did not run), and the time of the mining call alone (`mine_us`: stage 1 and the slice merge); --out FILE also writes
them there."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import retrieval_ops

SHAPES = [(1024, 1024), (8192, 8192), (32768, 32768)]
D = 128
K = 32


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    head = _example().retrieval_task_loss
    lines = []
    for b, n in SHAPES:
        q = (torch.randn((b, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16).requires_grad_(True)
        c = (torch.randn((n, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16).requires_grad_(True)
        ids = torch.randint(0, n, (n,), device=dev, generator=gen, dtype=torch.int32)
        prob = torch.rand(n, device=dev, generator=gen)
        bias = -torch.log(torch.clamp(prob, 1e-6, 1.0))

        def mined():
            q.grad = c.grad = None
            retrieval_ops.retrieval_xent(q, c, cand_bias=bias, cand_ids=ids, path="fused", num_hard_negatives=K,
                                         reduction="sum_over_batch_size").backward()

        def stored():
            q.grad = c.grad = None
            head(q, c, cand_ids=ids, cand_prob=prob, num_hard_negatives=K).backward()

        def mine():
            retrieval_ops.retrieval_mine(q.detach(), c.detach(), K, None, bias, ids, retrieval_ops.SMALLEST_FLOAT)

        rec = {"B": b, "N": n, "D": D, "k": K, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
               "score_matrix_fp32_bytes": b * n * 4,
               "mine_workspace_bytes": retrieval_ops.retrieval_mine_workspace_bytes(b, n, D, K)}
        rec["mined_us"], rec["mined_peak_bytes"] = measure(mined, args.steps, args.warmup)
        rec["mine_us"], _ = measure(mine, args.steps, args.warmup)
        rec["stored_us"], rec["stored_peak_bytes"] = measure(stored, args.steps, args.warmup)
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
