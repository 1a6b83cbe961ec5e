"""K11 retrieval loss: forward + backward of layers.CategoricalCrossentropy and of the whole retrieval_task_loss head
(examples/two_tower_retrieval.py) on the HIP path against the eager-torch composition of the same expressions
(log_softmax, multiply, sum; clip / log / subtract; argmax / take / equal; top-k / gather), at the three shapes of
DESIGN.md section 4 (K11) in fp32 and bf16, in one process, device events, warm-up first (development aid).
One JSON line per (shape, dtype, workload) with the peak memory of both; --out FILE also writes them there.

Bound of the loss: the algorithmic bytes rows * cols * (s_logit + 4 + s_grad) (logits and fp32 labels read once, the
gradient written once) over 8 TB/s, reported as `bound_us` and the achieved fraction `of_bound`."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import keras_rs_amd.layers as kl
from keras_rs_amd.retrieval_ops import MAX_FLOAT, SMALLEST_FLOAT

SHAPES = [("S1", 1024, 1024), ("S2", 8192, 8192), ("S3", 256, 65536)]
HBM_BYTES_PER_S = 8e12
D = 64              # embedding width of the head
HARD_NEGATIVES = 64


def _example():
    spec = importlib.util.spec_from_file_location("two_tower_retrieval",
                                                  os.path.join(ROOT, "examples", "two_tower_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def eager_loss(labels, scores):
    """keras.losses.CategoricalCrossentropy(from_logits=True) in eager torch: -sum(labels * log_softmax), mean."""
    return -(labels * torch.log_softmax(scores.float(), -1)).sum(-1).mean()


def eager_head(q, c, ids, prob, num_hard_negatives):
    """The head's stages as the reference writes them, in eager torch."""
    scores = q @ c.T
    labels = torch.eye(scores.shape[0], scores.shape[1], device=scores.device)
    scores = scores - torch.log(torch.clamp(prob, 1e-6, 1.0)).to(scores.dtype)
    pos = labels.argmax(-1, keepdim=True)
    dup = (ids[None, :] == ids[pos]).to(labels.dtype) - labels
    scores = scores + (dup * SMALLEST_FLOAT).to(scores.dtype)
    idx = torch.topk(scores.detach().float() + labels * MAX_FLOAT, num_hard_negatives + 1, dim=-1, sorted=False).indices
    return eager_loss(torch.gather(labels, -1, idx), torch.gather(scores, -1, idx))


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
    """(microseconds per call, peak bytes above what was allocated before)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    us = timed(fn, steps, warm)
    return us, torch.cuda.max_memory_allocated() - m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2,S3")
    ap.add_argument("--no-baseline", action="store_true", help="time the HIP path only (profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    head = _example().retrieval_task_loss
    loss = kl.CategoricalCrossentropy(from_logits=True)
    lines = []
    for name, b, n in SHAPES:
        if name not in args.shapes.split(","):
            continue
        for dtype in (torch.float32, torch.bfloat16):
            es = 4 if dtype == torch.float32 else 2
            labels = torch.eye(b, n, device=dev)
            x = torch.randn((b, n), device=dev, generator=gen).to(dtype).requires_grad_(True)
            q = torch.randn((b, D), device=dev, generator=gen).to(dtype).requires_grad_(True)
            c = torch.randn((n, D), device=dev, generator=gen).to(dtype).requires_grad_(True)
            ids = torch.randint(0, n, (n,), device=dev, generator=gen, dtype=torch.int32)
            prob = torch.rand(n, device=dev, generator=gen)

            def hip_loss():
                x.grad = None
                loss(labels, x).backward()

            def base_loss():
                x.grad = None
                eager_loss(labels, x).backward()

            def hip_head():
                q.grad = c.grad = None
                head(q, c, cand_ids=ids, cand_prob=prob, num_hard_negatives=HARD_NEGATIVES).backward()

            def base_head():
                q.grad = c.grad = None
                eager_head(q, c, ids.long(), prob, HARD_NEGATIVES).backward()

            bound_us = b * n * (es + 4 + es) / HBM_BYTES_PER_S * 1e6
            for what, hip, base in (("loss", hip_loss, base_loss), ("head", hip_head, base_head)):
                us, peak = measure(hip, args.steps, args.warmup)
                us_b, peak_b = float("nan"), None
                if not args.no_baseline:
                    try:
                        us_b, peak_b = measure(base, max(1, args.steps // 2), 2)
                    except torch.OutOfMemoryError:
                        us_b, peak_b = float("nan"), "OOM"
                rec = {"shape": name, "what": what, "dtype": str(dtype).replace("torch.", ""), "B": b, "N": n,
                       "hip_us": round(us, 1), "eager_us": round(us_b, 1), "speedup": round(us_b / us, 2),
                       "hip_peak_bytes": peak, "eager_peak_bytes": peak_b, "device": torch.cuda.get_device_name(0)}
                if what == "loss":
                    rec.update({"bound_us": round(bound_us, 1), "of_bound": round(bound_us / us, 3)})
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del labels, x, q, c, ids, prob
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
