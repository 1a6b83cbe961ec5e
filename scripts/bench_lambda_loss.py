"""K28 LambdaRank pair weights: loss + gradient of PairwiseLogisticLoss(lambda_weights=NDCGLambdaWeight(topn)) in one
process, bench_gru.py's method (device events, every shape warmed up first, the implementations alternating over
several repeats, every timed window at least --window seconds long) (development aid):
  lambda   the K28 kernel (krs_pairwise_lambda_loss);
  plain    the same loss without lambda weights, K9's krs_pairwise_loss, at the same shape;
  torch    an eager torch composition: argsort for the ranks, then the [B, L, L] weight and loss tensors, autograd.
bf16 and fp32 at (B, L) = (8192, 32), (1024, 256), (256, 2048), (64, 4096), topn none and 10.  One JSON line per (shape,
dtype, topn) with the median and the fastest repeat's time per call, the calls per window and the peak memory of each
implementation; --out FILE also writes them there."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import losses
from scripts.bench_gru import peak_of, timed

SHAPES = [(8192, 32), (1024, 256), (256, 2048), (64, 4096)]


def torch_lambda(s, y, topn):
    """NDCGLambdaWeight(topn) on the logistic loss in eager torch, mean over the items (every label is valid)."""
    b, n = s.shape
    topn = topn or n
    r1 = torch.arange(1, n + 1, device=s.device, dtype=torch.float32)
    disc = torch.where(r1 <= topn, 1.0 / torch.log2(1.0 + r1), torch.zeros_like(r1))
    order = torch.sort(s.detach().float(), dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(n, device=s.device).expand(b, n))
    gain = torch.pow(2.0, y) - 1.0
    ideal = (torch.sort(gain, dim=1, descending=True).values * disc).sum(1, keepdim=True)
    gain = torch.where(ideal > 0, gain / ideal, torch.zeros_like(gain))
    d = disc[rank]
    lam = (gain[:, :, None] - gain[:, None, :]).abs() * (d[:, :, None] - d[:, None, :]).abs()
    w = lam * (y[:, :, None] > y[:, None, :])
    x = s.float()[:, :, None] - s.float()[:, None, :]
    phi = torch.relu(-x) + torch.log(1.0 + torch.exp(-torch.abs(x)))
    return (phi * w).sum(-1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="fewest calls in a timed window")
    ap.add_argument("--window", type=float, default=0.5, help="fewest seconds in a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the two HIP paths only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for b, n in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            s = torch.randn((b, n), device=dev, generator=gen).to(dtype)
            y = torch.randint(0, 5, (b, n), device=dev, generator=gen).float()
            x = s.clone().requires_grad_(True)
            for topn in (None, 10):
                weighted = losses.PairwiseLogisticLoss(lambda_weights=losses.NDCGLambdaWeight(topn=topn))
                plain = losses.PairwiseLogisticLoss()

                def run(loss_fn):
                    x.grad = None
                    loss_fn().backward()

                live = {"lambda": lambda: run(lambda: weighted(y, x)), "plain": lambda: run(lambda: plain(y, x))}
                if not args.no_torch:
                    live["torch"] = lambda: run(lambda: torch_lambda(x, y, topn))
                for fn in live.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                rec = {"B": b, "L": n, "dtype": str(dtype).replace("torch.", ""), "topn": topn, "loss": "logistic",
                       "device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats}
                times = {name: [] for name in live}
                calls = {name: max(args.steps, math.ceil(args.window * 1e6 / timed(fn, 3))) for name, fn in live.items()}
                for _ in range(args.repeats):                             # the implementations alternate
                    for name, fn in live.items():
                        times[name].append(timed(fn, calls[name]))
                for name, fn in live.items():
                    rec[f"{name}_us"] = round(statistics.median(times[name]), 1)
                    rec[f"{name}_min_us"] = round(min(times[name]), 1)
                    rec[f"{name}_calls"] = calls[name]
                    rec[f"{name}_peak_bytes"] = peak_of(fn)
                rec["lambda_over_plain"] = round(rec["lambda_us"] / rec["plain_us"], 3)
                if "torch" in live:
                    rec["torch_over_lambda"] = round(rec["torch_us"] / rec["lambda_us"], 2)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del s, y, x
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
