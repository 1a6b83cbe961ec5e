"""K24 regression head: forward + backward + a RootMeanSquaredError update of two implementations in one process,
device events, every point warmed up first, the implementations alternating over --repeats repeats, every timed window
at least --window seconds long (development aid):
  krs      layers.MeanSquaredError(metrics=RootMeanSquaredError()) and autograd.grad: one krs_regression_fwd_bwd call
           (one or two launches), the backward's scaling of the stored gradient and the metric's 2-element add;
  torch    the composition a user writes without K24: ((p - y) ** 2).mean(), its autograd backward, and two torch
           reductions added into a {total, count} state.
Points: [B, 1] for B in {4096, 65536, 2^22} and [65536, 5], bf16 and fp32 predictions, fp32 targets.
One JSON line per point with the median and the fastest repeat's time per call of each side, the bytes the algorithm
has to move (pred and target read once, dpred written once) and, for krs, those bytes over the median as a share of
8 TB/s; --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import layers as kl

POINTS = [(4096, 1), (65536, 1), (1 << 22, 1), (65536, 5)]
PEAK_TBS = 8.0


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def pair(b, c, dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(b + c)
    y = (torch.randint(1, 11, (b, c), generator=g) * 0.5).to(dev)
    p = (y.cpu() + torch.randn(b, c, generator=g)).to(dtype).to(dev).requires_grad_(True)
    rmse = kl.RootMeanSquaredError()
    loss_fn = kl.MeanSquaredError(metrics=rmse)
    state = torch.zeros(2, device=dev)

    def krs():
        return torch.autograd.grad(loss_fn(y, p), p)

    def ref():
        e = p.float() - y
        (grad,) = torch.autograd.grad((e ** 2).mean(), p)
        with torch.no_grad():
            d = p.detach().float() - y
            state[0] += (d * d).sum()
            state[1] += d.numel()
        return grad

    return krs, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []
    for b, c in POINTS:
        for dtype in (torch.bfloat16, torch.float32):
            krs, ref = pair(b, c, dtype, dev)
            fns = {"krs": krs, "torch": ref}
            esize = 2 if dtype == torch.bfloat16 else 4
            rec = dict(b=b, c=c, dtype=str(dtype).split(".")[-1], needed_bytes=b * c * (2 * esize + 4))
            calls = {}
            for name, fn in fns.items():
                for _ in range(args.warmup):
                    fn()
                trial = timed(fn, 3)
                calls[name] = max(args.steps, int(args.window * 1e6 / max(trial, 1.0)) + 1)
            times = {name: [] for name in fns}
            for _ in range(args.repeats):
                for name, fn in fns.items():
                    times[name].append(timed(fn, calls[name]))
            for name in fns:
                rec[name] = dict(median_us=round(statistics.median(times[name]), 1), best_us=round(min(times[name]), 1),
                                 calls=calls[name])
            rec["speedup"] = round(rec["torch"]["median_us"] / rec["krs"]["median_us"], 3)
            rec["krs"]["wall_share_of_8tbs"] = round(rec["needed_bytes"] / (rec["krs"]["median_us"] * 1e-6) /
                                                     (PEAK_TBS * 1e12), 4)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del fns, krs, ref
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
