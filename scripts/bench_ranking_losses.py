"""K9 ranking losses: forward + backward of each loss on the HIP path against an eager-torch restatement that
materialises the (batch, list, list) pair tensors as the reference does (pairwise_loss_utils.py:pairwise_comparison),
at the four shapes of DESIGN.md section 4 (K9), in one process, device events, warm-up first (development aid).
One JSON line per (shape, loss) with the baseline's peak memory; --out FILE also writes them there.

Bound: S1 is launch-bound (one kernel launch, a few microseconds); the larger shapes are bound by VALU issue: the
ordered pairs are counted, B * L^2 per call, and reported as pairs/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from keras_rs_amd import losses

SHAPES = [("S1", 1024, 5), ("S2", 65536, 32), ("S3", 4096, 256), ("S4", 256, 2048)]
LOSSES = {"hinge": losses.PairwiseHingeLoss, "logistic": losses.PairwiseLogisticLoss,
          "soft_zero_one": losses.PairwiseSoftZeroOneLoss, "mse": losses.PairwiseMeanSquaredError,
          "listmle": losses.ListMLELoss}


def eager(kind, s, y):
    """The reference's arithmetic in eager torch (fp32, pair tensors materialised), mean over the batch."""
    valid = y >= 0
    vp = valid[:, :, None] & valid[:, None, :]
    if kind == "listmle":
        order = torch.sort(torch.where(valid, y, torch.full_like(y, -1e9)), dim=1, descending=True, stable=True).indices
        sl = torch.gather(s, 1, order)
        mx = sl.amax(1, keepdim=True)
        sl = sl - mx
        cs = torch.flip(torch.cumsum(torch.flip(torch.exp(sl), [1]), 1), [1])
        return -(sl - torch.log(cs + 1e-10)).sum(1).mean()
    if kind == "mse":
        d = (y[:, :, None] - y[:, None, :]) - (s[:, :, None] - s[:, None, :])
        eye = torch.eye(s.shape[1], device=s.device)
        return (torch.square(d) * ((1.0 - eye) * vp)).sum(-1).mean()
    x = s[:, :, None] - s[:, None, :]
    w = (y[:, :, None] - y[:, None, :] > 0).float() * vp
    if kind == "hinge":
        phi = torch.relu(1.0 - x)
    elif kind == "logistic":
        phi = torch.relu(-x) + torch.log(1.0 + torch.exp(-torch.abs(x)))
    else:
        phi = torch.where(x > 0, 1.0 - torch.sigmoid(x), torch.sigmoid(-x))
    return (phi * w).sum(-1).mean()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2,S3,S4")
    ap.add_argument("--losses", default=",".join(LOSSES))
    ap.add_argument("--no-baseline", action="store_true", help="time the HIP path only (profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, b, n in SHAPES:
        if name not in args.shapes.split(","):
            continue
        s = torch.randn((b, n), device=dev, generator=gen)
        y = torch.randint(0, 5, (b, n), device=dev, generator=gen).float()
        for kind in args.losses.split(","):
            loss = LOSSES[kind]()
            x = s.clone().requires_grad_(True)

            def hip():
                x.grad = None
                loss(y, x).backward()

            us = timed(hip, args.steps, args.warmup)
            us_b, peak = float("nan"), None
            if not args.no_baseline:
                def base():
                    x.grad = None
                    eager(kind, x, y).backward()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                m0 = torch.cuda.memory_allocated()
                try:
                    us_b = timed(base, max(1, args.steps // 4), 1)
                    peak = torch.cuda.max_memory_allocated() - m0
                except torch.OutOfMemoryError:
                    us_b, peak = float("nan"), "OOM"
                torch.cuda.empty_cache()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            hip()
            torch.cuda.synchronize()
            peak_hip = torch.cuda.max_memory_allocated() - m0
            pairs = float(b) * n * n
            rec = {"shape": name, "loss": kind, "B": b, "L": n, "hip_us": round(us, 1), "eager_us": round(us_b, 1),
                   "speedup": round(us_b / us, 2), "pairs_per_s": f"{pairs / (us * 1e-6):.3e}",
                   "eager_peak_bytes": peak, "hip_peak_bytes": peak_hip, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del s, y
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
