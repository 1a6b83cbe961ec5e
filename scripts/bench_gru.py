"""K20 GRU layer: forward + backward of three implementations in one process, device events, every shape warmed up
first, the implementations alternating over several repeats, every timed window at least --window seconds long (the
number of calls in a window is set per shape and implementation from a short trial) (development aid):
  krs      layers.GRU: the input projection on krs_gemm, the recurrence on the K20 kernels (one launch per sweep), the
           weight gradients on krs_gemm / krs_colsum;
  torch    torch.nn.GRU on the same device (MIOpen's fused RNN), whatever it supports for the dtype;
  steps    a per-step torch composition (one matmul and a handful of element-wise ops per time step), the only
           comparison left where torch's own call is unavailable for a dtype.
bf16 and fp32 at B = 4096, L = 10, U = D = 32 (examples/sequential_retrieval.py); B = 4096, L = 50, U = D = 128; and
B = 512, L = 200, U = D = 128.  No mask, no initial state, gradients arriving at the last output, as the example trains.
One JSON line per (shape, dtype) with the median and the fastest repeat's time per call, the calls per window and the
peak memory of each implementation (or why it did not run); --out FILE also writes them there."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import recurrent_ops

SHAPES = [(4096, 10, 32), (4096, 50, 128), (512, 200, 128)]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def peak_of(fn):
    """Peak bytes of one call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="fewest calls in a timed window")
    ap.add_argument("--window", type=float, default=0.5, help="fewest seconds in a timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", default="krs,torch,steps")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    paths = args.paths.split(",")
    lines = []
    for b, l, u in SHAPES:
        for dtype, policy in ((torch.bfloat16, "mixed_bfloat16"), (torch.float32, "float32")):
            d = u
            x = torch.randn((b, l, d), device=dev, generator=gen).to(dtype).requires_grad_(True)
            dout = torch.randn((b, u), device=dev, generator=gen).to(dtype)
            layer = kl.GRU(u, dtype=policy, device=dev)
            layer(x)
            ref = torch.nn.GRU(d, u, batch_first=True, device=dev, dtype=dtype)
            wi, wh = (torch.randn((n, 3 * u), device=dev, generator=gen).to(dtype).mul_(u ** -0.5).requires_grad_(True)
                      for n in (d, u))
            bi, bh = (torch.zeros(3 * u, device=dev, dtype=dtype, requires_grad=True) for _ in range(2))

            def krs():
                x.grad = None
                layer.zero_grad(set_to_none=True)
                layer(x).backward(dout)

            def torch_gru():
                x.grad = None
                ref.zero_grad(set_to_none=True)
                ref(x)[1][0].backward(dout)

            def steps():
                x.grad = wi.grad = wh.grad = bi.grad = bh.grad = None
                xz = (x.reshape(b * l, d) @ wi + bi).view(b, l, 3 * u)
                h = torch.zeros((b, u), device=dev, dtype=dtype)
                for t in range(l):
                    a = h @ wh + bh
                    z = torch.sigmoid(xz[:, t, :u] + a[:, :u])
                    r = torch.sigmoid(xz[:, t, u:2 * u] + a[:, u:2 * u])
                    c = torch.tanh(xz[:, t, 2 * u:] + r * a[:, 2 * u:])
                    h = z * h + (1 - z) * c
                h.backward(dout)

            rec = {"B": b, "L": l, "U": u, "D": d, "dtype": str(dtype).replace("torch.", ""),
                   "device": torch.cuda.get_device_name(0), "route": None, "window_s": args.window, "repeats": args.repeats}
            live = {}
            for name, fn in (("krs", krs), ("torch", torch_gru), ("steps", steps)):
                if name not in paths:
                    continue
                try:
                    for _ in range(args.warmup):
                        fn()
                    torch.cuda.synchronize()
                    live[name] = fn
                except (RuntimeError, NotImplementedError) as e:      # (a dtype torch's own call does not take)
                    rec[f"{name}_us"], rec[f"{name}_why"] = None, str(e).splitlines()[0][:160]
                if name == "krs":
                    rec["route"] = list(recurrent_ops.last_route())
            times = {name: [] for name in live}
            calls = {name: max(args.steps, math.ceil(args.window * 1e6 / timed(fn, 5))) for name, fn in live.items()}
            for _ in range(args.repeats):                             # the implementations alternate
                for name, fn in live.items():
                    times[name].append(timed(fn, calls[name]))
            for name, fn in live.items():
                rec[f"{name}_us"] = round(statistics.median(times[name]), 1)
                rec[f"{name}_min_us"] = round(min(times[name]), 1)
                rec[f"{name}_calls"] = calls[name]
                rec[f"{name}_peak_bytes"] = peak_of(fn)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x, dout, layer, ref, wi, wh, bi, bh
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
