"""K25 LSTM layer: forward + backward of two implementations in one process, bench_gru.py's method: device events, every
shape warmed up first, the implementations alternating over several repeats, every timed window at least --window
seconds long (the number of calls in a window is set per shape and implementation from a short trial) (development aid):
  krs      layers.LSTM: the input projection on krs_gemm, the recurrence on the K25 kernels (one launch per sweep), the
           recurrent weight gradient on krs_gemm;
  torch    torch.nn.LSTM on the same device (MIOpen's fused RNN), whatever it supports for the dtype.
bf16 and fp32 at bench_gru.py's shapes: B = 4096, L = 10, U = D = 32; B = 4096, L = 50, U = D = 128; B = 512, L = 200,
U = D = 128.  No mask, no initial state, gradients arriving at the last output, as examples/sequential_retrieval.py
trains.  One JSON line per (shape, dtype) with the median and the fastest repeat's time per call, the calls per window
and the peak memory of each implementation (or why it did not run); --out FILE also writes them there."""
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
from scripts.bench_gru import SHAPES, peak_of, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="fewest calls in a timed window")
    ap.add_argument("--window", type=float, default=0.5, help="fewest seconds in a timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for b, l, u in SHAPES:
        for dtype, policy in ((torch.bfloat16, "mixed_bfloat16"), (torch.float32, "float32")):
            d = u
            x = torch.randn((b, l, d), device=dev, generator=gen).to(dtype).requires_grad_(True)
            dout = torch.randn((b, u), device=dev, generator=gen).to(dtype)
            layer = kl.LSTM(u, dtype=policy, device=dev)
            layer(x)
            ref = torch.nn.LSTM(d, u, batch_first=True, device=dev, dtype=dtype)

            def krs():
                x.grad = None
                layer.zero_grad(set_to_none=True)
                layer(x).backward(dout)

            def torch_lstm():
                x.grad = None
                ref.zero_grad(set_to_none=True)
                ref(x)[1][0][0].backward(dout)

            rec = {"B": b, "L": l, "U": u, "D": d, "dtype": str(dtype).replace("torch.", ""),
                   "device": torch.cuda.get_device_name(0), "route": None, "window_s": args.window, "repeats": args.repeats}
            live = {}
            for name, fn in (("krs", krs), ("torch", torch_lstm)):
                try:
                    for _ in range(args.warmup):
                        fn()
                    torch.cuda.synchronize()
                    live[name] = fn
                except (RuntimeError, NotImplementedError) as e:      # (a dtype torch's own call does not take)
                    rec[f"{name}_us"], rec[f"{name}_why"] = None, str(e).splitlines()[0][:160]
                if name == "krs":
                    rec["route"] = list(recurrent_ops.lstm_last_route())
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
            del x, dout, layer, ref
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
