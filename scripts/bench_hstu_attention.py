"""K31 HSTU attention: forward + backward of the fused kernels against the stored torch composition
(sequence_ops.hstu_attention_stored) in one process (development aid).  bf16, causal, a shared position table, a
right-padding mask; (B, H, L, Dh) = (64, 2, 50, 50), (128, 2, 200, 64), (1024, 2, 200, 64), (64, 2, 1024, 64).
Times: device events around windows of at least 0.5 s, five repeats that alternate the two paths, the median per path.
One JSON line per shape with both times and both peak memories; --out FILE also writes them there."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import sequence_ops

SHAPES = [(64, 2, 50, 50), (128, 2, 200, 64), (1024, 2, 200, 64), (64, 2, 1024, 64)]
WINDOW_S, REPEATS = 0.5, 5


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3          # microseconds per call


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for b, h, l, dh in SHAPES:
        q, k, v = (torch.randn((b, l, h, dh), device=dev, generator=gen).to(torch.bfloat16).requires_grad_(True)
                   for _ in range(3))
        pos = (0.1 * torch.randn((1, 2 * l - 1), device=dev, generator=gen)).requires_grad_(True)
        dout = torch.randn((b, l, h, dh), device=dev, generator=gen).to(torch.bfloat16)
        lengths = torch.randint(l // 2, l + 1, (b,), device=dev, generator=gen)
        valid = torch.arange(l, device=dev)[None, :] < lengths[:, None]
        kw = dict(pos_bias=pos, valid=valid, causal=True, alpha=1.0 / math.sqrt(dh), inv_n=1.0 / l)

        def run(op):
            q.grad = k.grad = v.grad = pos.grad = None
            op(q, k, v, **kw).backward(dout)

        paths = {"fused": lambda: run(sequence_ops.hstu_attention), "stored": lambda: run(sequence_ops.hstu_attention_stored)}
        rec = {"B": b, "H": h, "L": l, "Dh": dh, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
               "score_tensor_fp32_bytes": b * h * l * l * 4}
        calls, times = {}, {name: [] for name in paths}
        for name, fn in paths.items():
            rec[f"{name}_peak_bytes"] = peak_of(fn)                      # (also the warm-up)
            calls[name] = max(1, math.ceil(WINDOW_S * 1e6 / window(fn, 3)))
        run(sequence_ops.hstu_attention)
        route = sequence_ops.hstu_last_route()
        rec["route"] = [route.kernel, route.dpad, route.vec, route.lds_bytes]
        for _ in range(REPEATS):
            for name, fn in paths.items():
                times[name].append(window(fn, calls[name]))
        for name in paths:
            rec[f"{name}_us"] = round(statistics.median(times[name]), 1)
        rec["speedup"] = round(rec["stored_us"] / rec["fused_us"], 2)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, k, v, pos, dout, valid
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
