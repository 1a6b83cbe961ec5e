"""K19 fused self-attention: forward + backward of three implementations in one process, device events, warm-up first
(development aid):
  fused   sequence_ops.seq_attention: the K19 kernels, scores and probabilities never stored;
  stored  a torch composition that keeps the probabilities for autograd (matmul, masked softmax, matmul);
  sdpa    torch.nn.functional.scaled_dot_product_attention on the device, whatever backend torch picks.
bf16, causal with a right-padding mask, no dropout; B = 4096 with L in {50, 200} x (H, Dh) in {(1, 50), (2, 64), (4, 32)},
and B = 512, L = 1024, H = 2, Dh = 64.  One JSON line per shape with the time and the peak memory of each (or why it
did not run); --out FILE also writes them there."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import sequence_ops

SHAPES = [(4096, l, h, dh) for l in (50, 200) for (h, dh) in ((1, 50), (2, 64), (4, 32))] + [(512, 1024, 2, 64)]


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
    ap.add_argument("--paths", default="fused,stored,sdpa")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    paths = args.paths.split(",")
    lines = []
    for b, l, h, dh in SHAPES:
        q, k, v = ((torch.randn((b, l, h, dh), device=dev, generator=gen)).to(torch.bfloat16).requires_grad_(True)
                   for _ in range(3))
        dout = torch.randn((b, l, h, dh), device=dev, generator=gen).to(torch.bfloat16)
        lengths = torch.randint(l // 2, l + 1, (b,), device=dev, generator=gen)
        valid = torch.arange(l, device=dev)[None, :] < lengths[:, None]                       # [B, L]
        allowed = valid[:, None, None, :] & torch.tril(torch.ones(l, l, dtype=torch.bool, device=dev))   # [B, 1, L, L]
        scale = 1.0 / math.sqrt(dh)

        def fused():
            q.grad = k.grad = v.grad = None
            sequence_ops.seq_attention(q, k, v, key_valid=valid, causal=True, scale=scale).backward(dout)

        def stored():
            q.grad = k.grad = v.grad = None
            s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
            p = torch.softmax(s.float().masked_fill(~allowed, -math.inf), dim=-1).to(torch.bfloat16)
            torch.einsum("bhij,bjhd->bihd", p, v).backward(dout)

        def sdpa():
            q.grad = k.grad = v.grad = None
            o = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                                                 attn_mask=allowed, scale=scale)
            o.transpose(1, 2).backward(dout)

        rec = {"B": b, "L": l, "H": h, "Dh": dh, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
               "route": None, "score_tensor_fp32_bytes": b * h * l * l * 4}
        for name, fn in (("fused", fused), ("stored", stored), ("sdpa", sdpa)):
            if name in paths:
                q.grad = k.grad = v.grad = None          # (the last path's gradients are not this path's baseline)
                rec[f"{name}_us"], rec[f"{name}_peak_bytes"] = measure(fn, args.steps, args.warmup)
                if name == "fused":
                    rec["route"] = list(sequence_ops.last_route())
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, k, v, dout, valid, allowed
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
