"""K29 sampled-item BCE: loss forward + backward down to d emb and the dense table gradient, two implementations in
one process, device events, every point warmed up first, the implementations alternating over --repeats repeats, every
timed window at least --window seconds long (development aid):
  fused    layers.SampledItemCrossentropy and autograd.grad: one krs_sampled_bce_fwd_bwd call, the two in-place
           multiplies by the upstream scalar, one K2 plan + dense apply over the (1 + N) B L lookups, one host read of
           the error word;
  stored   layers.losses.sampled_item_crossentropy_stored, the composition examples/sas_rec.py ran before K29: two
           layers.Embedding lookups (K1, each with its host read) that store the embedded items, three fp32 blocks, the
           logits, the element-wise BCE, and in the backward torch's element-wise chain and two K2 calls.
Points (B, L, d, V, N): (64, 50, 50, 500, 1) the example's shape, (128, 200, 64, 50000, 1), (1024, 200, 128, 2^20, 1)
and the last with N = 4; "bf16" is the mixed_bfloat16 policy (bf16 sequence embedding, fp32 table), "fp32" all fp32.
`scale_us` is the time of the fused side's two upstream-scaling multiplies alone, on buffers of its shapes (it is
inside `fused`).  peak_mb: torch's peak allocation during one call above what the operands hold.
One JSON line per point; --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd.layers.losses import sampled_item_crossentropy_stored

POINTS = [(64, 50, 50, 500, 1), (128, 200, 64, 50000, 1), (1024, 200, 128, 1 << 20, 1), (1024, 200, 128, 1 << 20, 4)]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def sides(b, length, d, v, n, dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(b + d + n)
    layer = kl.Embedding(v, d, device=dev, dtype="mixed_bfloat16" if dtype == torch.bfloat16 else "float32")
    emb = (torch.randn(b, length, d, generator=g) * 0.3).to(dtype).to(dev).requires_grad_(True)
    pos = torch.randint(1, v, (b, length), generator=g, dtype=torch.int32).to(dev)
    neg = torch.randint(1, v, (b, length) if n == 1 else (b, length, n), generator=g, dtype=torch.int32).to(dev)
    mask = (torch.rand(b, length, generator=g) > 0.25).to(dev)
    layer(pos[:1])                                            # (builds the table)
    loss_fn = kl.SampledItemCrossentropy()
    demb = torch.empty(b * length, d, dtype=dtype, device=dev)
    glog = torch.empty(b * length, 1 + n, device=dev)
    up = torch.ones((), device=dev)

    def fused():
        return torch.autograd.grad(loss_fn(layer, emb, pos, neg, mask), (emb, layer.embeddings))

    def stored():
        return torch.autograd.grad(sampled_item_crossentropy_stored(layer, emb, pos, neg, mask), (emb, layer.embeddings))

    def scale():
        demb.mul_(up)
        glog.mul_(up)

    return {"fused": fused, "stored": stored, "scale": scale}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []
    for b, length, d, v, n in POINTS:
        for dtype in (torch.bfloat16, torch.float32):
            fns = sides(b, length, d, v, n, dtype, dev)
            rec = dict(b=b, l=length, d=d, v=v, n=n, dtype=str(dtype).split(".")[-1])
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
            for name in ("fused", "stored"):
                rec[name] = dict(median_us=round(statistics.median(times[name]), 1), best_us=round(min(times[name]), 1),
                                 calls=calls[name], peak_mb=peak_mb(fns[name]))
            rec["scale_us"] = round(statistics.median(times["scale"]), 1)
            rec["speedup"] = round(rec["stored"]["median_us"] / rec["fused"]["median_us"], 3)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del fns
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
