"""K30 sampled softmax: loss forward + backward down to d emb and the dense table gradient, two implementations in one
process, device events after a warm-up, the implementations alternating over --repeats repeats (development aid):
  fused    layers.SampledSoftmaxCrossentropy and autograd.grad: one krs_sampled_softmax_fwd_bwd call, the in-place
           multiplies by the upstream scalar, two K2 plan + dense applies, one host read of the error word;
  stored   layers.losses.sampled_softmax_crossentropy_stored: two layers.Embedding lookups, the [B, L, N] fp32 logits
           by a batched product, the masked log-softmax, and torch's backward through them, with two K2 calls.
Points (B, L, d) x N x G in {B, 1}; mixed_bfloat16 (bf16 sequence embedding, fp32 table), V = 2^17.
peak_mb: torch's peak allocation during one call above what the operands hold.
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
from keras_rs_amd.layers.losses import sampled_softmax_crossentropy_stored

SHAPES = [(4096, 50, 50), (4096, 200, 64), (512, 1024, 128)]
V = 1 << 17


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def point(b, length, d, n, shared, iters, repeats, dev):
    g = torch.Generator().manual_seed(b + d + n)
    layer = kl.Embedding(V, d, device=dev, dtype="mixed_bfloat16")
    layer.build()
    emb = (torch.randn(b, length, d, generator=g) * 0.3).bfloat16().to(dev).requires_grad_(True)
    pos = torch.randint(1, V, (b, length), generator=g, dtype=torch.int32).to(dev)
    neg = torch.randint(1, V, (n,) if shared else (b, n), generator=g, dtype=torch.int32).to(dev)
    mask = (torch.rand(b, length, generator=g) > 0.25).to(dev)
    loss_fn = kl.SampledSoftmaxCrossentropy()
    fused = lambda: torch.autograd.grad(loss_fn(layer, emb, pos, neg, mask), (emb, layer.embeddings))      # noqa: E731
    stored = lambda: torch.autograd.grad(sampled_softmax_crossentropy_stored(layer, emb, pos, neg, mask),  # noqa: E731
                                         (emb, layer.embeddings))
    times = {"fused": [], "stored": []}
    for name, fn in (("fused", fused), ("stored", stored)):
        fn()
    for _ in range(repeats):
        for name, fn in (("fused", fused), ("stored", stored)):
            times[name].append(timed(fn, iters))
    row = {"b": b, "l": length, "d": d, "n": n, "g": 1 if shared else b}
    for name, fn in (("fused", fused), ("stored", stored)):
        row[name + "_us"] = round(statistics.median(times[name]), 1)
        row[name + "_peak_mb"] = round(peak_mb(fn), 1)
    row["speedup"] = round(row["stored_us"] / row["fused_us"], 2)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for b, length, d in SHAPES:
        for n in (128, 1024):
            for shared in (False, True):
                rows.append(point(b, length, d, n, shared, a.iters, a.repeats, dev))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
