"""Micro-benchmark of K16 against K1 at the C3 shape: the int8 lookup (krs_embed_bag_fwd_q8) and the bf16 lookup
(krs_embed_bag_fwd) on the SAME ids, bf16 out, alternated in one process, for the multi-hot and the L = 1 calls; and the
quantizer (krs_quantize_rows_q8) over one 1 M x 128 table.  Development aid; prints one JSON line per measurement and
writes them all to --out.  The yardstick of the int8 kernel is the bf16 K1 of the same run, never its own earlier runs.

    python scripts/bench_k1_q8.py [--out k16.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from keras_rs_amd import embedding_ops as E

ap = argparse.ArgumentParser()
ap.add_argument("--tables", type=int, default=26)
ap.add_argument("--vocab", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5, help="alternations of the two kernels")
ap.add_argument("--iters", type=int, default=20, help="timed launches per kernel per round")
ap.add_argument("--forms", default="multihot,hot1,quantize", help="which measurements to run (a counter pass takes one)")
ap.add_argument("--out", default="")
a = ap.parse_args()

dev = torch.device("cuda:0")
HOTS = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]
g = torch.Generator(device=dev).manual_seed(1337)
tables = [(torch.rand(a.vocab, a.dim, device=dev, generator=g) * 0.1 - 0.05).to(torch.bfloat16) for _ in range(a.tables)]
quant = [E.quantize_rows(t) for t in tables]
feats = [(t, "sum", t * a.dim) for t in range(a.tables)]
fb = E.FusedBags(tables, feats)
qb = E.QuantizedBags([q for q, _ in quant], [s for _, s in quant], feats)
out = torch.empty(a.batch, a.tables * a.dim, dtype=torch.bfloat16, device=dev)
results = []


def emit(rec):
    results.append(rec)
    print(json.dumps(rec), flush=True)


def timed(fn, iters):
    """per-launch times in seconds, from device events around every launch"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]) * 1e-3


emit({"what": "table_bytes", "tables": a.tables, "vocab": a.vocab, "dim": a.dim,
      "bf16": sum(t.numel() * 2 for t in tables), "int8": sum(q.numel() + s.numel() * 4 for q, s in quant)})

forms = a.forms.split(",")
for name, hots in (("multihot", (HOTS * 4)[: a.tables]), ("hot1", [1] * a.tables)):
    if name not in forms:
        continue
    gi = torch.Generator(device=dev).manual_seed(1338)
    ids = torch.cat([torch.randint(0, a.vocab, (a.batch * h,), device=dev, generator=gi, dtype=torch.int32) for h in hots])
    nnz, bags = ids.numel(), a.batch * a.tables
    runs = {"bf16": lambda: fb.forward(ids, a.batch, hots=hots, out=out),
            "int8": lambda: qb.forward(ids, a.batch, hots=hots, out=out)}
    for fn in runs.values():          # warm-up: code objects, descriptor uploads
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(a.rounds):         # alternate the two kernels
        for k, fn in runs.items():
            ts[k].append(timed(fn, a.iters))
    med = {k: float(np.median(np.concatenate(v))) for k, v in ts.items()}
    per_round = {k: [float(np.median(v)) * 1e6 for v in vs] for k, vs in ts.items()}
    # algorithmic bytes: per lookup the row + 4 (id) [+ 4 (step)], per bag the output row + 4
    bytes_ = {"bf16": nnz * (a.dim * 2 + 4) + bags * (a.dim * 2 + 4), "int8": nnz * (a.dim + 4 + 4) + bags * (a.dim * 2 + 4)}
    for k in runs:
        emit({"what": name, "kernel": k, "route": (E.embed_fwd_last_route() if k == "bf16" else E.embed_fwd_q8_last_route())["kernel"],
              "nnz": nnz, "median_us": med[k] * 1e6, "round_medians_us": per_round[k], "bytes": bytes_[k],
              "frac_of_8TBps": bytes_[k] / med[k] / 8e12})
    emit({"what": name, "int8_over_bf16": med["int8"] / med["bf16"], "by_bytes_alone": bytes_["int8"] / bytes_["bf16"]})

# the quantizer over one table
if "quantize" in forms:
    src = tables[0]
    for _ in range(3):
        E.quantize_rows(src)
    torch.cuda.synchronize()
    tq = np.concatenate([timed(lambda: E.quantize_rows(src), a.iters) for _ in range(a.rounds)])
    qbytes = src.numel() * 2 + src.numel() + src.shape[0] * 4
    emit({"what": "quantize_rows", "rows": src.shape[0], "dim": a.dim, "source": "bf16", "median_us": float(np.median(tq)) * 1e6,
          "bytes": qbytes, "frac_of_8TBps": qbytes / float(np.median(tq)) / 8e12})
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
