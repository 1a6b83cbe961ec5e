"""K17 against K8: krs_retrieval_topk_q8 over an int8 index and krs_retrieval_topk over the bf16 one, on the same
embeddings, at S1 (B = 64) and S2 (B = 8192) of DESIGN.md section 4 (K8): N = 2^20, D = 128, k = 100.  One process,
both kernels warmed up first, then timed in alternating rounds with device events, so that clocks and cache state drift
over both alike; the figure of a kernel is the median of its rounds (development aid).  The int8 call includes its query
quantizer.  One JSON line per shape; --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from keras_rs_amd import embedding_ops as E
from keras_rs_amd import retrieval_ops as R

SHAPES = [  # name, B, N, D, k
    ("S1", 64, 1 << 20, 128, 100),
    ("S2", 8192, 1 << 20, 128, 100),
]


def run(fn, n):
    """microseconds per call of n back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per kernel")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2", help="comma-separated subset of S1,S2")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, b, n, d, k in SHAPES:
        if name not in args.shapes.split(","):
            continue
        q = torch.randn((b, d), device=dev, generator=g).to(torch.bfloat16)
        c = torch.randn((n, d), device=dev, generator=g).to(torch.bfloat16)
        cq, cstep = E.quantize_rows(c)
        calls = {"bf16": lambda: R.retrieval_topk(q, c, k), "int8": lambda: R.retrieval_topk_q8(q, cq, cstep, k)}
        for fn in calls.values():
            run(fn, args.warmup)
        rounds = {key: [] for key in calls}
        for _ in range(args.rounds):
            for key, fn in calls.items():
                rounds[key].append(run(fn, args.steps))
        us = {key: statistics.median(v) for key, v in rounds.items()}
        # how much of the exact (bf16) top-k the int8 index returns at this shape
        exact, served = R.retrieval_topk(q[:64], c, k)[1], R.retrieval_topk_q8(q[:64], cq, cstep, k)[1]
        overlap = float((exact[:, :, None] == served[:, None, :]).any(dim=2).float().mean())
        rec = {"shape": name, "B": b, "N": n, "D": d, "k": k, "bf16_us": round(us["bf16"], 1),
               "int8_us": round(us["int8"], 1), "bf16_over_int8": round(us["bf16"] / us["int8"], 3),
               "bf16_rounds_us": [round(v, 1) for v in rounds["bf16"]],
               "int8_rounds_us": [round(v, 1) for v in rounds["int8"]],
               "index_bytes_bf16": n * d * 2, "index_bytes_int8": n * d + 4 * n, "overlap_at_k": round(overlap, 4),
               "steps": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, c, cq, cstep
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
