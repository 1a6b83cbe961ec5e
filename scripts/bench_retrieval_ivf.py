"""K21 against K8: PartitionedRetrieval (krs_retrieval_ivf) and BruteForceRetrieval (krs_retrieval_topk) on the same
bf16 candidates, at S1 (B = 64) and S2 (B = 8192) of DESIGN.md section 4 (K8): N = 2^20, D = 128, k = 100, with
num_leaves = 1024 and num_leaves_to_search in {8, 32, 128}.  One process, every layer warmed up first, then timed in
alternating rounds with device events, so that clocks and cache state drift over all alike; the figure of a layer is
the median of its rounds (development aid).  Two data sets: a mixture of 1024 Gaussians (clustered: the favourable case)
and plain normal rows (the unfavourable one).  Each point also records the index build time and recall@k against the
exact result.  One JSON line per point; --out FILE also writes them there (profiles/retrieval_ivf.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import keras_rs_amd.layers as kl
from keras_rs_amd import retrieval_ops as R

SHAPES = {"S1": 64, "S2": 8192}      # name -> B
N, D, K, LEAVES = 1 << 20, 128, 100, 1024
PROBES = (8, 32, 128)


def run(fn, n):
    """microseconds per call of n back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def make_data(kind, n, b, dev, g):
    """(candidates [n, D], queries [b, D]) in bf16: `mixture` draws both around the same 1024 centres (sigma 0.3 around
    unit-variance centres), `normal` is independent normal rows."""
    if kind == "mixture":
        centres = torch.randn((LEAVES, D), device=dev, generator=g)
        c = centres[torch.randint(0, LEAVES, (n,), device=dev, generator=g)]
        c = c + 0.3 * torch.randn((n, D), device=dev, generator=g)
        q = centres[torch.randint(0, LEAVES, (b,), device=dev, generator=g)]
        q = q + 0.3 * torch.randn((b, D), device=dev, generator=g)
    else:
        c = torch.randn((n, D), device=dev, generator=g)
        q = torch.randn((b, D), device=dev, generator=g)
    return c.to(torch.bfloat16), q.to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per layer")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2", help="comma-separated subset of S1,S2")
    ap.add_argument("--data", default="mixture,normal", help="comma-separated subset of mixture,normal")
    ap.add_argument("--n", type=int, default=N, help="candidates (the recorded points use the default)")
    ap.add_argument("--training-iterations", type=int, default=12)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for kind in args.data.split(","):
        g = torch.Generator(device=dev).manual_seed(0)
        cand, queries = make_data(kind, args.n, max(SHAPES.values()), dev, g)
        exact = kl.BruteForceRetrieval(cand, k=K, return_scores=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = kl.PartitionedRetrieval(cand, k=K, return_scores=False, num_leaves=LEAVES, num_leaves_to_search=PROBES[0],
                                        training_iterations=args.training_iterations)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        sizes = (index.leaf_offsets[1:] - index.leaf_offsets[:-1]).float()
        for name, b in SHAPES.items():
            if name not in args.shapes.split(","):
                continue
            q = queries[:b]

            def served(probes):
                def call():
                    index.num_leaves_to_search = probes
                    return index(q)
                return call

            calls = {"exact": lambda: exact(q)}
            calls.update({f"p{p}": served(p) for p in PROBES})
            for fn in calls.values():
                run(fn, args.warmup)
            rounds = {key: [] for key in calls}
            for _ in range(args.rounds):
                for key, fn in calls.items():
                    rounds[key].append(run(fn, args.steps))
            us = {key: statistics.median(v) for key, v in rounds.items()}
            want = exact(q[:256])
            for p in PROBES:
                got = calls[f"p{p}"]()[:256]
                hits = torch.stack([torch.isin(got[i], want[i]).sum() for i in range(got.shape[0])]).float()
                rec = {"shape": name, "data": kind, "B": b, "N": args.n, "D": D, "k": K, "num_leaves": LEAVES,
                       "num_leaves_to_search": p, "exact_us": round(us["exact"], 1), "ivf_us": round(us[f"p{p}"], 1),
                       "exact_over_ivf": round(us["exact"] / us[f"p{p}"], 3),
                       "exact_rounds_us": [round(v, 1) for v in rounds["exact"]],
                       "ivf_rounds_us": [round(v, 1) for v in rounds[f"p{p}"]],
                       "recall_at_k": round(float(hits.mean()) / K, 4), "build_s": round(build_s, 2),
                       "training_iterations": args.training_iterations,
                       "leaf_rows_min_mean_max": [int(sizes.min()), round(float(sizes.mean()), 1), int(sizes.max())],
                       "workspace_bytes": R.retrieval_ivf_workspace_bytes(b, args.n, D, LEAVES, p, K, torch.bfloat16),
                       "exact_workspace_bytes": R.retrieval_topk_workspace_bytes(b, args.n, D, K, torch.bfloat16),
                       "steps": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
        del cand, queries, exact, index
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
