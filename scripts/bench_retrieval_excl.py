"""K27: what per-query exclusion lists cost inside the fused top-k, and what they save.  bf16, N = 2^20, D = 128,
k = 100, at B = 64 and B = 8192, E in {0, 50, 200} exclusions per query (distinct random candidates).  Three calls on
the same operands:
  excl     retrieval_topk(q, c, k, exclusions=x)            -- K27: excluded candidates never enter the queues
  plain    retrieval_topk(q, c, k)                          -- (a) the same shape without lists: the price of the feature
  filter   retrieval_topk(q, c, k + E) and a torch filter   -- (b) what a user does without K27: at k + E > 128 the call
           leaves the fused path for the score slab
One process, every call warmed up first, then timed in alternating rounds with device events, each round a window of at
least --window seconds, so that clocks and cache state drift over all alike; a call's figure is the median of its rounds
(development aid).  One JSON line per (B, E); --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from keras_rs_amd import retrieval_ops as R

N, D, K = 1 << 20, 128, 100


def run(fn, n):
    """microseconds per call of n back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def filtered(q, c, k, x):
    """top-(k + E), drop each row's excluded ids, keep the first k: the filter in torch"""
    scores, ids = R.retrieval_topk(q, c, k + x.shape[1])
    keep = ~(ids[:, :, None] == x[:, None, :]).any(dim=2)
    pos = torch.where(keep, torch.cumsum(keep, dim=1) - 1, ids.shape[1])          # kept entries keep their order
    top = torch.argsort(pos, dim=1, stable=True)[:, :k]
    return torch.gather(scores, 1, top), torch.gather(ids, 1, top)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per call")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="64,8192")
    ap.add_argument("--lists", default="0,50,200", help="comma-separated E")
    ap.add_argument("--no-filter", action="store_true", help="skip (b), the top-(k + E) call and its torch filter")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    c = torch.randn((N, D), device=dev, generator=g).to(torch.bfloat16)
    lines = []
    for b in (int(v) for v in args.batches.split(",")):
        q = torch.randn((b, D), device=dev, generator=g).to(torch.bfloat16)
        for e in (int(v) for v in args.lists.split(",")):
            # distinct candidates per row, half of them the row's own best: a list that is ignored changes the answer
            own = R.retrieval_topk(q, c, max(1, e // 2))[1][:, : e // 2]
            x = torch.cat([own, torch.randint(0, N, (b, e - e // 2), device=dev, generator=g, dtype=torch.int32)], dim=1)
            calls = {"excl": lambda: R.retrieval_topk(q, c, K, exclusions=x), "plain": lambda: R.retrieval_topk(q, c, K)}
            if e and not args.no_filter:
                calls["filter"] = lambda: filtered(q, c, K, x)
            steps = {}
            for key, fn in calls.items():
                run(fn, args.warmup)
                steps[key] = max(1, int(args.window * 1e6 / run(fn, 1)) + 1)
            if "filter" in calls:      # both give the same ids wherever no tie at the k-th score decides
                agree = float((calls["excl"]()[1] == calls["filter"]()[1]).float().mean())
            rounds = {key: [] for key in calls}
            for _ in range(args.rounds):
                for key, fn in calls.items():
                    rounds[key].append(run(fn, steps[key]))
            us = {key: statistics.median(v) for key, v in rounds.items()}
            rec = {"B": b, "N": N, "D": D, "k": K, "E": e, "excl_us": round(us["excl"], 1),
                   "plain_us": round(us["plain"], 1), "excl_over_plain": round(us["excl"] / us["plain"], 3),
                   "excl_route": R.plan_route("topk_excl", b, N, D, K, torch.bfloat16)[1]["kernel"]}
            if "filter" in calls:
                rec.update({"filter_us": round(us["filter"], 1), "filter_over_excl": round(us["filter"] / us["excl"], 3),
                            "filter_route": R.plan_route("topk", b, N, D, K + e, torch.bfloat16)[1]["kernel"],
                            "ids_agree": round(agree, 5)})
            rec.update({"rounds_us": {key: [round(v, 1) for v in vals] for key, vals in rounds.items()},
                        "steps": steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
