"""K23 against K21 and K8: AsymmetricHashingRetrieval (krs_retrieval_ivf_ah) without and with the reorder stage,
PartitionedRetrieval (krs_retrieval_ivf) on the SAME partition and BruteForceRetrieval (krs_retrieval_topk) on the same bf16
candidates, at K21's shapes: N = 2^20, D = 128, 1024 leaves, B = 64 (S1) and 8192 (S2), num_leaves_to_search in
{8, 32, 128}, for (k, R) = (100, 128) and (10, 100).  The method is scripts/bench_retrieval_ivf.py's: one process, every
layer warmed up first, then timed in alternating rounds with device events, the figure of a layer being the median of its
rounds (development aid).  Two data sets: a mixture of 1024 Gaussians and plain normal rows.  Each point also records the
bytes of every index, recall@k of each against the exact result, and the build and encode times.  One JSON line per
point, printed as it is measured; --out FILE also appends them there (profiles/k23_bench_retrieval_ah.jsonl)."""
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
from scripts.bench_retrieval_ivf import D, LEAVES, N, PROBES, SHAPES, make_data, run

KR = ((100, 128), (10, 100))      # (k, num_reordering_candidates)


def recall(got, want, k):
    hits = torch.stack([torch.isin(got[i], want[i]).sum() for i in range(got.shape[0])]).float()
    return round(float(hits.mean()) / k, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per layer")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2", help="comma-separated subset of S1,S2")
    ap.add_argument("--data", default="mixture,normal", help="comma-separated subset of mixture,normal")
    ap.add_argument("--probes", default=",".join(str(p) for p in PROBES))
    ap.add_argument("--n", type=int, default=N, help="candidates (the recorded points use the default)")
    ap.add_argument("--training-iterations", type=int, default=12)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    probes_list = [int(p) for p in args.probes.split(",")]
    for kind in args.data.split(","):
        g = torch.Generator(device=dev).manual_seed(0)
        cand, queries = make_data(kind, args.n, max(SHAPES.values()), dev, g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = kl.AsymmetricHashingRetrieval(cand, k=KR[0][0], return_scores=False, num_leaves=LEAVES,
                                              num_leaves_to_search=probes_list[0], num_reordering_candidates=KR[0][1],
                                              training_iterations=args.training_iterations)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        row_leaf = first.assignments[first.row_index.long()].contiguous()
        encode_us = statistics.median(
            run(lambda: R.ah_encode(cand, row_leaf, first.centroids, first.codebooks, row_index=first.row_index), 3)
            for _ in range(3))
        float_bytes = cand.numel() * cand.element_size()
        for k, r in KR:
            exact = kl.BruteForceRetrieval(cand, k=k, return_scores=False)
            ivf = kl.PartitionedRetrieval.from_partition(cand, first.centroids, first.assignments, k=k,
                                                         return_scores=False, num_leaves_to_search=probes_list[0])
            scan = kl.AsymmetricHashingRetrieval.from_codebooks(cand, first.centroids, first.assignments, first.codebooks,
                                                                k=k, return_scores=False,
                                                                num_leaves_to_search=probes_list[0])
            reorder = kl.AsymmetricHashingRetrieval.from_codebooks(cand, first.centroids, first.assignments,
                                                                   first.codebooks, k=k, return_scores=False,
                                                                   num_leaves_to_search=probes_list[0],
                                                                   num_reordering_candidates=r)
            assert torch.equal(scan.codes, first.codes)
            layers = {"ivf": ivf, "ah": scan, "ah_reorder": reorder}
            for name, b in SHAPES.items():
                if name not in args.shapes.split(","):
                    continue
                q = queries[:b]
                for p in probes_list:
                    for layer in layers.values():
                        layer.num_leaves_to_search = p
                    calls = {"exact": lambda: exact(q)}
                    calls.update({key: (lambda layer=layer: layer(q)) for key, layer in layers.items()})
                    for fn in calls.values():
                        run(fn, args.warmup)
                    rounds = {key: [] for key in calls}
                    for _ in range(args.rounds):
                        for key, fn in calls.items():
                            rounds[key].append(run(fn, args.steps))
                    us = {key: statistics.median(v) for key, v in rounds.items()}
                    want = exact(q[:256])
                    rec = {"shape": name, "data": kind, "B": b, "N": args.n, "D": D, "k": k, "R": r, "num_leaves": LEAVES,
                           "num_leaves_to_search": p, "dimensions_per_block": 2}
                    rec.update({f"{key}_us": round(v, 1) for key, v in us.items()})
                    rec.update({"exact_over_ah": round(us["exact"] / us["ah"], 3),
                                "exact_over_ah_reorder": round(us["exact"] / us["ah_reorder"], 3),
                                "ivf_over_ah": round(us["ivf"] / us["ah"], 3),
                                "ivf_over_ah_reorder": round(us["ivf"] / us["ah_reorder"], 3)})
                    rec.update({f"{key}_recall_at_k": recall(layer(q[:256]), want, k) for key, layer in layers.items()})
                    rec.update({f"{key}_rounds_us": [round(v, 1) for v in vs] for key, vs in rounds.items()})
                    rec.update({"float_rows_bytes": float_bytes, "ivf_index_bytes": sum(
                                    t.numel() * t.element_size() for t in ivf.state_dict().values()),
                                "ah_index_bytes": scan.index_bytes(), "ah_reorder_index_bytes": reorder.index_bytes(),
                                "code_bytes": scan.codes.numel(), "build_s": round(build_s, 2),
                                "encode_us": round(encode_us, 1), "training_iterations": args.training_iterations,
                                "ah_workspace_bytes": R.retrieval_ivf_ah_workspace_bytes(
                                    b, args.n, D, LEAVES, p, k, r, 2, True, torch.bfloat16),
                                "steps": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)})
                    print(json.dumps(rec), flush=True)
                    if args.out:
                        with open(args.out, "a") as f:
                            f.write(json.dumps(rec) + "\n")
            del exact, ivf, scan, reorder, layers
            torch.cuda.empty_cache()
        del cand, queries, first
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
