"""Approximate retrieval from the MI355X layers: the flow of the reference's examples/scann.py on the synthetic data of
examples/two_tower_retrieval.py.  Train the two towers, enlarge the candidate set the way the reference does (the item
embeddings plus copies of them scaled by uniform noise), then serve the same queries from BruteForceRetrieval and
from PartitionedRetrieval and print both times and the recall of the approximate top-k against the exact one.

    python examples/approximate_retrieval.py          # needs an MI355X; no dataset is downloaded
    python examples/approximate_retrieval.py --ah [--reorder R]

The reference serves from the ScaNN library; PartitionedRetrieval is its partitioning ("tree") stage on float rows, with
the reference's settings: num_leaves=100, num_leaves_to_search=30, training_iterations=12 (include/krs.h, K21).
`--ah` also serves the same candidates from AsymmetricHashingRetrieval, the reference's other two stages
(score_ah(dimensions_per_block=2) and, with `--reorder R`, reorder(R); include/krs.h, K23), and prints the bytes of each
index beside its time and recall.
"""

from __future__ import annotations

import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402
from examples.two_tower_retrieval import fused_retrieval_task_loss  # noqa: E402


def enlarge(item_emb: torch.Tensor, copies: int, seed: int = 0) -> torch.Tensor:
    """The item embeddings followed by `copies` copies, each scaled elementwise by uniform [0, 1) noise (scann.py:
    "artificially duplicate candidate embeddings to simulate a large number of movies")."""
    gen = torch.Generator(device=item_emb.device).manual_seed(seed)
    noisy = [item_emb * torch.rand(item_emb.shape, device=item_emb.device, generator=gen) for _ in range(copies)]
    return torch.cat([item_emb] + noisy, dim=0)


def timed(layer, query, repeats: int = 5) -> tuple:
    """(the layer's output, seconds per call: the best of `repeats` after one call that pays for the first use)"""
    out = layer(query)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = layer(query)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best


def serve_both(query_emb: torch.Tensor, candidates: torch.Tensor, k: int = 10, num_leaves: int = 100,
               num_leaves_to_search: int = 30, training_iterations: int = 12) -> dict:
    """The same queries from the exact and from the partitioned index: {"recall": the mean share of the exact top-k
    that the partitioned index returns, "brute_force_s", "partitioned_s": seconds per call, "build_s", "ids"}."""
    exact = kl.BruteForceRetrieval(candidates, k=k, return_scores=False, device=candidates.device)
    t0 = time.perf_counter()
    approx = kl.PartitionedRetrieval(candidates, k=k, return_scores=False, num_leaves=num_leaves,
                                     num_leaves_to_search=num_leaves_to_search,
                                     training_iterations=training_iterations, device=candidates.device)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    want, exact_s = timed(exact, query_emb)
    got, approx_s = timed(approx, query_emb)
    hits = (want[:, :, None] == got[:, None, :]).any(dim=2).float().sum(dim=1)
    return {"recall": float((hits / k).mean()), "brute_force_s": exact_s, "partitioned_s": approx_s, "build_s": build_s,
            "ids": got}


def serve_ah(query_emb: torch.Tensor, candidates: torch.Tensor, reorder: int | None = None, k: int = 10,
             num_leaves: int = 100, num_leaves_to_search: int = 30, training_iterations: int = 12) -> dict:
    """The same queries from the asymmetric-hashing index: {"recall" against the exact top-k, "ah_s": seconds per call,
    "build_s", "index_bytes", "float_bytes": what the partitioned index stores for the same candidates, "ids"}."""
    want = kl.BruteForceRetrieval(candidates, k=k, return_scores=False, device=candidates.device)(query_emb)
    t0 = time.perf_counter()
    index = kl.AsymmetricHashingRetrieval(candidates, k=k, return_scores=False, num_leaves=num_leaves,
                                          num_leaves_to_search=num_leaves_to_search,
                                          training_iterations=training_iterations, dimensions_per_block=2,
                                          num_reordering_candidates=reorder, device=candidates.device)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    got, ah_s = timed(index, query_emb)
    hits = (want[:, :, None] == got[:, None, :]).any(dim=2).float().sum(dim=1)
    return {"recall": float((hits / k).mean()), "ah_s": ah_s, "build_s": build_s, "index_bytes": index.index_bytes(),
            "float_bytes": candidates.numel() * candidates.element_size(), "ids": got}


def main(steps: int = 20, batch: int = 256, users: int = 1000, items: int = 2000, dim: int = 32, copies: int = 100,
         ah: bool = False, reorder: int | None = None):
    dev = torch.device("cuda", torch.cuda.current_device())
    query_tower = kl.Embedding(users, dim, device=dev)
    cand_tower = kl.Embedding(items, dim, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    user_ids = torch.randint(0, users, (batch,), device=dev, generator=gen, dtype=torch.int32)
    item_ids = torch.randint(0, items, (batch,), device=dev, generator=gen, dtype=torch.int32)
    query_tower(user_ids), cand_tower(item_ids)                       # (builds the tables)
    opt = torch.optim.SGD(query_tower.weights + cand_tower.weights, lr=0.5)
    for step in range(steps):
        opt.zero_grad()
        value = fused_retrieval_task_loss(query_tower(user_ids), cand_tower(item_ids), cand_ids=item_ids)
        value.backward()
        opt.step()
    print(f"trained {steps} steps: loss {float(value.detach()):.4f}")
    all_items = torch.arange(items, device=dev, dtype=torch.int32)
    candidates = enlarge(cand_tower(all_items).detach(), copies)
    served = serve_both(query_tower(user_ids).detach(), candidates)
    print(f"{candidates.shape[0]} candidates, {batch} queries, k = 10")
    print(f"Time taken by brute force layer (sec): {served['brute_force_s']:.6f}")
    print(f"Time taken by partitioned layer (sec): {served['partitioned_s']:.6f}   (index build: "
          f"{served['build_s']:.3f} s)")
    print(f"recall of the partitioned top-10 against the exact one: {served['recall']:.4f}")
    if ah:
        hashed = serve_ah(query_tower(user_ids).detach(), candidates, reorder=reorder)
        stage = "without reordering" if reorder is None else f"reordering {reorder} candidates"
        print(f"Time taken by asymmetric hashing layer (sec), {stage}: {hashed['ah_s']:.6f}   (index build: "
              f"{hashed['build_s']:.3f} s)")
        print(f"index bytes: {hashed['index_bytes']} (asymmetric hashing) against {hashed['float_bytes']} of float rows")
        print(f"recall of the asymmetric hashing top-10 against the exact one: {hashed['recall']:.4f}")
        served["ah"] = hashed
    return served


if __name__ == "__main__":
    import argparse

    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--ah", action="store_true", help="also serve from AsymmetricHashingRetrieval")
    parser.add_argument("--reorder", type=int, default=None, metavar="R",
                        help="with --ah: rescore the best R candidates exactly (k <= R <= 128)")
    args = parser.parse_args()
    main(ah=args.ah, reorder=args.reorder)
