"""Two-tower retrieval from the MI355X layers: the in-batch softmax loss of the reference's retrieval examples
(examples/sequential_retrieval.py:344-360, examples/multi_task.py: scores = q c^T, labels = eye(batch),
CategoricalCrossentropy(from_logits=True)) with the three optional logit stages of a retrieval task in their usual
order, then serving with BruteForceRetrieval.

    python examples/two_tower_retrieval.py            # a few training steps on synthetic ids (needs an MI355X)

Stages of `retrieval_task_loss`: scores -> SamplingProbabilityCorrection -> RemoveAccidentalHits ->
HardNegativeMining -> CategoricalCrossentropy.  The scores are one GEMM; everything after it is K11 / K8 kernels.

    python examples/two_tower_retrieval.py --fused    # the same run on InBatchSoftmaxLoss (K13 / K14)

`fused_retrieval_task_loss` is the same loss, hard-negative mining included, computed from the embeddings by the fused
kernels: the [B, N] scores are never stored, so it also runs at batch sizes where the score matrix does not fit.  Both
runs train one objective (the fused one keeps its scores in fp32 and sends ties to the lowest index).

    python examples/two_tower_retrieval.py --eval     # then: top-k accuracies and MRR over all items (K15)

`evaluate` scores every query against the whole item table with FactorizedTopK: one sweep gives the positive's rank,
hence every top-k accuracy and the mean reciprocal rank, again without storing the scores.

    python examples/two_tower_retrieval.py --quantize # then: serve the same queries from an int8 index (K17)

`serve_quantized` builds the exact index and its `quantize("int8")` form from the same item embeddings, serves the same
queries through both and reports how many of the exact top-k the int8 index returns, and the bytes of both.
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_rs_amd.layers as kl  # noqa: E402


def retrieval_task_loss(query_emb: torch.Tensor, cand_emb: torch.Tensor, cand_ids: torch.Tensor | None = None,
                        cand_prob: torch.Tensor | None = None, num_hard_negatives: int | None = None,
                        loss=None) -> torch.Tensor:
    """The in-batch softmax loss of query_emb [B, D] against cand_emb [N, D] (N >= B; candidate i is the positive of
    query i).  cand_prob [N]: the candidates' sampling probabilities (logits -= log p).  cand_ids [N]: candidates with
    the positive's id are accidental hits.  num_hard_negatives: keep that many highest-scoring negatives per query."""
    loss = loss if loss is not None else kl.CategoricalCrossentropy(from_logits=True)
    scores = torch.matmul(query_emb, cand_emb.transpose(0, 1))
    labels = torch.eye(scores.shape[0], scores.shape[1], dtype=torch.float32, device=scores.device)
    if cand_prob is not None:
        scores = kl.SamplingProbabilityCorrection()(scores, cand_prob)
    if cand_ids is not None:
        scores = kl.RemoveAccidentalHits()(scores, labels, cand_ids)
    if num_hard_negatives is not None:
        scores, labels = kl.HardNegativeMining(num_hard_negatives)(scores, labels)
    return loss(labels, scores)


def fused_retrieval_task_loss(query_emb: torch.Tensor, cand_emb: torch.Tensor, cand_ids: torch.Tensor | None = None,
                              cand_prob: torch.Tensor | None = None,
                              num_hard_negatives: int | None = None) -> torch.Tensor:
    """retrieval_task_loss on InBatchSoftmaxLoss: the [B, N] scores are never stored."""
    return kl.InBatchSoftmaxLoss(num_hard_negatives=num_hard_negatives)(
        query_emb, cand_emb, candidate_ids=cand_ids, candidate_sampling_probability=cand_prob)


def evaluate(query_emb: torch.Tensor, item_emb: torch.Tensor, positive_item: torch.Tensor,
             ks=(1, 5, 10, 50, 100)) -> dict:
    """Top-k categorical accuracies and the mean reciprocal rank of query_emb [B, D] against the whole item table
    item_emb [items, D], positive_item [B] being the row of each query's item: floats by metric name."""
    metric = kl.FactorizedTopK(item_emb.detach(), ks=ks)
    metric.update_state(query_emb.detach(), positive_item)
    return {name: float(value) for name, value in metric.result().items()}


def serve_quantized(query_emb: torch.Tensor, item_emb: torch.Tensor, item_ids: torch.Tensor, k: int = 5) -> dict:
    """The same queries served from the exact index and from its int8 form: {"overlap": the mean share of the exact
    top-k ids that the int8 index also returns (its recall against the exact one), "index_bytes": of the float index,
    "quantized_index_bytes": int8 rows plus fp32 steps, "ids": the int8 index's ids}."""
    exact = kl.BruteForceRetrieval(item_emb.detach(), item_ids, k=k, return_scores=False, device=item_emb.device)
    quantized = kl.BruteForceRetrieval(item_emb.detach(), item_ids, k=k, return_scores=False, device=item_emb.device)
    index_bytes = exact.candidate_embeddings.numel() * exact.candidate_embeddings.element_size()
    quantized.quantize("int8")
    q_bytes = quantized.candidate_embeddings_q.numel() + 4 * quantized.candidate_embeddings_step.numel()
    want, got = exact(query_emb.detach()), quantized(query_emb.detach())
    hits = (want[:, :, None] == got[:, None, :]).any(dim=2).float().sum(dim=1)       # ids are unique per item
    return {"overlap": float((hits / k).mean()), "index_bytes": index_bytes, "quantized_index_bytes": q_bytes,
            "ids": got}


def main(steps: int = 5, batch: int = 256, users: int = 1000, items: int = 2000, dim: int = 32,
         fused: bool = False, evaluate_after: bool = False, quantize: bool = False):
    dev = torch.device("cuda", torch.cuda.current_device())
    query_tower = kl.Embedding(users, dim, device=dev)
    cand_tower = kl.Embedding(items, dim, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    user_ids = torch.randint(0, users, (batch,), device=dev, generator=gen, dtype=torch.int32)
    item_ids = torch.randint(0, items, (batch,), device=dev, generator=gen, dtype=torch.int32)
    item_prob = torch.full((batch,), 1.0 / items, device=dev)        # uniform in-batch sampling
    query_tower(user_ids), cand_tower(item_ids)                       # (builds the tables)
    opt = torch.optim.SGD(query_tower.weights + cand_tower.weights, lr=0.5)
    for step in range(steps):
        opt.zero_grad()
        if fused:
            value = fused_retrieval_task_loss(query_tower(user_ids), cand_tower(item_ids), cand_ids=item_ids,
                                              cand_prob=item_prob, num_hard_negatives=32)
        else:
            value = retrieval_task_loss(query_tower(user_ids), cand_tower(item_ids), cand_ids=item_ids,
                                        cand_prob=item_prob, num_hard_negatives=32)
        value.backward()
        opt.step()
        print(f"step {step}: loss {float(value):.4f}")
    all_items = torch.arange(items, device=dev, dtype=torch.int32)
    retrieval = kl.BruteForceRetrieval(cand_tower(all_items).detach(), all_items, k=5, device=dev)
    scores, top = retrieval(query_tower(user_ids[:4]).detach())
    print("top-5 items of the first queries:", top.tolist())
    if evaluate_after:
        for name, value in evaluate(query_tower(user_ids), cand_tower(all_items), item_ids).items():
            print(f"{name}: {value:.4f}")
    if quantize:
        served = serve_quantized(query_tower(user_ids), cand_tower(all_items), all_items, k=5)
        print(f"int8 index: mean overlap with the exact top-5 {served['overlap']:.4f}; index bytes "
              f"{served['index_bytes']} -> {served['quantized_index_bytes']}")
        print("top-5 items of the first queries from the int8 index:", served["ids"][:4].tolist())
        return served
    return None


if __name__ == "__main__":
    main(fused="--fused" in sys.argv[1:], evaluate_after="--eval" in sys.argv[1:], quantize="--quantize" in sys.argv[1:])
