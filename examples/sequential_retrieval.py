"""GRU4Rec-style sequential retrieval, the model of the reference's examples/sequential_retrieval.py, on this project's
kernels: the query tower is Embedding(V + 1, d) -> GRU(d) (the table on K1 / K2, the input projection on krs_gemm, the
recurrence on K20: all steps in one launch), the candidate tower an Embedding(V + 1, d); the loss is the in-batch
softmax (scores = q c^T against eye(batch) through CategoricalCrossentropy(from_logits=True), or InBatchSoftmaxLoss
(K13) with --fused, which never stores the scores); serving is BruteForceRetrieval(k=10) (K8) over the candidate table.

Every example is a context of up to 10 items, right-padded with item 0, and the item that follows it.  As in the
reference the GRU reads the padding like any other item (its Embedding passes no mask).  Sequences are synthetic (sas_rec.synthetic_sequences' walk); nothing is downloaded.

    python examples/sequential_retrieval.py --steps 30 --dtype bf16 [--fused]
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.sas_rec import synthetic_sequences   # noqa: E402
from keras_rs_amd import layers as kl              # noqa: E402
from keras_rs_amd.layers import base               # noqa: E402

MAX_CONTEXT_LENGTH = 10


def synthetic_examples(count: int, vocabulary_size: int, length: int = MAX_CONTEXT_LENGTH, seed: int = 0):
    """context [count, length] int32, right-padded with 0, and label [count] int32: the item that follows the context
    in the walk.  vocabulary_size counts the real items 1 .. V (the tables have V + 1 rows)."""
    item_ids, positive, _, mask = synthetic_sequences(count, vocabulary_size + 1, length, seed)
    lengths = mask.sum(axis=1)
    context = np.zeros_like(item_ids)
    for row in range(count):                         # (left-padded -> right-padded, as the reference pads)
        context[row, :lengths[row]] = item_ids[row, length - lengths[row]:]
    return context.astype(np.int32), positive[:, -1].astype(np.int32)


class SequentialRetrievalModel(base.Layer):
    def __init__(self, movies_count: int, embedding_dimension: int = 32, k: int = 10, fused: bool = False,
                 **kwargs):
        super().__init__(**kwargs)
        sub = dict(dtype=self.dtype_policy, device=self._device)
        self.movies_count, self.embedding_dimension = movies_count, embedding_dimension
        self.fused = bool(fused)
        self.query_embedding = kl.Embedding(movies_count + 1, embedding_dimension, name="query_embedding", **sub)
        self.gru = kl.GRU(embedding_dimension, name="gru", **sub)
        self.candidate_model = kl.Embedding(movies_count + 1, embedding_dimension, name="candidate_embedding", **sub)
        self.retrieval = kl.BruteForceRetrieval(k=k, return_scores=False, device=self._device)
        self.loss_fn = kl.InBatchSoftmaxLoss() if fused else kl.CategoricalCrossentropy(from_logits=True)
        self.built = True

    def train_weights(self):
        """The query table, the GRU's kernel, recurrent_kernel and bias, the candidate table."""
        return self.query_embedding.weights + self.gru.weights + self.candidate_model.weights

    def query_model(self, context):
        x = self.query_embedding(context).to(self.compute_dtype)
        return self.gru(x)

    def call(self, inputs, training: bool = False):
        query_embeddings = self.query_model(inputs)
        result = {"query_embeddings": query_embeddings}
        if not training:
            table = self.candidate_model.weights[0].detach()
            ids = torch.arange(self.movies_count + 1, device=table.device, dtype=torch.int32)
            self.retrieval.update_candidates(table.to(self.compute_dtype), ids)
            result["predictions"] = self.retrieval(query_embeddings.detach())
        return result

    def compute_loss(self, y, y_pred):
        query_embeddings = y_pred["query_embeddings"]
        candidate_embeddings = self.candidate_model(y).to(query_embeddings.dtype)
        if self.fused:
            return self.loss_fn(query_embeddings, candidate_embeddings)
        scores = torch.matmul(query_embeddings, candidate_embeddings.transpose(0, 1))
        labels = torch.eye(scores.shape[0], scores.shape[1], dtype=torch.float32, device=scores.device)
        return self.loss_fn(labels, scores)


def main(steps: int = 30, batch: int = 4096, vocabulary_size: int = 3000, hidden_dim: int = 32,
         length: int = MAX_CONTEXT_LENGTH, dtype: str = "bf16", lr: float = 0.005, fused: bool = False,
         seed: int = 0, quiet: bool = False):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    policy = {"bf16": "mixed_bfloat16", "fp32": "float32"}[dtype]
    model = SequentialRetrievalModel(vocabulary_size, hidden_dim, fused=fused, dtype=policy, device=dev)
    context, label = (torch.from_numpy(a).to(dev) for a in synthetic_examples(batch, vocabulary_size, length, seed))
    model.compute_loss(label, model(context, training=True))                                      # (builds every weight)
    opt = torch.optim.AdamW(model.weights, lr=lr)
    initial = [w.detach().clone() for w in model.train_weights()]
    losses = []
    for step in range(steps):
        opt.zero_grad()
        loss = model.compute_loss(label, model(context, training=True))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if not quiet:
            print(f"step {step}: loss {losses[-1]:.4f}")
    with torch.no_grad():
        out = model(context, training=False)
    if not quiet:
        print("top-10 next items of the first users:", out["predictions"][:2].tolist())
    return {"losses": losses, "model": model, "context": context, "label": label, "outputs": out,
            "initial_weights": initial}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--vocabulary", type=int, default=3000)
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    main(steps=a.steps, batch=a.batch, vocabulary_size=a.vocabulary, hidden_dim=a.hidden, dtype=a.dtype, fused=a.fused)
