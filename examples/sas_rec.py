"""SASRec (self-attentive sequential recommendation), the model of the reference's examples/sas_rec.py, on this
project's kernels: the item table on K1 / K2 (layers.Embedding), a learned position embedding, dropout,
N pre-norm TransformerDecoder blocks whose causal self-attention is K19 (the scores and the dropout mask are never
stored), whose projections and feed-forward are krs_gemm and whose layer norms, residual adds and residual dropout
are K22 (one fused kernel each), a final layer norm with epsilon 1e-8 (K22 too), and BruteForceRetrieval (K8) over the
item table for serving, on the last non-padding token.

Training follows the reference's compute_loss: positive and negative logits are row dot products of the sequence
embedding with the embedded positive / negative items, and the loss is the sample-weighted mean of the binary
cross-entropy with logits over the [B, 2 L] logits (a few element-wise torch ops).  The reference's L2 regulariser on
the item embeddings (0.001) is left out.  Sequences are synthetic (numpy.random.default_rng): every user walks the
item ids by a fixed map with a few random restarts, left-padded with item 0; nothing is downloaded.

    python examples/sas_rec.py --steps 30 --dtype bf16
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from keras_rs_amd import layers as kl              # noqa: E402
from keras_rs_amd.layers import base               # noqa: E402

PAD_ITEM_ID = 0


def synthetic_sequences(users: int, vocabulary_size: int, length: int, seed: int = 0):
    """item_ids, positive, negative [users, length] int32 and padding_mask [users, length] bool (True = a real token);
    sequences are left-padded.  The next item is (7 * item + 3) mod (V - 1) + 1, with a random restart now and then."""
    rng = np.random.default_rng(seed)
    v = vocabulary_size
    full = np.zeros((users, length + 1), dtype=np.int64)
    full[:, 0] = rng.integers(1, v, users)
    for t in range(1, length + 1):
        nxt = (7 * full[:, t - 1] + 3) % (v - 1) + 1
        restart = rng.random(users) < 0.05
        full[:, t] = np.where(restart, rng.integers(1, v, users), nxt)
    lengths = rng.integers(max(2, length // 2), length + 2, users)             # real tokens of full, 2 .. length + 1
    keep = np.arange(length + 1)[None, :] >= (length + 1 - lengths)[:, None]   # left padding
    full = np.where(keep, full, PAD_ITEM_ID)
    item_ids, positive = full[:, :-1], full[:, 1:]
    padding_mask = item_ids != PAD_ITEM_ID
    negative = rng.integers(1, v, positive.shape)
    negative = np.where(negative == positive, negative % (v - 1) + 1, negative)
    positive = np.where(padding_mask, positive, PAD_ITEM_ID)
    negative = np.where(padding_mask, negative, PAD_ITEM_ID)
    return (item_ids.astype(np.int32), positive.astype(np.int32), negative.astype(np.int32), padding_mask)


class SasRec(base.Layer):
    def __init__(self, vocabulary_size: int, num_layers: int, num_heads: int, hidden_dim: int, dropout: float = 0.0,
                 max_sequence_length: int = 100, k: int = 10, seed: int | None = None, **kwargs):
        super().__init__(**kwargs)
        sub = dict(dtype=self.dtype_policy, device=self._device)
        self.vocabulary_size, self.hidden_dim, self.dropout = vocabulary_size, hidden_dim, float(dropout)
        self.max_sequence_length = max_sequence_length
        self.item_embedding = kl.Embedding(vocabulary_size, hidden_dim, embeddings_initializer="glorot_uniform",
                                           name="item_embedding", **sub)
        self.position_embedding = self.add_weight((max_sequence_length, hidden_dim), "glorot_uniform", "position_embedding")
        self.transformer_layers = [                      # (a plain list: Layer.weights walks it, as Keras does)
            kl.TransformerDecoder(intermediate_dim=hidden_dim, num_heads=num_heads, dropout=dropout,
                                  layer_norm_epsilon=1e-5, activation="relu", kernel_initializer="glorot_uniform",
                                  normalize_first=True, seed=None if seed is None else seed + i,
                                  name=f"transformer_layer_{i}", **sub)
            for i in range(num_layers)]
        self.layer_norm = kl.LayerNormalization(1e-8, name="layer_norm", **sub)
        self.retrieval = kl.BruteForceRetrieval(k=k, return_scores=False, device=self._device)
        self.built = True

    def sequence_embedding(self, item_ids, padding_mask, training: bool = False):
        length = item_ids.shape[1]
        x = self.item_embedding(item_ids).to(self.compute_dtype)
        x = x + self.position_embedding[:length].to(self.compute_dtype)
        if training and self.dropout > 0.0:
            x = torch.nn.functional.dropout(x, self.dropout, True)
        for layer in self.transformer_layers:
            x = layer(x, decoder_padding_mask=padding_mask, training=training)
        return self.layer_norm(x)

    @staticmethod
    def last_non_padding_token(tensor, padding_mask):
        length = padding_mask.shape[1]
        pos = torch.arange(length, device=padding_mask.device).expand_as(padding_mask)
        last = torch.where(padding_mask, pos, torch.zeros_like(pos)).amax(dim=1)
        return tensor[torch.arange(tensor.shape[0], device=tensor.device), last]

    def call(self, inputs, training: bool = False):
        item_ids, padding_mask = inputs["item_ids"], inputs["padding_mask"]
        emb = self.sequence_embedding(item_ids, padding_mask, training)
        result = {"item_sequence_embedding": emb}
        if not training:
            table = self.item_embedding.weights[0].detach()
            ids = torch.arange(self.vocabulary_size, device=table.device, dtype=torch.int32)
            self.retrieval.update_candidates(table.to(self.compute_dtype), ids)
            result["predictions"] = self.retrieval(self.last_non_padding_token(emb, padding_mask).detach())
        return result

    def compute_loss(self, y, y_pred, sample_weight):
        emb = y_pred["item_sequence_embedding"].float()
        pos = self.item_embedding(y["positive_sequence"]).float()
        neg = self.item_embedding(y["negative_sequence"]).float()
        logits = torch.cat([(pos * emb).sum(-1), (neg * emb).sum(-1)], dim=1)                    # [B, 2 L]
        half = logits.shape[1] // 2
        labels = torch.cat([torch.ones_like(logits[:, :half]), torch.zeros_like(logits[:, half:])], dim=1)
        weight = torch.cat([sample_weight, sample_weight], dim=1).float()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels, reduction="none") * weight
        total = weight.sum()
        return torch.where(total > 0, loss.sum() / total.clamp_min(1e-30), torch.zeros_like(total))


def main(steps: int = 30, batch: int = 64, vocabulary_size: int = 500, length: int = 50, hidden_dim: int = 50,
         num_heads: int = 1, num_layers: int = 2, dropout: float = 0.2, dtype: str = "bf16", lr: float = 0.005,
         seed: int = 0, quiet: bool = False):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    policy = {"bf16": "mixed_bfloat16", "fp32": "float32"}[dtype]
    model = SasRec(vocabulary_size, num_layers, num_heads, hidden_dim, dropout=dropout, max_sequence_length=length,
                   seed=seed, dtype=policy, device=dev)
    item_ids, positive, negative, mask = (torch.from_numpy(a).to(dev) for a in
                                          synthetic_sequences(batch, vocabulary_size, length, seed))
    inputs = {"item_ids": item_ids, "padding_mask": mask}
    y = {"positive_sequence": positive, "negative_sequence": negative}
    model(inputs, training=True)                                                                  # (builds every weight)
    opt = torch.optim.Adam(model.weights, lr=lr, betas=(0.9, 0.98))
    losses = []
    for step in range(steps):
        opt.zero_grad()
        loss = model.compute_loss(y, model(inputs, training=True), mask)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if not quiet:
            print(f"step {step}: loss {losses[-1]:.4f}")
    with torch.no_grad():
        out = model(inputs, training=False)
    if not quiet:
        print("top-10 next items of the first users:", out["predictions"][:2].tolist())
    return {"losses": losses, "model": model, "inputs": inputs, "outputs": out}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--vocabulary", type=int, default=500)
    a = ap.parse_args()
    main(steps=a.steps, batch=a.batch, vocabulary_size=a.vocabulary, length=a.length, hidden_dim=a.hidden,
         num_heads=a.heads, num_layers=a.layers, dtype=a.dtype)
