"""HSTU as a sequential retriever: a stack of HSTUBlock over item embeddings (no position embedding: the blocks carry a
relative-position bias), trained with the sampled softmax over shared negatives (K30) on synthetic sequences and scored
with FactorizedTopK.

    python examples/hstu.py [--steps 30] [--stored]

--stored runs the attention as the torch composition that stores the [B, H, L, L] scores, for A/B against K31.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.sas_rec import SasRec, synthetic_sequences   # noqa: E402
from keras_rs_amd import layers as kl                        # noqa: E402
from keras_rs_amd.layers import base                         # noqa: E402


class Hstu(base.Layer):
    def __init__(self, vocabulary_size: int, num_layers: int, num_heads: int, hidden_dim: int, max_length: int,
                 dropout: float = 0.0, seed: int | None = None, **kwargs):
        super().__init__(**kwargs)
        sub = dict(dtype=self.dtype_policy, device=self._device)
        self.item_embedding = kl.Embedding(vocabulary_size, hidden_dim, embeddings_initializer="glorot_uniform",
                                           name="item_embedding", **sub)
        self.blocks = [kl.HSTUBlock(num_heads, hidden_dim // num_heads, max_length, dropout=dropout,
                                    seed=None if seed is None else seed + i, name=f"hstu_block_{i}", **sub)
                       for i in range(num_layers)]
        self.loss = kl.SampledSoftmaxCrossentropy()
        self.built = True

    def call(self, item_ids, padding_mask, training: bool = False):
        x = self.item_embedding(item_ids).to(self.compute_dtype)
        for block in self.blocks:
            x = block(x, padding_mask=padding_mask, training=training)
        return x


def main(steps: int = 30, batch: int = 64, vocabulary_size: int = 500, length: int = 50, hidden_dim: int = 64,
         num_heads: int = 2, num_layers: int = 2, dropout: float = 0.2, dtype: str = "bf16", lr: float = 0.005,
         seed: int = 0, quiet: bool = False, stored: bool = False, shared_negatives: int = 128):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(seed)
    model = Hstu(vocabulary_size, num_layers, num_heads, hidden_dim, length, dropout=dropout, seed=seed,
                 dtype={"bf16": "mixed_bfloat16", "fp32": "float32"}[dtype], device=dev)
    for block in model.blocks:
        block.stored_attention = stored
    item_ids, positive, _, mask = (torch.from_numpy(a).to(dev) for a in synthetic_sequences(batch, vocabulary_size, length, seed))
    gen = torch.Generator().manual_seed(seed)
    negatives = torch.randint(1, vocabulary_size, (batch, shared_negatives), generator=gen, dtype=torch.int32).to(dev)
    model(item_ids, mask, training=True)                                                          # (builds every weight)
    opt = torch.optim.Adam(model.weights, lr=lr, betas=(0.9, 0.98))
    losses = []
    for step in range(steps):
        opt.zero_grad()
        loss = model.loss(model.item_embedding, model(item_ids, mask, training=True), positive, negatives, mask)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if not quiet:
            print(f"step {step}: loss {losses[-1]:.4f}")
    with torch.no_grad():
        emb = model(item_ids, mask, training=False)
        table = model.item_embedding.weights[0].detach().to(emb.dtype)
        metric = kl.FactorizedTopK(candidate_embeddings=table, ks=(1, 10))
        metric.update_state(SasRec.last_non_padding_token(emb, mask), SasRec.last_non_padding_token(positive, mask).long())
        result = {k: float(v) for k, v in metric.result().items()}
    if not quiet:
        print("next-item metrics on the training sequences:", result)
    return {"losses": losses, "metrics": result, "model": model}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--stored", action="store_true", help="the torch composition of the attention, for A/B")
    a = ap.parse_args()
    main(steps=a.steps, batch=a.batch, dtype=a.dtype, length=a.length, stored=a.stored)
