"""HSTUBlock: the sequential-transduction block of "Actions Speak Louder than Words" (Zhai et al., ICML 2024) on K31
(sequence_ops.hstu_attention: SiLU attention with a relative-position bias, nothing of size L x L stored), krs_gemm (the
two projections) and K22 (both layer norms and the residual add with its dropout).

    U, V, Q, K = split(silu(f1(LayerNorm(x))))                  f1: d -> 4 H Dh, one product
    attn       = hstu_attention(Q, K, V, position table, padding mask, causal)
    y          = x + dropout(f2(LayerNorm(attn) * U))           f2: H Dh -> d
"""

from __future__ import annotations

import math
from typing import Any

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import norm_ops, sequence_ops
from keras_rs_amd.autograd import DenseFn
from keras_rs_amd.layers import base
from keras_rs_amd.layers.sequence import _fresh_seed

_POSITION_BIAS = ("shared", "per_head", None)


class HSTUBlock(base.Layer):
    """One HSTU block over [B, L, d] with L <= max_length.  Weights, in order: the input norm's gamma / beta [d], f1's
    kernel [d, 4 H Dh] and bias, the position table [1 ("shared") or H ("per_head"), 2 max_length - 1] in fp32 (absent
    with position_bias=None), the attention norm's gamma / beta [H Dh], f2's kernel [H Dh, d] and bias.  Q, K and V go to
    the kernel as column slices of silu(f1(.)), in place.  A shorter input reads the centred window of the table: entry
    max_length - 1 is offset 0 at every length.  Scores are scaled by 1 / sqrt(Dh) and weights by 1 / L, the padded
    length.  `padding_mask` [B, L] (truthy = a token) masks padded queries and keys; attention is causal.  Dropout sits
    on the block output: a hash of (seed, call number, position), as K22's."""

    def __init__(self, num_heads: int, key_dim: int, max_length: int, *, position_bias: str | None = "shared",
                 dropout: float = 0.0, epsilon: float = 1e-6, seed: int | None = None, **kwargs: Any):
        super().__init__(**kwargs)
        for name, value in (("num_heads", num_heads), ("key_dim", key_dim), ("max_length", max_length)):
            if int(value) <= 0:
                raise ValueError(f"`{name}` must be positive. Received: {name}={value}")
        if position_bias not in _POSITION_BIAS:
            raise ValueError(f"`position_bias` must be one of {_POSITION_BIAS}. Received: position_bias={position_bias!r}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"`dropout` must be in [0, 1). Received: dropout={dropout}")
        if int(max_length) > 4096 or int(key_dim) > 256:
            raise ValueError(f"K31 takes max_length <= 4096 and key_dim <= 256. Received: max_length={max_length}, "
                             f"key_dim={key_dim}")
        self.num_heads, self.key_dim, self.max_length = int(num_heads), int(key_dim), int(max_length)
        self.position_bias, self.dropout, self.epsilon = position_bias, float(dropout), float(epsilon)
        self.seed = _fresh_seed() if seed is None else int(seed)
        self._seed_given = seed
        self.stored_attention = False      # True: the torch composition that stores the scores, for A/B runs only
        for w in ("norm_gamma", "norm_beta", "f1_kernel", "f1_bias", "position_table", "attn_norm_gamma", "attn_norm_beta",
                  "f2_kernel", "f2_bias"):
            self.register_parameter(w, None)
        self._draw = None

    def build(self, input_shape, *_) -> None:
        d, hd = int(input_shape[-1]), self.num_heads * self.key_dim
        f32 = dict(dtype=torch.float32)
        self.norm_gamma = self.add_weight((d,), "ones", "norm_gamma", **f32)
        self.norm_beta = self.add_weight((d,), "zeros", "norm_beta", **f32)
        self.f1_kernel = self.add_weight((d, 4 * hd), "glorot_uniform", "f1_kernel")
        self.f1_bias = self.add_weight((4 * hd,), "zeros", "f1_bias", **f32)
        if self.position_bias is not None:
            rows = 1 if self.position_bias == "shared" else self.num_heads
            self.position_table = self.add_weight((rows, 2 * self.max_length - 1), "zeros", "position_table", **f32)
        self.attn_norm_gamma = self.add_weight((hd,), "ones", "attn_norm_gamma", **f32)
        self.attn_norm_beta = self.add_weight((hd,), "zeros", "attn_norm_beta", **f32)
        self.f2_kernel = self.add_weight((hd, d), "glorot_uniform", "f2_kernel")
        self.f2_bias = self.add_weight((d,), "zeros", "f2_bias", **f32)
        self.built = True

    def draw_counter(self) -> torch.Tensor:
        """The device int64 that numbers the output dropout masks; every training call advances it on the device."""
        if self._draw is None:
            self._draw = torch.zeros(1, dtype=torch.int64, device=self._device)
        return self._draw

    def call(self, x, padding_mask=None, training: bool = False):
        if x.dim() != 3:
            raise ValueError(f"HSTUBlock takes a [B, L, d] input, got shape {tuple(x.shape)}")
        b, l, d = x.shape
        if l > self.max_length:
            raise ValueError(f"input length {l} exceeds max_length={self.max_length}")
        L.require_device(x, "HSTUBlock input")
        h, dh = self.num_heads, self.key_dim
        hd = h * dh
        xc = x.to(self.compute_dtype)
        n = norm_ops.residual_layer_norm(xc, None, self.norm_gamma, self.norm_beta, epsilon=self.epsilon)
        p = DenseFn.apply(n.reshape(b * l, d), self.f1_kernel, self.f1_bias, L.ACT_NONE, self.compute_dtype, None, None, None)
        p = torch.nn.functional.silu(p).view(b, l, 4, h, dh)
        u, v, q, k = p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3]
        pos = None
        if self.position_table is not None:
            m = self.max_length
            pos = self.position_table[:, m - l:m + l - 1]
        attend = sequence_ops.hstu_attention_stored if self.stored_attention else sequence_ops.hstu_attention
        attn = attend(q, k, v, pos_bias=pos, valid=padding_mask, causal=True, alpha=1.0 / math.sqrt(dh), inv_n=1.0 / l)
        a = norm_ops.residual_layer_norm(attn.reshape(b, l, hd), None, self.attn_norm_gamma, self.attn_norm_beta,
                                         epsilon=self.epsilon)
        y = DenseFn.apply((a * u.reshape(b, l, hd)).reshape(b * l, hd), self.f2_kernel, self.f2_bias, L.ACT_NONE,
                          self.compute_dtype, None, None, None)
        drop = self.dropout if training else 0.0
        return norm_ops.residual_layer_norm(y.view(b, l, d), xc, norm=False, epsilon=0.0, dropout_p=drop, seed=self.seed,
                                            draw=self.draw_counter() if drop > 0.0 else None)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"num_heads": self.num_heads, "key_dim": self.key_dim, "max_length": self.max_length,
                       "position_bias": self.position_bias, "dropout": self.dropout, "epsilon": self.epsilon,
                       "seed": self._seed_given})
        return config
