"""Sequence layers for the reference's sequential recommenders (examples/sas_rec.py): MultiHeadAttention and the
decoder-only TransformerDecoder block, on K19 (sequence_ops.seq_attention: the scores, the probabilities and the
dropout mask are never stored), krs_gemm (the projections and the feed-forward) and K22 (norm_ops.residual_layer_norm:
each residual add, its dropout and the layer norm that follows in one kernel; no dropout mask is stored either).
KRS_FUSE_NORM=0 (or FUSE_NORM = False here, read at every call) puts the torch composition back for A/B.
"""

from __future__ import annotations

import math
import os
from typing import Any

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import norm_ops, sequence_ops
from keras_rs_amd.autograd import DenseFn, _switch
from keras_rs_amd.layers import base
from keras_rs_amd.layers.dense import Dense

# 1: layer norm, the residual adds and the residual dropout run on K22; 0: the torch composition of before K22 (A/B)
FUSE_NORM = _switch(os.environ.get("KRS_FUSE_NORM", "1"))
# what the decoder adds to its seed for its two residual dropouts (the attention layer hashes the seed itself)
_ATTN_RESIDUAL_SEED, _FF_RESIDUAL_SEED = 0x5851F42D4C957F2D, 0x14057B7EF767814F


def _keras_fans_init(init: base.Initializer, shape) -> base.Initializer:
    """Keras counts the leading axes of a kernel of rank > 2 as a receptive field (fan_in = shape[-2] * rf, fan_out =
    shape[-1] * rf); base.VarianceScaling reads the last two axes.  Returns an initializer whose scale makes up the
    difference, so a [d, H, Dh] kernel is drawn with Keras' limits."""
    if not isinstance(init, base.VarianceScaling) or len(shape) <= 2:
        return base.clone_initializer(init)
    rf = math.prod(shape[:-2])
    pick = {"fan_in": lambda i, o: i, "fan_out": lambda i, o: o, "fan_avg": lambda i, o: (i + o) / 2.0}[init.mode]
    have, want = max(1.0, pick(shape[-2], shape[-1])), max(1.0, pick(shape[-2] * rf, shape[-1] * rf))
    return base.VarianceScaling(scale=init.scale * have / want, mode=init.mode, distribution=init.distribution,
                                seed=init.seed)


def _fresh_seed() -> int:
    # (from torch's default CPU generator, so torch.manual_seed reproduces a run)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class MultiHeadAttention(base.Layer):
    """keras.layers.MultiHeadAttention for self-attention over one sequence.  Weights, in Keras' order and shapes: query,
    key and value kernels [d, H, Dh] with biases [H, Dh], the output kernel [H, Dh, d] with bias [d].  The projections
    are krs_gemm calls on [B L, d] views; the attention itself is K19.  A query row with no allowed key (left padding
    under the causal mask) gives a zero attention output, where Keras averages over all keys (include/krs.h, K19).
    `seed` (an extension, Keras' own argument): the dropout mask is a hash of (seed, call number, position)."""

    def __init__(self, num_heads: int, key_dim: int, value_dim: int | None = None, dropout: float = 0.0,
                 use_bias: bool = True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 seed: int | None = None, **kwargs: Any):
        super().__init__(**kwargs)
        if int(num_heads) <= 0 or int(key_dim) <= 0:
            raise ValueError(f"`num_heads` and `key_dim` must be positive. Received: num_heads={num_heads}, key_dim={key_dim}")
        if value_dim is not None and int(value_dim) != int(key_dim):
            raise NotImplementedError(f"value_dim={value_dim} != key_dim={key_dim}: K19 has one head width")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"`dropout` must be in [0, 1). Received: dropout={dropout}")
        self.num_heads, self.key_dim, self.value_dim = int(num_heads), int(key_dim), value_dim
        self.dropout, self.use_bias = float(dropout), bool(use_bias)
        self.kernel_initializer = base.get_initializer(kernel_initializer)
        self.bias_initializer = base.get_initializer(bias_initializer)
        self.seed = _fresh_seed() if seed is None else int(seed)
        self._seed_given = seed
        for w in ("query_kernel", "query_bias", "key_kernel", "key_bias", "value_kernel", "value_bias", "output_kernel",
                  "output_bias"):
            self.register_parameter(w, None)
        self._draw = None

    def build(self, query_shape, *_) -> None:
        d, h, dh = int(query_shape[-1]), self.num_heads, self.key_dim
        for part in ("query", "key", "value"):
            setattr(self, f"{part}_kernel", self.add_weight((d, h, dh), _keras_fans_init(self.kernel_initializer, (d, h, dh)),
                                                            f"{part}_kernel"))
            if self.use_bias:
                setattr(self, f"{part}_bias", self.add_weight((h, dh), base.clone_initializer(self.bias_initializer),
                                                              f"{part}_bias", dtype=torch.float32))
        self.output_kernel = self.add_weight((h, dh, d), _keras_fans_init(self.kernel_initializer, (h, dh, d)),
                                             "output_kernel")
        if self.use_bias:
            self.output_bias = self.add_weight((d,), base.clone_initializer(self.bias_initializer), "output_bias",
                                               dtype=torch.float32)
        self.draw_counter()
        self.built = True

    def draw_counter(self) -> torch.Tensor:
        """The device int64 that numbers this layer's dropout masks; every training call advances it on the device."""
        if self._draw is None:
            self._draw = torch.zeros(1, dtype=torch.int64, device=self._device)
        return self._draw

    def call(self, query, value=None, key=None, *, attention_mask=None, padding_mask=None, use_causal_mask: bool = False,
             return_attention_scores: bool = False, training: bool = False):
        if attention_mask is not None:
            raise NotImplementedError("an arbitrary attention_mask is not supported: K19 takes a padding_mask [B, L] and "
                                      "use_causal_mask")
        if return_attention_scores:
            raise NotImplementedError("return_attention_scores: K19 never stores the attention scores")
        value = query if value is None else value
        key = value if key is None else key
        if query.dim() != 3 or value.dim() != 3 or key.dim() != 3:
            raise ValueError(f"MultiHeadAttention takes [B, L, d] inputs, got query {tuple(query.shape)}, value "
                             f"{tuple(value.shape)}, key {tuple(key.shape)}")
        if not (query.shape[1] == value.shape[1] == key.shape[1]):
            raise NotImplementedError(f"query length {query.shape[1]} and key / value lengths {key.shape[1]} / "
                                      f"{value.shape[1]} differ: K19 is self-attention over one sequence")
        L.require_device(query, "MultiHeadAttention query")
        b, l, d = query.shape
        h, dh = self.num_heads, self.key_dim
        hd = h * dh
        parts = []
        for x, kernel, bias in ((query, self.query_kernel, self.query_bias), (key, self.key_kernel, self.key_bias),
                                (value, self.value_kernel, self.value_bias)):
            y = DenseFn.apply(x.reshape(b * l, d), kernel.reshape(d, hd), None if bias is None else bias.reshape(hd),
                              L.ACT_NONE, self.compute_dtype, None, None, None)
            parts.append(y.view(b, l, h, dh))
        p = self.dropout if training else 0.0
        attn = sequence_ops.seq_attention(parts[0], parts[1], parts[2], key_valid=padding_mask, causal=use_causal_mask,
                                          scale=1.0 / math.sqrt(dh), dropout_p=p, seed=self.seed,
                                          draw=self.draw_counter() if p > 0.0 else None)
        out = DenseFn.apply(attn.reshape(b * l, hd), self.output_kernel.reshape(hd, d), self.output_bias, L.ACT_NONE,
                            self.compute_dtype, None, None, None)
        return out.view(b, l, d)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({
            "num_heads": self.num_heads, "key_dim": self.key_dim, "value_dim": self.value_dim, "dropout": self.dropout,
            "use_bias": self.use_bias, "kernel_initializer": self.kernel_initializer.serialize(),
            "bias_initializer": self.bias_initializer.serialize(), "seed": self._seed_given,
        })
        return config


class LayerNormalization(base.Layer):
    """keras.layers.LayerNormalization over the last axis: gamma (scale=True) and beta (center=True) in fp32, on K22.  An
    input K22 does not take (more than 4096 columns, a tensor off the device) keeps torch's arithmetic, in fp32."""

    def __init__(self, epsilon: float = 1e-3, *, axis=-1, center: bool = True, scale: bool = True,
                 rms_scaling: bool = False, gamma_initializer="ones", beta_initializer="zeros", **kwargs: Any):
        super().__init__(**kwargs)
        if isinstance(axis, (list, tuple)) and len(axis) == 1:
            axis = axis[0]
        if axis != -1:
            raise NotImplementedError(f"axis={axis}: K22 normalises the last axis only (axis=-1)")
        if rms_scaling:
            raise NotImplementedError("rms_scaling=True: K22 has no RMS norm")
        self.epsilon = float(epsilon)
        self.center, self.scale = bool(center), bool(scale)
        self.gamma_initializer = base.get_initializer(gamma_initializer)
        self.beta_initializer = base.get_initializer(beta_initializer)
        for w in ("gamma", "beta"):
            self.register_parameter(w, None)

    def build(self, input_shape, *_) -> None:
        d = int(input_shape[-1])
        if self.scale:
            self.gamma = self.add_weight((d,), base.clone_initializer(self.gamma_initializer), "gamma", dtype=torch.float32)
        if self.center:
            self.beta = self.add_weight((d,), base.clone_initializer(self.beta_initializer), "beta", dtype=torch.float32)
        self.built = True

    def call(self, x):
        xc = x.to(self.compute_dtype)
        if FUSE_NORM and norm_ops.supported(xc):
            return norm_ops.residual_layer_norm(xc, None, self.gamma, self.beta, epsilon=self.epsilon)
        y = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), self.gamma, self.beta, self.epsilon)
        return y.to(self.compute_dtype)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"epsilon": self.epsilon, "center": self.center, "scale": self.scale,
                       "gamma_initializer": self.gamma_initializer.serialize(),
                       "beta_initializer": self.beta_initializer.serialize()})
        return config


class TransformerDecoder(base.Layer):
    """The decoder-only form of keras_hub.layers.TransformerDecoder that the reference's SASRec stacks: causal
    self-attention with a padding mask, dropout, residual, layer norm; then Dense(intermediate_dim, activation),
    Dense(hidden), dropout, residual, layer norm.  normalize_first=True norms each sublayer's INPUT instead.
    key_dim = hidden // num_heads.  Weights: the attention's eight, its layer norm's gamma / beta, the two Dense
    layers' kernel / bias, the feed-forward layer norm's gamma / beta.
    Each `dropout, residual, layer norm` is one K22 call (post-norm: two launches for the block's glue; pre-norm: the
    norm form, K19, add-norm, the feed-forward, the add form).  The two residual dropouts hash the attention layer's
    `seed` plus two fixed offsets with one draw counter of the decoder's own; the attention keeps its counter."""

    def __init__(self, intermediate_dim: int, num_heads: int, dropout: float = 0.0, activation="relu",
                 layer_norm_epsilon: float = 1e-5, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 normalize_first: bool = False, seed: int | None = None, **kwargs: Any):
        super().__init__(**kwargs)
        self.intermediate_dim, self.num_heads = int(intermediate_dim), int(num_heads)
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"`dropout` must be in [0, 1). Received: dropout={dropout}")
        self.dropout = float(dropout)
        self.activation = base.get_activation(activation)
        self.layer_norm_epsilon = float(layer_norm_epsilon)
        self.kernel_initializer = base.get_initializer(kernel_initializer)
        self.bias_initializer = base.get_initializer(bias_initializer)
        self.normalize_first = bool(normalize_first)
        self._seed_given = seed
        self.self_attention = None
        self._draw = None

    def draw_counter(self) -> torch.Tensor:
        """The device int64 that numbers the residual dropout masks; each of the two advances it on the device."""
        if self._draw is None:
            self._draw = torch.zeros(1, dtype=torch.int64, device=self._device)
        return self._draw

    def build(self, decoder_sequence_shape, *_) -> None:
        hidden = int(decoder_sequence_shape[-1])
        if hidden % self.num_heads:
            raise ValueError(f"hidden size {hidden} is not a multiple of num_heads={self.num_heads}")
        sub = dict(dtype=self.dtype_policy, device=self._device)
        self.self_attention = MultiHeadAttention(self.num_heads, hidden // self.num_heads, dropout=self.dropout,
                                                 kernel_initializer=base.clone_initializer(self.kernel_initializer),
                                                 bias_initializer=base.clone_initializer(self.bias_initializer),
                                                 seed=self._seed_given, name=f"{self.name}_self_attention", **sub)
        self.self_attention_layer_norm = LayerNormalization(self.layer_norm_epsilon, name=f"{self.name}_self_attention_norm", **sub)
        self.feedforward_intermediate_dense = Dense(self.intermediate_dim, activation=self.activation,
                                                    kernel_initializer=base.clone_initializer(self.kernel_initializer),
                                                    bias_initializer=base.clone_initializer(self.bias_initializer),
                                                    name=f"{self.name}_ff_intermediate", **sub)
        self.feedforward_output_dense = Dense(hidden, kernel_initializer=base.clone_initializer(self.kernel_initializer),
                                              bias_initializer=base.clone_initializer(self.bias_initializer),
                                              name=f"{self.name}_ff_output", **sub)
        self.feedforward_layer_norm = LayerNormalization(self.layer_norm_epsilon, name=f"{self.name}_ff_norm", **sub)
        shape = tuple(decoder_sequence_shape)
        self.self_attention.build(shape)
        self.self_attention_layer_norm.build(shape)
        self.feedforward_intermediate_dense.build(shape)
        self.feedforward_output_dense.build(shape[:-1] + (self.intermediate_dim,))
        self.feedforward_layer_norm.build(shape)
        self.built = True

    def _drop(self, x, training):
        return torch.nn.functional.dropout(x, self.dropout, True) if training and self.dropout > 0.0 else x

    def call(self, decoder_sequence, encoder_sequence=None, decoder_padding_mask=None, training: bool = False):
        if encoder_sequence is not None:
            raise NotImplementedError("an encoder_sequence (cross-attention) is not supported: decoder-only blocks")
        x = decoder_sequence.to(self.compute_dtype)
        if FUSE_NORM and norm_ops.supported(x):
            return self._call_fused(x, decoder_padding_mask, training)
        residual = x
        if self.normalize_first:
            x = self.self_attention_layer_norm(x)
        x = self.self_attention(x, padding_mask=decoder_padding_mask, use_causal_mask=True, training=training)
        x = self._drop(x, training) + residual
        if not self.normalize_first:
            x = self.self_attention_layer_norm(x)
        residual = x
        if self.normalize_first:
            x = self.feedforward_layer_norm(x)
        x = self.feedforward_output_dense(self.feedforward_intermediate_dense(x))
        x = self._drop(x, training) + residual
        if not self.normalize_first:
            x = self.feedforward_layer_norm(x)
        return x

    def _call_fused(self, x, padding_mask, training):
        p = self.dropout if training else 0.0
        seed = self.self_attention.seed
        drop = lambda offset: dict(dropout_p=p, seed=seed + offset, draw=self.draw_counter() if p > 0.0 else None)
        attn_norm, ff_norm = self.self_attention_layer_norm, self.feedforward_layer_norm
        attend = lambda t: self.self_attention(t, padding_mask=padding_mask, use_causal_mask=True, training=training)
        feed = lambda t: self.feedforward_output_dense(self.feedforward_intermediate_dense(t))
        fused = norm_ops.residual_layer_norm
        if self.normalize_first:
            h = fused(x, None, attn_norm.gamma, attn_norm.beta, epsilon=attn_norm.epsilon)
            h, s = fused(attend(h), x, ff_norm.gamma, ff_norm.beta, epsilon=ff_norm.epsilon, return_sum=True,
                         **drop(_ATTN_RESIDUAL_SEED))
            return fused(feed(h), s, norm=False, epsilon=0.0, **drop(_FF_RESIDUAL_SEED))
        x = fused(attend(x), x, attn_norm.gamma, attn_norm.beta, epsilon=attn_norm.epsilon, **drop(_ATTN_RESIDUAL_SEED))
        return fused(feed(x), x, ff_norm.gamma, ff_norm.beta, epsilon=ff_norm.epsilon, **drop(_FF_RESIDUAL_SEED))

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({
            "intermediate_dim": self.intermediate_dim, "num_heads": self.num_heads, "dropout": self.dropout,
            "activation": base.serialize_activation(self.activation), "layer_norm_epsilon": self.layer_norm_epsilon,
            "kernel_initializer": self.kernel_initializer.serialize(),
            "bias_initializer": self.bias_initializer.serialize(), "normalize_first": self.normalize_first,
            "seed": self._seed_given,
        })
        return config
