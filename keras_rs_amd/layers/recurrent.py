"""Recurrent layers for the reference's sequential recommenders (examples/sequential_retrieval.py): GRU, on K20
(recurrent_ops.gru: all steps of the recurrence in one launch) and krs_gemm (the input projection, a DenseFn call on
the [B L, D] view).
"""

from __future__ import annotations

from typing import Any

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import recurrent_ops
from keras_rs_amd.autograd import DenseFn
from keras_rs_amd.layers import base


class GRU(base.Layer):
    """keras.layers.GRU with its defaults (reset_after=True, tanh, sigmoid).  Weights, in Keras' order and shapes and
    gate order z, r, h: kernel [D, 3 units], recurrent_kernel [units, 3 units], bias [2, 3 units] (row 0 the input
    bias, row 1 the recurrent bias; fp32).  call(sequences [B, L, D], initial_state [B, units], mask [B, L]) returns the
    last output [B, units], or the sequence output [B, L, units] with return_sequences; with return_state a pair
    (output, final state).  A masked step carries the state and repeats the previous output (zeros before the first
    valid step), as Keras' backend rnn does (include/krs.h, K20)."""

    def __init__(self, units: int, activation="tanh", recurrent_activation="sigmoid", use_bias: bool = True,
                 kernel_initializer="glorot_uniform", recurrent_initializer="orthogonal", bias_initializer="zeros",
                 dropout: float = 0.0, recurrent_dropout: float = 0.0, return_sequences: bool = False,
                 return_state: bool = False, go_backwards: bool = False, stateful: bool = False, unroll: bool = False,
                 reset_after: bool = True, **kwargs: Any):
        super().__init__(**kwargs)
        if int(units) <= 0:
            raise ValueError(f"`units` must be a positive integer. Received: units={units}")
        if not reset_after:
            raise NotImplementedError("reset_after=False is not supported: K20 applies the reset gate after the recurrent "
                                      "product (Keras' default and the cuDNN-compatible form)")
        if base.get_activation(activation) is not base.tanh:
            raise NotImplementedError(f"activation={activation!r} is not supported: K20 fuses tanh")
        if base.get_activation(recurrent_activation) is not base.sigmoid:
            raise NotImplementedError(f"recurrent_activation={recurrent_activation!r} is not supported: K20 fuses sigmoid")
        if float(dropout) != 0.0:
            raise NotImplementedError(f"dropout={dropout} is not supported: K20 has no input dropout mask")
        if float(recurrent_dropout) != 0.0:
            raise NotImplementedError(f"recurrent_dropout={recurrent_dropout} is not supported: K20 has no mask on the "
                                      "carried state")
        if go_backwards:
            raise NotImplementedError("go_backwards=True is not supported: K20 walks t = 0 .. L - 1")
        if stateful:
            raise NotImplementedError("stateful=True is not supported: pass the previous call's state as initial_state")
        if unroll:
            raise NotImplementedError("unroll=True is not supported: K20 is one launch for all steps already")
        self.units = int(units)
        self.activation, self.recurrent_activation = base.tanh, base.sigmoid
        self.use_bias = bool(use_bias)
        self.kernel_initializer = base.get_initializer(kernel_initializer)
        self.recurrent_initializer = base.get_initializer(recurrent_initializer)
        self.bias_initializer = base.get_initializer(bias_initializer)
        self.return_sequences, self.return_state = bool(return_sequences), bool(return_state)
        for w in ("kernel", "recurrent_kernel", "bias"):
            self.register_parameter(w, None)

    def build(self, sequences_shape, *_) -> None:
        d, u = int(sequences_shape[-1]), self.units
        self.kernel = self.add_weight((d, 3 * u), base.clone_initializer(self.kernel_initializer), "kernel")
        self.recurrent_kernel = self.add_weight((u, 3 * u), base.clone_initializer(self.recurrent_initializer),
                                                "recurrent_kernel")
        if self.use_bias:
            self.bias = self.add_weight((2, 3 * u), base.clone_initializer(self.bias_initializer), "bias",
                                        dtype=torch.float32)
        self.built = True

    def call(self, sequences, initial_state=None, mask=None, training: bool = False):
        if sequences.dim() != 3:
            raise ValueError(f"GRU takes [B, L, D] sequences, got {tuple(sequences.shape)}")
        L.require_device(sequences, "GRU sequences")
        b, l, d = sequences.shape
        if d != self.kernel.shape[0]:
            raise ValueError(f"GRU: input feature size {d} does not match the kernel {tuple(self.kernel.shape)}")
        if isinstance(initial_state, (list, tuple)):
            (initial_state,) = initial_state
        u = self.units
        xz = DenseFn.apply(sequences.reshape(b * l, d), self.kernel, None if self.bias is None else self.bias[0],
                           L.ACT_NONE, self.compute_dtype, None, None, None)
        out, state = recurrent_ops.gru(xz.view(b, l, 3 * u), self.recurrent_kernel,
                                       None if self.bias is None else self.bias[1], mask=mask,
                                       initial_state=initial_state, return_sequences=self.return_sequences)
        return (out, state) if self.return_state else out

    def compute_output_shape(self, sequences_shape):
        b, l = sequences_shape[0], sequences_shape[1]
        return (b, l, self.units) if self.return_sequences else (b, self.units)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({
            "units": self.units, "activation": base.serialize_activation(self.activation),
            "recurrent_activation": base.serialize_activation(self.recurrent_activation), "use_bias": self.use_bias,
            "kernel_initializer": self.kernel_initializer.serialize(),
            "recurrent_initializer": self.recurrent_initializer.serialize(),
            "bias_initializer": self.bias_initializer.serialize(), "dropout": 0.0, "recurrent_dropout": 0.0,
            "return_sequences": self.return_sequences, "return_state": self.return_state, "go_backwards": False,
            "stateful": False, "unroll": False, "reset_after": True,
        })
        return config
