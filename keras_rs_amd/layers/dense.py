"""Dense on MI355X: the counterpart of the keras.layers.Dense blocks around the hot path
(bottom / top MLP of the DLRM-DCN model, examples/ml_perf/model.py:105-163, 214-262; SURVEY.md
section 8f.3).  y = activation(x @ kernel + bias) runs as ONE krs_gemm launch with the bias +
activation epilogue; relu / sigmoid / tanh / linear are fused, any other callable is applied on the
host framework after a linear launch.
"""

from __future__ import annotations

from typing import Any

import torch

from keras_rs_amd import _lib as L
from keras_rs_amd.autograd import dense_layer
from keras_rs_amd.layers import base
from keras_rs_amd.layers.embed_reduce import (check_quantize_request, keep_fp32_steps, quantize_rows_checked,
                                               restore_fp32_steps)

_FUSED_ACTS = {None: L.ACT_NONE, base.linear: L.ACT_NONE, base.relu: L.ACT_RELU,
               base.sigmoid: L.ACT_SIGMOID, base.tanh: L.ACT_TANH}


def quantize_kernel(kernel: torch.Tensor, what: str):
    """(kernel_q [N, K] int8, kernel_step [N] fp32) of a Keras kernel [K, N]: one abs-max step per OUTPUT channel
    (keras' abs_max_quantize(kernel, axis=0)), stored transposed so that a channel is one K-contiguous row -- the rows
    of W^T through krs_quantize_rows_q8 (include/krs.h, K18).  A NaN or an infinity raises ValueError."""
    return quantize_rows_checked(kernel.detach().t().contiguous(), what)


def refuse_grad_input(layer, *inputs) -> None:
    """A quantized layer is inference only: an input that would carry a gradient is an error, not a silently cut graph."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in inputs):
        raise RuntimeError(f"{type(layer).__name__} '{layer.name}' is int8-quantized and serves inference only: its input "
                           "requires grad, and no gradient flows through a quantized layer.  Call it under "
                           "torch.no_grad() or detach the input.")


class Dense(base.Layer):
    """Args as keras.layers.Dense: units, activation, use_bias, kernel_initializer, bias_initializer
    (+ dtype / name).  Weights: kernel [input_dim, units], bias [units] (fp32).
    `quantize("int8")` turns the layer into its serving form (include/krs.h, K18): the kernel becomes the buffers
    kernel_q [units, input_dim] int8 / kernel_step [units] fp32, and a call quantizes its input per row and runs the int8
    product with the fused bias + activation."""

    def __init__(self, units: int, activation=None, use_bias: bool = True, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", **kwargs: Any):
        super().__init__(**kwargs)
        if int(units) <= 0:
            raise ValueError(f"`units` must be a positive integer. Received: units={units}")
        self.units = int(units)
        self.activation = base.get_activation(activation)
        self.use_bias = use_bias
        self.kernel_initializer = base.get_initializer(kernel_initializer)
        self.bias_initializer = base.get_initializer(bias_initializer)
        for w in ("kernel", "bias"):
            self.register_parameter(w, None)
        self.quantization_mode = None      # "int8" after quantize(): the kernel is two buffers, kernel_q / kernel_step

    def build(self, input_shape, *_) -> None:
        d = int(input_shape[-1])
        self.kernel = self.add_weight((d, self.units), base.clone_initializer(self.kernel_initializer), "kernel")
        if self.use_bias:
            self.bias = self.add_weight((self.units,), base.clone_initializer(self.bias_initializer), "bias",
                                        dtype=torch.float32)
        self.built = True

    # ---- int8 for inference (keras.layers.Dense.quantize("int8")) ------------------------------------------------------
    def quantize(self, mode: str = "int8") -> None:
        """Replaces the float kernel by int8 rows of its transpose and one fp32 step per unit and frees it: `weights`
        holds the bias only, state_dict() holds `kernel_q` / `kernel_step` (and loads into a layer quantized the same
        way), get_config() is unchanged.  Inference only: outputs do not require grad, an input that does is refused.  A
        kernel with a NaN or an infinity raises ValueError and leaves the layer as it was."""
        check_quantize_request(self, mode)
        q, step = quantize_kernel(self.kernel, f"{type(self).__name__} '{self.name}'")
        self.register_buffer("kernel_q", q, persistent=True)
        self.register_buffer("kernel_step", step, persistent=True)
        self.kernel = None
        self._weight_order[:] = [w for w in self._weight_order if w is self.bias]
        self.quantization_mode = mode

    def _apply(self, fn, recurse=True):
        """.to() / .bfloat16() / ...: the steps of a quantized kernel move with the module and stay fp32."""
        keep = keep_fp32_steps(self)
        out = super()._apply(fn, recurse)
        restore_fp32_steps(self, keep)
        return out

    def _call_quantized(self, x: torch.Tensor) -> torch.Tensor:
        from keras_rs_amd import dense_ops as D

        refuse_grad_input(self, x)
        lead, d = x.shape[:-1], x.shape[-1]
        if d != self.kernel_q.shape[1]:
            raise ValueError(f"Dense: input feature size {d} does not match the kernel "
                             f"{(self.kernel_q.shape[1], self.units)}")
        fused = self.activation in _FUSED_ACTS
        cd = self.compute_dtype
        with torch.no_grad():
            x2 = x.reshape(-1, d)
            if x2.dtype not in (torch.float32, torch.bfloat16):
                x2 = x2.to(cd)
            y, _ = D.gemm_q8(x2, self.kernel_q, self.kernel_step, bias=self.bias,
                             act=_FUSED_ACTS[self.activation] if fused else L.ACT_NONE, out_dtype=cd)
            if not fused:
                y = self.activation(y)
        return y.reshape(*lead, self.units)

    def call(self, x: torch.Tensor) -> torch.Tensor:
        L.require_device(x, "Dense input")
        if self.quantization_mode:
            return self._call_quantized(x)
        if x.shape[-1] != self.kernel.shape[0]:
            raise ValueError(f"Dense: input feature size {x.shape[-1]} does not match the kernel {tuple(self.kernel.shape)}")
        # (the hand-offs of the backward pass -- from a FeatureCross stack or another Dense layer below, to a Dense layer
        #  above -- are wired by autograd.dense_layer)
        if self.activation in _FUSED_ACTS:
            return dense_layer(x, self.kernel, self.bias, _FUSED_ACTS[self.activation], self.compute_dtype)
        return dense_layer(x, self.kernel, self.bias, L.ACT_NONE, self.compute_dtype, host_activation=self.activation)

    def compute_output_shape(self, input_shape):
        return tuple(input_shape[:-1]) + (self.units,)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({
            "units": self.units,
            "activation": base.serialize_activation(self.activation),
            "use_bias": self.use_bias,
            "kernel_initializer": self.kernel_initializer.serialize(),
            "bias_initializer": self.bias_initializer.serialize(),
        })
        return config
