"""What the backward hand-offs of keras_rs_amd.autograd pass from one layer's Function to the next: the three relays
(mutable, one per layer output) and the immutable records a forward or a backward leaves on them.  No logic lives here
but `Handoff.is_gradient`, the one check that decides whether a hand-off may be taken."""

from __future__ import annotations

from typing import Any, NamedTuple

import torch


def graph_task() -> int:
    """Id of the backward pass that is running on this thread; -1 outside one (a backward called directly)."""
    return torch._C._current_graph_task_id()


class CrossLower(NamedTuple):
    """Left by a cross layer's forward for the consumer of its output y: what that consumer needs to run THIS layer's
    elementwise backward inside its own data-gradient product (krs_gemm_cross_bwd)."""
    u: torch.Tensor            # the saved activation output
    act: int
    diag_scale: float
    has_bias: bool
    x_is_x0: bool
    x0c: torch.Tensor          # x0 in the compute dtype
    below: Any                 # Dx0Relay of the layer that produced this layer's x | None
    x_dtype: torch.dtype       # dtype of that x


class DenseLower(NamedTuple):
    """Left by a Dense layer's forward for the consumer of its output.  (No tensor: the output holds the relay as an
    attribute, a reference back would be a cycle that only the cyclic collector frees; the upper layer has that output
    anyway -- it is its saved input.)"""
    act: int
    has_bias: bool


class Handoff(NamedTuple):
    """Left by a consumer's backward when its data-gradient product G = dL/dy ran the elementwise backward of the layer
    that produced y: dz and dbias of that layer are done.  On a Dx0Relay `buf` then already holds that layer's term of
    dL/dx0 as well, unless `deferred`: then that layer's own data-gradient product computes it (u_upper) and no matrix
    exists yet."""
    g: torch.Tensor
    g_version: int
    dz: torch.Tensor
    dbias: torch.Tensor | None
    task: int
    deferred: bool = False

    def is_gradient(self, g: torch.Tensor, task: int) -> bool:
        """Is `g`, handed over by autograd in pass `task`, that G, untouched?  (The relay keeps G alive, so its memory
        cannot be reused meanwhile; a second consumer's gradient summed in is a new tensor, or in place: the version
        moves; a hook's replacement is a new tensor.)"""
        G = self.g
        return (self.task == task and g.data_ptr() == G.data_ptr() and g.shape == G.shape and g.stride() == G.stride()
                and g.dtype == G.dtype and g._version == self.g_version)


class Dx0Relay:
    """Carries dL/dx0 down a stack of cross layers that share x0 (`xl = layer(x0, xl)` repeated,
    examples/ml_perf/model.py:332-336).  Every layer of the stack contributes a [B, d] term to dL/dx0;
    left to autograd these are summed by separate elementwise adds (1.4 GB of traffic each at C3).
    Instead the layer whose backward runs first writes its term into a buffer and leaves it here, on the
    relay it shares with the layer that produced its `x`; that layer's backward -- which autograd is bound
    to run next on this path, since it is handed dL/dx -- accumulates into the buffer inside its
    elementwise kernel (`dx0_accumulate` of krs_cross_epilogue_bwd) and passes it on, and the bottom layer
    of the stack returns the total.  `task` is the autograd graph-task id of the pass that filled `buf`:
    a buffer left over from another backward pass is ignored."""

    __slots__ = ("x0", "buf", "task", "lower", "fused")

    def __init__(self, x0: torch.Tensor):
        self.x0, self.buf, self.task = x0, None, -1
        # lower: CrossLower, left by this layer's forward;
        # fused: Handoff, left by the backward of the consumer of y when it ran this layer's elementwise backward
        self.lower, self.fused = None, None

    def matches(self, x0: torch.Tensor) -> bool:
        a = self.x0
        return (a.data_ptr() == x0.data_ptr() and a.shape == x0.shape and a.stride() == x0.stride()
                and a.dtype == x0.dtype and a._version == x0._version)


class DenseActRelay:
    """Hand-off between two STACKED Dense layers (examples/ml_perf/model.py:214-262: `x = dense(x)` repeated): the upper
    layer's data-gradient product G = dz K^T is the lower layer's dL/dy, and the lower layer's first backward step --
    dz_low = dL/dy * act'(y_low), dbias_low = column sums -- rides in that product's epilogue (krs_gemm_cross_bwd, dense
    form): dL/dy is not read back for it.
      lower  DenseLower of the layer whose output carries this relay -- set by its forward;
      fused  Handoff -- set by the upper layer's backward, taken by the lower one's.
    What autograd receives from the upper layer is G itself, the true dL/dy, so everything that observes the output's
    gradient -- autograd.grad / backward(inputs=...) captures, tensor and node hooks, retain_grad -- sees the right value.
    The lower backward takes dz_low and dbias_low only when what it is handed IS that G, untouched (Handoff.is_gradient);
    anything else -- a second consumer's gradient summed in, a hook's replacement or in-place change -- goes through its
    own derivative.
      out_ref  weak reference to that output (`_dense_fusable_below`: one that retains its .grad is not fused)."""

    __slots__ = ("lower", "fused", "out_ref")

    def __init__(self):
        self.lower, self.fused, self.out_ref = None, None, None


class SlabGradRelay:
    """Lets the gradient of DotInteraction join the gradient of the concat of the same features inside the
    DotInteraction backward kernel instead of in a separate 1.4 GB add.  `layers.concat_features([dense,
    *embeddings])` returns the lookup slab itself, so the gradient of the concat IS the gradient of the slab: its
    backward (SlabFillFn) leaves that matrix here; when DotInteraction's backward runs later in the same pass --
    it does whenever the interaction was called before the concat, as in a DLRM forward -- and its trailing
    inputs are exactly the slab's feature views, it adds their gradients into the matrix
    (krs_dot_interaction_bwd_accumulate) and returns no gradient for them.  The leading inputs (the bottom-MLP
    output) keep their ordinary gradient tensors, so whatever else consumes them is unaffected.  Not used when
    the concat result is still referenced and retains its gradient or has hooks (its .grad would show the joined
    value), nor when one of the slab's feature views does (it would see no gradient from the interaction), nor once
    the slab has a second consumer (a second concat of the same features).  Known limit: a gradient of the concat
    result CAPTURED by torch.autograd.grad(..., inputs=[concat_out]) is the very tensor the interaction adds into,
    so it shows the joined value (the engine exposes no way to see a capture from inside a backward)."""

    __slots__ = ("buf", "task", "out_ref", "disabled")
    joined = 0   # times the in-kernel path was taken (read by the tests)

    def __init__(self):
        self.buf, self.task, self.out_ref = None, -1, None
        # set when the slab got a second consumer (a second concat of the same features): autograd then sums the two
        # gradients of the slab in a buffer of its own, and an in-place add into the first one could be lost
        self.disabled = False
