"""Host code on the step path that DistributedEmbedding and ShardedDistributedEmbedding share: fusing a call's inputs
into one feature-major id buffer per group, the out-of-range-id flag word, and counting a fused update."""

from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import graphs
from keras_rs_amd.embedding_ops import StepConstants
from keras_rs_amd.layers import base
from keras_rs_amd.layers.embed_reduce import Ragged


# ---- preprocess: concatenate a group's features feature-major into one buffer ------------------------
def fuse_group_inputs(paths, combiner_of, inputs: dict, weights: dict | None, device, offsets_dtype) -> dict:
    """One group's fused inputs: `ids` (flat, feature-major, int64 when any feature's are), `offsets` (CSR of
    `offsets_dtype` over all bags when any feature is ragged, else None), `hots` (ids per bag of every feature, None
    when ragged), `batch` and `weights` (fp32, flat like `ids`; None without weights).  `combiner_of`: path -> combiner."""
    id_parts, w_parts, hots, lens = [], [], [], []
    ragged = False
    batch = None
    for path in paths:
        x = inputs[path]
        w = None if weights is None else weights.get(path)
        x, w = _ragged_numpy_to_csr(x, w)
        if isinstance(x, Ragged):
            ragged = True
            vals = _to_tensor(x.values)
            offs = np.asarray(_to_numpy(x.row_offsets), dtype=np.int64)
            b = len(offs) - 1
            id_parts.append(vals.reshape(-1))
            lens.append(np.diff(offs))
            hots.append(None)
            if w is not None:
                w_parts.append(_to_tensor(w.values if isinstance(w, Ragged) else w).reshape(-1))
        else:
            t = _to_tensor(x)
            if t.dim() == 1:
                # rank-1: no reduction; weights only survive for "sum" (embed_reduce.py:224)
                if combiner_of(path) != "sum":
                    w = None if w is None else torch.ones(t.shape, device=t.device)
                t = t.reshape(-1, 1)
            elif t.dim() != 2:
                raise ValueError(f"Feature '{path}': inputs must be rank 1 or 2, got {tuple(t.shape)}")
            b = t.shape[0]
            id_parts.append(t.reshape(-1))
            hots.append(int(t.shape[1]))
            lens.append(np.full(b, t.shape[1], dtype=np.int64))
            if w is not None:
                wt = _to_tensor(w).float()
                if wt.numel() != t.numel():
                    raise ValueError(f"Feature '{path}': weights shape {tuple(wt.shape)} does not match "
                                     f"inputs shape {tuple(t.shape)}")
                w_parts.append(wt.reshape(-1))
        if batch is None:
            batch = b
        elif batch != b:
            raise ValueError("All features of a DistributedEmbedding call must share the batch size")
    ids = _cat_index(id_parts).to(device, non_blocking=True)
    offsets = None
    if ragged:
        offsets = torch.from_numpy(
            np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(offsets_dtype)).to(device, non_blocking=True)
    w = None
    if weights is not None:
        if len(w_parts) != len(paths):
            raise ValueError("weights must be given for every feature or for none")
        w = torch.cat([p.reshape(-1) for p in w_parts]).float().to(device, non_blocking=True)
    return {"ids": ids, "offsets": offsets, "hots": None if ragged else tuple(hots), "batch": batch, "weights": w}


def _to_numpy(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _to_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    if hasattr(x, "numpy") and callable(x.numpy):
        x = x.numpy()
    return torch.from_numpy(np.ascontiguousarray(x))


def _cat_index(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    dt = torch.int64 if any(p.dtype == torch.int64 for p in parts) else torch.int32
    parts = [p.to(dt) for p in parts]
    if all(p.device.type == "cpu" for p in parts) and torch.cuda.is_available():
        # host ids: concatenate straight into page-locked memory, so that the upload that follows is a
        # true asynchronous DMA (the loader threads of data.ThreadedDataLoader overlap it with compute)
        buf = torch.empty(sum(p.numel() for p in parts), dtype=dt, pin_memory=True)
        return torch.cat(parts, out=buf) if len(parts) > 1 else buf.copy_(parts[0].reshape(-1))
    return torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()


def _ragged_numpy_to_csr(x, w):
    """numpy object arrays of rows (the ragged form of base:31-92) -> Ragged CSR.
    Results equal the reference's pad-to-dense form (padding carries weight 0)."""
    if isinstance(x, np.ndarray) and x.dtype == object and len(x) > 0:
        rx = Ragged.from_rows(list(x), dtype=np.asarray(x[0]).dtype if np.asarray(x[0]).dtype.kind == "i" else np.int32)
        rw = None
        if w is not None:
            rw = Ragged(Ragged.from_rows(list(w), dtype=np.float32).values, rx.row_offsets)
        return rx, rw
    return x, w


# ---- out-of-range ids: flagged by the kernels, raised lazily (no per-step host sync) ------------------
class IdRangeCheck:
    """The word the lookup kernels OR their KRS_FLAG_* bits into, and its lazy check on the host."""

    def __init__(self, message: str):
        self.message = message    # of the IndexError
        self.dev = None           # device int32[1]
        self.host = None          # its page-locked mirror, refreshed asynchronously after every call
        self.event = None         # recorded behind the latest eager refresh
        self.in_graph = False     # the refresh is a node of a captured step: there is no event to poll

    def flag(self, device) -> torch.Tensor | None:
        if device.type != "cuda":
            return None
        if self.dev is None:
            self.dev = torch.zeros(1, dtype=torch.int32, device=device)
            self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        return self.dev

    def snapshot(self) -> None:
        """Queues a copy of the error word into page-locked memory behind the lookups just launched."""
        if self.dev is not None:
            self.host.copy_(self.dev, non_blocking=True)
            if base.stream_capturing():
                # inside a graph the copy is a node of every replay; there is no event to poll: check(wait=True)
                # between replays waits for the device instead
                self.event, self.in_graph = None, True
                return
            self.event = torch.cuda.Event()
            self.event.record()

    def check(self, wait: bool = False) -> None:
        """Raises IndexError if a snapshot that has arrived (wait=True: the latest one) carries the flag."""
        if base.stream_capturing():
            return
        ev = self.event
        if ev is None:
            if not (wait and self.in_graph):
                return
            torch.cuda.current_stream(self.dev.device).synchronize()   # replays of a captured step
        elif wait:
            ev.synchronize()
        elif not ev.query():
            return
        self.event = None
        if int(self.host.item()) & L.FLAG_ID_OUT_OF_RANGE:
            self.dev.zero_()
            self.host.zero_()
            raise IndexError(self.message)

    def reset(self) -> None:
        """The module moved (.to() / .cuda()): the word is allocated again on first use."""
        self.dev = self.host = self.event = None
        self.in_graph = False


# ---- one fused update: count it, refresh the constants that depend on the count ----------------------
def next_fused_hyper(owner, fused, table_opts, bags_of):
    """Called once per fused update of `owner` (a group: `step` count, `_constants` field), from the backward pass: counts
    the update, refreshes the constants that depend on the count -- scheduled learning rates (in the kernel descriptors of
    `bags_of()`) and Adam's bias correction, both kept in DEVICE memory (embedding_ops.StepConstants) -- and returns the
    Adam / FTRL constants of `fused` (None for SGD / Adagrad).  `table_opts`: per table, the FusedOptimizer holding its
    learning rate.  While a stream is capturing nothing is counted or written: GraphedStep does that before every replay."""
    scheduled = bool(table_opts) and any(callable(o.lr) for o in table_opts)
    adam = fused.kind == "adam"
    if not scheduled and not adam:
        graphs.count_update(owner)      # (per replay under GraphedStep)
        return fused.hyper(owner.step)
    if owner._constants is None:
        owner._constants = StepConstants(
            owner, bags_of, (lambda step: [o.lr_at(step) for o in table_opts]) if scheduled else None,
            fused.consts[:2] if adam else None)
    owner._constants.on_backward()
    if adam:
        b1, b2, eps = fused.consts
        return (b1, b2, eps, owner._constants.bias_correction)
    return fused.hyper(owner.step)
