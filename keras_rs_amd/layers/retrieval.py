"""Retrieval layers on MI355X: drop-ins for keras_rs.layers.BruteForceRetrieval
(keras_rs/src/layers/retrieval/brute_force_retrieval.py) and keras_rs.layers.HardNegativeMining
(hard_negative_mining.py), both on K8's exact top-k (include/krs.h: krs_retrieval_topk, krs_topk_rows), and for the two
logit corrections of the training head, keras_rs.layers.SamplingProbabilityCorrection
(sampling_probability_correction.py) and keras_rs.layers.RemoveAccidentalHits (remove_accidental_hits.py), on K11
(krs_sampling_correction, krs_remove_accidental_hits); and InBatchSoftmaxLoss, the whole in-batch softmax head computed
from the two embedding matrices without storing the scores (K13: krs_retrieval_xent_fwd / krs_retrieval_xent_bwd), and
FactorizedTopK, the evaluation metric that goes with it: every top-k accuracy and the mean reciprocal rank from the
positive's rank among all candidates, again without the scores (K15: krs_retrieval_rank).  BruteForceRetrieval also has a
serving form, `quantize("int8")`: an int8 candidate index scored on the int8 matrix cores (K17: krs_retrieval_topk_q8).
PartitionedRetrieval is the approximate index: the candidates are partitioned into leaves by spherical k-means and a query
is scored against the candidates of its best few leaves only (K21: krs_retrieval_ivf), the partitioning stage of the
ScaNN index the reference's examples/scann.py serves from.  AsymmetricHashingRetrieval adds that index's other two stages on
the same partition: 4-bit codes scored on the matrix cores and an exact rescoring of the best few (K23: krs_ah_encode,
krs_retrieval_ivf_ah, krs_retrieval_rescore).

Selection order: score descending, then candidate index ascending (-0.0 as +0.0, NaN above +inf); rows come back
sorted.  Known divergence: for bf16 inputs keras.ops.matmul rounds the scores to bf16 before top_k, so among
candidates whose scores round to one bf16 value the reference's order can differ from this one, which ranks the
fp32 scores and rounds only the returned values.
"""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import losses as _reductions
from keras_rs_amd import retrieval_ops
from keras_rs_amd.layers import base
from keras_rs_amd.layers.embed_reduce import keep_fp32_steps, quantize_rows_checked, restore_fp32_steps


def _as_tensor(x, device=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(np.asarray(x), device=device)


def _int32_ids(ids: torch.Tensor) -> torch.Tensor:
    """Candidate ids as an int32 vector (what the kernels' `ids` operand is)."""
    if ids.dim() != 1:
        raise ValueError(f"`candidate_ids` must be a tensor of rank 1, received shape {tuple(ids.shape)}")
    if ids.dtype != torch.int32:
        if ids.dtype.is_floating_point or (ids.numel() and (int(ids.min()) < -2**31 or int(ids.max()) >= 2**31)):
            raise ValueError("`candidate_ids` must be integers that fit int32")
        ids = ids.to(torch.int32)
    return ids


class Retrieval(base.Layer):
    """Common interface of retrieval layers (retrieval.py): `k` candidates per query, scores returned with the ids
    when `return_scores`."""

    def __init__(self, k: int = 10, return_scores: bool = True, **kwargs: Any):
        super().__init__(**kwargs)
        self.k = k
        self.return_scores = return_scores

    def _validate_candidate_embeddings_and_ids(self, candidate_embeddings, candidate_ids=None) -> None:
        if candidate_embeddings is None:
            raise ValueError("`candidate_embeddings` is required.")
        shape = tuple(candidate_embeddings.shape)
        if len(shape) != 2:
            raise ValueError("`candidate_embeddings` must be a tensor of rank 2 (num_candidates, embedding_size), "
                             f"received `candidate_embeddings` with shape {shape}")
        if shape[0] < self.k:
            raise ValueError(f"The number of candidates provided ({shape[0]}) is less than the number of "
                             f"candidates to retrieve (k={self.k}).")
        if candidate_ids is not None and candidate_ids.shape[0] != shape[0]:
            raise ValueError("The `candidate_embeddings` and `candidate_is` tensors must have the same number of "
                             f"rows, got tensors of shape {shape} and {tuple(candidate_ids.shape)}.")

    def update_candidates(self, candidate_embeddings, candidate_ids=None) -> None:
        raise NotImplementedError

    def compute_score(self, query_embedding: torch.Tensor, candidate_embedding: torch.Tensor) -> torch.Tensor:
        """The dot product of queries and candidates (retrieval.py compute_score)."""
        return torch.matmul(query_embedding, candidate_embedding.transpose(0, 1))

    def get_config(self) -> dict:
        config = super().get_config()
        # The reference stores `self.compute_score` (a bound method) under "return_scores"; the boolean is stored
        # here on purpose, so that from_config(get_config()) rebuilds the same layer.
        config.update({"k": self.k, "return_scores": self.return_scores})
        return config


class BruteForceRetrieval(Retrieval):
    """Exact top-k retrieval over a candidate set kept on the device (brute_force_retrieval.py).

    Candidates and ids are non-trainable weights; `update_candidates` with the same shape copies in place, so a graph
    captured around `call` keeps reading the current candidates.  `call(query)` returns (top scores, top ids), or the
    ids alone when `return_scores=False`; ids are the candidate indices when the layer has no candidate ids.

    `quantize("int8")` turns the index into its serving form (include/krs.h, K17): int8 rows and one fp32 step per row,
    scored on the int8 matrix cores against queries quantized on the way in.
    """

    def __init__(self, candidate_embeddings=None, candidate_ids=None, k: int = 10, return_scores: bool = True,
                 **kwargs: Any):
        super().__init__(k=k, return_scores=return_scores, **kwargs)
        self.register_parameter("candidate_embeddings", None)    # (weights once candidates arrive: add_weight)
        self.register_parameter("candidate_ids", None)
        self._converted: dict[torch.dtype, torch.Tensor] = {}   # candidates in another query dtype
        self.quantization_mode = None      # "int8" after quantize(): candidate_embeddings_q / candidate_embeddings_step
        if candidate_embeddings is None:
            if candidate_ids is not None:
                raise ValueError("You cannot provide `candidate_ids` without providing `candidate_embeddings`")
        else:
            self.update_candidates(candidate_embeddings, candidate_ids)

    def update_candidates(self, candidate_embeddings, candidate_ids=None) -> None:
        self._validate_candidate_embeddings_and_ids(candidate_embeddings, candidate_ids)
        emb = _as_tensor(candidate_embeddings)
        ids = None if candidate_ids is None else _as_tensor(candidate_ids)
        if emb.dtype not in (torch.float32, torch.bfloat16):
            emb = emb.to(torch.float32)
        if ids is not None:
            ids = _int32_ids(ids)
        if self.quantization_mode:
            return self._update_quantized(emb, ids)
        with torch.no_grad():
            if self.candidate_embeddings is not None:
                # assign: the variable keeps its shape (and its storage, which a captured graph reads)
                if tuple(emb.shape) != tuple(self.candidate_embeddings.shape):
                    raise ValueError(f"Cannot assign candidate_embeddings of shape {tuple(emb.shape)} to a variable "
                                     f"of shape {tuple(self.candidate_embeddings.shape)}")
                if self.candidate_ids is None:
                    if ids is not None:
                        raise ValueError("New `candidate_ids` cannot be provided as previous candidates did not have "
                                         "candidate IDs")
                self.candidate_embeddings.copy_(emb)
                if self.candidate_ids is not None and ids is not None:
                    self.candidate_ids.copy_(ids)
                for dt, conv in self._converted.items():
                    conv.copy_(self.candidate_embeddings)
            else:
                self.candidate_embeddings = self.add_weight(tuple(emb.shape), "zeros", "candidate_embeddings",
                                                            dtype=emb.dtype, trainable=False)
                self.candidate_embeddings.copy_(emb)
                if ids is not None:
                    self.candidate_ids = self.add_weight(tuple(ids.shape), "zeros", "candidate_ids",
                                                         dtype=torch.int32, trainable=False)
                    self.candidate_ids.copy_(ids)
        self.built = True

    # ---- the int8 index (keras' quantize("int8") on the one large serving-time state of a two-tower model) -------------
    def quantize(self, mode: str = "int8") -> None:
        """Replaces the float index by int8 rows and one fp32 step per row (krs_quantize_rows_q8) and frees it and every
        converted copy: `weights` then holds candidate_ids only, state_dict() holds `candidate_embeddings_q` /
        `candidate_embeddings_step`, and `call` runs krs_retrieval_topk_q8 on fp32 or bf16 queries.  k <= 128 and
        D <= 512 only: the int8 index has no slab path.  A candidate row with a NaN or an infinity raises ValueError and
        leaves the layer as it was."""
        if mode != "int8":
            raise ValueError(f"Invalid quantization mode {mode!r}: BruteForceRetrieval supports 'int8' only.")
        if self.quantization_mode:
            raise ValueError(f"{type(self).__name__} '{self.name}' is already quantized ({self.quantization_mode}).")
        if self.candidate_embeddings is None:
            raise ValueError(f"{type(self).__name__} '{self.name}' has no candidates: call `update_candidates` before "
                             "quantize().")
        if self.k > retrieval_ops.Q8_MAX_K:
            raise ValueError(f"The int8 index retrieves at most k = {retrieval_ops.Q8_MAX_K} candidates per query, this "
                             f"layer has k = {self.k}.")
        if self.candidate_embeddings.shape[1] > retrieval_ops.Q8_MAX_D:
            raise ValueError(f"The int8 index takes embeddings of at most D = {retrieval_ops.Q8_MAX_D} columns, the "
                             f"candidates have D = {self.candidate_embeddings.shape[1]}.")
        q, step = quantize_rows_checked(self.candidate_embeddings.detach(), f"{type(self).__name__} '{self.name}'")
        self.register_buffer("candidate_embeddings_q", q, persistent=True)
        self.register_buffer("candidate_embeddings_step", step, persistent=True)
        self._weight_order[:] = [w for w in self._weight_order if w is not self.candidate_embeddings]
        self.candidate_embeddings = None
        self._converted.clear()
        self.quantization_mode = mode

    def _update_quantized(self, emb: torch.Tensor, ids) -> None:
        """update_candidates on the int8 index: the new float rows are quantized into temporaries, checked with one host
        read, and only then copied into the buffers a captured graph reads."""
        if tuple(emb.shape) != tuple(self.candidate_embeddings_q.shape):
            raise ValueError(f"Cannot assign candidate_embeddings of shape {tuple(emb.shape)} to a variable of shape "
                             f"{tuple(self.candidate_embeddings_q.shape)}")
        if self.candidate_ids is None and ids is not None:
            raise ValueError("New `candidate_ids` cannot be provided as previous candidates did not have candidate IDs")
        emb = emb.detach().to(self.candidate_embeddings_q.device)
        q, step = quantize_rows_checked(emb, f"{type(self).__name__} '{self.name}'")
        with torch.no_grad():
            self.candidate_embeddings_q.copy_(q)
            self.candidate_embeddings_step.copy_(step)
            if ids is not None:
                self.candidate_ids.copy_(ids)

    def _apply(self, fn, recurse=True):
        """.to() / .cuda() / .bfloat16(): the steps of the int8 index move with the module and stay fp32."""
        keep = keep_fp32_steps(self)
        out = super()._apply(fn, recurse)
        restore_fp32_steps(self, keep)
        return out

    def _call_quantized(self, inputs):
        q = _as_tensor(inputs)
        d = self.candidate_embeddings_q.shape[1]
        if q.dim() != 2 or q.shape[1] != d:
            raise ValueError(f"The query must have shape (batch, {d}), received {tuple(q.shape)}")
        L.require_device(q, "BruteForceRetrieval query")
        L.require_device(self.candidate_embeddings_q, "BruteForceRetrieval candidates")
        if q.dtype not in (torch.float32, torch.bfloat16):
            raise L.KrsError(f"BruteForceRetrieval: unsupported query dtype {q.dtype} (float32 / bfloat16)")
        ids = None if self.candidate_ids is None else self.candidate_ids.detach()
        # (no error word: a call reads nothing back, so it stays capturable; a non-finite query row scores 0 everywhere)
        scores, top_ids = retrieval_ops.retrieval_topk_q8(q.detach(), self.candidate_embeddings_q,
                                                          self.candidate_embeddings_step, self.k, ids=ids,
                                                          want_scores=self.return_scores)
        if self.return_scores:
            return scores, top_ids
        return top_ids

    def _candidates_as(self, dtype: torch.dtype) -> torch.Tensor:
        cand = self.candidate_embeddings
        if cand.dtype == dtype:
            return cand.detach()
        conv = self._converted.get(dtype)
        if conv is None:
            conv = cand.detach().to(dtype)
            self._converted[dtype] = conv
        return conv

    def call(self, inputs):
        if self.quantization_mode:
            return self._call_quantized(inputs)
        if self.candidate_embeddings is None:
            raise ValueError("No candidates: call `update_candidates` before using the layer.")
        q = _as_tensor(inputs)
        if q.dim() != 2 or q.shape[1] != self.candidate_embeddings.shape[1]:
            raise ValueError(f"The query must have shape (batch, {self.candidate_embeddings.shape[1]}), "
                             f"received {tuple(q.shape)}")
        L.require_device(q, "BruteForceRetrieval query")
        L.require_device(self.candidate_embeddings, "BruteForceRetrieval candidates")
        # keras.ops.matmul promotion: float32 x bfloat16 -> float32
        dt = torch.promote_types(q.dtype, self.candidate_embeddings.dtype)
        if dt not in (torch.float32, torch.bfloat16):
            raise L.KrsError(f"BruteForceRetrieval: unsupported query dtype {q.dtype} (float32 / bfloat16)")
        q = q.detach().to(dt)
        ids = None if self.candidate_ids is None else self.candidate_ids.detach()
        scores, top_ids = retrieval_ops.retrieval_topk(q, self._candidates_as(dt), self.k, ids=ids,
                                                       want_scores=self.return_scores)
        if self.return_scores:
            return scores, top_ids
        return top_ids


def partition_layout(assignments: torch.Tensor, num_leaves: int):
    """The stored layout of a partition: (row_index int32 [N], leaf_offsets int32 [num_leaves + 1]).  row_index is a
    stable sort of the original indices by leaf, so it ascends inside every leaf; leaf l owns the stored rows
    [leaf_offsets[l], leaf_offsets[l + 1]).  Torch ops on the assignments' device."""
    a = assignments.to(torch.int64)
    row_index = torch.sort(a, stable=True).indices.to(torch.int32)
    counts = torch.bincount(a, minlength=num_leaves)
    leaf_offsets = torch.zeros((num_leaves + 1,), dtype=torch.int64, device=a.device)
    leaf_offsets[1:] = torch.cumsum(counts, 0)
    return row_index, leaf_offsets.to(torch.int32)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class PartitionedRetrieval(Retrieval):
    """Approximate top-k retrieval over a partitioned candidate set (the tree stage of ScaNN, which the reference's
    examples/scann.py serves from): the candidates are grouped into `num_leaves` leaves, a query ranks the leaves by
    q . centroid and is scored against the candidates of its `num_leaves_to_search` best leaves only (include/krs.h,
    K21).  Inside those leaves the result is BruteForceRetrieval's: fp32 score descending, then candidate index
    ascending.  With num_leaves_to_search == num_leaves it IS BruteForceRetrieval's, bit for bit.  A query whose leaves
    hold fewer than k candidates ends in id -1, score -inf.  k <= 128, D <= 512, num_leaves_to_search <= 128.

    `update_candidates` builds the index and is not capturable (it waits on the host): spherical k-means, ScaNN's choice
    for dot products.  The first centroids are `num_leaves` candidates drawn on the host from `seed`, normalized; each of
    the `training_iterations` Lloyd steps assigns every candidate to its best centroid with K8 (k = 1: a tie goes to the
    lowest leaf) and replaces a centroid by the normalized sum of its members, summed in stored order by K1's CSR bags (a
    fixed order: the same input and seed give the same assignments); an empty leaf keeps its centroid.
    `from_partition` takes a clustering made elsewhere.  state_dict() holds the index (`candidate_rows` regrouped leaf
    by leaf, `leaf_offsets`, `row_index`, `centroids`, `candidate_ids`); loading it restores the index without training.
    `call` reads nothing back and replays from a captured graph."""

    _INDEX = ("candidate_rows", "leaf_offsets", "row_index", "centroids", "candidate_ids")
    _ASSIGN_CHUNK = 1 << 18       # candidates per assignment call: 64 workspace bytes each

    def __init__(self, candidate_embeddings=None, candidate_ids=None, k: int = 10, return_scores: bool = True,
                 num_leaves: int | None = None, num_leaves_to_search: int | None = None, training_iterations: int = 12,
                 seed: int = 0, **kwargs: Any):
        super().__init__(k=k, return_scores=return_scores, **kwargs)
        if not _is_int(k) or not 1 <= k <= retrieval_ops.IVF_MAX_K:
            raise ValueError(f"`k` should be an integer in [1, {retrieval_ops.IVF_MAX_K}]. Received: k={k!r}")
        if num_leaves is not None and (not _is_int(num_leaves) or num_leaves < 1):
            raise ValueError(f"`num_leaves` should be an integer >= 1 or None. Received: num_leaves={num_leaves!r}")
        if num_leaves_to_search is not None and (
                not _is_int(num_leaves_to_search) or not 1 <= num_leaves_to_search <= retrieval_ops.IVF_MAX_PROBES
                or (num_leaves is not None and num_leaves_to_search > num_leaves)):
            raise ValueError("`num_leaves_to_search` should be an integer in [1, min(num_leaves, "
                             f"{retrieval_ops.IVF_MAX_PROBES})] or None. Received: "
                             f"num_leaves_to_search={num_leaves_to_search!r}, num_leaves={num_leaves!r}")
        if not _is_int(training_iterations) or training_iterations < 0:
            raise ValueError("`training_iterations` should be an integer >= 0. Received: "
                             f"training_iterations={training_iterations!r}")
        if not _is_int(seed):
            raise ValueError(f"`seed` should be an integer. Received: seed={seed!r}")
        self.num_leaves, self.num_leaves_to_search = num_leaves, num_leaves_to_search
        self.training_iterations, self.seed = int(training_iterations), int(seed)
        for name in self._INDEX:
            self.register_buffer(name, None, persistent=True)
        self._converted: dict[torch.dtype, tuple] = {}     # (rows, centroids) in another query dtype
        if candidate_embeddings is None:
            if candidate_ids is not None:
                raise ValueError("You cannot provide `candidate_ids` without providing `candidate_embeddings`")
        else:
            self.update_candidates(candidate_embeddings, candidate_ids)

    @classmethod
    def from_partition(cls, candidate_embeddings, centroids, assignments, candidate_ids=None, **kwargs: Any):
        """An index over a clustering made elsewhere: centroids [leaves, D], assignments integer [N] in [0, leaves), the
        leaf of each candidate.  No training; the other arguments are the constructor's (num_leaves is the centroids')."""
        cen = _as_tensor(centroids)
        if cen.dim() != 2 or cen.shape[0] < 1:
            raise ValueError(f"`centroids` must be a tensor of rank 2 (num_leaves, embedding_size), received shape "
                             f"{tuple(cen.shape)}")
        if kwargs.setdefault("num_leaves", cen.shape[0]) != cen.shape[0]:
            raise ValueError(f"`num_leaves` = {kwargs['num_leaves']} differs from the {cen.shape[0]} rows of `centroids`")
        layer = cls(**kwargs)
        emb, ids = layer._checked_candidates(candidate_embeddings, candidate_ids)
        if cen.shape[1] != emb.shape[1]:
            raise ValueError(f"`centroids` has {cen.shape[1]} columns, `candidate_embeddings` has {emb.shape[1]}")
        a = _as_tensor(assignments)
        if a.dtype.is_floating_point or a.dtype == torch.bool or tuple(a.shape) != (emb.shape[0],):
            raise ValueError(f"`assignments` should be {emb.shape[0]} integers, one leaf per candidate. Received: "
                             f"`assignments.shape` = {tuple(a.shape)}, dtype {a.dtype}")
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= cen.shape[0]):
            raise ValueError(f"`assignments` should be inside [0, {cen.shape[0]}). Received values from {int(a.min())} "
                             f"to {int(a.max())}")
        layer._set_index(emb, cen.detach().to(emb.device, emb.dtype), a.detach().to(emb.device), ids)
        return layer

    def _checked_candidates(self, candidate_embeddings, candidate_ids):
        self._validate_candidate_embeddings_and_ids(candidate_embeddings, candidate_ids)
        emb = _as_tensor(candidate_embeddings).detach()
        ids = None if candidate_ids is None else _int32_ids(_as_tensor(candidate_ids).detach())
        if emb.dtype not in (torch.float32, torch.bfloat16):
            emb = emb.to(torch.float32)
        if emb.shape[1] > retrieval_ops.IVF_MAX_D:
            raise ValueError(f"The partitioned index takes embeddings of at most D = {retrieval_ops.IVF_MAX_D} columns, "
                             f"the candidates have D = {emb.shape[1]}.")
        return emb.to(self._device), None if ids is None else ids.to(self._device)

    def _leaves_for(self, n: int) -> int:
        leaves = self.num_leaves if self.num_leaves is not None else max(1, int(round(float(np.sqrt(n)))))
        if leaves > n:
            raise ValueError(f"`num_leaves` = {leaves} is more than the number of candidates ({n}).")
        return leaves

    def probes(self) -> int:
        """Leaves searched per query: num_leaves_to_search, or max(1, leaves // 10) capped at 128."""
        leaves = self.centroids.shape[0] if self.centroids is not None else self.num_leaves
        if self.num_leaves_to_search is not None:
            return self.num_leaves_to_search
        return min(retrieval_ops.IVF_MAX_PROBES, max(1, leaves // 10))

    def update_candidates(self, candidate_embeddings, candidate_ids=None) -> None:
        emb, ids = self._checked_candidates(candidate_embeddings, candidate_ids)
        leaves = self._leaves_for(emb.shape[0])
        L.require_device(emb, "PartitionedRetrieval candidates")
        centroids, assignments = self._train(emb, leaves)
        self._set_index(emb, centroids, assignments, ids)

    def _assign(self, emb: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        out = torch.empty((emb.shape[0],), dtype=torch.int32, device=emb.device)
        for r0 in range(0, emb.shape[0], self._ASSIGN_CHUNK):
            r1 = min(emb.shape[0], r0 + self._ASSIGN_CHUNK)
            out[r0:r1] = retrieval_ops.retrieval_topk(emb[r0:r1], centroids, 1, want_scores=False)[1][:, 0]
        return out

    def _train(self, emb: torch.Tensor, leaves: int):
        """Spherical k-means (class docstring).  Returns (centroids [leaves, D] in emb's dtype, assignments int32 [N])."""
        from keras_rs_amd import embedding_ops

        n = emb.shape[0]
        sample = np.sort(np.random.default_rng(self.seed).choice(n, size=leaves, replace=False))
        cen32 = torch.nn.functional.normalize(emb[torch.as_tensor(sample, device=emb.device)].to(torch.float32), dim=1)
        bags = embedding_ops.FusedBags([emb.contiguous()], [(0, "sum", 0)])
        for _ in range(self.training_iterations):
            a = self._assign(emb, cen32.to(emb.dtype))
            row_index, leaf_offsets = partition_layout(a, leaves)
            sums, _ = bags.forward(row_index, leaves, offsets=leaf_offsets, out_dtype=torch.float32)
            filled = (leaf_offsets[1:] > leaf_offsets[:-1])[:, None]
            cen32 = torch.where(filled, torch.nn.functional.normalize(sums, dim=1), cen32)
        centroids = cen32.to(emb.dtype)
        return centroids, self._assign(emb, centroids)

    def _set_index(self, emb, centroids, assignments, ids) -> None:
        leaves = centroids.shape[0]
        if self.num_leaves_to_search is not None and self.num_leaves_to_search > leaves:
            raise ValueError(f"`num_leaves_to_search` = {self.num_leaves_to_search} is more than the {leaves} leaves.")
        row_index, leaf_offsets = partition_layout(assignments, leaves)
        self.candidate_rows = emb[row_index.to(torch.int64)].contiguous()
        self.leaf_offsets, self.row_index = leaf_offsets, row_index
        self.centroids = centroids.contiguous()
        self.candidate_ids = None if ids is None else ids.contiguous()
        self._converted.clear()
        self.built = True

    @property
    def assignments(self) -> torch.Tensor:
        """The leaf of every candidate, int32 [N] by original index (read off the stored layout)."""
        counts = (self.leaf_offsets[1:] - self.leaf_offsets[:-1]).to(torch.int64)
        leaf = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int32, device=counts.device), counts)
        out = torch.empty_like(leaf)
        out[self.row_index.to(torch.int64)] = leaf
        return out

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A saved index replaces whatever the layer holds: the buffers take the saved shapes and dtypes."""
        for name in self._INDEX:
            saved = state_dict.get(prefix + name)
            if saved is not None:
                setattr(self, name, torch.empty_like(saved, device=self._device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._converted.clear()
        self.built = self.candidate_rows is not None

    def _apply(self, fn, recurse=True):
        self._converted.clear()       # (.to() / .cuda(): the converted copies follow the buffers at the next call)
        return super()._apply(fn, recurse)

    def quantize(self, mode: str = "int8") -> None:
        raise NotImplementedError("PartitionedRetrieval has no quantized form: the int8 candidate index lives in "
                                  "BruteForceRetrieval.quantize('int8') (K17, krs_retrieval_topk_q8).")

    def _index_as(self, dtype: torch.dtype):
        if self.candidate_rows.dtype == dtype:
            return self.candidate_rows, self.centroids
        conv = self._converted.get(dtype)
        if conv is None:
            conv = self._converted[dtype] = (self.candidate_rows.to(dtype), self.centroids.to(dtype))
        return conv

    def call(self, inputs, return_leaves: bool = False):
        if self.candidate_rows is None:
            raise ValueError("No candidates: call `update_candidates` before using the layer.")
        q = _as_tensor(inputs)
        if q.dim() != 2 or q.shape[1] != self.candidate_rows.shape[1]:
            raise ValueError(f"The query must have shape (batch, {self.candidate_rows.shape[1]}), "
                             f"received {tuple(q.shape)}")
        L.require_device(q, "PartitionedRetrieval query")
        L.require_device(self.candidate_rows, "PartitionedRetrieval candidates")
        # keras.ops.matmul promotion: float32 x bfloat16 -> float32
        dt = torch.promote_types(q.dtype, self.candidate_rows.dtype)
        if dt not in (torch.float32, torch.bfloat16):
            raise L.KrsError(f"PartitionedRetrieval: unsupported query dtype {q.dtype} (float32 / bfloat16)")
        rows, centroids = self._index_as(dt)
        out = retrieval_ops.retrieval_ivf(q.detach().to(dt), centroids, rows, self.leaf_offsets, self.row_index, self.k,
                                          self.probes(), ids=self.candidate_ids, want_scores=self.return_scores,
                                          want_leaves=return_leaves)
        if return_leaves:          # (an extension: the probed leaves [batch, probes] as a last item)
            return (out[0], out[1], out[2]) if self.return_scores else (out[1], out[2])
        return (out[0], out[1]) if self.return_scores else out[1]

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"num_leaves": self.num_leaves, "num_leaves_to_search": self.num_leaves_to_search,
                       "training_iterations": self.training_iterations, "seed": self.seed})
        return config


def unpack_codes(codes: torch.Tensor, blocks: int) -> torch.Tensor:
    """The nibbles of code rows uint8 [N, bytes] as int64 [N, blocks]: block j is nibble j, the low half of byte j // 2
    for even j (include/krs.h, K23)."""
    c = codes.to(torch.int64)
    return torch.stack((c & 15, c >> 4), dim=2).reshape(codes.shape[0], -1)[:, :blocks]


class AsymmetricHashingRetrieval(PartitionedRetrieval):
    """PartitionedRetrieval with ScaNN's other two stages (the reference's examples/scann.py: tree(...),
    score_ah(dimensions_per_block), reorder(n)); include/krs.h, K23.  A candidate is stored as one 4-bit code per block
    of `dimensions_per_block` columns of its residual x - centroid[leaf(x)]: 16 centres per block, so D / (2 m) bytes a
    row instead of D floats.  A query is scored against the codes of its best leaves, q . decode(code) + q . centroid
    (the AH score), on the matrix cores.

    * `num_reordering_candidates=None`: `call` returns K21's tuple and THE SCORES ARE AH SCORES, approximations of
      q . x, ranked as they are (AH score descending, candidate index ascending).  The float rows are not kept: not on
      the device, not in state_dict().
    * `num_reordering_candidates=R` (k <= R <= 128): the best R by AH score are rescored against the float rows and the k
      best of those returned: the scores are exact (K8's bits), the order is BruteForceRetrieval's over those R.

    `update_candidates` partitions as PartitionedRetrieval does, then trains the codebooks (not capturable, host-driven):
    Lloyd's k-means with Euclidean distance, per block, on the residuals of `training_sample_size` rows drawn on the host
    from `seed`; the first centres of every block are the sub-vectors of 16 sampled residuals; each of the
    `training_iterations` steps codes the sample with krs_ah_encode (the lowest code on a tie) and replaces a centre by
    the float64 mean of its members, summed by a plain reduction over the sample axis (a fixed order: the same input and
    seed give the same codebooks and codes); an empty centre keeps its value.  Then every row is coded in one pass.
    `from_codebooks` takes partition and codebooks from outside and only encodes.  state_dict() holds the index
    (`centroids`, `leaf_offsets`, `row_index`, `candidate_ids`, `codebooks`, `codes`, and `float_rows` in ORIGINAL order
    only when reordering); loading it restores the index without training.  `anisotropic_quantization_threshold` other
    than None raises NotImplementedError: the codebooks minimise the plain reconstruction error."""

    _INDEX = ("leaf_offsets", "row_index", "centroids", "candidate_ids", "codebooks", "codes", "float_rows")

    def __init__(self, candidate_embeddings=None, candidate_ids=None, k: int = 10, return_scores: bool = True,
                 num_leaves: int | None = None, num_leaves_to_search: int | None = None, training_iterations: int = 12,
                 seed: int = 0, dimensions_per_block: int = 2, num_reordering_candidates: int | None = None,
                 training_sample_size: int = 100_000, anisotropic_quantization_threshold=None, **kwargs: Any):
        super().__init__(k=k, return_scores=return_scores, num_leaves=num_leaves,
                         num_leaves_to_search=num_leaves_to_search, training_iterations=training_iterations, seed=seed,
                         **kwargs)
        if not _is_int(dimensions_per_block) or dimensions_per_block not in retrieval_ops.AH_BLOCK_DIMS:
            raise ValueError(f"`dimensions_per_block` should be one of {retrieval_ops.AH_BLOCK_DIMS}. Received: "
                             f"dimensions_per_block={dimensions_per_block!r}")
        if num_reordering_candidates is not None and (
                not _is_int(num_reordering_candidates) or not k <= num_reordering_candidates <= retrieval_ops.AH_MAX_R):
            raise ValueError(f"`num_reordering_candidates` should be None or an integer in [k = {k}, "
                             f"{retrieval_ops.AH_MAX_R}]. Received: num_reordering_candidates="
                             f"{num_reordering_candidates!r}")
        if not _is_int(training_sample_size) or training_sample_size < 16:
            raise ValueError("`training_sample_size` should be an integer >= 16. Received: "
                             f"training_sample_size={training_sample_size!r}")
        if anisotropic_quantization_threshold is not None:
            raise NotImplementedError("`anisotropic_quantization_threshold`: the score-aware quantization loss is not "
                                      "implemented; pass None (plain reconstruction error).")
        self.dimensions_per_block = int(dimensions_per_block)
        self.num_reordering_candidates = None if num_reordering_candidates is None else int(num_reordering_candidates)
        self.training_sample_size = int(training_sample_size)
        self.anisotropic_quantization_threshold = None
        self._converted: dict[torch.dtype, tuple] = {}     # (centroids, float rows or None) in another query dtype
        if candidate_embeddings is None:
            if candidate_ids is not None:
                raise ValueError("You cannot provide `candidate_ids` without providing `candidate_embeddings`")
        else:
            self.update_candidates(candidate_embeddings, candidate_ids)

    @classmethod
    def from_codebooks(cls, candidate_embeddings, centroids, assignments, codebooks, candidate_ids=None, **kwargs: Any):
        """An index over a partition AND codebooks made elsewhere: centroids and assignments as from_partition's,
        codebooks [ceil(D / m), 16, m] (rounded to bfloat16).  Nothing is trained: the rows are encoded, that is all."""
        cb = _as_tensor(codebooks).detach()
        if cb.dim() != 3 or cb.shape[1] != 16 or cb.shape[2] not in retrieval_ops.AH_BLOCK_DIMS:
            raise ValueError("`codebooks` must have shape (blocks, 16, dimensions_per_block) with dimensions_per_block in "
                             f"{retrieval_ops.AH_BLOCK_DIMS}, received shape {tuple(cb.shape)}")
        if kwargs.setdefault("dimensions_per_block", cb.shape[2]) != cb.shape[2]:
            raise ValueError(f"`dimensions_per_block` = {kwargs['dimensions_per_block']} differs from the codebooks' "
                             f"{cb.shape[2]}")
        d = _as_tensor(candidate_embeddings).shape[-1]
        if cb.shape[0] != -(-d // cb.shape[2]):
            raise ValueError(f"`codebooks` has {cb.shape[0]} blocks, D = {d} columns in blocks of {cb.shape[2]} need "
                             f"{-(-d // cb.shape[2])}")
        cls._next_codebooks = cb
        try:
            return cls.from_partition(candidate_embeddings, centroids, assignments, candidate_ids, **kwargs)
        finally:
            cls._next_codebooks = None

    _next_codebooks = None        # from_codebooks -> the _set_index of the layer from_partition makes

    def _train_codebooks(self, emb: torch.Tensor, centroids: torch.Tensor, assignments: torch.Tensor) -> torch.Tensor:
        """Lloyd's k-means per block (class docstring).  Returns the codebooks bfloat16 [blocks, 16, m]."""
        n, d = emb.shape
        m = self.dimensions_per_block
        blocks = -(-d // m)
        rng = np.random.default_rng(self.seed)
        s = min(n, self.training_sample_size)
        sample = torch.as_tensor(np.sort(rng.choice(n, size=s, replace=False)), device=emb.device)
        first = torch.as_tensor(rng.choice(s, size=16, replace=s < 16), device=emb.device)
        x = emb[sample].contiguous()
        leaf = assignments[sample].to(torch.int32).contiguous()
        res = torch.zeros((s, blocks * m), dtype=torch.float64, device=emb.device)
        res[:, :d] = (x.to(torch.float32) - centroids[leaf.to(torch.int64)].to(torch.float32)).to(torch.float64)
        res = res.view(s, blocks, m)
        cb = res[first].permute(1, 0, 2).contiguous()                        # [blocks, 16, m] float64
        for _ in range(self.training_iterations):
            codes = unpack_codes(retrieval_ops.ah_encode(x, leaf, centroids, cb.to(torch.bfloat16)), blocks)
            for c in range(16):
                member = (codes == c)[:, :, None]                            # [s, blocks, 1]
                count = member.sum(0)                                        # [blocks, 1]
                mean = (res * member).sum(0) / count.clamp(min=1)
                cb[:, c, :] = torch.where(count > 0, mean, cb[:, c, :])
        return cb.to(torch.bfloat16).contiguous()

    def _set_index(self, emb, centroids, assignments, ids) -> None:
        leaves = centroids.shape[0]
        if self.num_leaves_to_search is not None and self.num_leaves_to_search > leaves:
            raise ValueError(f"`num_leaves_to_search` = {self.num_leaves_to_search} is more than the {leaves} leaves.")
        L.require_device(emb, "AsymmetricHashingRetrieval candidates")
        given = type(self)._next_codebooks
        centroids = centroids.contiguous()
        codebooks = (self._train_codebooks(emb, centroids, assignments) if given is None
                     else given.to(emb.device, torch.bfloat16).contiguous())
        row_index, leaf_offsets = partition_layout(assignments, leaves)
        row_leaf = assignments.to(torch.int32)[row_index.to(torch.int64)].contiguous()
        self.codes = retrieval_ops.ah_encode(emb, row_leaf, centroids, codebooks, row_index=row_index)
        self.codebooks = codebooks
        self.leaf_offsets, self.row_index = leaf_offsets, row_index
        self.centroids = centroids
        self.candidate_ids = None if ids is None else ids.contiguous()
        self.float_rows = emb.contiguous() if self.num_reordering_candidates is not None else None
        self._converted.clear()
        self.built = True

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A saved index replaces whatever the layer holds: the buffers take the saved shapes and dtypes."""
        for name in self._INDEX:
            saved = state_dict.get(prefix + name)
            setattr(self, name, None if saved is None else torch.empty_like(saved, device=self._device))
        torch.nn.Module._load_from_state_dict(self, state_dict, prefix, *args, **kwargs)
        self._converted.clear()
        self.built = self.codes is not None

    def index_bytes(self) -> int:
        """Bytes of the stored index (every buffer of state_dict())."""
        return sum(t.numel() * t.element_size() for t in self.state_dict().values())

    def _index_as(self, dtype: torch.dtype):
        if self.centroids.dtype == dtype:
            return self.centroids, self.float_rows
        conv = self._converted.get(dtype)
        if conv is None:
            conv = self._converted[dtype] = (self.centroids.to(dtype),
                                             None if self.float_rows is None else self.float_rows.to(dtype))
        return conv

    def call(self, inputs, return_leaves: bool = False):
        if self.codes is None:
            raise ValueError("No candidates: call `update_candidates` before using the layer.")
        d = self.centroids.shape[1]
        q = _as_tensor(inputs)
        if q.dim() != 2 or q.shape[1] != d:
            raise ValueError(f"The query must have shape (batch, {d}), received {tuple(q.shape)}")
        L.require_device(q, "AsymmetricHashingRetrieval query")
        reorder = self.num_reordering_candidates is not None
        if reorder and self.float_rows is None:
            raise ValueError("`num_reordering_candidates` is set but the index holds no float rows (it was built or saved "
                             "without reordering): rebuild it with `update_candidates`.")
        dt = torch.promote_types(q.dtype, self.centroids.dtype)
        if dt not in (torch.float32, torch.bfloat16):
            raise L.KrsError(f"AsymmetricHashingRetrieval: unsupported query dtype {q.dtype} (float32 / bfloat16)")
        centroids, rows = self._index_as(dt)
        out = retrieval_ops.retrieval_ivf_ah(q.detach().to(dt), centroids, self.codebooks, self.codes, self.leaf_offsets,
                                             self.row_index, self.k, self.probes(), rows=rows if reorder else None,
                                             num_reordering_candidates=self.num_reordering_candidates,
                                             ids=self.candidate_ids, want_scores=self.return_scores,
                                             want_leaves=return_leaves)
        if return_leaves:
            return (out[0], out[1], out[2]) if self.return_scores else (out[1], out[2])
        return (out[0], out[1]) if self.return_scores else out[1]

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"dimensions_per_block": self.dimensions_per_block,
                       "num_reordering_candidates": self.num_reordering_candidates,
                       "training_sample_size": self.training_sample_size,
                       "anisotropic_quantization_threshold": self.anisotropic_quantization_threshold})
        return config


class HardNegativeMining(base.Layer):
    """Logits and labels of the `num_hard_negatives` highest-scoring negatives plus the positive of each row
    (hard_negative_mining.py).  Output order: the key logits + labels * MAX_FLOAT descending, then the index ascending
    (the reference's sorted=False permits any order).  The logits gradient flows through torch.gather."""

    def __init__(self, num_hard_negatives: int, **kwargs: Any):
        super().__init__(**kwargs)
        self._num_hard_negatives = num_hard_negatives
        self.built = True

    def num_sampled(self, num_logits: int) -> int:
        return min(self._num_hard_negatives + 1, num_logits)

    def call(self, logits: torch.Tensor, labels: torch.Tensor):
        if logits.dim() not in (1, 2, 3):
            raise ValueError(f"`logits` must have rank 1 to 3, received shape {tuple(logits.shape)}")
        if tuple(labels.shape) != tuple(logits.shape):
            raise ValueError(f"`labels` shape {tuple(labels.shape)} differs from `logits` shape {tuple(logits.shape)}")
        L.require_device(logits, "HardNegativeMining logits")
        L.require_device(labels, "HardNegativeMining labels")
        c = logits.shape[-1]
        k = self.num_sampled(c)
        x = logits.detach().reshape(-1, c)
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        boost = labels.detach().reshape(-1, c).to(x.dtype)
        idx = retrieval_ops.topk_rows(x, k, boost=boost, boost_scale=retrieval_ops.MAX_FLOAT)
        idx = idx.to(torch.int64).reshape(*logits.shape[:-1], k)
        return torch.gather(logits, -1, idx), torch.gather(labels, -1, idx)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"num_hard_negatives": self._num_hard_negatives})
        return config


def _check_logits_rank(logits: torch.Tensor) -> None:
    if logits.dim() not in (1, 2, 3):
        raise ValueError(f"`logits` must have rank 1 to 3, received shape {tuple(logits.shape)}")


class SamplingProbabilityCorrection(base.Layer):
    """logits - log(clip(candidate_sampling_probability, epsilon, 1)) (sampling_probability_correction.py:56-58).  The
    probabilities have the logits' shape or that of its last axes (`[num_candidates]` against `[batch,
    num_candidates]`): they are broadcast inside the kernel.  The gradient reaches the logits unchanged; the
    probabilities get none."""

    def __init__(self, epsilon: float = 1e-6, **kwargs: Any):
        super().__init__(**kwargs)
        self.epsilon = epsilon
        self.built = True

    def call(self, logits: torch.Tensor, candidate_sampling_probability: torch.Tensor) -> torch.Tensor:
        _check_logits_rank(logits)
        p = _as_tensor(candidate_sampling_probability, logits.device)
        if p.dim() == 0:
            p = p.expand(logits.shape[-1:])
        if p.dim() > logits.dim() or tuple(p.shape) != tuple(logits.shape[logits.dim() - p.dim():]):
            raise ValueError("`candidate_sampling_probability` should have the same shape as the last dimensions of "
                             f"`logits`. Received: `candidate_sampling_probability.shape` = {tuple(p.shape)}, "
                             f"`logits.shape` = {tuple(logits.shape)}.")
        L.require_device(logits, "SamplingProbabilityCorrection logits")
        L.require_device(p, "SamplingProbabilityCorrection candidate_sampling_probability")
        return retrieval_ops.corrected(retrieval_ops.sampling_correction, logits, p.detach(), self.epsilon)

    def get_config(self) -> dict:
        config = super().get_config()
        config.update({"epsilon": self.epsilon})
        return config


class RemoveAccidentalHits(base.Layer):
    """logits + ((candidate_ids == the positive's id) - labels) * SMALLEST_FLOAT (remove_accidental_hits.py:84-97), the
    positive of a row being the first argmax of its labels.  SMALLEST_FLOAT is the reference's 1.1754944e-40, a
    positive subnormal: as in the reference, a logit changes only where it is itself of about that magnitude, and for
    ordinary logits the layer is the identity.  The gradient reaches the logits unchanged."""

    def __init__(self, **kwargs: Any):
        super().__init__(**kwargs)
        self.built = True

    def call(self, logits: torch.Tensor, labels: torch.Tensor, candidate_ids: torch.Tensor) -> torch.Tensor:
        labels = _as_tensor(labels, logits.device)
        candidate_ids = _as_tensor(candidate_ids, logits.device)
        labels_shape, logits_shape, ids_shape = tuple(labels.shape), tuple(logits.shape), tuple(candidate_ids.shape)
        if labels_shape != logits_shape:
            raise ValueError("`labels` and `logits` should have the same shape. Received: "
                             f"`labels.shape` = {labels_shape}, `logits.shape` = {logits_shape}.")
        if len(ids_shape) == 0 or labels_shape[-len(ids_shape):] != ids_shape:
            raise ValueError("`candidate_ids` should have the same shape as the last dimensions of `labels`. "
                             f"Received: `candidate_ids.shape` = {ids_shape}, `labels.shape` = {labels_shape}.")
        _check_logits_rank(logits)
        L.require_device(logits, "RemoveAccidentalHits logits")
        L.require_device(labels, "RemoveAccidentalHits labels")
        L.require_device(candidate_ids, "RemoveAccidentalHits candidate_ids")
        return retrieval_ops.corrected(retrieval_ops.remove_accidental_hits, logits, labels.detach(),
                                       candidate_ids.detach(), retrieval_ops.SMALLEST_FLOAT)


class InBatchSoftmaxLoss:
    """The in-batch softmax loss of a two-tower retrieval model, from the embeddings: scores = query . candidates^T,
    SamplingProbabilityCorrection, RemoveAccidentalHits and CategoricalCrossentropy(from_logits=True) against the
    positives, with the [batch, candidates] scores, labels and logit gradient never stored (include/krs.h, K13;
    memory O((B + N) D)).  With num_hard_negatives, HardNegativeMining sits in front of the cross-entropy (K14).

        loss(query_embeddings [B, D], candidate_embeddings [N, D], positive_index=None, candidate_ids=None,
             candidate_sampling_probability=None, sample_weight=None)

    positive_index [B]: the candidate that is each query's positive (None: candidate i for query i, the eye(B, N)
    labels of the reference's examples); an index outside [0, N) makes that row's loss and gradients NaN.
    candidate_sampling_probability [N]: logits -= log(clip(p, epsilon, 1)).  candidate_ids [N]: candidates with the
    positive's id, other than the positive itself, have accidental_hit_value added to their logit; the default is the
    reference's constant, which changes no ordinary logit, a large negative finite value
    removes them.  bf16 embeddings of up to 256 columns run on the fused kernels, with fp32 scores (the stored-matrix
    head rounds them to bf16 first); other inputs run krs_gemm + K11 slab by slab in fp32.

    num_hard_negatives (an integer >= 1, default None: every candidate counts): the cross-entropy runs over each
    query's positive and its k = min(num_hard_negatives, N - 1) highest corrected scores among the other candidates,
    as keras_rs.layers.HardNegativeMining(k) in front of the loss does, and label_smoothing spreads over those k + 1
    logits.  Equal scores at the k-th place go to the lowest candidate index (the reference leaves that choice open;
    the loss does not depend on it).  The selection runs inside the fused scoring kernel for fp32 and bf16 embeddings
    with k <= 128 and D <= 512 (include/krs.h, K14): memory is the inputs plus B * S * k (score, index) pairs, S
    the number of candidate slices; larger k or D mine slab by slab on stored fp32 scores."""

    def __init__(self, label_smoothing: float = 0.0, reduction: str | None = "sum_over_batch_size",
                 epsilon: float = 1e-6, accidental_hit_value: float = retrieval_ops.SMALLEST_FLOAT,
                 name: str | None = None, num_hard_negatives: int | None = None):
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"`label_smoothing` should be in [0, 1). Received: label_smoothing={label_smoothing}")
        if reduction not in _reductions.REDUCTIONS:
            raise ValueError(f"Invalid value for argument `reduction`. Expected one of {_reductions.REDUCTIONS}. "
                             f"Received: reduction={reduction}")
        if not np.isfinite(accidental_hit_value):
            raise ValueError(f"`accidental_hit_value` should be finite. Received: {accidental_hit_value}")
        self.label_smoothing, self.reduction = float(label_smoothing), reduction
        self.epsilon, self.accidental_hit_value = float(epsilon), float(accidental_hit_value)
        if num_hard_negatives is not None and (isinstance(num_hard_negatives, bool)
                                               or not isinstance(num_hard_negatives, (int, np.integer))
                                               or num_hard_negatives < 1):
            raise ValueError("`num_hard_negatives` should be an integer >= 1 or None. Received: "
                             f"num_hard_negatives={num_hard_negatives!r}")
        self.num_hard_negatives = None if num_hard_negatives is None else int(num_hard_negatives)
        self.name = name or "in_batch_softmax_loss"

    def __call__(self, query_embeddings, candidate_embeddings, positive_index=None, candidate_ids=None,
                 candidate_sampling_probability=None, sample_weight=None) -> torch.Tensor:
        q = _as_tensor(query_embeddings)
        c = _as_tensor(candidate_embeddings, q.device)
        shapes = f"`query_embeddings.shape` = {tuple(q.shape)}, `candidate_embeddings.shape` = {tuple(c.shape)}"
        if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1] or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError("`query_embeddings` [batch, dim] and `candidate_embeddings` [candidates, dim] should be "
                             f"matrices of one width with at least one candidate. Received: {shapes}.")
        if q.dtype != c.dtype or q.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("`query_embeddings` and `candidate_embeddings` should share a dtype, float32 or bfloat16. "
                             f"Received: {q.dtype} and {c.dtype} ({shapes}).")
        b, n = q.shape[0], c.shape[0]
        pos = ids = bias = None
        if positive_index is not None:
            pos = _as_tensor(positive_index, q.device)
            if tuple(pos.shape) != (b,) or pos.dtype.is_floating_point or pos.dtype == torch.bool:
                raise ValueError(f"`positive_index` should be {b} integers, one per query. Received: "
                                 f"`positive_index.shape` = {tuple(pos.shape)}, dtype {pos.dtype} ({shapes}).")
        if candidate_ids is not None:
            ids = _as_tensor(candidate_ids, q.device)
            if tuple(ids.shape) != (n,) or ids.dtype.is_floating_point or ids.dtype == torch.bool:
                raise ValueError(f"`candidate_ids` should be {n} integers, one per candidate. Received: "
                                 f"`candidate_ids.shape` = {tuple(ids.shape)}, dtype {ids.dtype} ({shapes}).")
        if candidate_sampling_probability is not None:
            prob = _as_tensor(candidate_sampling_probability, q.device)
            if tuple(prob.shape) != (n,):
                raise ValueError(f"`candidate_sampling_probability` should have one entry per candidate. Received: "
                                 f"`candidate_sampling_probability.shape` = {tuple(prob.shape)} ({shapes}).")
            bias = -torch.log(torch.clamp(prob.detach().to(torch.float32), self.epsilon, 1.0))
        w = _reductions._sample_weight(sample_weight, (b,), q.device)
        L.require_device(q, "InBatchSoftmaxLoss query_embeddings")
        L.require_device(c, "InBatchSoftmaxLoss candidate_embeddings")
        return retrieval_ops.retrieval_xent(q, c, positive_index=None if pos is None else pos.detach(), cand_bias=bias,
                                            cand_ids=None if ids is None else ids.detach(),
                                            hit_value=self.accidental_hit_value, label_smoothing=self.label_smoothing,
                                            sample_weight=w, reduction=self.reduction,
                                            num_hard_negatives=self.num_hard_negatives)

    def get_config(self) -> dict:
        config = {"name": self.name, "label_smoothing": self.label_smoothing, "reduction": self.reduction,
                  "epsilon": self.epsilon, "accidental_hit_value": self.accidental_hit_value}
        if self.num_hard_negatives is not None:      # (an unset layer keeps the config it always had)
            config["num_hard_negatives"] = self.num_hard_negatives
        return config

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)


def rank_totals(rank: torch.Tensor, weight: torch.Tensor | None, ks: torch.Tensor) -> torch.Tensor:
    """What one batch adds to FactorizedTopK's state, with torch ops in a fixed order on any device: fp32
    [len(ks) + 2] = (sum_i w_i [0 <= rank_i < k] for each k, sum_i w_i / (rank_i + 1), sum_i w_i).  rank int [B]
    (-1: no positive; the row counts in the last total only), weight None, a scalar or [B], ks int [K]."""
    b = rank.shape[0]
    w = torch.ones((b,), dtype=torch.float32, device=rank.device) if weight is None else \
        weight.to(torch.float32).expand((b,))
    found = rank >= 0
    hit = found[:, None] & (rank[:, None] < ks[None, :])
    top = (w[:, None] * hit.to(torch.float32)).sum(dim=0)
    rr = torch.where(found, 1.0 / (rank.clamp(min=0).to(torch.float32) + 1.0), torch.zeros_like(w))
    return torch.cat((top, (w * rr).sum()[None], w.sum()[None]))


class FactorizedTopK:
    """Top-k categorical accuracies and the mean reciprocal rank of a two-tower model, from the embeddings -- the idea of
    tfrs.metrics.FactorizedTopK: score every query against all candidates and ask where its positive lands.  Here one
    sweep (include/krs.h, K15: krs_retrieval_rank) counts the candidates that beat the positive, so every k and the
    reciprocal rank come from one pass and the [B, N] scores are never stored (memory O((B + N) D)).

        metric = FactorizedTopK(candidate_embeddings [N, D], candidate_ids=None, ks=(1, 5, 10, 50, 100))
        metric.update_state(query_embeddings [B, D], positive_index [B], sample_weight=None)
        metric.result() -> {"top_1_categorical_accuracy": ..., ..., "mean_reciprocal_rank": ...}

    rank_i is the number of candidates other than the positive that precede it in BruteForceRetrieval's order (score
    descending, then candidate index ascending), so `rank_i < k` is "the positive is among BruteForceRetrieval(k)'s
    ids".  With candidate_ids, other candidates that carry the positive's id are not counted (accidental hits are
    removed).  A positive_index outside [0, N) counts as a miss for every k and adds 0 to the reciprocal rank.
    Values: top-k = sum w_i [rank_i < k] / sum w_i, MRR = sum w_i / (rank_i + 1) / sum w_i, 0 when sum w = 0.

    Candidates given to update_state override the stored ones for that call (the in-batch use: candidates = the batch's
    item embeddings, positive_index=None for candidate i of query i).  `update_candidates` with the same shape copies
    in place, so a graph captured around update_state keeps reading the current candidates.  The totals are a device
    tensor; nothing waits for the device.  bf16 embeddings of up to 256 columns run on the fused kernel, other inputs
    on a slab path of krs_gemm."""

    def __init__(self, candidate_embeddings=None, candidate_ids=None, ks=(1, 5, 10, 50, 100),
                 name: str = "factorized_top_k"):
        ks = tuple(ks)
        if not ks or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 for k in ks):
            raise ValueError(f"`ks` should be a non-empty sequence of integers >= 1. Received: ks={ks!r}")
        self.ks = tuple(int(k) for k in ks)
        self.name = name
        self.candidate_embeddings = None
        self.candidate_ids = None
        self._state = None
        self._ks_on: dict = {}
        if candidate_embeddings is None:
            if candidate_ids is not None:
                raise ValueError("You cannot provide `candidate_ids` without providing `candidate_embeddings`")
        else:
            self.update_candidates(candidate_embeddings, candidate_ids)

    @staticmethod
    def _check_candidates(c, ids, what="candidate_embeddings"):
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError(f"`{what}` must be a tensor of rank 2 (num_candidates, embedding_size) with at least one "
                             f"candidate, received shape {tuple(c.shape)}")
        if c.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"`{what}` should be float32 or bfloat16. Received: {c.dtype}.")
        if ids is not None and (tuple(ids.shape) != (c.shape[0],) or ids.dtype.is_floating_point
                                or ids.dtype == torch.bool):
            raise ValueError(f"`candidate_ids` should be {c.shape[0]} integers, one per candidate. Received: "
                             f"`candidate_ids.shape` = {tuple(ids.shape)}, dtype {ids.dtype}.")

    def update_candidates(self, candidate_embeddings, candidate_ids=None) -> None:
        if candidate_embeddings is None:
            raise ValueError("`candidate_embeddings` is required.")
        emb = _as_tensor(candidate_embeddings).detach()
        ids = None if candidate_ids is None else _as_tensor(candidate_ids, emb.device).detach()
        self._check_candidates(emb, ids)
        if ids is not None and ids.dtype not in (torch.int32, torch.int64):
            ids = ids.to(torch.int64)
        if self.candidate_embeddings is None:
            self.candidate_embeddings = emb.clone()
            self.candidate_ids = None if ids is None else ids.clone()
            return
        # assign: the stored tensors keep their shape and storage, which a captured graph reads
        if tuple(emb.shape) != tuple(self.candidate_embeddings.shape):
            raise ValueError(f"Cannot assign candidate_embeddings of shape {tuple(emb.shape)} to a variable of shape "
                             f"{tuple(self.candidate_embeddings.shape)}")
        if self.candidate_ids is None and ids is not None:
            raise ValueError("New `candidate_ids` cannot be provided as previous candidates did not have candidate IDs")
        self.candidate_embeddings.copy_(emb)
        if ids is not None:
            self.candidate_ids.copy_(ids)

    def _device_state(self, device) -> torch.Tensor:
        if self._state is None or self._state.device != device:
            self._state = torch.zeros((len(self.ks) + 2,), dtype=torch.float32, device=device)
        return self._state

    def _device_ks(self, device) -> torch.Tensor:
        ks = self._ks_on.get(device)
        if ks is None:
            ks = self._ks_on[device] = torch.tensor(self.ks, dtype=torch.int32, device=device)
        return ks

    def accumulate(self, rank: torch.Tensor, sample_weight=None) -> None:
        """Adds the ranks of one batch (int [B], -1 for a row without a positive) to the totals, on rank's device."""
        w = _reductions._sample_weight(sample_weight, (rank.shape[0],), rank.device)
        self._device_state(rank.device).add_(rank_totals(rank, w, self._device_ks(rank.device)))

    def update_state(self, query_embeddings, positive_index=None, sample_weight=None, candidate_embeddings=None,
                     candidate_ids=None) -> None:
        q = _as_tensor(query_embeddings)
        if candidate_embeddings is not None:
            c = _as_tensor(candidate_embeddings, q.device)
            ids = None if candidate_ids is None else _as_tensor(candidate_ids, q.device)
        elif candidate_ids is not None:
            raise ValueError("You cannot provide `candidate_ids` without providing `candidate_embeddings`")
        elif self.candidate_embeddings is None:
            raise ValueError("No candidates: give `candidate_embeddings` or call `update_candidates` first.")
        else:
            c, ids = self.candidate_embeddings, self.candidate_ids
        shapes = f"`query_embeddings.shape` = {tuple(q.shape)}, `candidate_embeddings.shape` = {tuple(c.shape)}"
        if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1] or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError("`query_embeddings` [batch, dim] and `candidate_embeddings` [candidates, dim] should be "
                             f"matrices of one width with at least one candidate. Received: {shapes}.")
        if q.dtype != c.dtype or q.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("`query_embeddings` and `candidate_embeddings` should share a dtype, float32 or bfloat16. "
                             f"Received: {q.dtype} and {c.dtype} ({shapes}).")
        b, n = q.shape[0], c.shape[0]
        pos = None
        if positive_index is not None:
            pos = _as_tensor(positive_index, q.device)
            if tuple(pos.shape) != (b,) or pos.dtype.is_floating_point or pos.dtype == torch.bool:
                raise ValueError(f"`positive_index` should be {b} integers, one per query. Received: "
                                 f"`positive_index.shape` = {tuple(pos.shape)}, dtype {pos.dtype} ({shapes}).")
        if ids is not None and (tuple(ids.shape) != (n,) or ids.dtype.is_floating_point or ids.dtype == torch.bool):
            raise ValueError(f"`candidate_ids` should be {n} integers, one per candidate. Received: "
                             f"`candidate_ids.shape` = {tuple(ids.shape)}, dtype {ids.dtype} ({shapes}).")
        w = _reductions._sample_weight(sample_weight, (b,), q.device)
        L.require_device(q, "FactorizedTopK query_embeddings")
        L.require_device(c, "FactorizedTopK candidate_embeddings")
        rank, _ = retrieval_ops.retrieval_rank(q.detach(), c.detach(), None if pos is None else pos.detach(),
                                               None if ids is None else ids.detach())
        self.accumulate(rank, w)

    def result(self) -> dict:
        state = torch.zeros((len(self.ks) + 2,), dtype=torch.float32) if self._state is None else self._state
        total = state[-1]
        nz = total != 0
        values = torch.where(nz, state[:-1] / torch.where(nz, total, torch.ones_like(total)),
                             torch.zeros_like(state[:-1]))
        out = {f"top_{k}_categorical_accuracy": values[i] for i, k in enumerate(self.ks)}
        out["mean_reciprocal_rank"] = values[len(self.ks)]
        return out

    def reset_state(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def __call__(self, query_embeddings, positive_index=None, sample_weight=None, candidate_embeddings=None,
                 candidate_ids=None) -> dict:
        self.update_state(query_embeddings, positive_index, sample_weight, candidate_embeddings, candidate_ids)
        return self.result()

    def get_config(self) -> dict:
        return {"name": self.name, "ks": list(self.ks)}

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)
