"""float64 restatement of the keras_rs.metrics ranking metrics (written from their formulas and from DESIGN.md's
description of K10's order, used by the K10 tests): the rank order with its tie rule -- the tie hash in integer
arithmetic --, sort_by_scores, get_list_weights, compute_dcg and the six compute_metric methods."""

import numpy as np

U32 = 2.0 ** -24          # fp32 unit roundoff
KINDS = ("dcg", "ndcg", "map", "mrr", "precision", "recall")
_M64 = (1 << 64) - 1


def order_key(s):
    """fp32 -> uint32 preserving the total order of K8 / K9: -0 == +0, NaN above +inf."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0xFFFFFFFF, key).astype(np.uint64)


def _mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix64_array(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def tie_r20(seed: int, draw: int, batch: int, n: int):
    """[batch, n] 20-bit tie keys: the top 20 bits of mix64(salt + (row << 12 | index)),
    salt = mix64(seed ^ mix64(draw + 0x9E3779B97F4A7C15)), all modulo 2^64."""
    salt = _mix64((seed & _M64) ^ _mix64((draw + 0x9E3779B97F4A7C15) & _M64))
    ctr = (np.arange(batch, dtype=np.uint64)[:, None] << np.uint64(12)) | np.arange(n, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        h = _mix64_array(ctr + np.uint64(salt))
    return (h >> np.uint64(44)).astype(np.int64)


def prepare(y, mask=None, weight=None):
    """(labels, weights, valid) as float64 / bool [B, L]: an item is valid when label >= 0, mask set, weight > 0;
    an invalid item gets label 0 and weight 0."""
    y = np.asarray(y, dtype=np.float64)
    w = np.ones_like(y) if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), y.shape)
    valid = (y >= 0) & (w > 0)
    if mask is not None:
        valid = valid & np.asarray(mask, dtype=bool)
    return np.where(valid, y, 0.0), np.where(valid, w, 0.0), valid


def rank_order(scores, valid, shuffle_ties=False, seed=0, draw=0, ties="ascending"):
    """[B, L] item index at each rank: valid first, score descending, then the tie key.  ties="ascending" is the
    rule of K10 (hash descending when shuffling, then index ascending); "descending" reverses the tie level only
    (used to show that a case does not depend on it)."""
    s = np.asarray(scores, dtype=np.float32)
    b, n = s.shape
    okey = order_key(s).astype(np.int64)
    r20 = tie_r20(seed, draw, b, n) if shuffle_ties else np.zeros((b, n), dtype=np.int64)
    idx = np.broadcast_to(np.arange(n, dtype=np.int64), (b, n))
    tie = (r20 << 12) | (4095 - idx)                   # larger first
    if ties == "descending":
        tie = -tie
    okey = np.where(valid, okey, 1)
    return np.lexsort((-tie, -okey), axis=-1)           # (last key is the primary one)


def default_gain(y):
    return np.power(2.0, y) - 1.0


def default_discount(rank):
    return 1.0 / np.log2(1.0 + rank)


def list_weights(w, relevance):
    """get_list_weights: [B] per-list weights from item weights and relevances [B, L]."""
    sw, sr, swr = w.sum(1), relevance.sum(1), (w * relevance).sum(1)
    plw = np.where(sr != 0, swr / np.where(sr != 0, sr, 1.0), 0.0)
    both = (sw > 0) & (sr > 0)
    avg = plw.sum() / both.sum() if both.sum() > 0 else 1.0
    return np.where(sw > 0, np.where(sr > 0, plw, avg), 0.0)


def _dnn(a, b):
    return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def _dcg(y_sorted, w_sorted, gain_sorted, discount_fn):
    rank = np.arange(1, y_sorted.shape[1] + 1, dtype=np.float64)
    return (w_sorted * (gain_sorted * discount_fn(rank)[None, :])).sum(1)


def metric(kind, scores, y_true, mask=None, weight=None, k=None, shuffle_ties=False, seed=0, draw=0,
           ties="ascending", gain_fn=default_gain, discount_fn=default_discount):
    """(per-list values [B], per-list weights [B], order [B, L]) of one metric as its compute_metric states it."""
    y, w, valid = prepare(y_true, mask, weight)
    n = y.shape[1]
    k_eff = n if k is None else min(k, n)
    order = rank_order(scores, valid, shuffle_ties, seed, draw, ties)
    top = order[:, :k_eff]
    take = lambda t, o: np.take_along_axis(t, o, axis=1)   # noqa: E731
    rel = (y >= 1).astype(np.float64)
    if kind in ("dcg", "ndcg"):
        gain = gain_fn(y)
        weights = list_weights(w, gain)
        dcg = _dcg(take(y, top), take(w, top), take(gain, top), discount_fn)
        if kind == "dcg":
            return _dnn(dcg, weights), weights, order
        ideal_top = np.argsort(-(w * gain), axis=1, kind="stable")[:, :k_eff]
        ideal = _dcg(take(y, ideal_top), take(w, ideal_top), take(gain, ideal_top), discount_fn)
        return _dnn(dcg, ideal), weights, order
    weights = list_weights(w, rel)
    srel, sw = take(rel, top), take(w, top)
    rank = np.arange(1, k_eff + 1, dtype=np.float64)[None, :]
    if kind == "map":
        prec = np.cumsum(srel, 1) / rank
        return _dnn((prec * (sw * srel)).sum(1), (w * rel).sum(1)), weights, order
    if kind == "mrr":
        return (srel / rank).max(1), weights, order
    if kind == "precision":
        return _dnn(srel.sum(1), np.minimum(k_eff, valid.sum(1)).astype(np.float64)), weights, order
    if kind == "recall":
        return _dnn(srel.sum(1), rel.sum(1)), weights, order
    raise ValueError(kind)


def broadcast_weight(sample_weight, shape):
    """sample_weight (None, scalar, [B], [B, L], or [L] for one list) as float64 [B, L]; shape is y_true's."""
    if sample_weight is None:
        return None
    w = np.asarray(sample_weight, dtype=np.float64)
    if len(shape) == 2 and w.ndim == 1:
        w = w[:, None]
    full = shape if len(shape) == 2 else (1,) + tuple(shape)
    return np.broadcast_to(w, full)


class Mean:
    """keras.metrics.Mean over updates of (values, weights)."""

    def __init__(self):
        self.total = self.count = 0.0

    def update(self, values, weights):
        self.total += float((values * weights).sum())
        self.count += float(weights.sum())

    def result(self):
        return self.total / self.count if self.count != 0 else 0.0
