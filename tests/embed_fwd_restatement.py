"""K1 (krs_embed_bag_fwd) restated in float64, plain numpy -- the reference of tests/test_embed_fwd_matrix_gpu.py.  It
shares nothing with the kernels or with oracle/: no windows, no groups, no summation order of theirs.

Per bag (f, b) with lookups q (ids[q], weight w_q = 1 without weights) on the table T of feature f:
    num  = sum of w_q * T[ids[q]] over the lookups whose id lies in [0, vocab)
    den  = 1 (sum) | sum of w_q (mean) | sqrt(sum of w_q^2) (sqrtn), over ALL lookups of the bag: an out-of-range id adds
           nothing to num and still counts in the denominator (the kernels' rule: sw += w unconditionally)
    out  = 0 where den == 0, else num / den
    bag_scale = 1 (sum) | 0 where den == 0, else 1 / den
and for the error bound  M = sum of |w_q * T[ids[q]]|  over the valid lookups and  n = the bag's lookup count.
"""

import numpy as np

SUM, MEAN, SQRTN = 0, 1, 2
U = 2.0 ** -24      # fp32 unit roundoff
UB = 2.0 ** -8      # bf16 unit roundoff (the constant of tests/test_embed_bag_apply_matrix_gpu.py)


def gamma(k):
    return k * U / (1.0 - k * U)


def bag_bounds(n_feats, batch, hots=None, offsets=None):
    """(start, end) of every bag into the flat id buffer, bags numbered feature-major."""
    if offsets is not None:
        off = np.asarray(offsets, np.int64)
        return off[:-1].copy(), off[1:].copy()
    hots = np.asarray(hots, np.int64)
    base = np.concatenate([[0], np.cumsum(hots * batch)[:-1]])
    start = (base[:, None] + np.arange(batch, dtype=np.int64)[None, :] * hots[:, None]).reshape(-1)
    return start, start + np.repeat(hots, batch)


def restate(tables, feats, batch, dim, ids, hots=None, offsets=None, weights=None):
    """tables: float arrays [vocab, dim] (values already rounded to the table dtype); feats: [(table index, combiner)].
    Returns dict(out [n_feats, batch, dim], scale, den, M [n_feats, batch, dim], n, comb, bad) in float64 / int64, `bad` True
    when any id is out of range."""
    n_feats = len(feats)
    start, end = bag_bounds(n_feats, batch, hots, offsets)
    n = end - start
    n_bags = n_feats * batch
    bag_of = np.repeat(np.arange(n_bags, dtype=np.int64), n)          # bag of every lookup, in buffer order
    q = np.concatenate([np.arange(s, e, dtype=np.int64) for s, e in zip(start, end)] + [np.zeros(0, np.int64)])
    idv = np.asarray(ids)[q].astype(np.int64)
    w = np.ones(q.shape[0], np.float64) if weights is None else np.asarray(weights, np.float64)[q]
    num = np.zeros((n_bags, dim), np.float64)
    M = np.zeros((n_bags, dim), np.float64)
    bad = False
    for f, (t, _) in enumerate(feats):
        T = np.asarray(tables[t], np.float64)
        mine = (bag_of // batch) == f
        ok = mine & (idv >= 0) & (idv < T.shape[0])
        bad = bad or bool((mine & ~ok).any())
        term = w[ok, None] * T[idv[ok]]
        np.add.at(num, bag_of[ok], term)
        np.add.at(M, bag_of[ok], np.abs(term))
    sw = np.zeros(n_bags, np.float64)
    sw2 = np.zeros(n_bags, np.float64)
    np.add.at(sw, bag_of, w)
    np.add.at(sw2, bag_of, w * w)
    comb = np.repeat(np.array([c for _, c in feats], np.int64), batch)
    den = np.where(comb == SUM, 1.0, np.where(comb == MEAN, sw, np.sqrt(sw2)))
    safe = np.where(den == 0, 1.0, den)
    out = np.where((den == 0)[:, None], 0.0, num / safe[:, None])
    scale = np.where(comb == SUM, 1.0, np.where(den == 0, 0.0, 1.0 / safe))
    shape = (n_feats, batch, dim)
    return dict(out=out.reshape(shape), scale=scale.reshape(n_feats, batch), den=den.reshape(n_feats, batch),
                M=M.reshape(shape), n=n.reshape(n_feats, batch), comb=comb.reshape(n_feats, batch), bad=bad)


def bound(ref, out_is_bf16):
    """The bound of the pooled and generic kernels on |got - ref.out| (fp32 accumulation of n products in any order, one
    division, one rounding to the output type), twice the first-order term as in the K2 matrix test:
        2 * (gamma(n + 2) * M / |den| + gamma(n + 1) * |ref|) + u_out * |ref|
    Infinite where den == 0: those bags are asserted to be exactly 0 instead."""
    n = ref["n"][:, :, None].astype(np.float64)
    den = np.abs(ref["den"])[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        first = gamma(n + 2) * np.where(den == 0, np.inf, ref["M"] / np.where(den == 0, 1.0, den))
    a = np.abs(ref["out"])
    return 2 * (first + gamma(n + 1) * a) + (UB if out_is_bf16 else U) * a


def scale_bound(ref):
    """bag_scale: 2 * gamma(n + 1) relative; exactly 1.0 for the sum combiner (the bound is 0 there)."""
    return np.where(ref["comb"] == SUM, 0.0, 2 * gamma(ref["n"].astype(np.float64) + 1) * np.abs(ref["scale"]))


def evaluate_fp32(tables, feats, batch, dim, ids, hots=None, offsets=None, weights=None):
    """The same sums evaluated in fp32, lookup after lookup (product rounded, then the sum; no fused multiply-add): what a
    correct fp32 implementation may return.  (out [n_feats, batch, dim], scale) in float32."""
    n_feats = len(feats)
    start, end = bag_bounds(n_feats, batch, hots, offsets)
    n = end - start
    ids = np.asarray(ids)
    out = np.zeros((n_feats * batch, dim), np.float32)
    scale = np.zeros(n_feats * batch, np.float32)
    for f, (t, comb) in enumerate(feats):
        T = np.asarray(tables[t], np.float32)
        bags = np.arange(f * batch, (f + 1) * batch)
        acc = np.zeros((batch, dim), np.float32)
        sw = np.zeros(batch, np.float32)
        sw2 = np.zeros(batch, np.float32)
        for k in range(int(n[bags].max()) if batch else 0):
            live = np.nonzero(n[bags] > k)[0]
            q = start[bags][live] + k
            idv = ids[q].astype(np.int64)
            w = np.ones(live.shape[0], np.float32) if weights is None else np.asarray(weights, np.float32)[q]
            sw[live] += w
            sw2[live] += w * w
            ok = (idv >= 0) & (idv < T.shape[0])
            acc[live[ok]] += w[ok, None] * T[idv[ok]]
        den = np.ones(batch, np.float32) if comb == SUM else (sw if comb == MEAN else np.sqrt(sw2))
        safe = np.where(den == 0, np.float32(1), den)
        out[bags] = np.where((den == 0)[:, None], np.float32(0), acc / safe[:, None])
        scale[bags] = 1.0 if comb == SUM else np.where(den == 0, np.float32(0), np.float32(1) / safe)
    return out.reshape(n_feats, batch, dim), scale.reshape(n_feats, batch)
