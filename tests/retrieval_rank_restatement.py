"""A float64 / int64 torch-CPU restatement of K15 (krs_retrieval_rank, include/krs.h) and of FactorizedTopK's values,
with the input builders of tests/test_retrieval_rank_host.py and tests/test_retrieval_rank_gpu.py.  A helper, not a
test: data and CPU code only, nothing here touches a device.

Shapes: the case table of tests/retrieval_xent_cases.py (11 widths on both sides of every DPAD step x (40, 161) /
(161, 40): sliced and unsliced sweeps, partial tiles, a wave with one row) and its TESTED_BEFORE.

Two builders per shape:
  * integers(b, n, d): q, c = randint(-3, 4) as bf16, so every score is an integer of magnitude <= 9 d < 2^24, exact in
    fp32 in any summation order: the expected rank and score are exact;
  * normal(b, n, d): retrieval_xent_cases.inputs as it is, checked against a band (band()).
"""

import torch

from tests import retrieval_xent_cases as T

SHAPES = [(c.b, c.n, c.d) for c in T.CASES] + list(T.TESTED_BEFORE)
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _positives(b, n, gen):
    return torch.randperm(n, generator=gen)[:b] if b <= n else torch.randint(0, n, (b,), generator=gen)


def integers(b, n, d):
    """(q, c, pos): integer-valued bf16 embeddings; pos a permutation prefix when b <= n, else drawn with repeats"""
    gen = torch.Generator().manual_seed(3000 + 7 * d + b)
    q = torch.randint(-3, 4, (b, d), generator=gen).to(torch.bfloat16)
    c = torch.randint(-3, 4, (n, d), generator=gen).to(torch.bfloat16)
    return q, c, _positives(b, n, gen)


def normal(b, n, d, seed=None):
    q, c, pos, _, _ = T.inputs(b, n, d, seed=1000 + 7 * d + b if seed is None else seed)
    return q, c, pos


def scores64(q, c):
    return q.to(torch.float64) @ c.to(torch.float64).T


def rank_of(scores, pos, ids=None):
    """(int64 rank [B], float64 score of the positive [B]) from stored scores [B, N]: the number of candidates
    j != pos that precede pos -- score descending, then index ascending; -0.0 == +0.0, NaN above +inf and all NaN
    equal -- leaving out, with ids, those whose id is the positive's.  pos outside [0, N): -1 and NaN."""
    b, n = scores.shape
    p = pos.to(torch.int64)
    found = (p >= 0) & (p < n)
    at = p.clamp(0, n - 1)[:, None]
    t = scores.gather(1, at)
    nan_s, nan_t = torch.isnan(scores), torch.isnan(t)
    above = torch.where(nan_t, torch.zeros_like(nan_s), (scores > t) | nan_s)
    level = torch.where(nan_t, nan_s, scores == t)
    j = torch.arange(n)[None, :]
    counts = (above | (level & (j < at))) & (j != at)
    if ids is not None:
        counts &= ids[None, :] != ids[at[:, 0]][:, None]
    rank = torch.where(found, counts.sum(dim=1), torch.full_like(p, -1))
    return rank, torch.where(found, t[:, 0], torch.full_like(t[:, 0], float("nan")))


def argsort_position(scores, pos):
    """the positive's position in a stable descending argsort (finite scores, no ids): what rank_of must equal"""
    order = torch.argsort(scores, dim=1, descending=True, stable=True)
    return (order == pos.to(torch.int64)[:, None]).to(torch.int64).argmax(dim=1)


def band(q, c, pos, drop=None):
    """(lo [B], hi [B], float64 s_pos [B], delta_pos [B]) for bf16 inputs scored in fp32: with
    delta_ij = d 2^-23 sum_k |q_ik| |c_jk| (the fp32 accumulation bound of a d-term product sum in any order) and
    delta_i = delta_{i,pos_i},
        lo_i = #{j != pos : s_ij > s_pos + delta_ij + delta_i},   hi_i = #{j != pos : s_ij >= s_pos - delta_ij - delta_i}
    `drop` [B, N] bool leaves candidates out of both counts."""
    d = q.shape[1]
    s = scores64(q, c)
    delta = d * 2.0 ** -23 * (q.to(torch.float64).abs() @ c.to(torch.float64).abs().T)
    p = pos.to(torch.int64)[:, None]
    sp, dp = s.gather(1, p), delta.gather(1, p)
    other = torch.arange(c.shape[0])[None, :] != p
    if drop is not None:
        other = other & ~drop
    lo = ((s > sp + delta + dp) & other).sum(dim=1)
    hi = ((s >= sp - delta - dp) & other).sum(dim=1)
    return lo, hi, sp[:, 0], dp[:, 0]


def metric_values(rank, weight, ks):
    """FactorizedTopK's result in float64: top-k = sum w [0 <= rank < k] / sum w, MRR = sum w / (rank + 1) / sum w,
    all 0 when sum w = 0; a row with rank -1 counts in the denominator only."""
    rank = rank.to(torch.int64)
    w = torch.ones(rank.shape[0], dtype=torch.float64) if weight is None else weight.to(torch.float64)
    total = float(w.sum())
    found = rank >= 0
    out = {}
    for k in ks:
        out[f"top_{k}_categorical_accuracy"] = float((w * (found & (rank < k))).sum()) / total if total else 0.0
    rr = torch.where(found, 1.0 / (rank.clamp(min=0) + 1).to(torch.float64), torch.zeros_like(w))
    out["mean_reciprocal_rank"] = float((w * rr).sum()) / total if total else 0.0
    return out
