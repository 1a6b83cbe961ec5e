"""K17 (krs_retrieval_topk_q8) restated in plain numpy -- the reference of tests/test_retrieval_q8_gpu.py and
tests/test_retrieval_q8_host.py.  It shares nothing with the kernel.

    qq, qstep = quantize(query)                                  (tests/embed_q8_restatement: the rule of K16)
    idot_ij   = sum_e qq[i, e] * cq[j, e]                         int32, exact
    s_ij      = float32(float32(float32(idot_ij) * cstep_j) * qstep_i)      two rounded fp32 multiplies, in that order
    order     = s descending (-0.0 as +0.0), then the candidate index ascending (a stable sort)
A query row holding a NaN or an infinity has qq = 0 and qstep = 0: its scores are +0.0 and it returns 0 .. k-1.
Integer dot products are exact, so the kernel must return these ids and these score bits, with no tolerance.
"""

import numpy as np

from tests import embed_q8_restatement as Q8

FLAG_NONFINITE_ROW = Q8.FLAG_NONFINITE_ROW
quantize = Q8.quantize


def idot(qq, cq):
    """[B, N] int32 dot products of int8 rows ([B, D] against [N, D]); |idot| <= 512 * 128 * 128 needs no wider type."""
    qq, cq = np.asarray(qq), np.asarray(cq)
    assert qq.dtype == np.int8 and cq.dtype == np.int8 and qq.shape[1] == cq.shape[1] <= 512
    out = qq.astype(np.int32) @ cq.astype(np.int32).T
    assert out.dtype == np.int32
    return out


def scores(qq, qstep, cq, cstep):
    """[B, N] float32 scores of the contract: (float32(idot) * cstep_j) * qstep_i, each product rounded to fp32."""
    qstep, cstep = np.asarray(qstep), np.asarray(cstep)
    assert qstep.dtype == np.float32 and cstep.dtype == np.float32
    f = idot(qq, cq).astype(np.float32)                 # exact: |idot| < 2^24
    first = f * cstep[None, :]
    assert first.dtype == np.float32
    s = first * qstep[:, None]
    assert s.dtype == np.float32
    return s


def order(s, k):
    """[B, k] candidate indices in K8's total order: the score descending with -0.0 as +0.0, then the index ascending."""
    s = np.asarray(s, np.float32)
    assert np.isfinite(s).all()
    key = -(s + np.float32(0.0))                        # x + 0.0 turns -0.0 into +0.0; negation is exact
    key[key == 0] = 0.0                                 # (and the negated +0.0 back into +0.0)
    return np.argsort(key, axis=1, kind="stable")[:, :k]


def to_bf16(x):
    """float32 -> the float32 value of its bf16 rounding (round to nearest even; the inputs here are finite)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def restate(query, cq, cstep, k, ids=None, out_bf16=False):
    """What krs_retrieval_topk_q8 returns for float32 queries [B, D] (bf16 ones widened exactly):
    {"scores": float32 [B, k] (rounded to bf16 when out_bf16; -0.0 returned as +0.0), "ids": int32 [B, k],
     "index": the candidate indices, "bad": bool [B], "flag": FLAG_NONFINITE_ROW or 0, "qq", "qstep", "s": all scores}."""
    query = np.asarray(query, np.float32)
    qq, qstep, bad = quantize(query)
    s = scores(qq, qstep, cq, cstep)
    idx = order(s, k)
    top = np.take_along_axis(s, idx, axis=1) + np.float32(0.0)
    if out_bf16:
        top = to_bf16(top)
    out_ids = idx.astype(np.int32) if ids is None else np.asarray(ids, np.int32)[idx]
    return {"scores": top.astype(np.float32), "ids": out_ids, "index": idx, "bad": bad,
            "flag": FLAG_NONFINITE_ROW if bad.any() else 0, "qq": qq, "qstep": qstep, "s": s}


def exact_scores(query, cand):
    """The float64 scores query . cand^T of the unquantized rows, for the quantization bound."""
    return np.asarray(query, np.float64) @ np.asarray(cand, np.float64).T


def quantization_bound(query, cand, qstep, cstep):
    """[B, N] float64: 1.01 * [ (cstep_j ||q_i||_1 + qstep_i ||c_j||_1) / 2 + d qstep_i cstep_j / 4 ].
    With the dequantized rows q^ = q - eq and c^ = c - ec, |eq| <= qstep / 2 and |ec| <= cstep / 2 per element (abs-max
    scaling never clips): q . c - q^ . c^ = q . ec + eq . c - eq . ec, whose three terms are bounded by the three terms
    above.  The 1 % covers the fp32 roundings of inv, step and the two multiplies (each about 6e-8 relative)."""
    q64, c64 = np.abs(np.asarray(query, np.float64)), np.abs(np.asarray(cand, np.float64))
    d = q64.shape[1]
    qs, cs = np.asarray(qstep, np.float64)[:, None], np.asarray(cstep, np.float64)[None, :]
    return 1.01 * (0.5 * (cs * q64.sum(axis=1)[:, None] + qs * c64.sum(axis=1)[None, :]) + 0.25 * d * qs * cs)
