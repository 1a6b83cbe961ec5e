"""K16 (krs_quantize_rows_q8, krs_embed_bag_fwd_q8) restated in plain numpy -- the reference of tests/test_embed_q8_gpu.py
and tests/test_embed_q8_host.py.  It shares nothing with the kernels.

The quantizer, per row x[0..D) of an fp32 table (bf16 widened exactly), every operation in np.float32 (IEEE, correctly
rounded, np.rint = round half to even):
    a    = max |x[c]|
    inv  = 127 / (a + 1e-7)
    q[c] = clip(rint(x[c] * inv), -127, 127)
    step = (a + 1e-7) / 127
A row holding a NaN or an infinity gets q = 0 and step = 0 and is reported.

The lookup is tests/embed_fwd_restatement.restate (float64) on the float64 tables q * step; its bound is that module's
with one more rounding per product for w * step: gamma(n + 3) where it has gamma(n + 2).
"""

import numpy as np

from tests import embed_fwd_restatement as RS

SUM, MEAN, SQRTN = RS.SUM, RS.MEAN, RS.SQRTN
FLAG_ID_OUT_OF_RANGE, FLAG_NONFINITE_ROW = 1, 8


def quantize(x):
    """(q int8 [V, D], step float32 [V], nonfinite bool [V]) of a float32 [V, D] table."""
    x = np.asarray(x, np.float32)
    assert x.dtype == np.float32 and x.ndim == 2
    bad = ~np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(bad, np.float32(0), np.abs(x).max(axis=1)).astype(np.float32)
        d = a + np.float32(1e-7)
        inv = np.float32(127.0) / d
        step = d / np.float32(127.0)
        assert d.dtype == inv.dtype == step.dtype == np.float32
        prod = x * inv[:, None]
        assert prod.dtype == np.float32
        q = np.clip(np.rint(prod), np.float32(-127), np.float32(127))
    q[bad] = 0
    step = np.where(bad, np.float32(0), step).astype(np.float32)
    return q.astype(np.int8), step, bad


def dequantized(q, step):
    """the float64 table q * step (exact: an 8-bit integer times a 24-bit significand)"""
    return np.asarray(q, np.float64) * np.asarray(step, np.float64)[:, None]


def restate(q_tables, steps, feats, batch, dim, ids, hots=None, offsets=None, weights=None):
    """embed_fwd_restatement.restate on the float64 tables q * step."""
    return RS.restate([dequantized(q, s) for q, s in zip(q_tables, steps)], feats, batch, dim, ids, hots=hots,
                      offsets=offsets, weights=weights)


def bound(ref, out_is_bf16):
    """embed_fwd_restatement.bound with gamma(n + 3) for gamma(n + 2): the factor w * step is rounded once more.
        2 * (gamma(n + 3) * M / |den| + gamma(n + 1) * |ref|) + u_out * |ref|
    Infinite where den == 0: those bags are asserted to be exactly 0 instead."""
    n = ref["n"][:, :, None].astype(np.float64)
    den = np.abs(ref["den"])[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        first = RS.gamma(n + 3) * np.where(den == 0, np.inf, ref["M"] / np.where(den == 0, 1.0, den))
    a = np.abs(ref["out"])
    return 2 * (first + RS.gamma(n + 1) * a) + (RS.UB if out_is_bf16 else RS.U) * a


def evaluate_fp32(q_tables, steps, feats, batch, dim, ids, hots=None, offsets=None, weights=None):
    """The lookup in plain fp32, lookup after lookup, every product and sum rounded (no fused multiply-add): what a
    correct fp32 implementation may return.  out [n_feats, batch, dim] float32."""
    with np.errstate(invalid="ignore"):
        tables = [np.asarray(q, np.float32) * np.asarray(s, np.float32)[:, None] for q, s in zip(q_tables, steps)]
    return RS.evaluate_fp32(tables, feats, batch, dim, ids, hots=hots, offsets=offsets, weights=weights)[0]
