"""A float64 numpy restatement of K22 (include/krs.h): residual add + dropout + layer norm over rows [n, d], forward and
backward, with the dropout hash bit for bit.  No torch, no GPU.

`dtype=None` is the float64 reference: nothing is rounded.  `dtype="bf16"` / `"fp32"` rounds where the kernel rounds:
x * keep / (1 - p) + residual is one fp32 fused multiply-add, s is rounded to dtype and the statistics are taken from
the rounded s; mean and rstd are kept in fp32; y, dx and dres are rounded to dtype once; the backward reads the rounded
s, mean and rstd.  (The fp32 sums themselves are not restated: their error is 2^-24 a step against the 2^-9 of bf16.)
"""

import numpy as np

from tests.seq_attention_restatement import M32, mix32, round_bf16

__all__ = ["round_to", "row_hash", "drop_threshold", "keep_factor", "forward", "backward", "magnitudes"]


def round_to(a, dtype):
    a = np.asarray(a, dtype=np.float64)
    if dtype is None:
        return a
    if dtype == "bf16":
        return round_bf16(a)
    return a.astype(np.float32).astype(np.float64)


def row_hash(seed, draw, n, d):
    """uint32 hash of every (row, column) as a uint64 array [n, d]: mix(base(seed, draw, row) + column)."""
    seed, draw = int(seed) & (2**64 - 1), int(draw) & (2**64 - 1)
    x = mix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    x = mix32(x ^ np.uint64(seed >> 32))
    x = mix32(x ^ np.uint64(draw & 0xFFFFFFFF))
    x = mix32(x ^ np.uint64(draw >> 32))
    base = mix32(x ^ np.arange(n, dtype=np.uint64).reshape(n, 1))
    return mix32((base + np.arange(d, dtype=np.uint64).reshape(1, d)) & M32)


def drop_threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def kept(seed, draw, n, d, p):
    """bool [n, d]."""
    if p == 0:
        return np.ones((n, d), dtype=bool)
    return row_hash(seed, draw, n, d) >= np.uint64(drop_threshold(p))


def keep_factor(seed, draw, n, d, p):
    """keep / (1 - p) as float64 [n, d]; 1 / (1 - p) is the contract's fp32 quotient (include/krs.h), in the reference
    too: s is then one exactly rounded fp32 multiply-add away from the reference, however residual and x cancel."""
    if p == 0:
        return np.ones((n, d))
    inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return np.where(kept(seed, draw, n, d, p), inv, 0.0)


def forward(x, residual=None, gamma=None, beta=None, *, eps, p=0.0, seed=0, draw=0, norm=True, dtype=None):
    """{"s", "y", "mean", "rstd"} (y, mean, rstd only with norm)."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    s = x * keep_factor(seed, draw, n, d, p)
    if residual is not None:
        s = s + np.asarray(residual, dtype=np.float64)
    if dtype is not None and (residual is not None or p > 0):
        s = round_to(s.astype(np.float32), dtype)           # the fused multiply-add's fp32 result, then the store
    out = {"s": s}
    if not norm:
        return out
    mean = s.mean(axis=1)
    if dtype is not None:
        mean = round_to(mean, "fp32")
    c = s - mean[:, None]
    rstd = 1.0 / np.sqrt((c * c).mean(axis=1) + float(np.float32(eps)))
    if dtype is not None:
        rstd = round_to(rstd, "fp32")
    g = np.ones(d) if gamma is None else np.asarray(gamma, dtype=np.float64)
    b = np.zeros(d) if beta is None else np.asarray(beta, dtype=np.float64)
    out.update(y=round_to(g * (c * rstd[:, None]) + b, dtype), mean=mean, rstd=rstd)
    return out


def backward(s, mean, rstd, gamma=None, dy=None, dsum=None, *, p=0.0, seed=0, draw=0, dtype=None):
    """{"dres", "dx", "dgamma", "dbeta"} from the forward's s, mean, rstd (dy None: the add form; then no dgamma, dbeta)."""
    s = np.asarray(s, dtype=np.float64)
    n, d = s.shape
    out = {}
    ds = np.zeros((n, d))
    if dy is not None:
        dy = np.asarray(dy, dtype=np.float64)
        xh = (s - mean[:, None]) * rstd[:, None]
        g = dy * (np.ones(d) if gamma is None else np.asarray(gamma, dtype=np.float64))
        ds = rstd[:, None] * (g - g.mean(axis=1, keepdims=True) - xh * (g * xh).mean(axis=1, keepdims=True))
        out.update(dgamma=round_to((dy * xh).sum(axis=0), None if dtype is None else "fp32"),
                   dbeta=round_to(dy.sum(axis=0), None if dtype is None else "fp32"))
    if dsum is not None:
        ds = ds + np.asarray(dsum, dtype=np.float64)
    if dtype is not None:
        ds = round_to(ds, "fp32")
    out.update(dres=round_to(ds, dtype), dx=round_to(ds * keep_factor(seed, draw, n, d, p), dtype))
    return out


def magnitudes(fwd, bwd, gamma=None, dy=None, *, p=0.0, seed=0, draw=0):
    """What an error of delta = 2^-8 |s| in every element of s does, to first order, to each output, from the float64
    reference alone (the derivation is in tests/layer_norm_cases.py).  Returns the brackets WITHOUT the output's own
    rounding: s, y, mean, rstd, dres, dx, dgamma, dbeta (those that exist; dbeta does not depend on s)."""
    s = fwd["s"]
    n, d = s.shape
    delta = 2.0 ** -8 * np.abs(s)
    out = {"s": np.zeros_like(s)}
    if "y" not in fwd:
        if bwd is not None:
            out.update(dres=np.zeros_like(s), dx=np.zeros_like(s))
        return out
    mean, rstd = fwd["mean"][:, None], fwd["rstd"][:, None]
    g1 = np.ones(d) if gamma is None else np.abs(np.asarray(gamma, dtype=np.float64))
    xh = (s - mean) * rstd
    a = rstd * (delta + delta.mean(axis=1, keepdims=True) + np.abs(xh) * (np.abs(xh) * delta).mean(axis=1, keepdims=True))
    rho = rstd * (np.abs(xh) * delta).mean(axis=1, keepdims=True)          # |d rstd| / rstd
    out.update(y=g1 * a, mean=delta.mean(axis=1), rstd=(rstd * rho)[:, 0])
    if bwd is None:
        return out
    if dy is None:
        out.update(dres=np.zeros_like(s), dx=np.zeros_like(s))
        return out
    dy = np.asarray(dy, dtype=np.float64)
    g = dy * (np.ones(d) if gamma is None else np.asarray(gamma, dtype=np.float64))
    m2 = (g * xh).mean(axis=1, keepdims=True)
    term = rstd * (g - g.mean(axis=1, keepdims=True) - xh * m2)            # the norm's share of ds
    dds = rho * np.abs(term) + rstd * (a * np.abs(m2) + np.abs(xh) * (np.abs(g) * a).mean(axis=1, keepdims=True))
    out.update(dres=dds, dx=dds * keep_factor(seed, draw, n, d, p),
               dgamma=(np.abs(dy) * a).sum(axis=0), dbeta=np.zeros(d))
    return out
