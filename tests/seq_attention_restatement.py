"""A float64 numpy restatement of K19 (include/krs.h): masked multi-head self-attention, forward and backward, with the
fully-masked-row rule and the dropout hash bit for bit.  No torch, no GPU.

Layouts: q, k, v, out, dout, dq, dk, dv are [B, L, H, Dh]; lse is [B, H, L]; key_valid is [B, L] (truthy = token).

`bf16=True` rounds where the fast path rounds: P~ before the P~ V product, dS and P~ before the gradient products, and
out / dq / dk / dv once at the end (delta is then formed from the ROUNDED out, which is what the backward is handed).
`defect` names one deliberate mistake (tests/test_seq_attention_host.py shows the bounds catch each):
    "causal_edge"  j < i instead of j <= i          "heads"      head h reads head (h + 1) % H of k and v
    "no_key_valid" the padding mask is ignored       "draw"       the dropout mask of draw + 1
    "no_scale"     scale = 1                         "no_delta"   delta dropped from dS (backward only)
"""

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def round_bf16(x):
    """float64 -> nearest-even bf16 value, as float64 (finite inputs)."""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def dropout_hash(seed, draw, B, H, L):
    """uint32 hash of every (b, h, i, j) as a uint64 array [B, H, L, L]."""
    seed, draw = int(seed) & (2**64 - 1), int(draw) & (2**64 - 1)
    x = mix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    x = mix32(x ^ np.uint64(seed >> 32))
    x = mix32(x ^ np.uint64(draw & 0xFFFFFFFF))
    x = mix32(x ^ np.uint64(draw >> 32))
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    base = mix32(x ^ bh)
    i = np.arange(L, dtype=np.uint64).reshape(1, 1, L, 1)
    j = np.arange(L, dtype=np.uint64).reshape(1, 1, 1, L)
    return mix32((base + ((i << np.uint64(12)) | j)) & M32)


def drop_threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def keep_factor(seed, draw, B, H, L, p):
    """keep_ij / (1 - p) in the kernel's fp32 arithmetic, as float64 [B, H, L, L]."""
    if p == 0:
        return np.ones((B, H, L, L))
    inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return np.where(dropout_hash(seed, draw, B, H, L) >= np.uint64(drop_threshold(p)), inv, 0.0)


def allowed_mask(B, L, key_valid, causal, defect=None):
    """[B, 1, L, L] bool."""
    i = np.arange(L).reshape(L, 1)
    j = np.arange(L).reshape(1, L)
    ok = np.ones((B, 1, L, L), dtype=bool)
    if causal:
        ok &= (j < i) if defect == "causal_edge" else (j <= i)
    if key_valid is not None and defect != "no_key_valid":
        ok &= np.asarray(key_valid).astype(bool).reshape(B, 1, 1, L)
    return ok


def _parts(q, k, v, key_valid, causal, scale, p, seed, draw, defect):
    B, L, H, _ = q.shape
    if defect == "heads":
        k, v = np.roll(k, -1, axis=2), np.roll(v, -1, axis=2)
    if defect == "no_scale":
        scale = 1.0
    if defect == "draw":
        draw = draw + 1
    s = scale * np.einsum("bihd,bjhd->bhij", q, k)
    ok = np.broadcast_to(allowed_mask(B, L, key_valid, causal, defect), s.shape)
    kf = keep_factor(seed, draw, B, H, L, p)
    return k, v, scale, s, ok, kf


def forward(q, k, v, *, key_valid=None, causal=False, scale=1.0, dropout_p=0.0, seed=0, draw=0, bf16=False,
            defect=None):
    """-> dict(out [B, L, H, Dh], lse [B, H, L], P [B, H, L, L] (before dropout), Pt (after))."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    k, v, scale, s, ok, kf = _parts(q, k, v, key_valid, causal, scale, dropout_p, seed, draw, defect)
    sm = np.where(ok, s, -np.inf)
    m = sm.max(axis=-1, keepdims=True)
    live = np.isfinite(m)                                  # rows with an allowed key
    e = np.where(ok, np.exp(np.where(ok, s, 0.0) - np.where(live, m, 0.0)), 0.0)
    z = e.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = np.where(live, np.where(live, m, 0.0) + np.log(np.where(live, z, 1.0)), -np.inf)[..., 0]
    et = e * kf
    if bf16:
        et = round_bf16(et)
    out = np.einsum("bhij,bjhd->bihd", et, v) / np.where(live, z, 1.0)[..., 0].transpose(0, 2, 1)[..., None]
    if bf16:
        out = round_bf16(out)
    P = e / np.where(live, z, 1.0)
    return {"out": out, "lse": lse, "P": P, "Pt": P * kf}


def backward(q, k, v, dout, *, key_valid=None, causal=False, scale=1.0, dropout_p=0.0, seed=0, draw=0, bf16=False,
             defect=None, fwd=None):
    """-> dict(dq, dk, dv [B, L, H, Dh], plus the magnitudes the bounds are made of).  `fwd`: the forward's result the
    backward is handed (default: this restatement's, with the same switches)."""
    q, k, v, dout = (np.asarray(t, dtype=np.float64) for t in (q, k, v, dout))
    if fwd is None:
        fwd = forward(q, k, v, key_valid=key_valid, causal=causal, scale=scale, dropout_p=dropout_p, seed=seed, draw=draw,
                      bf16=bf16, defect=defect)
    k, v, scale, s, ok, kf = _parts(q, k, v, key_valid, causal, scale, dropout_p, seed, draw, defect)
    lse = fwd["lse"][..., None]
    live = np.isfinite(lse)
    P = np.where(ok & live, np.exp(np.where(ok & live, s - np.where(live, lse, 0.0), 0.0)), 0.0)
    delta = np.einsum("bihd,bihd->bhi", dout, fwd["out"])[..., None]
    if defect == "no_delta":
        delta = np.zeros_like(delta)
    dP = np.einsum("bihd,bjhd->bhij", dout, v)
    dS = P * (kf * dP - delta)
    Pt = P * kf
    if bf16:
        dS, Pt = round_bf16(dS), round_bf16(Pt)
    dv = np.einsum("bhij,bihd->bjhd", Pt, dout)
    dq = scale * np.einsum("bhij,bjhd->bihd", dS, k)
    dk = scale * np.einsum("bhij,bihd->bjhd", dS, q)
    if defect == "heads":                                  # (the gradients of the heads that were read)
        dk, dv = np.roll(dk, 1, axis=2), np.roll(dv, 1, axis=2)
    if bf16:
        dq, dk, dv = round_bf16(dq), round_bf16(dk), round_bf16(dv)
    return {"dq": dq, "dk": dk, "dv": dv}


def magnitudes(q, k, v, dout, *, key_valid=None, causal=False, scale=1.0, dropout_p=0.0, seed=0, draw=0):
    """The cancellation-free sums the bf16 bounds are multiples of (all from the float64 reference):
         out  sum_j P~_ij |v_jd|
         dv   sum_i P~_ij |dO_id|
         dq   scale sum_j A_ij |k_jd|,  dk  scale sum_i A_ij |q_id|,
              A_ij = P_ij (keep_ij / (1 - p) |dP~_ij| + sum_d |dO_id o_id|)
         lse  1 + scale max_j sum_d |q_id k_jd|   (over all keys)"""
    q, k, v, dout = (np.asarray(t, dtype=np.float64) for t in (q, k, v, dout))
    f = forward(q, k, v, key_valid=key_valid, causal=causal, scale=scale, dropout_p=dropout_p, seed=seed, draw=draw)
    B, L, H, _ = q.shape
    kf = keep_factor(seed, draw, B, H, L, dropout_p)
    dP = np.einsum("bihd,bjhd->bhij", dout, v)
    dabs = np.einsum("bihd,bihd->bhi", np.abs(dout), np.abs(f["out"]))[..., None]
    A = f["P"] * (kf * np.abs(dP) + dabs)
    return {
        "out": np.einsum("bhij,bjhd->bihd", f["Pt"], np.abs(v)),
        "dv": np.einsum("bhij,bihd->bjhd", f["Pt"], np.abs(dout)),
        "dq": scale * np.einsum("bhij,bjhd->bihd", A, np.abs(k)),
        "dk": scale * np.einsum("bhij,bihd->bjhd", A, np.abs(q)),
        "lse": 1.0 + scale * np.einsum("bihd,bjhd->bhij", np.abs(q), np.abs(k)).max(axis=-1),
    }
