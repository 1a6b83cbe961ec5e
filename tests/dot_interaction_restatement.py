"""DotInteraction (K4) restated in plain numpy float64, for tests/test_dot_interaction_matrix_gpu.py and
tests/test_dot_interaction_routes_host.py.  Inputs are taken as stored (a bf16 value widened exactly), so the only error
a kernel may show is its own accumulation and its one rounding to the storage type.

forward   P = X X^T per sample, packed as the row-major lower triangle without / with the diagonal, or as the [F, F]
          layout with zeros in the masked part (skip_gather).  S = sum_c |x_ic x_jc|.
backward  dX_i = sum_j (G_ij + G_ji) X_j, G the incoming gradient scattered to [F, F] (zero in the masked part), plus the
          existing gradient of the features the mask names.  S = sum_j |Gs_ij x_jd| + |existing|.

bound     fp32 accumulation of n exact products and one final rounding:
              |got - exact| <= (n + 2) * 2^-24 * S + r * |exact|
          n = D forward, F (+ 1 with an existing gradient) backward; r = 0 for fp32 storage and 2^-8 * 1.01 for bf16
          storage (the project's figure for an fp32 sum rounded once, tests/test_dense_ops_gpu.py).  The block backward
          rounds a bf16 gradient once per chunk of 128 features: each earlier chunk adds r * |the partial sum it stored|.
"""

import numpy as np

U32 = 2.0 ** -24
R_BF16 = 2.0 ** -8 * 1.01
CHUNK = 128      # features per launch of dot_bwd_block_kernel (kBlockJ)


def out_cols(F, self_i, skip):
    return F * F if skip else (F * (F + 1) // 2 if self_i else F * (F - 1) // 2)


def kept_pairs(F, self_i):
    """(i, j) of the kept pairs in the order of the gathered output: row-major lower triangle"""
    i, j = np.tril_indices(F, 0 if self_i else -1)
    return i, j


def forward(X, self_i, skip):
    """X [B, F, D] float64 -> (out [B, cols], S [B, cols])"""
    B, F, _ = X.shape
    P = np.einsum("bic,bjc->bij", X, X)
    S = np.einsum("bic,bjc->bij", np.abs(X), np.abs(X))
    i, j = kept_pairs(F, self_i)
    if not skip:
        return P[:, i, j], S[:, i, j]
    keep = np.zeros((F, F), dtype=bool)
    keep[i, j] = True
    return np.where(keep, P, 0.0).reshape(B, F * F), np.where(keep, S, 0.0).reshape(B, F * F)


def scatter_gradient(G, F, self_i, skip):
    """the incoming gradient [B, cols] as Gs = G + G^T over the kept pairs, [B, F, F]"""
    B = G.shape[0]
    i, j = kept_pairs(F, self_i)
    full = np.zeros((B, F, F))
    full[:, i, j] = G.reshape(B, F, F)[:, i, j] if skip else G
    return full + full.transpose(0, 2, 1)


def backward(X, G, self_i, skip, existing=None, mask=0, chunked=False):
    """X [B, F, D], G [B, cols], existing [B, F, D] or None -> (dX, S, partial): partial is the sum of |what the block
    kernel stored after each chunk but the last| (zero unless chunked and F > 128)."""
    B, F, D = X.shape
    Gs = scatter_gradient(G, F, self_i, skip)
    base = np.zeros((B, F, D))
    if existing is not None:
        for f in range(min(F, 64)):
            if (mask >> f) & 1:
                base[:, f] = existing[:, f]
    dX, S, partial = base.copy(), np.abs(base), np.zeros((B, F, D))
    for j0 in range(0, F, CHUNK if chunked else F):
        j1 = min(F, j0 + (CHUNK if chunked else F))
        dX = dX + np.einsum("bij,bjd->bid", Gs[:, :, j0:j1], X[:, j0:j1])
        S = S + np.einsum("bij,bjd->bid", np.abs(Gs[:, :, j0:j1]), np.abs(X[:, j0:j1]))
        if j1 < F:
            partial = partial + np.abs(dX)
    return dX, S, partial


def bound(exact, S, n, bf16, partial=None):
    r = R_BF16 if bf16 else 0.0
    tol = (n + 2) * U32 * S + r * np.abs(exact)
    return tol if partial is None else tol + r * partial


def to_storage(x32, bf16):
    """an fp32 array rounded once to the storage type, widened back (exactly) to float32"""
    if not bf16:
        return x32.astype(np.float32)
    import torch

    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def forward_fp32(X, self_i, skip, bf16):
    """the forward in numpy float32: products accumulated in order of c, one rounding to the storage type"""
    B, F, D = X.shape
    x = X.astype(np.float32)
    P = np.zeros((B, F, F), dtype=np.float32)
    for c in range(D):
        P += x[:, :, None, c] * x[:, None, :, c]
    i, j = kept_pairs(F, self_i)
    if not skip:
        return to_storage(P[:, i, j], bf16)
    keep = np.zeros((F, F), dtype=bool)
    keep[i, j] = True
    return to_storage(np.where(keep, P, np.float32(0)).reshape(B, F * F), bf16)


def backward_fp32(X, G, self_i, skip, bf16, existing=None, mask=0, chunked=False):
    """the backward in numpy float32: products accumulated in order of j, the existing gradient added last (first on
    the chunked kernel, which also rounds once per chunk), one rounding to the storage type"""
    B, F, D = X.shape
    x = X.astype(np.float32)
    Gs = scatter_gradient(G, F, self_i, skip).astype(np.float32)     # (one element of G or twice one: exact)
    base = np.zeros((B, F, D), dtype=np.float32)
    if existing is not None:
        for f in range(min(F, 64)):
            if (mask >> f) & 1:
                base[:, f] = existing[:, f].astype(np.float32)
    if not chunked:
        acc = np.zeros((B, F, D), dtype=np.float32)
        for j in range(F):
            acc += Gs[:, :, j, None] * x[:, None, j, :]
        return to_storage(acc + base, bf16)
    out = base
    for j0 in range(0, F, CHUNK):
        acc = np.zeros((B, F, D), dtype=np.float32)
        for j in range(j0, min(F, j0 + CHUNK)):
            acc += Gs[:, :, j, None] * x[:, None, j, :]
        out = to_storage(acc + out, bf16)
    return out
