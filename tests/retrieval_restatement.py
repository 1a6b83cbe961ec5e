"""K8's contract restated in numpy, for the retrieval tests: the total order as a uint32 key, the top-k it selects from
float64 scores, and the float64 score matrix of dtype-rounded inputs.  Nothing here runs on the GPU or reads the planner."""

import numpy as np
import torch

TORCH_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def order_key(x: np.ndarray) -> np.ndarray:
    """The contract's total order as uint32 (-0.0 == +0.0, NaN above +inf)."""
    u = x.astype(np.float32).view(np.uint32).copy()
    nan = np.isnan(x)
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    key[nan] = 0xFFFFFFFF
    return key


def expected_topk(scores64: np.ndarray, k: int) -> np.ndarray:
    """[rows, k] int64 indices of the k first entries of each row in the contract's order: the key of the score (as fp32)
    descending, then the index ascending.  For scores that fp32 holds exactly."""
    with np.errstate(over="ignore", invalid="ignore"):
        keys = order_key(scores64)
    out = np.empty((keys.shape[0], k), np.int64)
    index = np.arange(keys.shape[1])
    for r, row in enumerate(keys):
        out[r] = np.lexsort((index, -row.astype(np.int64)))[:k]
    return out


def rounded(a: np.ndarray, dtype: str) -> np.ndarray:
    """a (fp32 values) as `dtype` holds it, in float64."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH_DTYPES[dtype])
    return t.float().numpy().astype(np.float64)


def scores64(q: np.ndarray, c: np.ndarray, dtype: str) -> np.ndarray:
    """The float64 score matrix q . c^T of the dtype-rounded inputs.  Inputs with a NaN or an infinity are multiplied
    out column by column, so that 0 * inf is the NaN of IEEE arithmetic whatever the BLAS does with zeros."""
    qq, cc = rounded(q, dtype), rounded(c, dtype)
    if np.isfinite(qq).all() and np.isfinite(cc).all():
        return qq @ cc.T
    with np.errstate(invalid="ignore"):
        s = np.zeros((qq.shape[0], cc.shape[0]), np.float64)
        for j in range(qq.shape[1]):
            s += qq[:, j:j + 1] * cc[None, :, j]
    return s


def abs_scores64(q: np.ndarray, c: np.ndarray, dtype: str) -> np.ndarray:
    """|q| . |c|^T of the dtype-rounded inputs: what the rounding error of a score is proportional to."""
    return np.abs(rounded(q, dtype)) @ np.abs(rounded(c, dtype)).T
