"""krs_topk_rows with a boost operand and HardNegativeMining on the GPU (K8)."""

import numpy as np
import pytest
import torch

from keras_rs_amd import retrieval_ops
from keras_rs_amd.layers import HardNegativeMining
from tests.retrieval_restatement import order_key as _order_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _expected(keys: np.ndarray, k: int) -> np.ndarray:
    out = np.empty((keys.shape[0], k), np.int64)
    for r, row in enumerate(keys):
        order = np.lexsort((np.arange(row.size), -row.astype(np.int64)))
        out[r] = order[:k]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,k", [(3, 100000, 50), (2, 1000000, 129), (5, 1000, 7), (4, 3000, 3000)])
def test_topk_rows_boost(dtype, rows, cols, k):
    rng = np.random.default_rng(rows + cols + k)
    x = rng.integers(-50, 50, size=(rows, cols)).astype(np.float32)     # many ties
    lab = (rng.random((rows, cols)) < 0.001).astype(np.float32)
    xt = torch.from_numpy(x).to(DEV, dtype)
    bt = torch.from_numpy(lab).to(DEV, dtype)
    scale = retrieval_ops.MAX_FLOAT
    idx, keys = retrieval_ops.topk_rows(xt, k, boost=bt, boost_scale=scale, want_keys=True)
    kf = (xt.float() + bt.float() * scale).cpu().numpy()
    exp = _expected(_order_key(kf), k)
    np.testing.assert_array_equal(idx.cpu().numpy(), exp)
    np.testing.assert_array_equal(keys.cpu().numpy(), np.take_along_axis(kf, exp, 1))
    again = retrieval_ops.topk_rows(xt, k, boost=bt, boost_scale=scale)
    assert torch.equal(idx, again)


def test_topk_rows_special_values():
    x = np.array([[1.0, np.nan, 0.0, -0.0, np.inf, -np.inf, 0.0, -0.0, 2.0, -1.0] * 300], np.float32)
    xt = torch.from_numpy(x).to(DEV)
    for cols in (10, 3000):
        for k in (1, 3, 6, 10):
            idx, keys = retrieval_ops.topk_rows(xt[:, :cols], k, want_keys=True)
            exp = _expected(_order_key(x[:, :cols]), k)
            np.testing.assert_array_equal(idx.cpu().numpy(), exp)
            assert np.isnan(keys.cpu().numpy()[0, 0])
    idx = retrieval_ops.topk_rows(xt[:, :10], 10).cpu().numpy()[0]
    # NaN, +inf, 2, 1, then the four zeros in index order (-0.0 == +0.0), -1, -inf
    np.testing.assert_array_equal(idx, [1, 4, 8, 0, 2, 3, 6, 7, 9, 5])


@pytest.mark.parametrize("h", [3, 30])
@pytest.mark.parametrize("shape", [(20,), (16, 40), (4, 6, 25)])
def test_hard_negative_mining_properties(h, shape):
    rng = np.random.default_rng(h + len(shape))
    c = shape[-1]
    logits = rng.normal(size=shape).astype(np.float32)
    pos = rng.integers(0, c, size=shape[:-1])
    labels = np.zeros(shape, np.float32)
    np.put_along_axis(labels, np.expand_dims(pos, -1), 1.0, -1)
    lt = torch.from_numpy(logits).to(DEV).requires_grad_(True)
    lb = torch.from_numpy(labels).to(DEV)
    out_l, out_y = HardNegativeMining(h)(lt, lb)
    ns = min(h + 1, c)
    assert out_l.shape == shape[:-1] + (ns,) and out_y.shape == out_l.shape
    ol, oy = out_l.detach().cpu().numpy(), out_y.cpu().numpy()
    # the positive is always kept
    np.testing.assert_array_equal(oy.sum(-1), np.ones(shape[:-1]))
    np.testing.assert_array_equal(ol[oy == 1], np.take_along_axis(logits, np.expand_dims(pos, -1), -1)[..., 0].ravel())
    # with boosted labels the highest h + 1 logits come back, in order
    boosted = np.where(labels == 1, 1e30, logits)
    want = -np.sort(-boosted, axis=-1)[..., :ns]
    np.testing.assert_array_equal(np.where(oy == 1, 1e30, ol), want)
    # the gradient reaches logits as through torch.gather with the same indices
    g = torch.from_numpy(rng.normal(size=out_l.shape).astype(np.float32)).to(DEV)
    (out_l * g).sum().backward()
    keys = lt.detach() + lb * retrieval_ops.MAX_FLOAT
    idx = torch.sort(keys, dim=-1, descending=True, stable=True).indices[..., :ns]
    lt2 = lt.detach().clone().requires_grad_(True)
    (torch.gather(lt2, -1, idx) * g).sum().backward()
    assert torch.equal(lt.grad, lt2.grad)
