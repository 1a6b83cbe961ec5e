"""Host-side checks of the retrieval layers (K8): constructor / update errors, config round trip, HardNegativeMining's
sample count, and the C ABI's symbols and workspace sizes -- none of it needs a GPU."""

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import retrieval_ops
from keras_rs_amd.layers import BruteForceRetrieval, HardNegativeMining, Retrieval

RNG = np.random.default_rng(7)
EMB = RNG.normal(size=(50, 8)).astype(np.float32)


def test_ids_without_embeddings():
    with pytest.raises(ValueError, match="without providing `candidate_embeddings`"):
        BruteForceRetrieval(candidate_ids=np.arange(50), k=5)


@pytest.mark.parametrize("shape", [(50,), (5, 10, 8)])
def test_rank_not_two(shape):
    with pytest.raises(ValueError, match="rank 2"):
        BruteForceRetrieval(np.zeros(shape, np.float32), k=1)


def test_fewer_candidates_than_k():
    with pytest.raises(ValueError, match=r"less than the number of candidates to retrieve \(k=51\)"):
        BruteForceRetrieval(EMB, k=51)
    layer = BruteForceRetrieval(k=60)
    with pytest.raises(ValueError, match="less than"):
        layer.update_candidates(EMB)


def test_id_length_mismatch():
    with pytest.raises(ValueError, match="same number of rows"):
        BruteForceRetrieval(EMB, np.arange(49), k=5)


def test_new_ids_on_idless_layer():
    layer = BruteForceRetrieval(EMB, k=5)
    with pytest.raises(ValueError, match="did not have candidate IDs"):
        layer.update_candidates(EMB, np.arange(50))


def test_update_changed_shape_raises_and_same_shape_copies_in_place():
    layer = BruteForceRetrieval(EMB, np.arange(50), k=5)
    w = layer.candidate_embeddings
    ptr = w.data_ptr()
    with pytest.raises(ValueError, match="Cannot assign"):
        layer.update_candidates(EMB[:40], np.arange(40))
    new = EMB[::-1].copy()
    layer.update_candidates(new, np.arange(100, 150))
    assert layer.candidate_embeddings is w and w.data_ptr() == ptr
    np.testing.assert_array_equal(w.detach().cpu().numpy(), new)
    np.testing.assert_array_equal(layer.candidate_ids.detach().cpu().numpy(), np.arange(100, 150))
    assert layer.candidate_ids.dtype == torch.int32
    assert not w.requires_grad and layer.trainable_weights == []


def test_get_config_round_trip():
    layer = BruteForceRetrieval(EMB, k=7, return_scores=False, name="retr")
    cfg = layer.get_config()
    assert cfg["k"] == 7 and cfg["return_scores"] is False
    clone = BruteForceRetrieval.from_config(cfg)
    assert clone.k == 7 and clone.return_scores is False and clone.get_config() == cfg
    assert isinstance(clone, Retrieval) and clone.candidate_embeddings is None
    h = HardNegativeMining(num_hard_negatives=3)
    assert HardNegativeMining.from_config(h.get_config()).get_config() == h.get_config()


def test_query_shape_checked_before_device():
    layer = BruteForceRetrieval(EMB, k=5)
    with pytest.raises(ValueError, match="query must have shape"):
        layer(torch.zeros(3, 9))


def test_hard_negative_mining_num_sampled():
    assert HardNegativeMining(3).num_sampled(100) == 4
    assert HardNegativeMining(30).num_sampled(10) == 10
    assert HardNegativeMining(9).num_sampled(10) == 10


def test_symbols_exported_by_build():
    from keras_rs_amd.build import build

    build()
    lib = L.lib()
    for name in ("krs_topk_rows", "krs_topk_rows_workspace_bytes", "krs_retrieval_topk",
                 "krs_retrieval_topk_workspace_bytes"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.krs_version() == 100


def test_workspace_sizes_without_gpu():
    from keras_rs_amd.build import build

    build()
    # fused path: per-slice lists (b x S x k pairs); no GPU is touched
    fused = retrieval_ops.retrieval_topk_workspace_bytes(64, 1 << 20, 128, 100, torch.bfloat16)
    assert fused >= 64 * 100 * 8
    assert retrieval_ops.retrieval_topk_workspace_bytes(16, 100, 4, 20, torch.float32) >= 16 * 20 * 8
    # two-step path (k > 128): one fp32 slab chunk, bounded near 1 GiB
    two = retrieval_ops.retrieval_topk_workspace_bytes(8192, 1 << 20, 128, 129, torch.bfloat16)
    assert (1 << 20) * 4 <= two <= (1 << 30) + (1 << 26)
    assert retrieval_ops.retrieval_topk_workspace_bytes(0, 100, 4, 20, torch.float32) == 0
    # row top-k: short rows sort in LDS (no workspace), long rows keep a list of k pairs per row
    assert retrieval_ops.topk_rows_workspace_bytes(10, 2048, 5) == 0
    assert retrieval_ops.topk_rows_workspace_bytes(10, 100000, 31) == 10 * 32 * 8
