"""K14 without a device: the float64 restatement against the stored-matrix head's restatement with mining, its tie
rule, the layer's new argument and config, and the new entry points of the C ABI (declared, bound, exported, and their
argument checks, which return before any device work)."""

import re

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_loss_restatement as R
from tests import retrieval_mined_restatement as M

NEW = ("krs_retrieval_mine_workspace_bytes", "krs_retrieval_mine")


@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd.build import build

    build()
    return L.lib()


@pytest.mark.parametrize("k", [1, 3, 10, 50])
def test_restatement_matches_the_stored_matrix_head_with_mining(k):
    g = torch.Generator().manual_seed(5)
    q, c = torch.randn(7, 5, generator=g).double(), torch.randn(11, 5, generator=g).double()
    prob = torch.rand(11, generator=g).double()
    ids = torch.tensor([0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 0])
    bias = -torch.log(torch.clamp(prob, 1e-6, 1.0))
    kk = min(k, 10)
    mine = M.row_loss(q, c, kk, bias=bias, ids=ids, hit_value=-50.0).mean()
    theirs, kept, labels = R.retrieval_head(q, c, cand_ids=ids, cand_prob=prob, num_hard_negatives=k, value=-50.0)
    assert tuple(kept.shape) == (7, kk + 1)
    assert abs(float(mine) - float(theirs)) < 1e-12
    ref = M.reference(q, c, kk, bias=bias, ids=ids, hit_value=-50.0, ls=0.1)
    assert torch.allclose(ref["loss"], M.row_loss(q, c, kk, bias=bias, ids=ids, hit_value=-50.0, ls=0.1))
    assert bool((ref["loss_tol"] > 0).all() and (ref["dq_tol"] > 0).all())
    # the kept set is the head's: the same negatives, whatever their order
    their_negatives = torch.sort(kept[labels == 0].view(7, kk), -1).values
    assert torch.equal(torch.sort(ref["scores"], -1).values, their_negatives.detach())
    # candidates nobody mined get no gradient and no tolerance
    mined = torch.zeros(11, dtype=torch.bool)
    mined[ref["idx"].reshape(-1)] = True
    mined[:7] = True
    assert bool((ref["dc"][~mined] == 0).all() and (ref["dc_tol"][~mined] == 0).all())


def test_restatement_breaks_a_tie_at_the_kth_place_by_index():
    # candidates 2, 4 and 5 are one vector: with k = 2 the winner 1 and the FIRST of the three are kept
    c = torch.tensor([[1.0, 0.0], [3.0, 0.0], [2.0, 0.0], [0.5, 0.0], [2.0, 0.0], [2.0, 0.0], [-0.0, 0.0], [0.0, 0.0]],
                     dtype=torch.float64)
    q = torch.tensor([[1.0, 0.0], [1.0, 0.0], [-1.0, 0.0]], dtype=torch.float64)
    pos = torch.tensor([0, 2, 1])
    ref = M.reference(q, c, 2, pos=pos)
    assert ref["idx"].tolist() == [[1, 2], [1, 4], [6, 7]]      # row 1: its positive 2 is skipped; row 2: -0.0 == +0.0
    assert ref["gap"].tolist() == [0.0, 0.0, 0.5]
    assert M.reference(q, c, 4, pos=pos)["idx"][0].tolist() == [1, 2, 4, 5]
    # a positive outside [0, N): nothing is excluded, the loss is NaN, the other rows are untouched
    bad = M.reference(q, c, 2, pos=torch.tensor([0, 8, -1]))
    assert bad["idx"].tolist() == [[1, 2], [1, 2], [6, 7]]
    assert bad["ok"].tolist() == [True, False, False]
    assert bool(torch.isnan(bad["loss"][1:]).all()) and float(bad["loss"][0]) == float(ref["loss"][0])
    assert bool(torch.isfinite(bad["dq"]).all() and torch.isfinite(bad["dc"]).all())
    assert torch.nonzero(bad["nan_dc"])[:, 0].tolist() == [1, 2, 6, 7]


def test_layer_argument_errors():
    for bad in (0, -3, 2.5, "32", True):
        with pytest.raises(ValueError, match="num_hard_negatives"):
            layers.InBatchSoftmaxLoss(num_hard_negatives=bad)
    q, c = torch.zeros(4, 8), torch.zeros(6, 8)
    for bad in (0, 1.5, True):
        with pytest.raises(L.KrsError, match="num_hard_negatives"):
            retrieval_ops.retrieval_xent(q, c, num_hard_negatives=bad)
    with pytest.raises(L.KrsError, match="path"):
        retrieval_ops.retrieval_xent(q, c, num_hard_negatives=2, path="fast")
    with pytest.raises(L.KrsError, match="label_smoothing"):
        retrieval_ops.retrieval_xent(q, c, num_hard_negatives=2, label_smoothing=1.0)
    # well-formed arguments on the host: there is no CPU fallback
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        layers.InBatchSoftmaxLoss(num_hard_negatives=2)(q, c)


def test_layer_config_round_trip_in_both_forms():
    unset = layers.InBatchSoftmaxLoss(label_smoothing=0.1, reduction="sum")
    assert "num_hard_negatives" not in unset.get_config() and unset.num_hard_negatives is None
    assert layers.InBatchSoftmaxLoss.from_config(unset.get_config()).get_config() == unset.get_config()
    mined = layers.InBatchSoftmaxLoss(label_smoothing=0.1, reduction="sum", num_hard_negatives=32)
    cfg = mined.get_config()
    assert cfg == dict(unset.get_config(), num_hard_negatives=32)
    again = layers.InBatchSoftmaxLoss.from_config(cfg)
    assert again.num_hard_negatives == 32 and again.get_config() == cfg


def test_new_symbols_are_declared_bound_and_exported(lib):
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "krs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared in include/krs.h"
        assert name in L.PROTOTYPES and name in L.SYMBOLS
        assert hasattr(lib, name), f"libkrs_hip.so does not export {name}"
    assert len(L.PROTOTYPES["krs_retrieval_mine"][1]) == 20


def test_workspace_is_the_slice_lists(lib):
    # b * S * k pairs of 8 bytes (S = 8 here) and nothing that scales with b * n
    assert lib.krs_retrieval_mine_workspace_bytes(4096, 4096, 32, 8, L.BF16) == 4096 * 8 * 8 * 8
    assert retrieval_ops.retrieval_mine_workspace_bytes(4096, 4096, 32, 8) == 4096 * 8 * 8 * 8
    for b, n in ((1, 2), (70, 3000), (65536, 65536), (256, 2**24)):
        for k in (1, 32, 128):
            if k > n - 1:
                continue
            size = lib.krs_retrieval_mine_workspace_bytes(b, n, 64, k, L.F32)
            tiles, cut = -(-b // 32), -(-n // 8192)
            slices = max(8, min(-(-2048 // tiles), cut) + 7)         # S, rounded up to a multiple of 8
            assert 0 < size <= 512 + b * 8 * (slices * k + 128), (b, n, k, size)
    assert lib.krs_retrieval_mine_workspace_bytes(0, 5, 8, 2, L.BF16) == 0


def test_entry_point_refuses_bad_arguments_before_any_launch(lib):
    def call(b=4, n=6, d=8, k=2, dtype=L.BF16, ldq=8, ldc=8, q=None, ws_bytes=0):
        return lib.krs_retrieval_mine(q, ldq, None, ldc, dtype, b, n, d, k, None, None, None, L.I32, 0.0, None, None,
                                      None, None, ws_bytes, None)

    assert call(k=0) == -1 and b"k = 0" in lib.krs_last_error()             # KRS_ERR_INVALID
    assert call(k=6) == -1 and b"k = 6" in lib.krs_last_error()             # k = n
    assert call(k=129, n=1000) == -1                                       # beyond the fused kernel
    assert call(d=513, ldq=513, ldc=513) == -1
    assert call(ldc=7) == -1
    assert call(dtype=7) == -1
    assert call() == -1 and b"null" in lib.krs_last_error()                 # null operands
    assert call(b=0) == 0                                                  # b == 0: a successful no-op
