"""K13 without a device: the workspace formula of krs_retrieval_xent_workspace_bytes (host only: it launches
nothing), the restatement's own consistency, and the argument errors of InBatchSoftmaxLoss and retrieval_xent that are
raised before any device work."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_xent_restatement as X

MIB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd.build import build

    build()
    return L.lib()


@pytest.mark.parametrize("b,n,d", [(256, 2**20, 128), (65536, 65536, 128), (1024, 1024, 256), (1, 1, 1)])
def test_workspace_is_linear_in_the_inputs(lib, b, n, d):
    size = lib.krs_retrieval_xent_workspace_bytes(b, n, d, L.BF16)
    assert 0 <= size <= 64 * MIB + 16 * (b + n) * d * 4
    assert size == retrieval_ops.retrieval_xent_workspace_bytes(b, n, d)


def test_workspace_never_scales_with_b_times_n(lib):
    for d in (1, 8, 64, 256):
        for b in (1, 100, 128, 129, 4096, 65535, 65536, 10**6):
            for n in (1, 31, 32, 33, 4096, 65536, 2**20, 2**24):
                size = lib.krs_retrieval_xent_workspace_bytes(b, n, d, L.BF16)
                assert size <= 64 * MIB + 16 * (b + n) * d * 4, (b, n, d, size)
    assert lib.krs_retrieval_xent_workspace_bytes(0, 5, 8, L.BF16) == 0


def test_small_shapes_that_must_split_have_a_workspace(lib):
    # few owner rows against many streamed rows: the sweeps are cut into slices, whose partials need room
    assert lib.krs_retrieval_xent_workspace_bytes(300, 1000, 128, L.BF16) > 0
    assert lib.krs_retrieval_xent_workspace_bytes(256, 2**20, 128, L.BF16) >= 2 * 256 * 128 * 4
    # enough owner rows on both sides: one slice, nothing to keep
    assert lib.krs_retrieval_xent_workspace_bytes(65536, 65536, 128, L.BF16) == 0


def test_entry_points_refuse_what_the_kernels_do_not_cover(lib):
    # (argument checks return before any launch or device call)
    args_tail = (None, None, None, L.I32, 0.0, 0.0, None, None, None, 0, None)
    assert lib.krs_retrieval_xent_fwd(None, 8, None, 8, L.F32, 4, 4, 8, *args_tail) != 0       # fp32 inputs
    assert b"bf16" in lib.krs_last_error()
    assert lib.krs_retrieval_xent_fwd(None, 300, None, 300, L.BF16, 4, 4, 300, *args_tail) != 0  # d > 256
    assert lib.krs_retrieval_xent_fwd(None, 8, None, 8, L.BF16, 4, 0, 8, *args_tail) != 0       # no candidate
    assert lib.krs_retrieval_xent_fwd(None, 8, None, 8, L.BF16, 4, 4, 0, *args_tail) != 0       # no column
    assert lib.krs_retrieval_xent_fwd(None, 8, None, 8, L.BF16, 0, 4, 8, *args_tail) == 0       # b == 0: no-op
    assert lib.krs_retrieval_xent_bwd(None, 8, None, 8, L.BF16, 4, 4, 8, None, None, None, L.I32, 0.0, 0.0, None, None,
                                      1.0, None, 8, None, 8, None, 0, None) != 0                # neither gradient


def test_restatement_matches_the_stored_matrix_restatement():
    from tests import retrieval_loss_restatement as R

    g = torch.Generator().manual_seed(3)
    q, c = torch.randn(7, 5, generator=g).double(), torch.randn(11, 5, generator=g).double()
    prob = torch.rand(11, generator=g).double()
    ids = torch.tensor([0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 0])
    bias = -torch.log(torch.clamp(prob, 1e-6, 1.0))
    mine = X.row_loss(q, c, bias=bias, ids=ids, hit_value=-50.0).mean()
    theirs, _, _ = R.retrieval_head(q, c, cand_ids=ids, cand_prob=prob, value=-50.0)
    assert abs(float(mine) - float(theirs)) < 1e-12
    ref = X.reference(q, c, bias=bias, ids=ids, hit_value=-50.0, ls=0.1)
    assert torch.allclose(ref["loss"], X.row_loss(q, c, bias=bias, ids=ids, hit_value=-50.0, ls=0.1))
    assert bool((ref["loss_tol"] > 0).all() and (ref["dq_tol"] > 0).all() and (ref["dc_tol"] > 0).all())


def test_layer_config_round_trip_and_export():
    loss = layers.InBatchSoftmaxLoss(label_smoothing=0.1, reduction="sum", epsilon=1e-5, accidental_hit_value=-1e30)
    cfg = loss.get_config()
    assert cfg == {"name": "in_batch_softmax_loss", "label_smoothing": 0.1, "reduction": "sum", "epsilon": 1e-5,
                   "accidental_hit_value": -1e30}
    assert layers.InBatchSoftmaxLoss.from_config(cfg).get_config() == cfg
    assert layers.InBatchSoftmaxLoss().accidental_hit_value == retrieval_ops.SMALLEST_FLOAT
    assert "InBatchSoftmaxLoss" in layers.__all__


def test_layer_constructor_errors():
    with pytest.raises(ValueError, match="label_smoothing"):
        layers.InBatchSoftmaxLoss(label_smoothing=1.0)
    with pytest.raises(ValueError, match="reduction"):
        layers.InBatchSoftmaxLoss(reduction="median")
    with pytest.raises(ValueError, match="finite"):
        layers.InBatchSoftmaxLoss(accidental_hit_value=float("-inf"))


def test_layer_shape_and_dtype_errors_name_both_shapes():
    loss = layers.InBatchSoftmaxLoss()
    q, c = torch.zeros(4, 8), torch.zeros(6, 8)
    both = r"\(4, 8\).*\(6, 8\)"
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(6, 7\)"):
        loss(q, torch.zeros(6, 7))
    with pytest.raises(ValueError, match=r"\(4,\).*\(6, 8\)"):
        loss(torch.zeros(4), c)
    with pytest.raises(ValueError, match=r"\(4, 8\).*\(0, 8\)"):
        loss(q, torch.zeros(0, 8))
    with pytest.raises(ValueError, match="share a dtype.*" + both):
        loss(q, c.to(torch.bfloat16))
    with pytest.raises(ValueError, match="float32 or bfloat16.*" + both):
        loss(q.to(torch.float16), c.to(torch.float16))
    with pytest.raises(ValueError, match="positive_index.*" + both):
        loss(q, c, positive_index=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="positive_index.*" + both):
        loss(q, c, positive_index=torch.zeros(4))
    with pytest.raises(ValueError, match="candidate_ids.*" + both):
        loss(q, c, candidate_ids=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="candidate_sampling_probability.*" + both):
        loss(q, c, candidate_sampling_probability=torch.zeros(4))
    with pytest.raises(ValueError, match="sample_weight"):
        loss(q, c, sample_weight=torch.zeros(3))
    # well-formed arguments on the host: there is no CPU fallback
    with pytest.raises(L.KrsError, match="no CPU fallback"):
        loss(q, c)


def test_op_argument_errors():
    q, c = torch.zeros(4, 8), torch.zeros(6, 8)
    with pytest.raises(L.KrsError, match="path"):
        retrieval_ops.retrieval_xent(q, c, path="fast")
    with pytest.raises(L.KrsError, match="label_smoothing"):
        retrieval_ops.retrieval_xent(q, c, label_smoothing=1.5)
