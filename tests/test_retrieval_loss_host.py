"""Host-side checks of the retrieval training head (K11): the float64 restatement the GPU tests compare against agrees
with an independent implementation and with closed forms, constructor / config round trips, every NotImplementedError
and the reference's two ValueErrors (raised on CPU tensors, before any device check), and the C ABI's refusals that
return before any launch -- none of it needs a GPU."""

import math

import numpy as np
import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_loss_restatement as R

ENTRIES = ["krs_softmax_xent", "krs_sampling_correction", "krs_remove_accidental_hits"]


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 2, 65, 1025])
def test_restatement_agrees_with_torch_cross_entropy(n, ls):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn((7, n), generator=g, dtype=torch.float64) * 30.0).requires_grad_(True)
    y = torch.softmax(torch.randn((7, n), generator=g, dtype=torch.float64), -1)     # soft targets that sum to 1
    ours = R.row_loss(x, y, ls)
    theirs = torch.nn.functional.cross_entropy(x, y, label_smoothing=ls, reduction="none")
    assert float((ours - theirs).detach().abs().max()) <= 1e-12
    w = torch.rand(7, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad((ours * w).sum(), x)
    assert float((gx - R.row_grad(x.detach(), y, ls, w)).abs().max()) <= 1e-12
    hot = torch.randint(0, n, (7,), generator=g)
    sparse = torch.nn.functional.cross_entropy(x, hot, reduction="none")
    assert float((R.row_loss(x, R.one_hot(hot, n)) - sparse).detach().abs().max()) <= 1e-12


@pytest.mark.parametrize("n", [1, 3, 1000])
def test_restatement_closed_forms(n):
    x = torch.full((2, n), 3.25, dtype=torch.float64)
    y = R.one_hot(torch.tensor([0, n - 1]), n)
    assert float((R.row_loss(x, y) - math.log(n)).abs().max()) <= 1e-12
    g = torch.tensor([0.5, -2.0], dtype=torch.float64)
    assert float((R.row_grad(x, y, 0.0, g) - (1.0 / n - y) * g[:, None]).abs().max()) <= 1e-15
    # labels are not renormalised: twice the labels, twice the loss
    assert float((R.row_loss(x, 2.0 * y) - 2.0 * math.log(n)).abs().max()) <= 1e-12


def test_restatement_reductions():
    v = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    w = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    assert float(R.reduce(v, None, "sum_over_batch_size")) == 2.5 and float(R.reduce(v, w, "sum")) == 24.0
    assert float(R.reduce(v, w, "mean")) == 6.0 and float(R.reduce(v, w, "mean_with_sample_weight")) == 3.0
    assert float(R.reduce(v, 0.0 * w, "mean_with_sample_weight")) == 0.0
    assert R.reduce(v, w, None).tolist() == [[1.0, 2.0], [9.0, 12.0]]


def test_restatement_of_the_accidental_hits_expression():
    ids = np.array([4, 7, 4, 9])
    labels = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]], np.float32)     # all-zero row: position 0
    got = R.remove_accidental_hits_f32(np.zeros((3, 4), np.float32), labels, ids, -1e9)
    assert got.tolist() == [[-1e9, 0, 0, 0], [0, 0, 0, 0], [-1e9, 0, -1e9, 0]]
    tiny = R.remove_accidental_hits_f32(np.zeros((3, 4), np.float32), labels, ids, retrieval_ops.SMALLEST_FLOAT)
    assert tiny[0, 0] == np.float32(retrieval_ops.SMALLEST_FLOAT) and 0 < tiny[0, 0] < np.finfo(np.float32).tiny


def test_the_constant_is_the_reference_value():
    tiny = float(np.finfo(np.float32).tiny)
    assert retrieval_ops.SMALLEST_FLOAT == pytest.approx(tiny / 100.0, rel=1e-5)
    assert np.float32(retrieval_ops.SMALLEST_FLOAT) == np.float32(1.1754944e-40)
    assert retrieval_ops.SMALLEST_FLOAT == float(np.float32(retrieval_ops.SMALLEST_FLOAT))    # exact in fp32


# ---- constructors and configs ------------------------------------------------------------------------------------------
def test_loss_config_round_trips():
    loss = layers.CategoricalCrossentropy(label_smoothing=0.25, reduction="sum", name="mine")
    cfg = loss.get_config()
    assert cfg == {"name": "mine", "reduction": "sum", "from_logits": True, "label_smoothing": 0.25, "axis": -1}
    assert layers.CategoricalCrossentropy.from_config(cfg).get_config() == cfg
    default = layers.CategoricalCrossentropy()
    assert default.name == "categorical_crossentropy" and default.reduction == "sum_over_batch_size"
    assert default.label_smoothing == 0.0 and default.from_logits
    sparse = layers.SparseCategoricalCrossentropy(reduction=None, name="s")
    cfg = sparse.get_config()
    assert cfg["reduction"] is None and cfg["name"] == "s" and cfg["from_logits"] is True
    assert layers.SparseCategoricalCrossentropy.from_config(cfg).get_config() == cfg
    assert layers.SparseCategoricalCrossentropy().name == "sparse_categorical_crossentropy"


def test_layer_config_round_trips():
    layer = layers.SamplingProbabilityCorrection(epsilon=1e-3, name="spc")
    cfg = layer.get_config()
    assert cfg["epsilon"] == 1e-3 and cfg["name"] == "spc"
    assert layers.SamplingProbabilityCorrection.from_config(cfg).get_config() == cfg
    assert layers.SamplingProbabilityCorrection().epsilon == 1e-6
    rah = layers.RemoveAccidentalHits(name="rah")
    assert layers.RemoveAccidentalHits.from_config(rah.get_config()).get_config() == rah.get_config()


@pytest.mark.parametrize("cls", [layers.CategoricalCrossentropy, layers.SparseCategoricalCrossentropy])
def test_unimplemented_arguments_say_so(cls):
    with pytest.raises(NotImplementedError, match="from_logits=False"):
        cls(from_logits=False)
    with pytest.raises(NotImplementedError, match="axis"):
        cls(axis=0)
    with pytest.raises(ValueError, match="reduction"):
        cls(reduction="max")


def test_ignore_class_and_label_smoothing_range():
    with pytest.raises(NotImplementedError, match="ignore_class"):
        layers.SparseCategoricalCrossentropy(ignore_class=-1)
    for ls in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            layers.CategoricalCrossentropy(label_smoothing=ls)


def test_reference_value_errors_come_before_the_device_check():
    layer = layers.RemoveAccidentalHits()
    with pytest.raises(ValueError, match="`labels` and `logits` should have the same shape"):
        layer(torch.zeros((10, 20)), torch.zeros((10, 30)), torch.zeros((20,), dtype=torch.int32))
    with pytest.raises(ValueError, match="`candidate_ids` should have the same shape as the last dimensions of "
                                         "`labels`"):
        layer(torch.zeros((10, 20)), torch.zeros((10, 20)), torch.zeros((30,), dtype=torch.int32))
    with pytest.raises(ValueError, match="last dimensions of `logits`"):
        layers.SamplingProbabilityCorrection()(torch.zeros((10, 20)), torch.full((30,), 0.5))
    with pytest.raises(ValueError, match="rank 1 to 3"):
        layers.SamplingProbabilityCorrection()(torch.zeros((2, 2, 2, 2)), torch.full((2,), 0.5))


def test_loss_shape_errors_come_before_the_device_check():
    with pytest.raises(ValueError, match="same shape"):
        layers.CategoricalCrossentropy()(torch.zeros((4, 5)), torch.zeros((4, 6)))
    with pytest.raises(ValueError, match="without its last axis"):
        layers.SparseCategoricalCrossentropy()(torch.zeros((5,), dtype=torch.int64), torch.zeros((4, 6)))
    with pytest.raises(ValueError, match="sample_weight"):
        layers.CategoricalCrossentropy()(torch.zeros((4, 6)), torch.zeros((4, 6)), sample_weight=torch.ones(3))


def test_cpu_tensors_are_refused():
    x = torch.zeros((4, 6))
    ids = torch.zeros((6,), dtype=torch.int32)
    for call in (lambda: layers.CategoricalCrossentropy()(x, x),
                 lambda: layers.SparseCategoricalCrossentropy()(torch.zeros((4,), dtype=torch.int64), x),
                 lambda: layers.SamplingProbabilityCorrection()(x, torch.full((6,), 0.5)),
                 lambda: layers.RemoveAccidentalHits()(x, x, ids)):
        with pytest.raises(L.KrsError, match="no CPU fallback"):
            call()


# ---- the C ABI's refusals (every one returns before a launch: the pointers below are never dereferenced) --------------
@pytest.fixture(scope="module")
def lib():
    from keras_rs_amd.build import build

    build()
    return L.lib()


def test_symbols_listed():
    for name in ENTRIES:
        assert name in L.SYMBOLS


def _refused(lib, rc, *words):
    assert rc == -1                                    # KRS_ERR_INVALID
    msg = lib.krs_last_error().decode()
    for w in words:
        assert w in msg, msg


P = 4096    # a non-null placeholder address


def xent_args(**kw):
    a = dict(logits=P, ld=8, dtype=0, labels=P, ld_labels=8, label_index=None, ls=0.0, g=None, g_scale=1.0, rows=2,
             cols=8, row_loss=P, dlogits=P, ld_dlogits=8, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,words", [
    (dict(logits=None), ["null logits"]),
    (dict(cols=0), ["0 columns"]),
    (dict(ls=1.0), ["label_smoothing", "[0, 1)"]),
    (dict(ls=-0.5), ["label_smoothing"]),
    (dict(label_index=P), ["exactly one"]),
    (dict(labels=None), ["exactly one"]),
    (dict(dtype=2), ["bad dtype"]),
    (dict(rows=-1), ["negative row count"]),
    (dict(ld=7), ["ld 7"]),
    (dict(ld_labels=7), ["ld_labels 7"]),
    (dict(ld_dlogits=7), ["ld_dlogits 7"]),
    (dict(row_loss=None, dlogits=None), ["neither"]),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_softmax_xent_refusals(lib, kw, words):
    _refused(lib, lib.krs_softmax_xent(*xent_args(**kw)), "krs_softmax_xent", *words)


def test_zero_rows_is_a_successful_no_op(lib):
    assert lib.krs_softmax_xent(*xent_args(rows=0, logits=None, labels=None, label_index=P)) == 0
    assert lib.krs_sampling_correction(None, 8, 0, None, 1, 1e-6, 0, 8, None, 8, None) == 0
    assert lib.krs_remove_accidental_hits(None, 8, 0, None, 8, None, 0, 1, 0.5, 0, 8, None, 8, None) == 0


def test_sampling_correction_refusals(lib):
    fn, name = lib.krs_sampling_correction, "krs_sampling_correction"
    _refused(lib, fn(None, 8, 0, P, 1, 1e-6, 2, 8, P, 8, None), name, "null logits")
    _refused(lib, fn(P, 8, 0, None, 1, 1e-6, 2, 8, P, 8, None), name, "null argument")
    _refused(lib, fn(P, 8, 0, P, 1, 1e-6, 2, 8, None, 8, None), name, "null argument")
    _refused(lib, fn(P, 8, 0, P, 1, 1e-6, 2, 0, P, 8, None), name, "0 columns")
    _refused(lib, fn(P, 8, 3, P, 1, 1e-6, 2, 8, P, 8, None), name, "bad dtype")
    _refused(lib, fn(P, 8, 0, P, 0, 1e-6, 2, 8, P, 8, None), name, "p_rows")
    _refused(lib, fn(P, 8, 0, P, 1, 1e-6, 2, 8, P, 7, None), name, "ld_out 7")


def test_remove_accidental_hits_refusals(lib):
    fn, name = lib.krs_remove_accidental_hits, "krs_remove_accidental_hits"
    _refused(lib, fn(None, 8, 0, P, 8, P, 0, 1, 0.5, 2, 8, P, 8, None), name, "null logits")
    _refused(lib, fn(P, 8, 0, None, 8, P, 0, 1, 0.5, 2, 8, P, 8, None), name, "null argument")
    _refused(lib, fn(P, 8, 0, P, 8, None, 0, 1, 0.5, 2, 8, P, 8, None), name, "null argument")
    _refused(lib, fn(P, 8, 0, P, 8, P, 0, 1, 0.5, 2, 0, P, 8, None), name, "0 columns")
    _refused(lib, fn(P, 8, 1 << 4, P, 8, P, 0, 1, 0.5, 2, 8, P, 8, None), name, "bad dtype")
    _refused(lib, fn(P, 8, 0, P, 8, P, 2, 1, 0.5, 2, 8, P, 8, None), name, "bad id dtype")
    _refused(lib, fn(P, 8, 0, P, 8, P, 0, 0, 0.5, 2, 8, P, 8, None), name, "id_rows")
    _refused(lib, fn(P, 8, 0, P, 7, P, 0, 1, 0.5, 2, 8, P, 8, None), name, "leading dimension")
