"""keras_rs_amd/layers/embedding_host.py without a GPU: the fused input form against expectations written out by hand, the
rank-1 weights rule, the input errors through both embedding layers, and that the two layers fuse a call alike."""

import numpy as np
import pytest
import torch

import keras_rs_amd.layers as kl
from keras_rs_amd.layers.embed_reduce import Ragged
from keras_rs_amd.layers.embedding_host import fuse_group_inputs
from keras_rs_amd.sharded import ShardedDistributedEmbedding


def _rows(rows, dtype):
    a = np.empty(len(rows), dtype=object)
    for i, r in enumerate(rows):
        a[i] = np.asarray(r, dtype)
    return a


# batch 3; every input form once
DENSE = np.array([[1, 2], [3, 4], [5, 6]], np.int32)
DENSE_W = np.array([[.1, .2], [.3, .4], [.5, .6]], np.float32)
RANK1 = np.array([7, 8, 9], np.int64)
RANK1_W = np.array([2.0, 0.0, -1.0], np.float32)
COLUMN = np.array([[4], [5], [6]], np.int32)
COLUMN_W = np.array([[1.5], [2.5], [3.5]], np.float32)
RAGGED = Ragged(np.array([1, 2, 3], np.int32), np.array([0, 1, 1, 3], np.int32))        # rows [1], [], [2, 3]
RAGGED_W = Ragged(np.array([.7, .8, .9], np.float32), np.array([0, 1, 1, 3], np.int32))
OBJECT = _rows([[4, 5], [6], [7, 8, 9]], np.int32)
OBJECT_W = _rows([[1., 2.], [3.], [4., 5., 6.]], np.float32)

# (name, three (ids, weights) features, ids, ids dtype, hots, offsets, weights with combiners sum / mean / sum)
CASES = [
    ("dense_rank1_column", [(DENSE, DENSE_W), (RANK1, RANK1_W), (COLUMN, COLUMN_W)],
     [1, 2, 3, 4, 5, 6, 7, 8, 9, 4, 5, 6], torch.int64, (2, 1, 1), None,
     [.1, .2, .3, .4, .5, .6, 1., 1., 1., 1.5, 2.5, 3.5]),
    ("dense_rank1_ragged", [(DENSE, DENSE_W), (RANK1, RANK1_W), (RAGGED, RAGGED_W)],
     [1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 2, 3], torch.int64, None, [0, 2, 4, 6, 7, 8, 9, 10, 10, 12],
     [.1, .2, .3, .4, .5, .6, 1., 1., 1., .7, .8, .9]),
    ("ragged_dense_object", [(RAGGED, RAGGED_W), (DENSE, DENSE_W), (OBJECT, OBJECT_W)],
     [1, 2, 3, 1, 2, 3, 4, 5, 6, 4, 5, 6, 7, 8, 9], torch.int32, None, [0, 1, 1, 3, 5, 7, 9, 11, 12, 15],
     [.7, .8, .9, .1, .2, .3, .4, .5, .6, 1., 2., 3., 4., 5., 6.]),
]
COMBINERS = {"a": "sum", "b": "mean", "c": "sum"}


@pytest.mark.parametrize("offsets_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_fuse_group_inputs_against_hand_written_expectations(case, weighted, offsets_dtype):
    _, feats, ids, ids_dtype, hots, offsets, w = case
    inputs = dict(zip("abc", (f[0] for f in feats)))
    weights = dict(zip("abc", (f[1] for f in feats))) if weighted else None
    got = fuse_group_inputs(["a", "b", "c"], COMBINERS.get, inputs, weights, torch.device("cpu"), offsets_dtype)
    assert sorted(got) == ["batch", "hots", "ids", "offsets", "weights"]
    assert got["ids"].dtype == ids_dtype and got["ids"].tolist() == ids         # feature-major
    assert got["hots"] == hots and got["batch"] == 3
    if offsets is None:
        assert got["offsets"] is None
    else:
        assert got["offsets"].dtype == torch.from_numpy(np.zeros(1, offsets_dtype)).dtype
        assert got["offsets"].tolist() == offsets
    if weighted:
        assert got["weights"].dtype == torch.float32
        np.testing.assert_array_equal(got["weights"].numpy(), np.array(w, np.float32))
    else:
        assert got["weights"] is None


@pytest.mark.parametrize("combiner,expected", [("mean", [1., 1., 1.]), ("sqrtn", [1., 1., 1.]), ("sum", [2., 0., -1.])])
def test_weights_on_a_rank1_input_survive_only_for_sum(combiner, expected):
    for ids in (RANK1, torch.from_numpy(RANK1)):
        got = fuse_group_inputs(["a"], lambda path: combiner, {"a": ids}, {"a": RANK1_W}, torch.device("cpu"), np.int32)
        assert got["hots"] == (1,) and got["weights"].tolist() == expected


def _both_layers(combiners=("sum", "mean")):
    """DistributedEmbedding and ShardedDistributedEmbedding (world 1, no process group) on the CPU over the same two tables:
    features a, b on the first (10 rows), c on the second (7 rows)."""
    layers = []
    for cls, placement in ((kl.DistributedEmbedding, "default_device"), (ShardedDistributedEmbedding, "sparsecore")):
        tcs = [kl.TableConfig(f"t{i}", v, 8, optimizer="sgd", combiner=combiners[i], placement=placement)
               for i, v in enumerate((10, 7))]
        fcs = {k: kl.FeatureConfig(k, tcs[t], (3, 2), (3, 8)) for k, t in (("a", 0), ("b", 0), ("c", 1))}
        layers.append(cls(fcs, device="cpu"))
    return layers


def _groups_of(layer, pre):
    pre = pre["preprocessed_inputs_per_placement"]
    if isinstance(layer, ShardedDistributedEmbedding):
        return pre["sparsecore"]["groups"]
    pre = pre["default_device"]
    return [dict(fi, weights=pre.get("weights", {}).get(key)) for key, fi in pre["inputs"].items()]


@pytest.mark.parametrize("which", [0, 1], ids=["DistributedEmbedding", "ShardedDistributedEmbedding"])
def test_both_layers_reject_malformed_inputs(which):
    layer = _both_layers()[which]
    ok = {"a": DENSE, "b": RANK1, "c": COLUMN}
    ok_w = {"a": DENSE_W, "b": RANK1_W, "c": COLUMN_W}
    layer.preprocess(ok, ok_w)
    with pytest.raises(ValueError, match="rank 1 or 2"):
        layer.preprocess(dict(ok, a=DENSE.reshape(3, 2, 1)))
    with pytest.raises(ValueError, match="does not match"):
        layer.preprocess(ok, dict(ok_w, a=DENSE_W[:, :1]))
    with pytest.raises(ValueError, match="every feature or for none"):
        layer.preprocess(ok, dict(ok_w, b=None))
    with pytest.raises(ValueError, match="share the batch size"):
        layer.preprocess(dict(ok, b=RANK1[:2]))


@pytest.mark.parametrize("weighted", [False, True])
def test_both_layers_fuse_a_call_alike(weighted):
    single, sharded = _both_layers()
    inputs = {"a": RAGGED, "b": RANK1, "c": OBJECT}
    weights = {"a": RAGGED_W, "b": RANK1_W, "c": OBJECT_W} if weighted else None
    one, two = (_groups_of(la, la.preprocess(inputs, weights)) for la in (single, sharded))
    assert len(one) == len(two) == 1
    for a, b in zip(one, two):
        assert torch.equal(a["ids"], b["ids"]) and a["ids"].dtype == b["ids"].dtype
        assert a["hots"] == b["hots"] and a["batch"] == b["batch"] == 3
        assert a["offsets"].tolist() == b["offsets"].tolist() == [0, 1, 1, 3, 4, 5, 6, 8, 9, 12]
        assert (a["offsets"].dtype, b["offsets"].dtype) == (torch.int32, torch.int64)      # each layer keeps its own
        if weighted:
            assert torch.equal(a["weights"], b["weights"])
            # b is rank-1 on a "sum" table: its weights are kept
            assert a["weights"].tolist() == pytest.approx([.7, .8, .9, 2., 0., -1., 1., 2., 3., 4., 5., 6.])
        else:
            assert a["weights"] is None and b["weights"] is None


@pytest.mark.parametrize("combiner", ["mean", "sqrtn", "sum"])
def test_sharded_layer_follows_the_reference_on_rank1_weights(combiner):
    """A rank-1 input is not reduced; its weights count only under "sum" (embed_reduce.py:224).  Zero and negative weights
    are where dividing the weights out again, as the sharded layer once did, gives something else."""
    from tests._sharded_worker import OracleShardKernels

    tc = kl.TableConfig("t", 10, 8, optimizer="sgd", combiner=combiner, placement="sparsecore")
    layer = ShardedDistributedEmbedding({"a": kl.FeatureConfig("a", tc, (4,), (4, 8))}, kernels=OracleShardKernels(),
                                        device="cpu")
    table = np.random.default_rng(0).uniform(-1, 1, (10, 8)).astype(np.float32)
    layer.set_embedding_tables({"t": table})
    ids = np.array([3, 9, 0, 3], np.int32)
    w = np.array([2.0, 0.0, -1.0, 0.5], np.float32)
    with torch.no_grad():
        out = layer({"a": ids}, {"a": w})["a"].numpy()
    np.testing.assert_array_equal(out, w[:, None] * table[ids] if combiner == "sum" else table[ids])
