"""K15 without a GPU: the restatement of tests/retrieval_rank_restatement.py against a stable argsort, the id rule by
hand, FactorizedTopK's accumulation and SparseTopKCategoricalAccuracy on CPU tensors against hand-computed values,
every ValueError of update_state before a device is needed, the config round trip, and
krs_retrieval_rank_workspace_bytes against the bound stated in include/krs.h."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from keras_rs_amd.layers.retrieval import rank_totals
from tests import retrieval_rank_restatement as R


@pytest.fixture(scope="module")
def bands():
    return {s: R.band(*R.normal(*s)) for s in R.SHAPES}


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_the_restatement_is_the_position_in_a_stable_argsort(shape):
    for q, c, pos in (R.integers(*shape), R.normal(*shape)):
        s = R.scores64(q, c)
        rank, sp = R.rank_of(s, pos)
        assert torch.equal(rank, R.argsort_position(s, pos))
        assert torch.equal(sp, s.gather(1, pos[:, None])[:, 0])


def test_the_integer_builder_is_exact_in_fp32_and_full_of_ties():
    tied = rows = 0
    for shape in R.SHAPES:
        q, c, pos = R.integers(*shape)
        s = R.scores64(q, c)
        assert float(s.abs().max()) < 2 ** 24 and torch.equal(s, s.round())
        assert torch.equal(s.to(torch.float32).to(torch.float64), s)
        r32, sp32 = retrieval_ops.rank_in_scores(s.to(torch.float32), pos.to(torch.int32))
        rank, sp = R.rank_of(s, pos)
        assert torch.equal(r32.to(torch.int64), rank) and torch.equal(sp32.to(torch.float64), sp)
        sp = s.gather(1, pos[:, None])
        tied += int((((s == sp).sum(dim=1)) > 1).sum())
        rows += shape[0]
    print(f"integer builder: {tied} of {rows} rows have a candidate tied with the positive")
    assert rows == 3446 and tied > rows // 2


def test_the_band_of_the_normal_builder_hides_nothing(bands):
    exact = rows = 0
    for shape, (lo, hi, _, _) in bands.items():
        same = int((lo == hi).sum())
        print(f"{shape}: lo == hi on {same} of {shape[0]} rows")
        assert same >= 0.80 * shape[0], shape
        exact += same
        rows += shape[0]
        rank, _ = R.rank_of(R.scores64(*R.normal(*shape)[:2]), R.normal(*shape)[2])
        assert bool(((lo <= rank) & (rank <= hi)).all())
    print(f"all shapes: lo == hi on {exact} of {rows} rows ({100.0 * exact / rows:.1f} %)")
    assert exact >= 0.95 * rows


def test_the_id_rule_by_hand():
    #            j:   0    1    2    3    4    5
    s = torch.tensor([[5.0, 3.0, 4.0, 3.0, 9.0, 1.0],
                      [2.0, 2.0, 2.0, 7.0, 2.0, 8.0]], dtype=torch.float64)
    pos = torch.tensor([1, 2])
    ids = torch.tensor([10, 11, 12, 13, 11, 12])
    # row 0, pos 1 (3.0): ahead are 0 (5), 2 (4), 4 (9); 3 ties at a higher index.  Candidate 4 carries id 11: removed.
    # row 1, pos 2 (2.0): ahead are 0, 1 (ties, lower index), 3 (7), 5 (8); 4 ties above.  Candidate 5 carries id 12.
    assert R.rank_of(s, pos)[0].tolist() == [3, 4]
    assert R.rank_of(s, pos, ids)[0].tolist() == [2, 3]
    for fn_ids, want in ((None, [3, 4]), (ids, [2, 3]), (ids.to(torch.int32), [2, 3])):
        got, sp = retrieval_ops.rank_in_scores(s.to(torch.float32), pos.to(torch.int32), fn_ids)
        assert got.tolist() == want and sp.tolist() == [3.0, 2.0]
    # special values: NaN above +inf, all NaN equal, -0.0 == +0.0, a positive outside [0, N)
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[nan, inf, 1.0, nan], [0.0, -0.0, 0.0, -1.0], [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]],
                     dtype=torch.float64)
    pos = torch.tensor([3, 1, -1, 4])
    want = [1, 1, -1, -1]
    assert R.rank_of(s, pos)[0].tolist() == want
    got, sp = retrieval_ops.rank_in_scores(s.to(torch.float32), pos.to(torch.int32))
    assert got.tolist() == want and torch.isnan(sp[2:]).all() and torch.isnan(sp[0]) and float(sp[1]) == 0.0
    assert R.rank_of(s, torch.tensor([1, 0, 0, 0]))[0].tolist() == [2, 0, 3, 3]


KS = (1, 2, 5)
RANK1, W1 = torch.tensor([0, 1, 4, -1, 7], dtype=torch.int32), torch.tensor([1.0, 2.0, 0.5, 3.0, 1.5])
RANK2 = torch.tensor([2, 0], dtype=torch.int32)


def _values(metric):
    return {k: float(v) for k, v in metric.result().items()}


def test_factorized_top_k_accumulates_on_cpu_tensors_as_computed_by_hand():
    m = layers.FactorizedTopK(ks=KS)
    assert _values(m) == {"top_1_categorical_accuracy": 0.0, "top_2_categorical_accuracy": 0.0,
                          "top_5_categorical_accuracy": 0.0, "mean_reciprocal_rank": 0.0}
    m.accumulate(RANK1, W1)
    # sum w = 8; top-1: 1; top-2: 1 + 2; top-5: 1 + 2 + 0.5; rr: 1 + 2 / 2 + 0.5 / 5 + 0 + 1.5 / 8
    want = {"top_1_categorical_accuracy": 1.0 / 8, "top_2_categorical_accuracy": 3.0 / 8,
            "top_5_categorical_accuracy": 3.5 / 8, "mean_reciprocal_rank": (1.0 + 1.0 + 0.1 + 0.1875) / 8}
    assert _values(m) == pytest.approx(want, rel=1e-6)
    assert _values(m) == pytest.approx(R.metric_values(RANK1, W1, KS), rel=1e-6)
    m.accumulate(RANK2)             # unweighted: sum w = 10; top-1 + 1, top-2 + 1, top-5 + 2, rr + 1 / 3 + 1
    want = {"top_1_categorical_accuracy": 2.0 / 10, "top_2_categorical_accuracy": 4.0 / 10,
            "top_5_categorical_accuracy": 5.5 / 10, "mean_reciprocal_rank": (2.2875 + 1.0 / 3 + 1.0) / 10}
    assert _values(m) == pytest.approx(want, rel=1e-6)
    both = torch.cat((RANK1, RANK2))
    assert _values(m) == pytest.approx(R.metric_values(both, torch.cat((W1, torch.ones(2))), KS), rel=1e-6)
    assert all(v.dtype == torch.float32 and v.dim() == 0 for v in m.result().values())
    m.reset_state()
    assert all(v == 0.0 for v in _values(m).values())
    m.accumulate(RANK2, 2.0)        # a scalar weight
    assert _values(m) == pytest.approx(R.metric_values(RANK2, torch.full((2,), 2.0), KS), rel=1e-6)


def test_a_zero_total_weight_gives_zero_and_a_missing_positive_counts_in_the_denominator_only():
    m = layers.FactorizedTopK(ks=KS)
    m.accumulate(RANK1, torch.zeros(5))
    assert all(v == 0.0 for v in _values(m).values())
    m.accumulate(torch.tensor([-1, 0], dtype=torch.int32))
    assert _values(m) == pytest.approx({"top_1_categorical_accuracy": 0.5, "top_2_categorical_accuracy": 0.5,
                                        "top_5_categorical_accuracy": 0.5, "mean_reciprocal_rank": 0.5})
    t = rank_totals(RANK1, W1, torch.tensor(KS, dtype=torch.int32))
    assert t.dtype == torch.float32 and t.tolist() == pytest.approx([1.0, 3.0, 3.5, 2.2875, 8.0])


def test_sparse_top_k_categorical_accuracy_from_sorted_ids():
    y_pred = torch.tensor([[4, 2, 9], [1, 7, 3], [5, 5, 5], [8, 0, 6]], dtype=torch.int32)
    y_true = torch.tensor([2, 3, 4, 8])
    w = torch.tensor([1.0, 2.0, 3.0, 4.0])
    for k, hits in ((1, [0, 0, 0, 1]), (2, [1, 0, 0, 1]), (3, [1, 1, 0, 1]), (7, [1, 1, 0, 1])):
        m = layers.SparseTopKCategoricalAccuracy(k=k, from_sorted_ids=True)
        assert float(m.result()) == 0.0
        m.update_state(y_true, y_pred)
        assert float(m.result()) == pytest.approx(sum(hits) / 4)
        m.update_state(y_true[:, None], y_pred, sample_weight=w)
        h = torch.tensor(hits, dtype=torch.float32)
        assert float(m.result()) == pytest.approx((sum(hits) + float((h * w).sum())) / (4 + 10.0))
        m.reset_state()
        m.update_state(y_true, y_pred, sample_weight=torch.zeros(4))
        assert float(m.result()) == 0.0
        assert layers.SparseTopKCategoricalAccuracy.from_config(m.get_config()).get_config() == m.get_config()
    # the same ranks through both metrics
    ranks = torch.tensor([1, 2, -1, 0], dtype=torch.int32)
    f = layers.FactorizedTopK(ks=(1, 2, 3))
    f.accumulate(ranks, w)
    for k in (1, 2, 3):
        m = layers.SparseTopKCategoricalAccuracy(k=k, from_sorted_ids=True)
        m.update_state(y_true, y_pred, sample_weight=w)
        assert float(m.result()) == pytest.approx(float(f.result()[f"top_{k}_categorical_accuracy"]))
    with pytest.raises(NotImplementedError, match="FactorizedTopK"):
        layers.SparseTopKCategoricalAccuracy(k=5)
    with pytest.raises(ValueError, match="integer >= 1"):
        layers.SparseTopKCategoricalAccuracy(k=0, from_sorted_ids=True)
    with pytest.raises(ValueError, match="one id per row"):
        layers.SparseTopKCategoricalAccuracy(k=1, from_sorted_ids=True).update_state(y_true[:3], y_pred)
    with pytest.raises(ValueError, match="integer ids"):
        layers.SparseTopKCategoricalAccuracy(k=1, from_sorted_ids=True).update_state(y_true, y_pred.float())
    with pytest.raises(ValueError, match="sample_weight"):
        layers.SparseTopKCategoricalAccuracy(k=1, from_sorted_ids=True).update_state(y_true, y_pred, torch.ones(3))


def test_every_value_error_of_update_state_comes_before_any_device_check():
    q, c = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(6, 8, dtype=torch.bfloat16)
    pos = torch.arange(4)
    m = layers.FactorizedTopK(c, candidate_ids=torch.arange(6))
    bad = [
        (dict(query_embeddings=q[0]), "matrices of one width"),
        (dict(query_embeddings=q[:, :7]), "matrices of one width"),
        (dict(query_embeddings=q, candidate_embeddings=c[:0]), "at least one candidate"),
        (dict(query_embeddings=q.float()), "share a dtype"),
        (dict(query_embeddings=q.half(), candidate_embeddings=c.half()), "float32 or bfloat16"),
        (dict(query_embeddings=q, positive_index=pos[:3]), "`positive_index` should be 4 integers"),
        (dict(query_embeddings=q, positive_index=pos.float()), "`positive_index` should be 4 integers"),
        (dict(query_embeddings=q, positive_index=pos > 1), "`positive_index` should be 4 integers"),
        (dict(query_embeddings=q, candidate_embeddings=c, candidate_ids=torch.arange(5)),
         "`candidate_ids` should be 6 integers"),
        (dict(query_embeddings=q, candidate_embeddings=c, candidate_ids=torch.rand(6)),
         "`candidate_ids` should be 6 integers"),
        (dict(query_embeddings=q, candidate_ids=torch.arange(6)), "without providing `candidate_embeddings`"),
        (dict(query_embeddings=q, sample_weight=torch.ones(3)), "sample_weight"),
    ]
    for kwargs, text in bad:
        kwargs.setdefault("positive_index", pos)
        with pytest.raises(ValueError, match=text):
            m.update_state(**kwargs)
    with pytest.raises(ValueError, match="No candidates"):
        layers.FactorizedTopK().update_state(q, pos)
    # the same call with good arguments reaches the device check (these are CPU tensors)
    with pytest.raises(L.KrsError):
        m.update_state(q, pos)
    # the constructor and update_candidates
    for ks in ((), (0,), (1.5,), (True,)):
        with pytest.raises(ValueError, match="`ks`"):
            layers.FactorizedTopK(ks=ks)
    with pytest.raises(ValueError, match="without providing `candidate_embeddings`"):
        layers.FactorizedTopK(candidate_ids=torch.arange(6))
    with pytest.raises(ValueError, match="rank 2"):
        layers.FactorizedTopK(c[0])
    with pytest.raises(ValueError, match="Cannot assign candidate_embeddings of shape"):
        m.update_candidates(c[:5])
    with pytest.raises(ValueError, match="previous candidates did not have candidate IDs"):
        layers.FactorizedTopK(c).update_candidates(c, torch.arange(6))
    stored = m.candidate_embeddings
    m.update_candidates(torch.ones(6, 8, dtype=torch.bfloat16), torch.arange(6) + 10)
    assert m.candidate_embeddings is stored and float(stored.float().sum()) == 48.0      # copied in place
    assert m.candidate_ids.tolist() == list(range(10, 16))


def test_config_round_trip_and_exports():
    m = layers.FactorizedTopK(ks=(1, 3), name="eval")
    assert m.get_config() == {"name": "eval", "ks": [1, 3]}
    again = layers.FactorizedTopK.from_config(m.get_config())
    assert again.get_config() == m.get_config() and again.ks == (1, 3)
    assert layers.FactorizedTopK().ks == (1, 5, 10, 50, 100) and layers.FactorizedTopK().name == "factorized_top_k"
    assert list(layers.FactorizedTopK(ks=(1, 3)).result()) == ["top_1_categorical_accuracy",
                                                               "top_3_categorical_accuracy", "mean_reciprocal_rank"]
    assert "FactorizedTopK" in layers.__all__ and "SparseTopKCategoricalAccuracy" in layers.__all__
    assert "tfrs.metrics.FactorizedTopK" in layers.FactorizedTopK.__doc__
    with pytest.raises(L.KrsError, match="path must be"):
        retrieval_ops.retrieval_rank(torch.zeros(1, 8), torch.zeros(1, 8), path="eager")


def test_workspace_bytes_stay_under_the_bound_of_krs_h():
    # include/krs.h, K15: at most 4 b + 32 (b + n) + 512 bytes; host only
    shapes = R.SHAPES + [(64, 1 << 20, 128), (8192, 1 << 20, 128), (32768, 32768, 128), (2048, 8192, 64), (1, 1, 1)]
    for b, n, d in shapes:
        size = retrieval_ops.retrieval_rank_workspace_bytes(b, n, d)
        assert 4 * b <= size <= 4 * b + 32 * (b + n) + 512, (b, n, d, size)
        assert size % 256 == 0
    assert retrieval_ops.retrieval_rank_workspace_bytes(0, 5, 8) == 0
    # the sliced shape of the table keeps one count per slice and query; the unsliced one the scores alone
    assert retrieval_ops.retrieval_rank_workspace_bytes(40, 161, 64) == 256 + 512
    assert retrieval_ops.retrieval_rank_workspace_bytes(161, 40, 64) == 768
