"""The ranking metrics on the GPU (K10): every value of the reference's tests through the HIP path, random fp32 / bf16
lists with dense score ties against the float64 restatement (the rank permutation exactly, values and list weights
within a derived bound), custom gain / discount functions, the group against separate updates, determinism, graph
capture with the device draw counter, the distribution of shuffled ties and the list-length limit.

Tolerance of the random cases (stated, not tuned): |got - ref| <= C (k_eff + 16) u M with u = 2^-24, C = 8 and M the
float64 sum of the absolute values of the terms of the quantity, which is the quantity itself as no term is
negative.  Where C comes from: every per-list output is at most a quotient of fp32 sums, or (DCG) a sum divided by a
list weight that is itself a quotient of two sums -- at most three sums and two divisions.  A term of a sum carries at
most 9 u: the labels of these tests are integers, so 2^y - 1 is exact; 1 + r is exact, log2f is within 1 ulp (2 u),
the division within 2.5 ulp (5 u), and the two products add 1 u each.  A sum adds its terms as a tree -- up to 4
items of a thread in sequence, 6 butterfly levels in a wave, 4 butterfly levels over the waves: at most 14 additions
on any path, 14 u whatever L is -- and stage B's batch-wide default weight is a tree of the same kind (B / 1024 in
sequence for these B <= 1024, then 6 + 4).  So a sum is within 23 u of its value, a quotient of two within 47 u, and
DCG / weight within 3 * 23 + 2 = 71 u, first order; the ideal order of NDCG compares fp32 products where the
restatement compares float64 ones, which can swap two terms that differ by at most 2 u of their size.  C = 8 is the
power of two for which C (k_eff + 16) >= 136 at
k_eff = 1 covers 71 u with room for the second-order terms."""

import json
import os

import numpy as np
import pytest
import torch

from keras_rs_amd import KrsError, metric_ops, metrics
from tests import ranking_metric_restatement as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ranking_metrics.json")))
KINDS = {"DCG": "dcg", "NDCG": "ndcg", "MeanAveragePrecision": "map", "MeanReciprocalRank": "mrr",
         "PrecisionAtK": "precision", "RecallAtK": "recall"}
CLASSES = {k: getattr(metrics, n) for n, k in KINDS.items()}
C_BOUND = 8
GAINS = {"default": metrics.default_gain_fn, "linear": lambda y: y.to(torch.float32)}
DISCOUNTS = {"default": metrics.default_rank_discount_fn, "inverse": lambda r: 1.0 / r}


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.tensor(x, dtype=dtype, device=DEV)


@pytest.mark.parametrize("shuffle_ties", [True, False])
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['metric']}-{c['case']}")
def test_reference_values(c, shuffle_ties):
    m = getattr(metrics, c["metric"])(k=c["k"], shuffle_ties=shuffle_ties, seed=3,
                                      **({"gain_fn": GAINS[c["gain"]], "rank_discount_fn": DISCOUNTS[c["discount"]]}
                                         if c["metric"] in ("DCG", "NDCG") else {}))
    for u in c["updates"]:
        y = _dev(u["y_true"])
        y_true = y if u["mask"] is None else {"labels": y, "mask": _dev(u["mask"], torch.bool)}
        w = u["sample_weight"]
        w = w if w is None or isinstance(w, (int, float)) else _dev(w)
        m.update_state(y_true, _dev(u["y_pred"]), sample_weight=w)
        got = m.result()
        assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
        print(c["metric"], c["case"], float(got), u["expected"])
        assert abs(float(got) - u["expected"]) <= u["atol"] + u["rtol"] * abs(u["expected"])
    if c["reset_expected"] is not None:
        m.reset_state()
        assert abs(float(m.result()) - c["reset_expected"]) <= 1e-6


def _inputs(b, n, dtype, seed):
    """Dense score ties (scores rounded to integers), 10 % negative labels, 10 % masked, 10 % zero weights."""
    g = torch.Generator().manual_seed(seed)
    s = torch.round(torch.randn((b, n), generator=g) * 2.0)
    y = torch.randint(0, 5, (b, n), generator=g).float()
    y = torch.where(torch.rand((b, n), generator=g) < 0.1, torch.full_like(y, -1.0), y)
    mask = torch.rand((b, n), generator=g) >= 0.1
    w = 0.25 + 1.75 * torch.rand((b, n), generator=g)
    w = torch.where(torch.rand((b, n), generator=g) < 0.1, torch.zeros_like(w), w)
    return s.to(dtype), y, mask, w


def _close(got, ref, k_eff, what, scale=1.0):
    tol = C_BOUND * (k_eff + 16) * MR.U32 * np.abs(ref) * scale
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    print(what, "max err", float(err.max()), "tol there", float(np.atleast_1d(tol)[np.argmax(err)]))
    assert (err <= tol).all(), f"{what}: err {float(err.max())} at tol {float(np.atleast_1d(tol)[np.argmax(err)])}"


LENGTHS = [1, 2, 5, 63, 64, 65, 256, 2048, 4096]
BATCH = {1: 300, 2: 257, 5: 300, 63: 40, 64: 33, 65: 17, 256: 9, 2048: 5, 4096: 3}
SEED = 5


@pytest.mark.parametrize("shuffle_ties", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", LENGTHS)
def test_random_against_float64(n, dtype, shuffle_ties):
    b = BATCH[n]
    kinds = list(CLASSES)
    for k in (None, 1, 10, n):
        k_eff = n if k is None else min(k, n)
        # one launch of each stage, by hand: the order, per-list values and per-list weights at draw 0
        s, y, mask, w = _inputs(b, n, dtype, seed=n)
        draw = torch.zeros(1, dtype=torch.int64, device=DEV)
        states = [torch.zeros(2, device=DEV) for _ in kinds]
        values, sums, order = metric_ops.ranking_metrics([(kind, k) for kind in kinds], s.to(DEV), y.to(DEV),
                                                         mask.to(DEV), w.to(DEV), shuffle_ties=shuffle_ties,
                                                         seed=SEED, draw=draw, want_order=True)
        lv, lw = metric_ops.ranking_metrics_accumulate(kinds, values, sums, states, draw=draw, want_lists=True)
        assert int(draw) == 1
        for j, kind in enumerate(kinds):
            rv, rw, ro = MR.metric(kind, s.float().numpy(), y.numpy(), mask.numpy(), w.double().numpy(), k,
                                   shuffle_ties=shuffle_ties, seed=SEED, draw=0)
            assert np.array_equal(order.cpu().numpy(), ro), f"{kind}: rank permutation differs"
            _close(lv[j].cpu().numpy(), rv, k_eff, f"{kind}@{k} L={n} values")
            _close(lw[j].cpu().numpy(), rw, k_eff, f"{kind}@{k} L={n} weights")
        # three updates through the public interface (draws 0, 1, 2)
        group = metrics.RankingMetricGroup([CLASSES[kind](k=k, shuffle_ties=shuffle_ties, seed=SEED) for kind in kinds])
        means = [MR.Mean() for _ in kinds]
        for d in range(3):
            s, y, mask, w = _inputs(b, n, dtype, seed=100 * n + d)
            group.update_state({"labels": y.to(DEV), "mask": mask.to(DEV)}, s.to(DEV), sample_weight=w.to(DEV))
            for kind, mean in zip(kinds, means):
                rv, rw, _ = MR.metric(kind, s.float().numpy(), y.numpy(), mask.numpy(), w.double().numpy(), k,
                                      shuffle_ties=shuffle_ties, seed=SEED, draw=d)
                mean.update(rv, rw)
        for kind, mean, m in zip(kinds, means, group.metrics):
            _close(float(m.result()), np.float64(mean.result()), k_eff, f"{kind}@{k} L={n} result", scale=3 * b)


@pytest.mark.parametrize("b", [1024, 1025, 2049, 5000])
def test_batches_on_either_side_of_stage_bs_one_workgroup_limit(b):
    """Stage B runs in one workgroup up to 1024 lists and over ceil(b / 1024) workgroups above: a batch at the limit,
    one list past it (a second workgroup with one list), three workgroups of which the last has one list, and
    workgroups that are not full.  Lists of 3 items, so that many have no relevant item and take the batch-wide
    default weight, which is what the workgroups have to agree on.  Per-list outputs within the bound of the module
    docstring; the two state words are sums of b terms, each within that bound, added as a tree whose depth does
    not grow with b here (one term per thread, 10 butterfly levels, then at most 5 workgroups in sequence): within
    the bound scaled by b, as the issue sets it for accumulated results."""
    n, k = 3, 2
    kinds = list(CLASSES)
    s, y, mask, w = _inputs(b, n, torch.float32, seed=b)
    draw = torch.zeros(1, dtype=torch.int64, device=DEV)
    states = [torch.zeros(2, device=DEV) for _ in kinds]
    values, sums, _ = metric_ops.ranking_metrics([(kind, k) for kind in kinds], s.to(DEV), y.to(DEV), mask.to(DEV),
                                                 w.to(DEV), shuffle_ties=True, seed=SEED, draw=draw)
    lv, lw = metric_ops.ranking_metrics_accumulate(kinds, values, sums, states, draw=draw, want_lists=True)
    assert int(draw) == 1
    yy, ww, _ = MR.prepare(y.numpy(), mask.numpy(), w.double().numpy())
    assert ((ww.sum(1) > 0) & (yy.max(1) < 1)).any()       # lists that take the default weight
    for j, kind in enumerate(kinds):
        rv, rw, _ = MR.metric(kind, s.numpy(), y.numpy(), mask.numpy(), w.double().numpy(), k, shuffle_ties=True,
                              seed=SEED, draw=0)
        _close(lv[j].cpu().numpy(), rv, k, f"{kind} B={b} values")
        _close(lw[j].cpu().numpy(), rw, k, f"{kind} B={b} weights")
        ref = np.array([(rv * rw).sum(), rw.sum()])
        _close(states[j].cpu().numpy(), ref, k, f"{kind} B={b} state", scale=b)
    # without the per-list outputs, and a second time: the same bits
    again = [torch.zeros(2, device=DEV) for _ in kinds]
    metric_ops.ranking_metrics_accumulate(kinds, values, sums, again, draw=draw)
    for a, c in zip(states, again):
        assert torch.equal(a, c)
    # a member alone gets the bits it gets in the group
    for j, kind in enumerate(kinds):
        alone = [torch.zeros(2, device=DEV)]
        metric_ops.ranking_metrics_accumulate([kind], values[j:j + 1].contiguous(), sums, alone)
        assert torch.equal(alone[0], states[j]), kind


def test_non_finite_scores_order_as_order_key_orders_them():
    s = torch.tensor([[float("nan"), 1.0, float("inf"), -float("inf"), -0.0, 0.0, float("nan"), 1.0]])
    y = torch.tensor([[1.0, 0.0, 2.0, 1.0, 0.0, 3.0, 0.0, -1.0]])
    _, _, order = metric_ops.ranking_metrics([("ndcg", None), ("map", 3)], s.to(DEV), y.to(DEV), want_order=True)
    ref = MR.rank_order(s.numpy(), (y >= 0).numpy())
    assert ref.tolist() == [[0, 6, 2, 1, 4, 5, 3, 7]]
    assert order.cpu().tolist() == ref.tolist()


@pytest.mark.parametrize("cls", [metrics.DCG, metrics.NDCG])
@pytest.mark.parametrize("k", [None, 7])
def test_custom_functions_stating_the_defaults(cls, k):
    s, y, mask, w = _inputs(64, 50, torch.float32, seed=21)
    a = cls(k=k, shuffle_ties=False)
    b = cls(k=k, shuffle_ties=False, gain_fn=lambda label: torch.pow(2.0, label) - 1.0,
            rank_discount_fn=lambda rank: 1.0 / torch.log2(1.0 + rank))
    for m in (a, b):
        m.update_state({"labels": y.to(DEV), "mask": mask.to(DEV)}, s.to(DEV), sample_weight=w.to(DEV))
    ref = np.float64(float(a.result()))
    assert ref > 0
    # Not bit for bit: the custom functions run as torch ops (torch.pow, torch.log2 and a division on the device), the
    # defaults as exp2f, log2f and a division in the kernel, and the two may round a gain or a discount differently
    # by an ulp.  Each result is within the derived bound of the exact value, so the two are within twice that bound
    # of each other, which is what "the same result" can mean for two fp32 evaluations of one formula.
    _close(float(b.result()), ref, 50 if k is None else k, f"{cls.__name__}@{k} custom against default", scale=2 * 64)


def _members(seed=9, shuffle_ties=True):
    return [metrics.NDCG(k=10, shuffle_ties=shuffle_ties, seed=seed), metrics.DCG(shuffle_ties=shuffle_ties, seed=seed),
            metrics.MeanReciprocalRank(shuffle_ties=shuffle_ties, seed=seed),
            metrics.MeanAveragePrecision(k=10, shuffle_ties=shuffle_ties, seed=seed),
            metrics.PrecisionAtK(k=10, shuffle_ties=shuffle_ties, seed=seed),
            metrics.RecallAtK(k=10, shuffle_ties=shuffle_ties, seed=seed)]


def _three_updates(target, n=70, dtype=torch.bfloat16):
    for d in range(3):
        s, y, mask, w = _inputs(96, n, dtype, seed=40 + d)
        target.update_state({"labels": y.to(DEV), "mask": mask.to(DEV)}, s.to(DEV), sample_weight=w.to(DEV))


@pytest.mark.parametrize("n", [70, 1500])
def test_group_update_is_bit_identical_to_separate_updates(n):
    alone = _members()
    for m in alone:
        _three_updates(m, n)
    group = metrics.RankingMetricGroup(_members())
    _three_updates(group, n)
    for a, g in zip(alone, group.metrics):
        assert torch.equal(a._state, g._state), a.name
        assert torch.equal(a.result(), group.result()[a.name])


def test_two_identical_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        group = metrics.RankingMetricGroup(_members())
        _three_updates(group, 300)
        runs.append([m._state.clone() for m in group.metrics])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_graph_replays_advance_the_draw_counter():
    s, y, mask, w = _inputs(128, 40, torch.float32, seed=17)
    s, y, mask, w = s.to(DEV), y.to(DEV), mask.to(DEV), w.to(DEV)

    def fresh():
        # one warm-up update on a side stream (it allocates the state and the counter), then an empty state; both
        # metrics go on from draw number 1
        group = metrics.RankingMetricGroup(_members())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            group.update_state({"labels": y, "mask": mask}, s, sample_weight=w)
        torch.cuda.current_stream().wait_stream(side)
        group.reset_state()
        return group

    eager = fresh()
    for _ in range(3):
        eager.update_state({"labels": y, "mask": mask}, s, sample_weight=w)
    one = fresh()
    one.update_state({"labels": y, "mask": mask}, s, sample_weight=w)
    captured = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.update_state({"labels": y, "mask": mask}, s, sample_weight=w)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(captured._draw) == int(eager._draw) == 4
    for a, b in zip(eager.metrics, captured.metrics):
        assert torch.equal(a._state, b._state), a.name
        assert torch.equal(a.result(), b.result())
    # the three draws differ: three updates at one draw number would have given exactly three times one update
    assert not torch.equal(eager.metrics[0]._state, one.metrics[0]._state * 3)


def test_shuffled_ties_are_uniform():
    """All-equal scores, one relevant item, B = 65 536 lists of 8: the relevant item lands on each rank with
    frequency within 5 standard deviations of 1/8 (fixed seed: the test is deterministic)."""
    b, n = 65536, 8
    s = torch.zeros((b, n), device=DEV)
    y = torch.zeros((b, n), device=DEV)
    y[:, 3] = 1.0
    draw = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    values, _, order = metric_ops.ranking_metrics([("mrr", None)], s, y, shuffle_ties=True, seed=1234, draw=draw,
                                                  want_order=True)
    order = order.cpu().numpy()
    assert np.array_equal(order, MR.rank_order(s.cpu().numpy(), np.ones((b, n), dtype=bool), True, 1234, 2))
    tol = 5.0 * np.sqrt((1 / 8) * (7 / 8) / b)
    freq = (order == 3).mean(0)
    print("frequencies", freq.tolist(), "tolerance", tol)
    assert (np.abs(freq - 1 / 8) <= tol).all()
    # every item, not only the relevant one, and the first rank in particular
    for item in range(n):
        assert (np.abs((order == item).mean(0) - 1 / 8) <= tol).all()
    rank = np.argmax(order == 3, axis=1) + 1
    assert np.allclose(values[0].cpu().numpy(), 1.0 / rank, rtol=2.0 ** -22, atol=0)


@pytest.mark.parametrize("cls", list(CLASSES.values()))
def test_list_of_4097_raises(cls):
    s = torch.zeros((2, 4097), device=DEV)
    with pytest.raises(KrsError, match="4096"):
        cls().update_state(torch.ones_like(s), s)


def test_strided_scores_and_unbatched_weights():
    s, y, _, _ = _inputs(12, 80, torch.float32, seed=9)
    wide = torch.randn((12, 200), device=DEV)
    wide[:, 50:130] = s.to(DEV)
    a, b = metrics.NDCG(shuffle_ties=False), metrics.NDCG(shuffle_ties=False)
    a.update_state(y.to(DEV), wide[:, 50:130])
    b.update_state(y.to(DEV), s.to(DEV))
    assert torch.equal(a._state, b._state)
    # per-list weights [B] against the same weights written out [B, L]
    wl = torch.rand(12, generator=torch.Generator().manual_seed(1)).to(DEV)
    c, d = metrics.MeanAveragePrecision(shuffle_ties=False), metrics.MeanAveragePrecision(shuffle_ties=False)
    c.update_state(y.to(DEV), s.to(DEV), sample_weight=wl)
    d.update_state(y.to(DEV), s.to(DEV), sample_weight=wl[:, None].expand(12, 80))
    assert torch.equal(c._state, d._state)
