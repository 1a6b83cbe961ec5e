"""K15 on the device: krs_retrieval_rank (csrc/retrieval_xent.hip, MODE_POS + MODE_RANK of xent_kernel) through
retrieval_ops.retrieval_rank, layers.FactorizedTopK and the C ABI, against the float64 / int64 restatement of
tests/retrieval_rank_restatement.py.

Integer-valued inputs make every score exact in fp32, so ranks and scores are compared exactly, ties and all; normal
inputs are checked row by row against the band of the restatement, which tests/test_retrieval_rank_host.py shows to be
a single value on 97 % of the rows."""

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers, retrieval_ops
from tests import retrieval_rank_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KRS_ERR_INVALID, KRS_ERR_UNSUPPORTED, KRS_ERR_WORKSPACE = -1, -2, -4
NAN = float("nan")


def _rank(q, c, pos=None, ids=None, path="auto"):
    """retrieval_rank on CPU inputs: (int64 rank, float64 score of the positive), back on the CPU"""
    rank, sp = retrieval_ops.retrieval_rank(q.to(DEV), c.to(DEV), None if pos is None else pos.to(DEV),
                                            None if ids is None else ids.to(DEV), path=path)
    assert rank.dtype == torch.int32 and sp.dtype == torch.float32 and rank.shape == sp.shape == (q.shape[0],)
    return rank.cpu().to(torch.int64), sp.cpu().to(torch.float64)


# ---- 1. ranks against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_integer_inputs_give_the_exact_rank_and_score_on_every_path(shape):
    q, c, pos = R.integers(*shape)
    want_rank, want_sp = R.rank_of(R.scores64(q, c), pos)
    for name, got in (("fused", _rank(q, c, pos, path="fused")), ("slab", _rank(q, c, pos, path="slab")),
                      ("fp32 auto", _rank(q.float(), c.float(), pos))):
        wrong = int((got[0] != want_rank).sum())
        print(f"{shape} {name}: {wrong} wrong ranks of {shape[0]}")
        assert torch.equal(got[0], want_rank), name
        assert torch.equal(got[1], want_sp), name


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.IDS)
def test_normal_inputs_stay_inside_the_band(shape):
    q, c, pos = R.normal(*shape)
    lo, hi, sp, dp = R.band(q, c, pos)
    rank, got_sp = _rank(q, c, pos, path="fused")
    print(f"{shape}: band of one value on {int((lo == hi).sum())} of {shape[0]} rows; rank outside on "
          f"{int(((rank < lo) | (rank > hi)).sum())}; worst |s_pos error| / delta = "
          f"{float(((got_sp - sp).abs() / dp.clamp(min=1e-300)).max()):.3g}")
    assert bool(((lo <= rank) & (rank <= hi)).all())
    assert bool(((got_sp - sp).abs() <= dp).all())


# ---- 2. ties, ids and special values ---------------------------------------------------------------------------------
DUP_SEED = 1


def duplicates_case(seed=DUP_SEED):
    """(33, 300, 16) of the normal builder; for each of the first 8 queries its positive's row copied byte for byte
    onto one candidate below and one above pos.  Returns (q, c, pos, drop) with drop [B, N] marking a row's own
    two copies."""
    b, n, d, rows = 33, 300, 16, 8
    q, c, pos = R.normal(b, n, d, seed=seed)
    taken = set(pos.tolist())
    drop = torch.zeros((b, n), dtype=torch.bool)
    c = c.clone()
    for i in range(rows):
        p = int(pos[i])
        below = next(j for j in range(p - 1, -1, -1) if j not in taken)
        above = next(j for j in range(p + 1, n) if j not in taken)
        taken.update((below, above))
        c[below], c[above] = c[p], c[p]
        drop[i, below] = drop[i, above] = True
    return q, c, pos, drop


def test_byte_identical_rows_tie_exactly_and_the_index_decides():
    q, c, pos, drop = duplicates_case()
    lo, hi, _, _ = R.band(q, c, pos, drop=drop)
    assert bool((lo[:8] == hi[:8]).all()), "pick another DUP_SEED: the band must be one value on the first 8 rows"
    rank, sp = _rank(q, c, pos, path="fused")
    print("duplicates: rank - lo of the first 8 rows", (rank[:8] - lo[:8]).tolist())
    assert torch.equal(rank[:8], lo[:8] + 1)            # the lower copy counts, the upper one does not
    assert bool(((lo[8:] <= rank[8:]) & (rank[8:] <= hi[8:])).all())


def _ids_case():
    """integer builder (40, 161, 64); each positive's id goes to two other candidates, the first of which (3 q_i)
    scores above the positive"""
    q, c, pos = R.integers(40, 161, 64)
    c = c.clone()
    free = [j for j in range(161) if j not in set(pos.tolist())]
    ids = torch.arange(161, dtype=torch.int64) + 1000
    for i in range(40):
        a, z = free[2 * i], free[2 * i + 1]
        c[a] = (3 * q[i].float()).to(torch.bfloat16)
        ids[a] = ids[z] = ids[pos[i]]
    s = R.scores64(q, c)
    assert float(s.abs().max()) < 2 ** 24
    a = torch.tensor(free[0:80:2])
    assert bool((s[torch.arange(40), a] > s[torch.arange(40), pos]).all())
    return q, c, pos, ids, s


def test_candidates_with_the_positives_id_are_not_counted():
    q, c, pos, ids, s = _ids_case()
    plain, with_ids = R.rank_of(s, pos)[0], R.rank_of(s, pos, ids)[0]
    assert bool((with_ids < plain).all())
    assert torch.equal(_rank(q, c, pos, path="fused")[0], plain)
    for path in ("fused", "slab"):
        for cast in (torch.int64, torch.int32):
            got, sp = _rank(q, c, pos, ids.to(cast), path=path)
            assert torch.equal(got, with_ids), (path, cast)
            assert torch.equal(sp, s.gather(1, pos[:, None])[:, 0])
    # negative ids, and ids that differ in the high word of an int64 only: no hits
    assert torch.equal(_rank(q, c, pos, -ids, path="fused")[0], with_ids)
    j = torch.arange(161, dtype=torch.int64)
    high = (j % 20) | ((j // 20) << 32)
    assert len(set(high.tolist())) == 161 and len(set((high & 0xffffffff).tolist())) == 20
    assert torch.equal(_rank(q, c, pos, high, path="fused")[0], plain)
    assert torch.equal(_rank(q, c, pos, high, path="slab")[0], plain)


def test_a_positive_outside_the_candidates_is_no_address():
    q, c, pos = R.integers(40, 161, 64)
    want_rank, want_sp = R.rank_of(R.scores64(q, c), pos)
    bad = pos.to(torch.int64).clone()
    bad[0], bad[1], bad[2], bad[3], bad[39] = -1, 161, 2 ** 32 + 1, -2 ** 32, 2 ** 31
    hit = torch.tensor([0, 1, 2, 3, 39])
    for path in ("fused", "slab"):
        rank, sp = _rank(q, c, bad, path=path)
        assert rank[hit].tolist() == [-1] * 5 and bool(torch.isnan(sp[hit]).all())
        keep = torch.ones(40, dtype=torch.bool)
        keep[hit] = False
        assert torch.equal(rank[keep], want_rank[keep]) and torch.equal(sp[keep], want_sp[keep])


def test_nan_ranks_above_everything_and_signed_zeros_tie():
    gen = torch.Generator().manual_seed(5)
    n, d = 40, 8
    c = torch.randint(-3, 4, (n, d), generator=gen).to(torch.bfloat16)
    q = torch.randint(-3, 4, (6, d), generator=gen).to(torch.bfloat16)
    c[2], c[5] = NAN, NAN                 # two candidates score NaN against every query
    q[4] = 0.0                            # every finite score of query 4 is +0.0
    c[9], c[20] = 0.0, 0.0
    q[5] = 0.0
    q[5, 0] = -1e-30                      # against candidate 9 below: -1e-60, -0.0 in fp32 where the product rounds
    c[:, 0] = 0.0                         # (column 0 is zero elsewhere -- the NaN rows too, it changes nothing there)
    c[9, 0] = 1e-30
    c[2], c[5] = NAN, NAN
    pos = torch.tensor([7, 5, 2, 30, 20, 9])
    s = R.scores64(q, c)
    s[5, 9] = -0.0                        # (what fp32 makes of -1e-60)
    want, _ = R.rank_of(s, pos)
    assert bool(torch.isnan(s[:, [2, 5]]).all()) and want[1] == 1 and want[2] == 0
    assert want[4] == 20 and want[5] == 9                  # zeros of either sign tie: every lower index counts
    for path in ("fused", "slab"):
        rank, sp = _rank(q, c, pos, path=path)
        assert torch.equal(rank, want), path
        assert bool(torch.isnan(sp[1:3]).all()) and sp[4] == 0.0 and sp[5] == 0.0
    finite = torch.tensor([0, 3])
    no_nan, _ = R.rank_of(torch.nan_to_num(s, nan=-1e9), pos)
    assert torch.equal(want[finite], no_nan[finite] + 2)   # both NaN candidates rank ahead of a finite positive


def test_degenerate_shapes_and_the_default_positive():
    q, c, _ = R.integers(40, 161, 64)
    s = R.scores64(q, c)
    for path in ("fused", "slab"):
        rank, sp = _rank(q, c, None, path=path)            # pos = None: candidate i for query i
        want = R.rank_of(s, torch.arange(40))
        assert torch.equal(rank, want[0]) and torch.equal(sp, want[1])
        rank, sp = _rank(q, c[:1], torch.zeros(40, dtype=torch.int64), path=path)       # N = 1
        assert rank.tolist() == [0] * 40 and torch.equal(sp, s[:, 0])
        rank, sp = _rank(q[:1], c, torch.tensor([160]), path=path)                      # B = 1
        assert torch.equal(rank, R.rank_of(s[:1], torch.tensor([160]))[0])
        rank, sp = _rank(q[:0], c, torch.zeros(0, dtype=torch.int64), path=path)        # B = 0
        assert rank.shape == (0,) and sp.shape == (0,)
    more, _, _ = R.integers(161, 40, 64)                   # pos = None with more queries than candidates
    rank, sp = _rank(more, c[:40], None, path="fused")
    want = R.rank_of(R.scores64(more, c[:40]), torch.arange(161))
    assert torch.equal(rank, want[0]) and bool(torch.isnan(sp[40:]).all()) and rank[40:].tolist() == [-1] * 121


@pytest.mark.parametrize("b,n,d,off,pad", [(40, 161, 64, 8, 8), (161, 40, 64, 8, 8), (40, 161, 40, 1, 2),
                                           (161, 40, 40, 1, 2), (40, 161, 37, 0, 3)],
                         ids=["aligned-sliced", "aligned", "misaligned-sliced", "misaligned", "odd-width"])
def test_column_slices_of_wider_matrices_need_no_copy(b, n, d, off, pad):
    q, c, pos = R.integers(b, n, d)
    wide_q = torch.full((b, off + d + pad), NAN, dtype=torch.bfloat16)
    wide_c = torch.full((n, off + d + pad), NAN, dtype=torch.bfloat16)
    wide_q[:, off:off + d], wide_c[:, off:off + d] = q, c
    vq, vc = wide_q.to(DEV)[:, off:off + d], wide_c.to(DEV)[:, off:off + d]
    assert vq.stride(0) == off + d + pad and not vq.is_contiguous()
    vec = vq.data_ptr() % 16 == 0 and vc.data_ptr() % 16 == 0 and vq.stride(0) % 8 == 0 and d % 8 == 0
    assert vec == (off == 8)
    rank, sp = retrieval_ops.retrieval_rank(vq, vc, pos.to(DEV), path="fused")
    want = R.rank_of(R.scores64(q, c), pos)
    assert torch.equal(rank.cpu().to(torch.int64), want[0]) and torch.equal(sp.cpu().to(torch.float64), want[1])


# ---- 3. interplay with the existing kernels and metrics ----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(161, 40, 64), (300, 1000, 128)], ids=["161x40x64", "300x1000x128"])
def test_agreement_with_brute_force_retrieval_and_sparse_top_k_accuracy(shape):
    q, c, pos = R.integers(*shape)
    qd, cd, posd = q.to(DEV), c.to(DEV), pos.to(DEV)
    rank, _ = retrieval_ops.retrieval_rank(qd, cd, posd)
    w = (torch.rand(shape[0], generator=torch.Generator().manual_seed(9)) * 2.0).to(DEV)
    ks = (1, 5, 40)
    for weight in (None, w):
        fact = layers.FactorizedTopK(cd, ks=ks)
        fact.update_state(qd, posd, sample_weight=weight)
        for k in ks:
            top = layers.BruteForceRetrieval(cd, k=k, return_scores=False)(qd)
            inside = (top.to(torch.int64) == posd.to(torch.int64)[:, None]).any(dim=1)
            assert torch.equal(inside, rank < k), k
            sparse = layers.SparseTopKCategoricalAccuracy(k=k, from_sorted_ids=True)
            sparse.update_state(posd, top, sample_weight=weight)
            assert float(sparse.result()) == pytest.approx(float(fact.result()[f"top_{k}_categorical_accuracy"]),
                                                           rel=1e-6)
        want = R.metric_values(rank.cpu(), None if weight is None else weight.cpu(), ks)
        got = {name: float(v) for name, v in fact.result().items()}
        assert got == pytest.approx(want, rel=1e-5)
        assert all(v.device.type == "cuda" and v.dtype == torch.float32 for v in fact.result().values())


def test_two_calls_on_a_sliced_shape_are_bit_identical():
    q, c, pos = R.normal(40, 161, 64)
    a, z = (retrieval_ops.retrieval_rank(q.to(DEV), c.to(DEV), pos.to(DEV), path="fused") for _ in range(2))
    assert torch.equal(a[0], z[0]) and torch.equal(a[1], z[1])


def test_update_state_in_a_captured_graph_equals_eager_updates():
    b, n, d = 40, 161, 64
    q0, c, p0 = R.normal(b, n, d)
    fresh = [R.normal(b, n, d, seed=70 + i) for i in range(2)]
    cd = c.to(DEV)
    w = torch.linspace(0.5, 1.5, b).to(DEV)
    metric = layers.FactorizedTopK(cd, ks=(1, 5, 40))
    qs, ps = q0.to(DEV), p0.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            metric.update_state(qs, ps, sample_weight=w)
    torch.cuda.current_stream().wait_stream(side)
    metric.reset_state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        metric.update_state(qs, ps, sample_weight=w)
    eager = layers.FactorizedTopK(cd, ks=(1, 5, 40))
    for fq, _, fp in fresh:
        qs.copy_(fq)
        ps.copy_(fp)
        graph.replay()
        eager.update_state(fq.to(DEV), fp.to(DEV), sample_weight=w)
    torch.cuda.synchronize()
    assert float(metric._state[-1]) == pytest.approx(2.0 * float(w.sum()))
    assert torch.equal(metric._state, eager._state)
    for name, v in metric.result().items():
        assert torch.equal(v, eager.result()[name])


# ---- 4. the C ABI, called directly, and memory -------------------------------------------------------------------------
class _Abi:
    def __init__(self, b, n, d):
        self.b, self.n, self.d = b, n, d
        q, c, pos = R.integers(b, n, d)
        self.want = R.rank_of(R.scores64(q, c), pos)
        self.q, self.c, self.pos = q.to(DEV), c.to(DEV), pos.to(torch.int32).to(DEV)
        self.size = retrieval_ops.retrieval_rank_workspace_bytes(b, n, d)

    def call(self, ws, ws_bytes, *, q="q", c="c", rank="new", sp="new", dtype=L.BF16, b=None, n=None, d=None):
        q = self.q if isinstance(q, str) else q
        c = self.c if isinstance(c, str) else c
        rank = torch.full((self.b,), 7, dtype=torch.int32, device=DEV) if isinstance(rank, str) else rank
        sp = torch.full((self.b,), 7.0, dtype=torch.float32, device=DEV) if isinstance(sp, str) else sp
        rc = L.lib().krs_retrieval_rank(L.ptr(q), self.d, L.ptr(c), self.d, dtype, self.b if b is None else b,
                                        self.n if n is None else n, self.d if d is None else d, L.ptr(self.pos), None,
                                        L.I32, L.ptr(rank), L.ptr(sp), L.ptr(ws), ws_bytes, L.stream_ptr())
        return rc, rank, sp


@pytest.fixture(scope="module", params=[(40, 161, 40), (161, 40, 40)], ids=["40x161x40", "161x40x40"])
def abi(request):
    return _Abi(*request.param)


def test_abi_runs_in_exactly_the_advertised_workspace_and_reads_nothing_it_did_not_write(abi):
    ws = torch.full((abi.size + 4096,), 0xFF, dtype=torch.uint8, device=DEV)       # NaN to a float read
    rc, rank, sp = abi.call(ws, abi.size)
    assert rc == 0
    assert torch.equal(rank.cpu().to(torch.int64), abi.want[0]) and torch.equal(sp.cpu().to(torch.float64), abi.want[1])
    assert bool((ws[abi.size:] == 0xFF).all())
    ws.fill_(0xFF)
    rc, rank, sp = abi.call(ws, abi.size, sp=None)              # out_pos_score = NULL: the scores stay in the workspace
    assert rc == 0 and sp is None and torch.equal(rank.cpu().to(torch.int64), abi.want[0])
    assert bool((ws[abi.size:] == 0xFF).all())


def test_abi_refusals_launch_nothing_and_say_why(abi):
    ws = torch.empty((abi.size,), dtype=torch.uint8, device=DEV)
    f32 = torch.zeros((max(abi.b, abi.n), abi.d), dtype=torch.float32, device=DEV)
    cases = [
        (dict(dtype=L.F32, q=f32, c=f32), KRS_ERR_UNSUPPORTED, b"bf16 inputs only"),
        (dict(d=257), KRS_ERR_UNSUPPORTED, b"above 256"),
        (dict(q=None), KRS_ERR_INVALID, b"null operand"),
        (dict(c=None), KRS_ERR_INVALID, b"null operand"),
        (dict(rank=None), KRS_ERR_INVALID, b"null output"),
        (dict(d=0), KRS_ERR_INVALID, b"bad shape"),
        (dict(n=0), KRS_ERR_INVALID, b"bad shape"),
        (dict(b=-1), KRS_ERR_INVALID, b"bad shape"),
    ]
    for kwargs, code, text in cases:
        rc, rank, sp = abi.call(ws, abi.size, **kwargs)
        assert rc == code and text in L.lib().krs_last_error(), (kwargs, rc, L.lib().krs_last_error())
        assert (rank is None or bool((rank == 7).all())) and bool((sp == 7.0).all())
    for args in ((ws, abi.size - 1), (None, abi.size), (None, 0)):
        rc, rank, sp = abi.call(*args)
        assert rc == KRS_ERR_WORKSPACE and b"workspace" in L.lib().krs_last_error()
        assert bool((rank == 7).all()) and bool((sp == 7.0).all())
    rc, rank, sp = abi.call(None, 0, q=None, c=None, rank=None, sp=None, b=0)      # b == 0: nothing to do
    assert rc == 0
    with pytest.raises(L.KrsError):
        retrieval_ops.retrieval_rank(f32[:4], f32[:5], path="fused")               # the wrapper reports a refusal


def test_the_scores_are_never_stored():
    b, n, d = 2048, 8192, 64                                   # one fp32 score matrix would be 64 MiB
    gen = torch.Generator().manual_seed(11)
    q = (torch.randn(b, d, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    c = (torch.randn(n, d, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    pos = torch.randint(0, n, (b,), generator=gen).to(torch.int32).to(DEV)
    retrieval_ops.retrieval_rank(q, c, pos)                     # (first use: the library and its kernels are loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rank, sp = retrieval_ops.retrieval_rank(q, c, pos)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    budget = retrieval_ops.retrieval_rank_workspace_bytes(b, n, d) + (1 << 20)
    print(f"peak rise {rise} bytes, budget {budget}")
    assert rise <= budget < 4 * b * n // 8
    assert int(rank.min()) >= 0 and int(rank.max()) < n and bool(torch.isfinite(sp).all())


def test_the_examples_evaluate_reports_the_restated_values():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("two_tower_retrieval",
                                                  os.path.join(root, "examples", "two_tower_retrieval.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    q, c, pos = R.integers(161, 40, 64)
    want = R.metric_values(R.rank_of(R.scores64(q, c), pos)[0], None, (1, 5, 10))
    for cast in (torch.bfloat16, torch.float32):           # the fused kernel, and the slab path of fp32 towers
        got = example.evaluate(q.to(DEV).to(cast), c.to(DEV).to(cast), pos.to(DEV), ks=(1, 5, 10))
        assert got == pytest.approx(want, rel=1e-6) and all(isinstance(v, float) for v in got.values())
