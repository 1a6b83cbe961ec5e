"""K16 on the GPU: krs_quantize_rows_q8 bit for bit against the numpy restatement, krs_embed_bag_fwd_q8 on every kernel
instantiation and branch against float64 (tests/embed_q8_cases.py, tests/embed_q8_restatement.py), and the layers'
quantize("int8").

Lookup, per case: embed_fwd_q8_last_route() equals the expected record;
    |got - ref| <= 2 * (gamma(n + 3) * M / |den| + gamma(n + 1) * |ref|) + u_out * |ref|
(gamma(k) = k u / (1 - k u), u = 2^-24, M = sum |w step q|, n the bag's lookups, u_out = 2^-24 or 2^-8 for bf16 output);
a bag whose divisor is exactly 0 gives exactly 0; step[0] is NaN on every table and no valid id is 0, so the outputs must
be finite; the NaN-filled columns around the feature slots stay NaN; the error word equals the expected one.
tests/test_embed_q8_host.py checks on the CPU that a plain fp32 evaluation stays inside this bound for every case.
"""

import functools

import numpy as np
import pytest
import torch

from tests import embed_q8_restatement as Q
from tests.embed_q8_cases import BY_NAME, CASES, LARGEST, R, inputs, q_table, step_array

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U = 2.0 ** -24


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the quantizer, bit for bit ------------------------------------------------------------------------------------------

def _source_table(vocab, dim, src):
    """float32 values exact in the source dtype: magnitudes over 14 decades, and for vocab 67 the special rows"""
    rng = np.random.default_rng(1000 * vocab + dim)
    x = (rng.standard_normal((vocab, dim)) * np.logspace(-8, 6, vocab)[:, None]).astype(np.float32)
    if vocab > 20:
        x[3] = 0                                              # an all-zero row
        x[4] = -np.abs(x[4]) - np.float32(1e-3)               # the largest element is negative
        x[4, 0] *= 3
        tie = np.array([127, 0.5, 1.5, 2.5, -0.5, -1.5], np.float32)
        x[6] = 0
        x[6, :min(dim, 6)] = tie[:min(dim, 6)]               # 127 + 1e-7 == 127 in fp32, inv == 1: ties go to even
        x[9, dim // 2] = np.nan                               # rows 8 and 10 are its neighbours
        x[12, dim - 1] = np.inf
        x[14, 0] = -np.inf
        x[20] = np.float32(2) ** -140                         # fp32 subnormals (zero in bf16)
    if src == "bf16":
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    return x


@pytest.mark.parametrize("src", ["f32", "bf16"])
@pytest.mark.parametrize("vocab", [1, 67])
@pytest.mark.parametrize("dim", [1, 16, 20, 128, 1040])
def test_the_quantizer_equals_the_restatement_bit_for_bit(dim, vocab, src):
    from keras_rs_amd import embedding_ops as E

    x = _source_table(vocab, dim, src)
    want_q, want_step, bad = Q.quantize(x)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    q, step = E.quantize_rows(torch.from_numpy(x).to(TORCH_DT[src]).to(DEV), flag)
    torch.cuda.synchronize()
    assert q.dtype == torch.int8 and step.dtype == torch.float32 and tuple(q.shape) == (vocab, dim)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(step.cpu().numpy().view(np.uint32), want_step.view(np.uint32))
    assert int(flag.item()) == (Q.FLAG_NONFINITE_ROW if bad.any() else 0)
    if vocab > 20:
        assert bad.nonzero()[0].tolist() == [9, 12, 14]
        assert (want_q[[9, 12, 14]] == 0).all() and (want_step[[9, 12, 14]] == 0).all()
        assert (want_step[[8, 10, 11, 13, 15]] > 0).all() and np.abs(want_q[[8, 10, 11, 13, 15]]).max() > 0
        if dim >= 6:
            assert want_q[6, :6].tolist() == [127, 0, 2, 2, 0, -2] and want_step[6] == 1.0
        assert want_q[4].min() == -127 and (want_q[3] == 0).all()


def test_the_quantizer_on_a_table_off_its_16_byte_alignment():
    """dim % 16 == 0 with a base pointer 4 bytes off: the element-by-element form, same bits"""
    from keras_rs_amd import embedding_ops as E

    x = _source_table(67, 128, "f32")
    flat = torch.empty(67 * 128 + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(67, 128)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4
    q, step = E.quantize_rows(view)
    want_q, want_step, _ = Q.quantize(x)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(step.cpu().numpy().view(np.uint32), want_step.view(np.uint32))


# ---- the lookup against float64 ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(name):
    c, h = BY_NAME[name], inputs(name)
    return Q.restate(h["q_tables"], h["steps"], c.feats, c.batch, c.dim, h["ids"], hots=c.hots, offsets=h["offsets"],
                     weights=h["weights"])


def _device_inputs(h):
    return ([torch.from_numpy(t).to(DEV) for t in h["q_tables"]], [torch.from_numpy(s).to(DEV) for s in h["steps"]],
            torch.from_numpy(h["ids"]).to(DEV), None if h["offsets"] is None else torch.from_numpy(h["offsets"]).to(DEV),
            None if h["weights"] is None else torch.from_numpy(h["weights"]).to(DEV))


def _run(c, dev_in):
    """One krs_embed_bag_fwd_q8 of case c into a NaN-filled slab: (slab, flag word, route)."""
    from keras_rs_amd import embedding_ops as E

    q_tables, steps, ids, offsets, weights = dev_in
    qb = E.QuantizedBags(q_tables, steps, [(t, comb, col) for (t, comb), col in zip(c.feats, c.out_cols)])
    buf = torch.full((c.batch, c.width), float("nan"), dtype=TORCH_DT[c.odt], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = qb.forward(ids, c.batch, hots=c.hots, offsets=offsets, weights=weights, out=buf, err_flag=flag)
    route = E.embed_fwd_q8_last_route()
    torch.cuda.synchronize()
    assert out is buf
    return buf.cpu(), int(flag.item()), route


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_route_against_float64(case):
    c, h, ref = case, inputs(case.name), _reference(case.name)
    buf, flag, route = _run(c, _device_inputs(h))
    assert route == c.route
    assert flag == c.flag and ref["bad"] == bool(c.bad)
    untouched = torch.ones(c.width, dtype=torch.bool)
    for col in c.out_cols:
        untouched[col:col + c.dim] = False
    assert bool(buf[:, untouched].isnan().all()), "a column outside the feature slots was written"
    tol = Q.bound(ref, c.odt == "bf16")
    for f, col in enumerate(c.out_cols):
        got = buf[:, col:col + c.dim]
        what = f"{c.name} feature {f}"
        assert bool(got.isfinite().all()), what + ": the stand-in row leaked (NaN step) or a slot was not written"
        g64 = got.double().numpy()
        zero = ref["den"][f] == 0
        assert (g64[zero] == 0).all(), what
        err = np.abs(g64 - ref["out"][f])
        worst = float((err[~zero] / np.maximum(tol[f][~zero], 1e-300)).max()) if (~zero).any() else 0.0
        print(f"{what}: worst error / bound = {worst:.3f}")
        assert worst <= 1.0, what


def test_two_calls_of_the_largest_case_give_the_same_bytes():
    c = BY_NAME[LARGEST]
    dev_in = _device_inputs(inputs(c.name))
    a, _, route_a = _run(c, dev_in)
    b, _, route_b = _run(c, dev_in)
    assert route_a == route_b == c.route
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dim,kernel", [(128, "vec"), (1024, "vec"), (20, "generic"), (1, "generic")])
def test_a_pure_gather_is_one_correctly_rounded_multiply(dim, kernel):
    """hot = 1, unweighted, sum, fp32 out: bit-equal to q.float() * step[:, None] in torch"""
    from keras_rs_amd import embedding_ops as E

    vocab, batch = 300, 67
    q = torch.from_numpy(q_table(vocab, dim)).to(DEV)
    step = torch.from_numpy(step_array(vocab, 5)).to(DEV)
    ids = torch.from_numpy(((np.arange(2 * batch) * 37) % (vocab - 1) + 1).astype(np.int32)).to(DEV)
    ids[:2] = torch.tensor([1, 2], dtype=torch.int32)          # the -128 row and the +127 row
    qb = E.QuantizedBags([q], [step], [(0, "sum", 0), (0, "sum", dim)])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = qb.forward(ids, batch, hots=(1, 1), err_flag=flag)
    assert E.embed_fwd_q8_last_route()["kernel"] == kernel and int(flag.item()) == 0
    want = (q.float() * step[:, None])[ids.long()].reshape(2, batch, dim)
    assert out.dtype == torch.float32 and bool(out.isfinite().all())
    assert torch.equal(_bits(out[:, :dim]), _bits(want[0])) and torch.equal(_bits(out[:, dim:]), _bits(want[1]))
    s1, s2 = np.float32(step[1].item()), np.float32(step[2].item())
    assert np.float32(out[0, 0].item()) == np.float32(-128) * s1 and np.float32(out[1, 0].item()) == np.float32(127) * s2


@pytest.mark.parametrize("dim", [128, 20])
def test_out_of_range_ids_add_nothing_count_in_the_mean_and_raise_the_flag(dim):
    from keras_rs_amd import embedding_ops as E

    vocab = 37
    q = torch.from_numpy(q_table(vocab, dim)).to(DEV)
    step = torch.full((vocab,), 0.25, device=DEV)
    step[0] = float("nan")
    qb = E.QuantizedBags([q], [step], [(0, "mean", 0)])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for dt in (torch.int32, torch.int64):
        ids = torch.tensor([[5, 7], [-1, 9], [11, vocab], [-1, vocab]], dtype=dt, device=DEV)
        rows = q.float() * 0.25
        flag.zero_()
        out = qb.forward(ids[:1].reshape(-1).contiguous(), 1, hots=(2,), err_flag=flag)
        assert int(flag.item()) == 0 and torch.equal(out[0], (rows[5] + rows[7]) / 2)          # in range: the flag stays 0
        out = qb.forward(ids.reshape(-1), 4, hots=(2,), err_flag=flag)
        assert int(flag.item()) == Q.FLAG_ID_OUT_OF_RANGE
        assert torch.equal(out[0], (rows[5] + rows[7]) / 2) and torch.equal(out[1], rows[9] / 2)
        assert torch.equal(out[2], rows[11] / 2) and bool((out[3] == 0).all())


def test_a_lookup_captured_in_a_graph_and_replayed_twice_equals_the_eager_result():
    from keras_rs_amd import embedding_ops as E

    c = BY_NAME["vec-bf16-hot1-d128"]
    h = inputs(c.name)
    q_tables, steps, ids, _, _ = _device_inputs(h)
    qb = E.QuantizedBags(q_tables, steps, [(t, comb, f * c.dim) for f, (t, comb) in enumerate(c.feats)])
    other = ids.view(c.n_feats, c.batch).roll(1, dims=1).reshape(-1).contiguous()      # (every id stays on its own table)
    eager = [qb.forward(i, c.batch, hots=c.hots, out_dtype=torch.bfloat16).clone() for i in (ids, other)]
    static_ids, flag = ids.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros_like(eager[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        qb.forward(static_ids, c.batch, hots=c.hots, out=out, err_flag=flag)        # (descriptors are uploaded and cached here)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # (an allocation or a host wait in the entry would fail the capture)
        qb.forward(static_ids, c.batch, hots=c.hots, out=out, err_flag=flag)
    for src, want in ((other, eager[1]), (ids, eager[0])):
        static_ids.copy_(src)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)) and int(flag.item()) == 0


# ---- the layers ----------------------------------------------------------------------------------------------------------

def _dense_reference(T64, ids, w, combiner, per_row=False):
    """float64 EmbedReduce on dense [B, L] ids: (out, bound).  w: None, [B, L], [B, L, D], or with per_row [B] (the
    reference expands it at the end: mean divides by w_b, sqrtn by |w_b|)."""
    B, Ln = ids.shape
    x = T64[ids]
    if w is None:
        wl = np.ones((B, Ln, 1))
    elif per_row:
        wl = np.asarray(w, np.float64).reshape(B, 1, 1) * np.ones((1, Ln, 1))
    else:
        wl = np.asarray(w, np.float64).reshape(B, Ln, -1)
    num, M = (x * wl).sum(1), np.abs(x * wl).sum(1)
    if combiner == "sum":
        den = np.ones((B, 1))
    elif per_row:
        wb = np.asarray(w, np.float64).reshape(B, 1)
        den = wb if combiner == "mean" else np.abs(wb)
    else:
        den = wl.sum(1) if combiner == "mean" else np.sqrt((wl * wl).sum(1))
    safe = np.where(den == 0, 1.0, den)
    out = np.where(den == 0, 0.0, num / safe)
    g = Q.RS.gamma
    tol = 2 * (g(Ln + 3) * M / np.abs(safe) + g(Ln + 1) * np.abs(out)) + U * np.abs(out)
    return out, tol


def _pair(make):
    """(quantized layer, float layer holding q * step, the float64 table q * step)"""
    a, b = make(), make()
    a.build(), b.build()
    with torch.no_grad():
        a.embeddings.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-2, 2, tuple(a.embeddings.shape)).astype(np.float32)))
    a.quantize("int8")
    assert a.embeddings is None and a.weights == [] and a.trainable_weights == []
    assert sorted(k for k in a.state_dict()) == ["embeddings_q", "embeddings_step"]
    q, step = a.embeddings_q, a.embeddings_step
    with torch.no_grad():
        b.embeddings.copy_(q.float() * step[:, None])
    return a, b, Q.dequantized(q.cpu().numpy(), step.cpu().numpy())


@pytest.mark.parametrize("dim", [16, 20])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_embed_reduce_quantized_agrees_with_the_float_layer_on_q_times_step(combiner, dim):
    import keras_rs_amd.layers as kl

    vocab, B, Ln = 67, 5, 7
    a, b, T64 = _pair(lambda: kl.EmbedReduce(vocab, dim, combiner=combiner, device=DEV))
    rng = np.random.default_rng(dim)
    ids2 = rng.integers(0, vocab, (B, Ln)).astype(np.int32)
    w2 = rng.uniform(0.25, 1.0, (B, Ln)).astype(np.float32)
    wb = np.array([0.5, -1.5, 0.0, 2.0, 1.0], np.float32)
    w3 = rng.uniform(0.25, 1.0, (B, Ln, dim)).astype(np.float32)

    def check(what, got_a, got_b, ref, tol):
        assert not got_a.requires_grad and got_a.dtype == torch.float32, what
        ga, gb = got_a.double().cpu().numpy(), got_b.detach().double().cpu().numpy()
        assert ga.shape == ref.shape, what
        assert (np.abs(ga - gb) <= tol).all() and (np.abs(ga - ref) <= tol).all(), what

    check("rank 2", a(ids2), b(ids2), *_dense_reference(T64, ids2, None, combiner))
    check("rank 2, weights", a(ids2, w2), b(ids2, w2), *_dense_reference(T64, ids2, w2, combiner))
    check("rank 2, [B] weights", a(ids2, wb), b(ids2, wb), *_dense_reference(T64, ids2, wb, combiner, per_row=True))
    check("rank 2, per-dimension weights", a(ids2, w3), b(ids2, w3), *_dense_reference(T64, ids2, w3, combiner))
    # rank 1: no reduction (weights only survive for "sum")
    ids1, w1 = ids2[:, 0], w2[:, 0]
    ref1 = _dense_reference(T64, ids1[:, None], w1[:, None] if combiner == "sum" else None, "sum")
    check("rank 1", a(ids1, w1), b(ids1, w1), *ref1)
    # ragged: rows of 3, 0, 1, 4, 2 ids; an empty row gives zeros
    lens = [3, 0, 1, 4, 2]
    rows = [rng.integers(0, vocab, n).astype(np.int32) for n in lens]
    wrows = [rng.uniform(0.25, 1.0, n).astype(np.float32) for n in lens]
    rag = kl.Ragged.from_rows(rows)
    ragw = kl.Ragged(np.concatenate(wrows), rag.row_offsets)
    pad_ids = np.ones((B, 4), np.int64)
    pad_w = np.zeros((B, 4), np.float64)
    for i, (r, w) in enumerate(zip(rows, wrows)):
        pad_ids[i, :len(r)], pad_w[i, :len(r)] = r, w
    check("ragged", a(rag, ragw), b(rag, ragw), *_dense_reference(T64, pad_ids, pad_w, combiner))
    assert bool((a(rag, ragw)[1] == 0).all())
    with pytest.raises(IndexError):
        a(np.array([[1, vocab]], np.int32))
    # the checkpoint: int8 rows and steps, no float table; loaded into a quantized layer of the same config, same bits
    c = kl.EmbedReduce(vocab, dim, combiner=combiner, device=DEV)
    c.build()
    with pytest.raises(RuntimeError):
        c.load_state_dict(a.state_dict())          # not quantized yet
    c.quantize("int8")
    c.load_state_dict(a.state_dict())
    assert torch.equal(_bits(c(ids2, w2)), _bits(a(ids2, w2))) and torch.equal(_bits(c(rag, ragw)), _bits(a(rag, ragw)))
    with pytest.raises(RuntimeError, match="already quantized"):
        a.quantize("int8")
    # a dtype cast of the module leaves the int8 rows alone and the steps fp32, bit for bit: same outputs
    before, steps = a(ids2, w2).clone(), a.embeddings_step.clone()
    a.bfloat16()
    assert a.embeddings_step.dtype == torch.float32 and torch.equal(a.embeddings_step, steps)
    assert a.embeddings_q.dtype == torch.int8 and torch.equal(_bits(a(ids2, w2)), _bits(before))


def test_embedding_quantized_gathers_q_times_step_for_any_rank_and_refuses_a_nonfinite_table():
    import keras_rs_amd.layers as kl

    vocab, dim = 67, 48
    a, b, T64 = _pair(lambda: kl.Embedding(vocab, dim, device=DEV))
    ids = np.random.default_rng(1).integers(0, vocab, (3, 4, 5)).astype(np.int64)
    got = a(ids)
    assert tuple(got.shape) == (3, 4, 5, dim) and not got.requires_grad
    want = (a.embeddings_q.float() * a.embeddings_step[:, None])[torch.from_numpy(ids).to(DEV)]
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got), _bits(b(ids).detach()))
    bad = kl.Embedding(vocab, dim, device=DEV)
    bad.build()
    with torch.no_grad():
        bad.embeddings[5, 7] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        bad.quantize("int8")
    assert bad.quantization_mode is None and bad.embeddings is not None and len(bad.weights) == 1      # left as it was
    # bf16 table, bf16 compute: quantized from the bf16 values, gathered into bf16
    h = kl.Embedding(vocab, dim, dtype="bfloat16", device=DEV)
    h.build()
    table = h.embeddings.detach().float().cpu().numpy()
    h.quantize("int8")
    want_q, want_step, _ = Q.quantize(table)
    np.testing.assert_array_equal(h.embeddings_q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(h.embeddings_step.cpu().numpy(), want_step)
    out = h(ids[0])
    assert out.dtype == torch.bfloat16
    assert torch.equal(_bits(out), _bits((h.embeddings_q.float() * h.embeddings_step[:, None])[torch.from_numpy(ids[0]).to(DEV)]
                                         .to(torch.bfloat16)))


def _de_configs(kl, batch):
    """two widths (16: vector path, 20: generic), both placements, a named stack of two 'sparsecore' tables, a shared table"""
    def tc(name, vocab, dim, placement, combiner, opt):
        return kl.TableConfig(name, vocab, dim, placement=placement, optimizer=opt, combiner=combiner)

    s1, s2 = tc("s1", 67, 16, "sparsecore", "mean", "adagrad"), tc("s2", 37, 16, "sparsecore", "sum", "adagrad")
    s3 = tc("s3", 50, 20, "sparsecore", "sqrtn", "sgd")
    d1, d2 = tc("d1", 41, 16, "default_device", "sum", "sgd"), tc("d2", 300, 20, "default_device", "mean", "sgd")
    tables = dict(a=(s1, 3), b=(s2, 1), c=(s1, 2), d=(s3, 4), e=(d1, 2), f=(d2, 5))
    feats = {k: kl.FeatureConfig(k, t, (batch, hot), (batch, t.embedding_dim)) for k, (t, hot) in tables.items()}
    return feats, {k: hot for k, (_, hot) in tables.items()}


def test_distributed_embedding_quantized_serves_what_the_float_layer_on_q_times_step_serves():
    import keras_rs_amd.layers as kl

    batch = 5
    feats, hots = _de_configs(kl, batch)
    a = kl.DistributedEmbedding(feats, table_stacking=[["s1", "s2"]])
    a.build(None)
    assert any("slot" in n for n in a.state_dict()) and any("stack" in n for n in a.state_dict())
    floats = {k: v.clone() for k, v in a.get_embedding_tables().items()}
    a.quantize("int8")
    sd = a.state_dict()
    assert sorted(k for k in sd if k != "_extra_state") == sorted(
        f"{p}_{t}_{s}" for p, ts in (("sparsecore", ("s1", "s2", "s3")), ("default_device", ("d1", "d2"))) for t in ts
        for s in ("q", "step"))
    assert all(v.dtype in (torch.int8, torch.float32) and (v.dtype == torch.int8) == k.endswith("_q")
               for k, v in sd.items() if k != "_extra_state")
    assert a.weights == [] and list(a.parameters()) == []
    qt = a.get_quantized_tables()
    deq = a.get_embedding_tables()
    for name, (q, step) in qt.items():       # quantized row by row like any table, the stacked ones included
        want_q, want_step, _ = Q.quantize(floats[name].float().cpu().numpy())
        np.testing.assert_array_equal(q.cpu().numpy(), want_q)
        np.testing.assert_array_equal(step.cpu().numpy(), want_step)
        assert deq[name].dtype == torch.float32 and torch.equal(deq[name], q.float() * step[:, None])
    b = kl.DistributedEmbedding(_de_configs(kl, batch)[0], table_stacking=[["s1", "s2"]])
    b.set_embedding_tables(deq)
    rng = np.random.default_rng(8)
    vocab_of = {k: fc.table.vocabulary_size for k, fc in feats.items()}
    ids = {k: rng.integers(0, vocab_of[k], (batch, hots[k])).astype(np.int32) for k in feats}
    w = {k: rng.uniform(0.25, 1.0, (batch, hots[k])).astype(np.float32) for k in feats}
    for weights in (None, w):
        with torch.no_grad():
            out_a, out_b = a(ids, weights), b(ids, weights)
        a.check_ids(wait=True)
        for k, fc in feats.items():
            ref, tol = _dense_reference(deq[fc.table.name].double().cpu().numpy(), ids[k],
                                        None if weights is None else w[k], fc.table.combiner)
            ga, gb = out_a[k].double().cpu().numpy(), out_b[k].double().cpu().numpy()
            assert not out_a[k].requires_grad and ga.shape == (batch, fc.table.embedding_dim), k
            assert (np.abs(ga - gb) <= tol).all() and (np.abs(ga - ref) <= tol).all(), k
    with pytest.raises(RuntimeError, match="training=True"):
        a(ids, training=True)
    with pytest.raises(RuntimeError, match="cannot be set"):
        a.set_embedding_tables(deq)
    with pytest.raises(RuntimeError, match="already quantized"):
        a.quantize("int8")
    # the id check works as before: the flag is raised by the int8 kernel, read lazily
    bad_ids = dict(ids, a=np.full((batch, hots["a"]), 67, np.int32))
    a(bad_ids)
    with pytest.raises(IndexError):
        a.check_ids(wait=True)
    # the checkpoint round trip into a layer of the same config on which quantize("int8") was called: same bits
    c = kl.DistributedEmbedding(_de_configs(kl, batch)[0], table_stacking=[["s1", "s2"]])
    c.build(None)
    c.quantize("int8")
    c.load_state_dict(sd)
    out_c, out_a = c(ids, w), a(ids, w)
    for k in feats:
        assert torch.equal(_bits(out_c[k]), _bits(out_a[k])), k
    # .half() on the quantized layer: rows stay int8, steps stay fp32 with their bits, the descriptors follow
    c.half()
    assert all(v.dtype == (torch.int8 if k.endswith("_q") else torch.float32) and torch.equal(v, sd[k])
               for k, v in c.state_dict().items() if k != "_extra_state")
    out_h = c(ids, w)
    for k in feats:
        assert torch.equal(_bits(out_h[k]), _bits(out_a[k])), k


def test_distributed_embedding_quantized_keeps_the_slab_and_concat_features_in_place():
    import keras_rs_amd.layers as kl

    batch, dim, lead = 5, 16, 13
    t = kl.TableConfig("t", 67, dim, placement="sparsecore", optimizer="sgd", combiner="sum")
    feats = {k: kl.FeatureConfig(k, t, (batch, 2), (batch, dim)) for k in ("a", "b")}
    layer = kl.DistributedEmbedding(feats, slab_lead_cols=lead)
    layer.build(None)
    layer.quantize("int8")
    ids = {k: np.random.default_rng(i).integers(0, 67, (batch, 2)).astype(np.int32) for i, k in enumerate(feats)}
    out = layer(ids)
    dense = torch.arange(batch * lead, dtype=torch.float32, device=DEV).reshape(batch, lead)
    want = torch.cat([dense, out["a"], out["b"]], dim=-1)
    slab = out["a"]._krs_slab[0]
    cat = kl.concat_features([dense, out["a"], out["b"]])
    assert cat.data_ptr() == slab.data_ptr() and tuple(cat.shape) == (batch, lead + 2 * dim)      # written in place
    assert torch.equal(cat, want)
    q, step = layer.get_quantized_tables()["t"]
    T64 = Q.dequantized(q.cpu().numpy(), step.cpu().numpy())
    for k in feats:          # (the sum of two rows may cancel: the bound is on the terms, not on the result)
        ref, tol = _dense_reference(T64, ids[k], None, "sum")
        assert (np.abs(out[k].double().cpu().numpy() - ref) <= tol).all(), k


def test_the_keras_adapter_layer_forwards_quantize():
    from keras_rs_amd import keras_adapter
    from tests import keras_stub

    import keras_rs_amd.layers as kl

    before = keras_stub.Layer.DEVICE
    keras_stub.Layer.DEVICE = DEV
    try:
        ns = keras_adapter.make_layers(keras_stub)
        t = kl.TableConfig("t", 67, 16, placement="default_device", optimizer="sgd", combiner="mean")
        layer = ns.DistributedEmbedding({"a": kl.FeatureConfig("a", t, (5, 2), (5, 16))})
        layer.build(None)
        with pytest.raises(ValueError):
            layer.quantize("int4")
        assert len(layer.weights) == 1 and tuple(layer.weights[0].shape) == (67, 16)     # the float table, tracked at build()
        import weakref

        table = weakref.ref(layer.weights[0].value)
        layer.quantize("int8")
        # the float table is gone from every surface: Keras' tracked variables, the adapter's own list, the wrapped module
        assert layer.weights == [] and layer.trainable_weights == [] and layer.non_trainable_weights == []
        assert layer._table_variables == [] and list(layer._impl.parameters()) == []
        assert all(not b.is_floating_point() or b.dim() == 1 for b in layer._impl.buffers())      # int8 rows, [V] steps
        import gc

        gc.collect()
        assert table() is None, "something still holds the float table"
        q, step = layer.get_quantized_tables()["t"]
        assert q.dtype == torch.int8 and torch.equal(layer.get_embedding_tables()["t"], q.float() * step[:, None])
        ids = np.arange(10, dtype=np.int32).reshape(5, 2)
        ref, tol = _dense_reference(Q.dequantized(q.cpu().numpy(), step.cpu().numpy()), ids, None, "mean")
        assert (np.abs(layer.call({"a": ids})["a"].double().cpu().numpy() - ref) <= tol).all()
    finally:
        keras_stub.Layer.DEVICE = before
