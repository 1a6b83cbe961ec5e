"""K2 apply: the deep front of bag_apply_fast_kernel (KRS_EMBED_OPT_APPLY_DEPTH = 4 / 8 / 16: sixteen values of a longer
segment in one load, that many gradient rows requested together) against the remainder loop (depth 0), bit for bit, in
every apply form; and depth 0 against the oracle.

Segment lengths (lookups of one table row) cover every boundary of the schedule: kFastFirst = 2 (1, 2, 3), the trip
sizes 4 / 8 / 16 after the first two (4, 6, 7, 10, 11, 18), the 16-value block (16, 17, 18, 33 = two blocks and one),
kLongSeg = 128 (128, 129) and a row of 450 lookups for the workgroup-per-row kernel.  One row's eight lookups all
come from one bag, out-of-range ids form the trailing run, one table is shared by two features.

Tolerances against the oracle (depth 0 only).  Gradients, weights and bag scales are positive, so a row's sum has no
cancellation.  Rows of <= 128 lookups are summed in the oracle's order (ascending position, fmaf): 1e-6 as in
tests/test_embed_bag_bwd_gpu.py.  Longer rows are summed by a workgroup in another order; two fp32 sums of n positive
terms differ by at most 2 (n - 1) 2^-24 relative, n = 450: 5.4e-5.  SGD carries that into the row as lr * dg, Adagrad as
2 dg / g on the accumulator's g^2 and, through g / sqrt(acc), as no more than that times lr on the row; bf16 rows add
one rounding (2^-7 as in the harness)."""

import numpy as np
import pytest
import torch

from oracle import krs_oracle as ko
from tests.helpers import to_f32, to_np
from tests.test_embed_bag_bwd_gpu import ADAM, FTRL, TORCH_DT

pytestmark = pytest.mark.gpu

BATCH, HOT, HOT_SHARED = 96, 8, 2
VOCABS = [64, 5]
LENGTHS = [1, 2, 3, 4, 6, 7, 10, 11, 16, 17, 18, 33, 128, 129]       # rows 0 .. 13 of the 64-row table
SMALL_TABLE = [129, 128, 450, 17, 4]                                   # the five rows of the other
N_BAD = 40                                                             # out-of-range ids per 8-hot feature
LONG_RTOL = 2 * (450 - 1) * 2.0 ** -24
DEPTHS = (4, 8, 16)
MODES = ("dense", "sparse", "sgd", "adagrad", "adagrad_rowwise", "adam", "adam_dyn", "ftrl")
LRS = [0.01, 0.02]


def _ids():
    """Feature-major ids of f0 (64-row table, 8 per bag), f1 (5-row table, 8 per bag), f2 (64-row table again, 2 per
    bag, rows 15 .. 63 only, so that rows 0 .. 14 keep the lengths chosen here)."""
    rng = np.random.default_rng(17)
    n = BATCH * HOT
    bad = np.where(np.arange(N_BAD) % 2 == 0, -3, 1000)
    f0 = np.concatenate([np.repeat(np.arange(len(LENGTHS)), LENGTHS), bad])
    f0 = np.concatenate([f0, rng.integers(15, 64, n - HOT - f0.size)])
    f0 = np.concatenate([np.full(HOT, 14), rng.permutation(f0)])         # bag 0 looks row 14 up eight times
    f1 = np.concatenate([np.repeat(np.arange(5), SMALL_TABLE), bad])
    assert f0.size == n and f1.size == n
    f2 = rng.integers(15, 64, BATCH * HOT_SHARED)
    ids = np.concatenate([f0, rng.permutation(f1), f2]).astype(np.int32)
    valid0 = np.concatenate([f0, f2])
    counts0 = np.bincount(valid0[(valid0 >= 0) & (valid0 < 64)], minlength=64)
    assert list(counts0[:15]) == LENGTHS + [HOT]
    return ids, [counts0, np.asarray(SMALL_TABLE)]


def _case(tdt, gdt, dim, use_w, use_scale):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    ids_np, counts = _ids()
    hots = [HOT, HOT, HOT_SHARED]
    tix = [0, 1, 0]
    specs = [(tix[f], "sum", 2 + f * dim) for f in range(3)]
    cols = 2 + 3 * dim + 3
    tables = [torch.from_numpy(rng.uniform(-1, 1, (v, dim)).astype(np.float32)).to(TORCH_DT[tdt]).to(dev) for v in VOCABS]
    grad = torch.from_numpy(rng.uniform(0.05, 1, (BATCH, cols)).astype(np.float32)).to(TORCH_DT[gdt]).to(dev)
    w_np = rng.uniform(0.1, 1, ids_np.size).astype(np.float32)
    scale_np = rng.uniform(0.25, 1, 3 * BATCH).astype(np.float32)
    # oracle dense gradient: the out-of-range lookups removed by a zero weight
    table_of = np.repeat(tix, [BATCH * h for h in hots])
    ok = (ids_np >= 0) & (ids_np < np.asarray(VOCABS)[table_of])
    feats_np = ko.make_features(tix, ["sum"] * 3, [c for _, _, c in specs], hots=hots, batch=BATCH)
    de = [np.zeros((v, dim), np.float32) for v in VOCABS]
    ko.embed_bag_bwd_dense(ko.make_tables(de), feats_np, np.where(ok, ids_np, 0).astype(np.int32), None,
                           (w_np if use_w else np.ones_like(w_np)) * ok, scale_np if use_scale else None, to_np(grad),
                           BATCH, dim)
    return dict(dev=dev, ids=torch.from_numpy(ids_np).to(dev), hots=hots, specs=specs, tables=tables, grad=grad,
                w=torch.from_numpy(w_np).to(dev) if use_w else None,
                scale=torch.from_numpy(scale_np).to(dev) if use_scale else None, de=de, counts=counts, dim=dim,
                nnz=int(ids_np.size))


def _run(c, mode):
    """One apply call on fresh copies of the tables and slots; returns every tensor it wrote."""
    from keras_rs_amd.embedding_ops import FusedBags

    dev, dim = c["dev"], c["dim"]
    tables = [t.clone() for t in c["tables"]]
    if mode in ("adam", "adam_dyn"):
        slots = [torch.zeros((2, v, dim), device=dev) for v in VOCABS]
    elif mode == "ftrl":
        slots = [torch.zeros((2, v, dim), device=dev) for v in VOCABS]
        for s in slots:
            s[0].fill_(0.1)
    elif mode == "adagrad_rowwise":
        slots = [torch.full((v,), 0.1, device=dev) for v in VOCABS]
    else:
        slots = [torch.full((v, dim), 0.1, device=dev) for v in VOCABS]
    fb = FusedBags(tables, c["specs"], slots=slots, lrs=LRS)
    ws = fb.plan_backward(c["ids"], BATCH, hots=c["hots"])      # global sort: one trailing run of invalid keys
    kw = dict(hots=c["hots"], weights=c["w"], bag_scale=c["scale"])
    if mode == "dense":
        out = fb.backward_dense(ws, c["grad"], BATCH, c["nnz"], **kw)
    elif mode == "sparse":
        out = list(fb.backward_sparse(ws, c["grad"], BATCH, c["nnz"], **kw))
    else:
        hyper = None
        if mode == "adam":
            hyper = ADAM + (0.3,)
        elif mode == "adam_dyn":
            hyper = ADAM + (torch.full((1,), 0.3, device=dev),)
        elif mode == "ftrl":
            hyper = FTRL
        fb.backward_fused("adam" if mode == "adam_dyn" else mode, ws, c["grad"], BATCH, c["nnz"], hyper=hyper, **kw)
        out = tables + slots
    torch.cuda.synchronize()
    return out


def _close(got, exp, rtol, atol):
    bad = np.abs(got - exp) > atol + rtol * np.abs(exp)
    assert not bad.any(), f"{int(bad.sum())} elements off, worst {np.abs(got - exp).max():.3e}"


@pytest.mark.parametrize("use_w,use_scale", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("tdt,gdt,dim", [("bf16", "bf16", 128), ("f32", "f32", 64)])
def test_every_depth_gives_the_bits_of_depth_0_and_depth_0_matches_the_oracle(tdt, gdt, dim, use_w, use_scale):
    from keras_rs_amd import embedding_ops as eo

    c = _case(tdt, gdt, dim, use_w, use_scale)
    res = {}
    try:
        for depth in (0,) + DEPTHS:
            eo.set_apply_depth(depth)
            res[depth] = {m: _run(c, m) for m in MODES}
    finally:
        eo.set_apply_depth(eo.APPLY_DEPTH_DEFAULT)
    for m in MODES:
        if m not in ("dense", "sparse"):
            assert any(not torch.equal(a, b) for a, b in zip(res[0][m][:2], c["tables"])), f"{m}: the update did not run"
        for depth in DEPTHS:
            assert len(res[depth][m]) == len(res[0][m])
            for k, (a, b) in enumerate(zip(res[0][m], res[depth][m])):
                assert torch.equal(a, b), f"{m}, depth {depth}, output {k}: not the bits of depth 0"
    # adam and adam_dyn differ only in where the bias-correction factor comes from
    for a, b in zip(res[0]["adam"], res[0]["adam_dyn"]):
        assert torch.equal(a, b)

    # ---- depth 0 against the oracle ----
    rows, vals = res[0]["sparse"]
    n_valid = [int((cnt > 0).sum()) for cnt in c["counts"]]
    assert rows.numel() == sum(n_valid) and bool((rows[1:] > rows[:-1]).all())
    dense_all = np.concatenate(c["de"], 0)
    for t, v in enumerate(VOCABS):
        cnt = c["counts"][t][:, None]
        rtol = np.where(cnt > 128, LONG_RTOL, 1e-6)
        exp = c["de"][t]
        _close(res[0]["dense"][t].cpu().numpy(), exp, rtol, 1e-6)
        # SGD: w - lr g
        got_w = to_f32(to_np(res[0]["sgd"][t]))
        exp_w = to_np(c["tables"][t]).copy()
        touched = (c["counts"][t] > 0).astype(np.uint8)
        ko.apply_optimizer(exp_w, np.zeros((v, dim), np.float32), exp, touched, LRS[t], "sgd")
        row_rtol = 2.0 ** -7 if tdt == "bf16" else 1e-6
        _close(got_w, to_f32(exp_w), row_rtol, 1e-6 + LRS[t] * rtol * np.abs(exp))
        assert np.array_equal(got_w[touched == 0], to_f32(to_np(c["tables"][t]))[touched == 0])
        # Adagrad: acc += g^2, w -= lr g / sqrt(acc)
        exp_w = to_np(c["tables"][t]).copy()
        exp_a = np.full((v, dim), 0.1, np.float32)
        ko.apply_optimizer(exp_w, exp_a, exp, touched, LRS[t], "adagrad")
        _close(res[0]["adagrad"][2 + t].cpu().numpy(), exp_a, 1e-6 + 2 * rtol, 1e-6)
        _close(to_f32(to_np(res[0]["adagrad"][t])), to_f32(exp_w), row_rtol, 1e-6 + LRS[t] * 2 * rtol)
    _close(vals.cpu().numpy(), dense_all[rows.cpu().numpy()],
           np.where(np.concatenate(c["counts"])[rows.cpu().numpy()][:, None] > 128, LONG_RTOL, 1e-6), 1e-6)


def test_apply_depth_option_refuses_other_values():
    from keras_rs_amd import _lib as L
    from keras_rs_amd import embedding_ops as eo

    try:
        for bad in (-1, 1, 2, 3, 12, 32):
            assert L.lib().krs_embed_set_option(eo.KRS_EMBED_OPT_APPLY_DEPTH, bad) != 0
            with pytest.raises(L.KrsError):
                eo.set_apply_depth(bad)
        for good in (0, 4, 8, 16):
            eo.set_apply_depth(good)
    finally:
        eo.set_apply_depth(eo.APPLY_DEPTH_DEFAULT)
