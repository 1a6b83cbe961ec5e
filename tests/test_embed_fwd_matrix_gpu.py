"""krs_embed_bag_fwd (K1) on every kernel instantiation and route of keras_rs_amd/csrc/embed_bag_fwd.hip: the kernel each
case ran is asserted from krs_embed_bag_fwd_last_route, and its output is held to a float64 restatement of the operation
(tests/embed_fwd_restatement.py, plain numpy, no oracle/).

One table drives everything (tests/embed_fwd_cases.py; its coverage is checked without a GPU by
tests/test_embed_fwd_routes_host.py).  Every case runs through FusedBags.forward with want_scale=True and an error word,
into a buffer pre-filled with 7.0 that has lead, gap and tail columns around the feature slots.  Per case:

  * route: embed_fwd_last_route() equals the case's expected record;
  * pooled and generic kernels (and the slow loop of the gather kernels for a feature whose hot is not 1):
        |got - ref| <= 2 * (gamma(n + 2) * M / |den| + gamma(n + 1) * |ref|) + u_out * |ref|
    gamma(k) = k u / (1 - k u), u = 2^-24, M = sum |w T[id]|, n the bag's lookups, u_out = 2^-24 (fp32 output) or 2^-8
    (bf16 output, the project's constant); inputs are exact in the table dtype.  bag_scale within 2 gamma(n + 1)
    relative, exactly 1.0 for the sum combiner.  A bag whose divisor is exactly 0 (empty, or weights +0.5 / -0.5 under
    mean) gives exactly 0 and scale exactly 0.  tests/test_embed_fwd_routes_host.py checks on the CPU that the reference's
    own fp32 evaluation stays inside this bound for every case;
  * gather kernels, bags of one lookup: bit-exact -- the table's bits (equal types), table[ids].to(bfloat16) (fp32 ->
    bf16, with +-inf, subnormals, ties between two bf16 numbers; NaN compared as NaN), exact widening (bf16 -> fp32); a row
    for an invalid id is all zero bits; the scale is 1.0;
  * an out-of-range id (-1, vocab, and for int64 2^32 + 3 and -2^40) raises KRS_FLAG_ID_OUT_OF_RANGE, adds nothing to the
    sum and still counts in the denominator; the flag word equals the expected one exactly;
  * row 0 of every table is NaN and no valid id is 0, so a dropped mask of the stand-in row (invalid ids, padding slots
    of a partial window) makes an output NaN: the outputs must be finite;
  * the sentinel columns are untouched, bit for bit; a second run is bit-identical (K1 has no float atomics);
  * KRS_EMBED_OPT_HOTROWS 64 / 128: bit-identical to the run with the option off.
"""

import functools

import numpy as np
import pytest
import torch

from tests import embed_fwd_restatement as RS
from tests.embed_fwd_cases import CASES, R, inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
KRS_EMBED_OPT_HOTROWS = 3


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = next(k for k in CASES if k.name == name)
    h = inputs(name)
    return RS.restate(h["tables"], c.feats, c.batch, c.dim, h["ids"], hots=c.hots, offsets=h["offsets"], weights=h["weights"])


def _run(c, dev_in, hot_opt):
    """One krs_embed_bag_fwd of case c under KRS_EMBED_OPT_HOTROWS = hot_opt: (buffer, scale, flag word, route)."""
    from keras_rs_amd import _lib as L
    from keras_rs_amd import embedding_ops as E

    tables, ids, offsets, weights = dev_in
    fb = E.FusedBags(tables, [(t, comb, col) for (t, comb), col in zip(c.feats, c.out_cols)])
    buf = torch.full((c.batch, c.width), 7.0, dtype=TORCH_DT[c.odt], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(L.lib().krs_embed_set_option(KRS_EMBED_OPT_HOTROWS, hot_opt), "krs_embed_set_option")
    try:
        _, scale = fb.forward(ids, c.batch, hots=c.hots, offsets=offsets, weights=weights, out=buf[:, c.base_off:],
                              want_scale=True, err_flag=flag)
        route = E.embed_fwd_last_route()
    finally:
        L.lib().krs_embed_set_option(KRS_EMBED_OPT_HOTROWS, 0)
    torch.cuda.synchronize()
    return buf.cpu(), scale.cpu().reshape(c.n_feats, c.batch), int(flag.item()), route


def _gathered(c, h, f):
    """what a pure gather of feature f returns: the table rows converted to the output type, zeros for an invalid id"""
    tab = torch.from_numpy(h["tables"][c.feats[f][0]]).to(TORCH_DT[c.tdt])
    start = sum(c.hots[:f]) * c.batch            # the feature's base in the dense id buffer
    ids = torch.from_numpy(h["ids"][start:start + c.batch].astype(np.int64))
    ok = (ids >= 0) & (ids < tab.shape[0])
    rows = tab[torch.where(ok, ids, torch.zeros_like(ids))].to(TORCH_DT[c.odt])
    rows[~ok] = 0
    return rows


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_route_against_float64(case):
    c, h, ref = case, inputs(case.name), _reference(case.name)
    dev_in = ([torch.from_numpy(t).to(TORCH_DT[c.tdt]).to(DEV) for t in h["tables"]], torch.from_numpy(h["ids"]).to(DEV),
              None if h["offsets"] is None else torch.from_numpy(h["offsets"]).to(DEV),
              None if h["weights"] is None else torch.from_numpy(h["weights"]).to(DEV))
    buf, scale, flag, route = _run(c, dev_in, c.hot_opt)
    assert route == c.route
    assert flag == c.flag and ref["bad"] == bool(c.bad)

    # the sentinel columns: lead, gaps, tail and what lies before the base offset
    untouched = torch.ones(c.width, dtype=torch.bool)
    for col in c.out_cols:
        untouched[c.base_off + col:c.base_off + col + c.dim] = False
    seven = _bits(torch.full((1,), 7.0, dtype=buf.dtype))[0]
    assert bool((_bits(buf)[:, untouched] == seven).all()), "a sentinel column was written"

    gather = c.route["kernel"] in ("hot1", "hot1_rows")
    tol = RS.bound(ref, c.odt == "bf16")
    stol = RS.scale_bound(ref)
    for f, col in enumerate(c.out_cols):
        got = buf[:, c.base_off + col:c.base_off + col + c.dim]
        what = f"{c.name} feature {f}"
        if gather and c.hots[f] == 1:
            want = _gathered(c, h, f)
            nan = want.isnan()
            assert torch.equal(got.isnan(), nan), what
            assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), what
            assert bool((scale[f] == 1.0).all()), what
            continue
        assert bool(got.isfinite().all()), what + ": the stand-in row leaked (NaN) or the sum overflowed"
        g64 = got.double().numpy()
        zero = ref["den"][f] == 0
        assert (g64[zero] == 0).all() and (scale[f].numpy()[zero] == 0).all(), what
        err = np.abs(g64 - ref["out"][f])
        worst = float((err[~zero] / np.maximum(tol[f][~zero], 1e-300)).max()) if (~zero).any() else 0.0
        print(f"{what}: worst error / bound = {worst:.3f}")
        assert worst <= 1.0, what
        assert (np.abs(scale[f].double().numpy() - ref["scale"][f]) <= stol[f]).all(), what
        if c.feats[f][1] == RS.SUM:
            assert bool((scale[f] == 1.0).all()), what

    # a second run gives the same bits (no float atomics)
    buf2, scale2, flag2, route2 = _run(c, dev_in, c.hot_opt)
    assert route2 == c.route and flag2 == c.flag
    assert torch.equal(_bits(buf), _bits(buf2)) and torch.equal(_bits(scale), _bits(scale2))
    if c.hot_opt:      # ... and so does the run without the LDS copy of the hot rows
        buf0, scale0, flag0, route0 = _run(c, dev_in, 0)
        assert route0 == dict(c.route, hot_rows=0) and flag0 == c.flag
        assert torch.equal(_bits(buf), _bits(buf0)) and torch.equal(_bits(scale), _bits(scale0))


def test_the_layer_under_mixed_bfloat16_gathers_fp32_rows_into_bf16():
    """DistributedEmbedding under mixed_bfloat16 keeps fp32 tables and asks K1 for bf16: three one-hot features run
    embed_gather_hot1<float, bf16>, and the output is the table rows rounded to bf16."""
    import keras_rs_amd.layers as kl
    from keras_rs_amd import embedding_ops as E

    batch, dim = 70, 40
    rng = np.random.default_rng(40)
    vocabs = dict(a=300, b=37, c=150)
    feats = {k: kl.FeatureConfig(k, kl.TableConfig(f"t_{k}", v, dim, placement="default_device", optimizer="sgd",
                                                   combiner="sum"), (batch,), (batch, dim)) for k, v in vocabs.items()}
    layer = kl.DistributedEmbedding(feats, dtype="mixed_bfloat16")
    ids = {k: rng.integers(0, v, batch).astype(np.int32) for k, v in vocabs.items()}
    with torch.no_grad():
        out = layer({k: torch.from_numpy(v).to(DEV) for k, v in ids.items()})
    assert E.embed_fwd_last_route() == R("hot1", "f32", "bf16", 16, blocks=2)
    layer.check_ids(wait=True)
    tables = layer.get_embedding_tables()
    for k in vocabs:
        tab = tables[f"t_{k}"]
        assert tab.dtype == torch.float32 and out[k].dtype == torch.bfloat16 and tuple(out[k].shape) == (batch, dim)
        want = tab[torch.from_numpy(ids[k]).long().to(tab.device)].to(torch.bfloat16)
        assert bool(tab.abs().sum() > 0) and torch.equal(_bits(out[k].cpu()), _bits(want.cpu())), k
