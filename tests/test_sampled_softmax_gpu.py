"""K30 (krs_sampled_softmax_fwd_bwd through sampled_ops and layers.SampledSoftmaxCrossentropy) against a float64 torch
restatement of include/krs.h's formulas.  On the fast route the restatement is fed the bf16-rounded table rows.

Tolerances.  fp32 route: 1e-5 absolute plus 1e-5 relative on everything.  Fast route: lse, loss and gpos at the same 1e-5
(logits are kept within |x| <= 8); demb and dneg inside K19's per-element bound from the reference, C = 1.76:
  demb  C 2^-8 c_t sum_j p_tj |r_jc| (j from 0: the positive's row is a bf16 row too) + half a bf16 ulp of the value;
  dneg  C 2^-8 sum_t c_t p_tj |e_tc|.
The table gradient adds dneg over the negative lookups and gpos e over the positive ones in fp32 (K2): the dneg bounds
summed over a row's lookups plus the fp32 tolerance.  The worst observed fraction of a bound is printed (run with -s);
DESIGN.md (K30) records it."""

import math

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers as kl
from keras_rs_amd import sampled_ops as S
from keras_rs_amd.layers.losses import sampled_softmax_crossentropy_stored

pytestmark = pytest.mark.gpu
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
V, C = 211, 1.76
NAMES = ("loss", "lse", "gpos", "demb", "dneg")


def make(d, edt, tdt, lg, n, g, idt, weights, logq, hits, seed=0):
    """emb [T, d], table [V, d], pos [T], neg [G, N], w, pos_logq, neg_logq on the host.  hits: planted accidental hits,
    among them token 0 whose every negative is its positive; negatives repeat inside a group (n > V / 4 at the least,
    and neg[:, -1] = neg[:, 0])."""
    gen = torch.Generator().manual_seed(seed + 7 * d + 13 * lg + 17 * n + g)
    t = g * lg
    table = torch.randn(V, d, generator=gen).to(tdt)
    emb = (torch.randn(t, d, generator=gen) * 1.5 / math.sqrt(d)).to(edt)
    pos = torch.randint(0, V, (t,), generator=gen)
    neg = torch.randint(0, V, (g, n), generator=gen)
    neg[:, -1] = neg[:, 0]
    if hits:
        pos[::4] = neg[torch.arange(0, t, 4) // lg, (torch.arange(0, t, 4) * 5) % n]
        neg[0, :] = pos[0]
    w = pq = nq = None
    if weights:
        w = (torch.rand(t, generator=gen) > 0.3).float() * (0.5 + torch.rand(t, generator=gen))
        w[t // 2] = 0.0
    if logq:
        pq, nq = -torch.rand(t, generator=gen), -torch.rand(g, n, generator=gen)
    return emb, table, pos.to(idt), neg.to(idt), w, pq, nq


def half_ulp(x):
    """half a bf16 ulp at x: 8 significant bits"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 8)


def reference(emb, table, pos, neg, w, pq, nq, remove, fast):
    """float64 values of include/krs.h (K30) and, on the fast route, the bounds of the docstring."""
    (t, d), (g, n), v = emb.shape, neg.shape, table.shape[0]
    grp = torch.arange(t) // (t // g)
    pos, neg = pos.long(), neg.long()
    wv = torch.ones(t, dtype=torch.float64) if w is None else w.double()
    s = wv.sum()
    pos_ok, neg_ok = (pos >= 0) & (pos < v), (neg >= 0) & (neg < v)
    live = (wv != 0) & bool(s != 0) & pos_ok
    tab = (table.bfloat16() if fast else table).double()
    e = torch.where(live[:, None], emb.double(), 0.0)                       # (a dead token requests no row)
    r0 = torch.where(live[:, None], tab[pos.clamp(0, v - 1)], 0.0)
    rn = torch.where(neg_ok[..., None], tab[neg.clamp(0, v - 1)], 0.0)[grp]     # [T, N, d]
    x0 = (e * r0).sum(-1) - (0 if pq is None else pq.double())
    xn = torch.einsum("td,tnd->tn", e, rn) - (0 if nq is None else nq.double()[grp])
    keep = neg_ok[grp] & ~(remove & (neg[grp] == pos[:, None]))
    xn = torch.where(keep, xn, -math.inf)
    lse = torch.logsumexp(torch.cat([x0[:, None], xn], 1), 1)
    c = torch.where(live, wv / (s if s != 0 else 1.0), 0.0)
    p0, cp = torch.exp(x0 - lse), c[:, None] * torch.exp(xn - lse[:, None])
    out = dict(loss=(c * (lse - x0)).sum(), lse=torch.where(live, lse, 0.0), gpos=c * (p0 - 1))
    out["demb"] = out["gpos"][:, None] * r0 + torch.einsum("tn,tnd->td", cp, rn)
    out["dneg"] = torch.einsum("gtn,gtd->gnd", cp.reshape(g, -1, n), e.reshape(g, -1, d))
    bound = {k: 1e-5 + 1e-5 * x.abs() for k, x in out.items()}
    if emb.dtype == BF16:                 # (demb is stored in emb's dtype: half a bf16 ulp on either route)
        bound["demb"] = bound["demb"] + half_ulp(out["demb"])
    if fast:
        absum = (c * p0)[:, None] * r0.abs() + torch.einsum("tn,tnd->td", cp, rn.abs())
        bound["demb"] = C * 2.0 ** -8 * absum + half_ulp(out["demb"])
        bound["dneg"] = C * 2.0 ** -8 * torch.einsum("gtn,gtd->gnd", cp.reshape(g, -1, n), e.abs().reshape(g, -1, d))
    flat = neg.clamp(0, v - 1).reshape(-1)
    add = lambda rows_p, rows_n: torch.zeros(v, d, dtype=torch.float64).index_add_(0, pos.clamp(0, v - 1), rows_p) \
        .index_add_(0, flat, rows_n.reshape(-1, d))                                               # noqa: E731
    out["dtable"] = add(out["gpos"][:, None] * e, out["dneg"])
    bound["dtable"] = 1e-5 + 1e-5 * add((out["gpos"][:, None] * e).abs(), out["dneg"].abs()) + \
        (add(torch.zeros(t, d, dtype=torch.float64), bound["dneg"]) if fast else 0.0)
    return out, bound


def fraction(got, want, bound, what):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got.double().cpu() - want).abs()
    frac = float((err / bound.clamp_min(1e-300)).max()) if err.numel() and float(err.max()) > 0 else 0.0
    print(f"{what}: largest error / bound = {frac:.3f}")
    assert bool((err <= bound).all()), f"{what}: error {float(err.max()):.3e} is {frac:.2f} x its bound"


def run(case, dev="cuda", **kw):
    emb, table, pos, neg, w, pq, nq = (None if x is None else x.to(dev) for x in case)
    return S.sampled_softmax(emb, table, pos, neg, w, pq, nq, **kw)


FAST, GEN = L.SSM_FAST, L.SSM_GENERIC
# route, dpad, vec, splits | d, emb dtype, table dtype, Lg, N, G, id dtype, weights, logq, hits
CASES = [
    (FAST, 32, 1, 1, 8, BF16, BF16, 1, 1, 1, I32, 0, 0, 0),
    (FAST, 32, 1, 1, 8, BF16, F32, 31, 33, 3, I64, 1, 1, 1),
    (FAST, 32, 1, 5, 8, BF16, BF16, 129, 100, 1, I32, 1, 0, 1),
    (FAST, 64, 0, 1, 50, BF16, BF16, 31, 31, 3, I32, 1, 1, 1),
    (FAST, 64, 0, 2, 50, BF16, F32, 33, 100, 1, I64, 0, 0, 1),
    (FAST, 64, 0, 5, 50, BF16, F32, 129, 33, 3, I32, 1, 1, 0),
    (FAST, 64, 0, 1, 50, BF16, BF16, 1, 100, 3, I32, 0, 1, 1),
    (FAST, 64, 1, 2, 64, BF16, BF16, 33, 1, 1, I32, 1, 0, 1),
    (FAST, 64, 1, 1, 64, BF16, F32, 31, 100, 3, I32, 1, 1, 1),
    (FAST, 64, 1, 5, 64, BF16, BF16, 129, 31, 3, I64, 0, 1, 1),
    (FAST, 64, 1, 5, 64, BF16, F32, 129, 130, 1, I32, 1, 0, 1),       # two owner blocks of negatives
    (FAST, 64, 1, 1, 64, BF16, F32, 1, 33, 1, I32, 0, 0, 0),
    (FAST, 128, 1, 1, 128, BF16, BF16, 31, 33, 1, I32, 1, 1, 1),
    (FAST, 128, 1, 2, 128, BF16, F32, 33, 31, 3, I32, 0, 0, 1),
    (FAST, 128, 1, 5, 128, BF16, F32, 129, 100, 3, I32, 1, 1, 1),
    (FAST, 128, 1, 1, 128, BF16, BF16, 1, 1, 3, I64, 1, 0, 0),
    (FAST, 128, 0, 5, 100, BF16, F32, 129, 33, 1, I32, 1, 1, 1),      # d = 100: element loads at DPAD 128
    (GEN, 0, 0, 1, 50, F32, F32, 31, 33, 3, I32, 1, 1, 1),
    (GEN, 0, 0, 1, 50, F32, BF16, 129, 100, 1, I64, 0, 0, 1),
    (GEN, 0, 0, 1, 50, F32, F32, 1, 31, 3, I32, 1, 0, 1),
    (GEN, 0, 0, 1, 200, F32, F32, 33, 1, 1, I32, 1, 1, 0),
    (GEN, 0, 0, 1, 200, F32, BF16, 31, 100, 3, I32, 0, 1, 1),
    (GEN, 0, 0, 1, 200, BF16, BF16, 129, 33, 3, I32, 1, 0, 1),
    (GEN, 0, 0, 1, 200, BF16, F32, 33, 31, 1, I64, 1, 1, 1),
    (GEN, 0, 0, 1, 200, BF16, BF16, 1, 1, 1, I32, 0, 0, 0),
]


@pytest.mark.parametrize("route,dpad,vec,splits,d,edt,tdt,lg,n,g,idt,weights,logq,hits", CASES)
def test_kernel_against_float64(route, dpad, vec, splits, d, edt, tdt, lg, n, g, idt, weights, logq, hits):
    case = make(d, edt, tdt, lg, n, g, idt, weights, logq, hits)
    t = g * lg
    # poisoned outputs and workspace come back fully written
    nan = lambda shape, dt: torch.full(shape, math.nan, dtype=dt, device="cuda")                   # noqa: E731
    out = (nan((), F32), nan((t,), F32), nan((t,), F32), nan((t, d), edt), nan((g, n, d), F32))
    ws = torch.full((max(1, S.softmax_workspace_bytes(t, g, n, d, edt)),), 0xFF, dtype=torch.uint8, device="cuda")
    got = run(case, out=out, workspace=ws)
    r = S.softmax_last_route()
    assert (r.kernel, r.dpad, r.vec, r.splits) == (route, dpad, vec, splits)
    again = run(case)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two calls differ in their bits"
    want, bound = reference(*case, True, route == FAST)
    for name, x in zip(NAMES, got):
        fraction(x, want[name], bound[name], name)
    if hits:                              # token 0: every negative is its positive
        assert float(got[2][0]) == 0.0 and not got[3][0].any()


@pytest.mark.parametrize("d,edt", [(64, BF16), (50, F32)])
def test_contract_dead_tokens_zero_sum_bad_ids_and_no_hit_removal(d, edt):
    emb, table, pos, neg, w, pq, nq = make(d, edt, F32, 33, 40, 3, I32, 1, 1, 1)
    fast = edt == BF16
    # NaN under a zero weight: the token's embedding and its positive's row (an id nothing else uses)
    dead = int((w == 0).nonzero()[0])
    pos[dead] = V - 1
    neg[neg == V - 1] = 0
    pos[(pos == V - 1) & (torch.arange(99) != dead)] = 1
    emb[dead], table[V - 1] = math.nan, math.nan
    case = (emb, table, pos, neg, w, pq, nq)
    for remove in (True, False):
        got = run(case, remove_hits=remove)
        want, bound = reference(*case, remove, fast)
        for name, x in zip(NAMES, got):
            fraction(x, want[name], bound[name], f"remove_hits={remove} {name}")
        assert float(got[1][dead]) == 0.0 and float(got[2][dead]) == 0.0 and not got[3][dead].any()
    # S = 0: loss 0 and all zeros
    zero = run((emb, table, pos, neg, torch.zeros_like(w), pq, nq))
    assert all(not x.any() for x in zero)
    # an out-of-range negative and positive set the flag, take no part, and change nothing else
    neg[1, 3], pos[5] = V, -1
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = run((emb, table, pos, neg, w, pq, nq), err_flag=flag)
    assert int(flag.item()) & L.FLAG_ID_OUT_OF_RANGE
    want, bound = reference(emb, table, pos, neg, w, pq, nq, True, fast)
    for name, x in zip(NAMES, got):
        fraction(x, want[name], bound[name], f"out of range {name}")
    assert not got[4][1, 3].any() and not got[3][5].any()


def test_fast_route_against_the_generic_route_on_one_case():
    case = make(64, BF16, BF16, 129, 100, 3, I32, 1, 1, 1)
    fast = run(case)
    assert S.softmax_last_route().kernel == FAST
    generic = run(tuple(x.float() if i == 0 else x for i, x in enumerate(case)))       # (fp32 emb: the same values)
    assert S.softmax_last_route().kernel == GEN
    _, bound = reference(*case, True, True)
    for name, a, b in zip(NAMES, fast, generic):
        fraction(a.float(), b.double().cpu(), bound[name], f"fast vs generic {name}")


@pytest.mark.parametrize("dtype,shared", [(F32, False), (BF16, False), (BF16, True)])
def test_layer_matches_float64_through_autograd(dtype, shared):
    b, length, d, n, up = 3, 33, 64, 40, 1.75
    g = 1 if shared else b
    emb_h, table_h, pos_h, neg_h, w_h, pq_h, nq_h = make(d, dtype, F32, b * length // g, n, g, I32, 1, 1, 1)
    neg_h[:, 1] = pos_h[7]                                  # an id the positives and the negatives share
    layer = kl.Embedding(V, d, device="cuda", dtype="mixed_bfloat16" if dtype == BF16 else "float32")
    layer.build()
    with torch.no_grad():
        layer.embeddings.copy_(table_h)
    emb = emb_h.cuda().reshape(b, length, d).requires_grad_()
    shape = lambda x: x.cuda().reshape(b, length)                                                # noqa: E731
    negs = (neg_h[0], nq_h[0]) if shared else (neg_h, nq_h)
    loss = kl.SampledSoftmaxCrossentropy()(layer, emb, shape(pos_h), negs[0].cuda(), shape(w_h), shape(pq_h), negs[1].cuda())
    (loss * up).backward(retain_graph=True)
    want, bound = reference(emb_h, table_h, pos_h, neg_h, w_h, pq_h, nq_h, True, dtype == BF16)
    fraction(loss.detach(), want["loss"], bound["loss"], "layer loss")
    # (the backward scales demb by the upstream scalar in emb's dtype: half an ulp of the scaled value more under bf16)
    fraction(emb.grad.reshape(-1, d).double() / up, want["demb"], bound["demb"] + half_ulp(want["demb"] * up) / up, "layer demb")
    fraction(layer.embeddings.grad.double() / up, want["dtable"], bound["dtable"], "layer dtable")
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    stored = sampled_softmax_crossentropy_stored(layer, emb.detach(), shape(pos_h), negs[0].cuda(), shape(w_h), shape(pq_h),
                                                 negs[1].cuda())
    assert abs(float(stored.detach()) - float(want["loss"])) <= (2e-2 if dtype == BF16 else 1e-5) * (1 + abs(float(want["loss"])))


def test_layer_refusals(monkeypatch):
    layer = kl.Embedding(V, 16, device="cuda")
    emb, pos = torch.zeros(2, 5, 16, device="cuda"), torch.zeros(2, 5, dtype=torch.int32, device="cuda")
    loss = kl.SampledSoftmaxCrossentropy()
    with pytest.raises(ValueError, match="at most 4096"):
        loss(layer, emb, pos, torch.zeros(4097, dtype=torch.int32, device="cuda"))
    with pytest.raises(IndexError, match="out of range"):
        loss(layer, emb, pos, torch.full((2, 3), V, dtype=torch.int32, device="cuda"))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)       # (the guard only: no capture)
    with pytest.raises(L.KrsError, match="cannot be captured"):
        loss(layer, emb, pos, torch.zeros(3, dtype=torch.int32, device="cuda"))


def test_peak_memory_stays_far_below_the_logits():
    g, lg, n, d = 8, 1024, 2048, 64
    gen = torch.Generator().manual_seed(5)
    layer = kl.Embedding(5000, d, device="cuda", dtype="mixed_bfloat16")
    emb = (torch.randn(g, lg, d, generator=gen) * 0.2).bfloat16().cuda().requires_grad_()
    pos = torch.randint(0, 5000, (g, lg), generator=gen, dtype=torch.int32).cuda()
    neg = torch.randint(0, 5000, (g, n), generator=gen, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    kl.SampledSoftmaxCrossentropy()(layer, emb, pos, neg).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs: {peak / 2 ** 20:.1f} MiB (one fp32 [T, N] tensor: {g * lg * n * 4 / 2 ** 20:.0f} MiB)")
    assert peak < g * lg * n * 4 // 2
