"""K29 (krs_sampled_bce_fwd_bwd through sampled_ops and layers.SampledItemCrossentropy) against a float64 torch-CPU
restatement: gathers, dot, keras' BCE-with-logits form, autograd for d emb and d table.

Tolerances, from the order include/krs.h (K29) states, with u = 2^-24 and A_tj = sum_i |e_ti r_ji|:
  logit   one rounded product, at most 8 adds in the lane, log2 g in the butterfly (2 more for slack the issue grants):
          |dx_tj| <= (8 + log2 g + 2) u A_tj.
  element max(x, 0) - x y is exact (y is 0 or 1); expf is within 1 ulp (2u), log1pf within 2 ulp (4u) and
          u / (1 + u) <= log1p(u) carries expf's error over relatively, one more add: 8u l.  The element is 1-Lipschitz
          in x:  |dl_tj| <= |dx_tj| + 8u l_tj.
  loss    the longest chain of adds is N (items) + ceil(T / (tokens a sweep)) (a group's tokens) + 8 (the tree) + G
          (workgroups); one product by w_t; W = (1 + N) S carries S's chain of 1 + 10 + 1 adds and one product; one
          division:  |dloss| <= sum_t w_t sum_j |dl_tj| / W + (N + chain + 16) u loss   (weights are >= 0 here).
  glog    sigma is 1/4-Lipschitz; u, s = 1 + u and one division give sigma within 6u sigma, the subtraction of y one more
          u:  |dg| <= |dx| / 4 + 7u;  w g / W adds a product, W's 14u and a division:
          |dglog_tj| <= (w_t / W) (|dx_tj| / 4 + 7u) + 16u |glog_tj|.
  demb    1 + N products and adds, then ONE rounding to emb's dtype (bf16 keeps 8 significant bits: 2^-8 relative; none for fp32):
          |ddemb_tc| <= sum_j |r_jc| |dglog_tj| + (N + 3) u sum_j |glog_tj r_jc| + rho |demb_tc|.
  dtable  K2 adds a row's k lookups in fp32, each a rounded product of the scaled glog and e, and the result is rounded
          to the table's dtype; the upstream scalar is one more rounded product on glog:
          |ddtable_vc| <= up sum |e_tc| |dglog_tj| + (k + 4) u up sum |glog_tj e_tc| + rho |dtable_vc|.
The largest observed fraction of each bound is printed (run with -s) and recorded in DESIGN.md (K29)."""

import math

import pytest
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import layers as kl
from keras_rs_amd import sampled_ops as S
from keras_rs_amd.embedding_ops import FusedBags
from keras_rs_amd.layers.losses import sampled_item_crossentropy_stored

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
V = 97          # a small table: ids repeat within and across tokens


def make(t, d, n, edt, tdt, idt, flavour, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * t + 10 * d + n)
    table = torch.randn(V, d, generator=g).to(tdt)
    ids = torch.randint(0, V, (t, 1 + n), generator=g).to(idt)
    if n:
        ids[::3, -1] = ids[::3, 0]                       # a negative that repeats the positive
    emb = torch.randn(t, 2 * d if flavour == "strided" else d, generator=g)        # logits of unit scale times sqrt(d)..
    if flavour == "saturated":       # .. or +-30 at the positive: the positive's own row, scaled, under a random sign
        rows = table[ids[:, 0].long()].float()
        emb = rows * 30.0 / rows.square().sum(1, keepdim=True) * (torch.randint(0, 2, (t, 1), generator=g) * 2 - 1)
    else:
        emb = emb / math.sqrt(d)
    emb = emb.to(edt)
    w = None
    if flavour in ("padded", "strided", "saturated"):
        w = (torch.rand(t, generator=g) > 1 / 3).float() * (1 + torch.rand(t, generator=g))
        w[: t // 5] = 0.0                                 # fully padded leading rows
    elif flavour == "all_zero":
        w = torch.zeros(t)
    return emb, table, ids, w


def reference(emb, table, ids, w, up, g_lanes):
    """float64 values and the bounds of the docstring; emb [T, d] and table as stored (exact in float64)."""
    t, d = emb.shape
    n = ids.shape[1] - 1
    e = emb.double().requires_grad_()
    tb = table.double().requires_grad_()
    wv = torch.ones(t, dtype=torch.float64) if w is None else w.double()
    valid = ((ids >= 0) & (ids < table.shape[0])).double()
    rows = tb[ids.long().clamp(0, table.shape[0] - 1)] * valid[..., None]
    x = (rows * e[:, None, :]).sum(-1)
    y = torch.zeros_like(x)
    y[:, 0] = 1.0
    el = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))) * valid
    W = (1 + n) * wv.sum()
    live = (wv != 0).double() * float(W != 0)
    Wd = W if W != 0 else 1.0
    loss = (wv[:, None] * el).sum() / Wd * float(W != 0)
    glog = (torch.sigmoid(x) - y) * valid * (wv * live / Wd)[:, None]
    de, dt = torch.autograd.grad(loss * up, (e, tb), allow_unused=True)
    de = torch.zeros_like(e) if de is None else de / up
    dt = torch.zeros_like(tb) if dt is None else dt
    with torch.no_grad():
        blocks = min(L.SBCE_MAX_BLOCKS, -(-t // (L.SBCE_THREADS // g_lanes)))
        chain = n + -(-t // (L.SBCE_THREADS // g_lanes * blocks)) + 8 + blocks
        dx = (8 + math.log2(g_lanes) + 2) * U * (rows.abs() * e.abs()[:, None, :]).sum(-1) * live[:, None]
        b_loss = (wv[:, None] * (dx + 8 * U * el)).sum() / Wd + (n + chain + 16) * U * loss.abs()
        b_glog = (wv * live / Wd)[:, None] * (dx / 4 + 7 * U) * valid + 16 * U * glog.abs()
        rho_e = 2.0 ** -8 if emb.dtype == BF16 else 0.0
        rho_t = 2.0 ** -8 if table.dtype == BF16 else 0.0
        b_demb = (rows.abs() * b_glog[..., None]).sum(1) + (n + 3) * U * (rows.abs() * glog.abs()[..., None]).sum(1) + \
            rho_e * de.abs()
        flat = ids.long().clamp(0, table.shape[0] - 1).reshape(-1)
        k = torch.zeros(table.shape[0], dtype=torch.float64).index_add_(0, flat, valid.reshape(-1))
        contrib = lambda gl: torch.zeros_like(tb).index_add_(                                     # noqa: E731
            0, flat, (gl[..., None] * e.abs()[:, None, :]).reshape(-1, d))
        b_dt = up * contrib(b_glog) + (k[:, None] + 4) * U * up * contrib(glog.abs()) + rho_t * dt.abs()
    return dict(loss=loss.detach(), glog=glog.detach(), demb=de, dtable=dt, b_loss=b_loss, b_glog=b_glog, b_demb=b_demb,
                b_dtable=b_dt)


def fraction(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    assert torch.isfinite(got).all(), f"{what}: not finite"
    frac = float((err / bound.clamp_min(1e-300)).max()) if err.numel() and float(err.max()) > 0 else 0.0
    print(f"{what}: largest error / bound = {frac:.3f}")
    assert bool((err <= bound).all()), f"{what}: error {float(err.max()):.3e} is {frac:.2f} x its bound"


# T, d, N, emb dtype, table dtype, id dtype, flavour
CASES = [
    (1, 64, 1, F32, F32, torch.int32, "plain"),
    (37, 50, 1, BF16, BF16, torch.int32, "padded"),
    (37, 64, 0, BF16, F32, torch.int64, "plain"),
    (300, 50, 3, F32, BF16, torch.int64, "padded"),
    (300, 64, 9, BF16, BF16, torch.int32, "padded"),
    (37, 72, 3, F32, F32, torch.int32, "strided"),
    (300, 72, 1, BF16, BF16, torch.int64, "saturated"),
    (37, 128, 9, BF16, F32, torch.int32, "padded"),
    (300, 136, 1, F32, F32, torch.int32, "plain"),
    (37, 512, 3, BF16, BF16, torch.int32, "saturated"),
    (300, 512, 1, F32, BF16, torch.int64, "strided"),
    (37, 64, 3, BF16, BF16, torch.int32, "all_zero"),
]


@pytest.mark.parametrize("t,d,n,edt,tdt,idt,flavour", CASES)
def test_kernel_and_autograd_against_float64(t, d, n, edt, tdt, idt, flavour):
    emb_h, table_h, ids_h, w_h = make(t, d, n, edt, tdt, idt, flavour)
    dev = torch.device("cuda")
    emb = emb_h.to(dev)[:, :d]                     # ("strided": a column view of a wider block)
    table, ids = table_h.to(dev), ids_h.to(dev)
    w = None if w_h is None else w_h.to(dev)
    pos, neg = ids[:, 0].contiguous(), ids[:, 1:].contiguous() if n else None
    up = 1.75

    loss, glog, demb = S.sampled_bce(emb, table, pos, neg, w)
    route, planned = S.last_route(), S.plan_route(emb, table, n, w is not None)
    assert [route.kernel, route.g, route.blocks, route.launches] == \
        [planned.kernel, planned.g, planned.blocks, planned.launches]
    assert (route.g, route.kernel) == (next(g for g in (8, 16, 32, 64) if 8 * g >= d), 1 if d % 8 == 0 else 2)
    again = S.sampled_bce(emb, table, pos, neg, w)
    assert all(torch.equal(a, b) for a, b in zip((loss, glog, demb), again)), "two calls differ in their bits"

    ref = reference(emb_h[:, :d], table_h, ids_h, w_h, up, route.g)
    for name, got in (("loss", loss), ("glog", glog), ("demb", demb)):
        fraction(got, ref[name], ref["b_" + name], name)

    e_leaf, t_leaf = emb.detach().clone().requires_grad_(), table.detach().clone().requires_grad_()
    bags = FusedBags([t_leaf], [(0, "sum", 0)])
    out = S.SampledItemBceFn.apply(bags, e_leaf, pos, neg, w, None, t_leaf)
    assert torch.equal(out, loss)
    (out * up).backward()
    assert torch.equal(e_leaf.grad, demb.clone().mul_(torch.tensor(up, device=dev)))
    fraction(t_leaf.grad, ref["dtable"], ref["b_dtable"], "dtable")


def test_out_of_range_id_raises_in_the_layer_and_contributes_nothing_in_the_ops():
    emb_h, table_h, ids_h, _ = make(37, 64, 3, F32, F32, torch.int32, "plain")
    ids_h[5, 2], ids_h[9, 0] = V, -1
    dev = torch.device("cuda")
    emb, table, ids = emb_h.to(dev), table_h.to(dev), ids_h.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    loss, glog, demb = S.sampled_bce(emb, table, ids[:, 0].contiguous(), ids[:, 1:].contiguous(), None, err_flag=flag)
    assert int(flag.item()) & L.FLAG_ID_OUT_OF_RANGE
    ref = reference(emb_h, table_h, ids_h, None, 1.0, 8)
    assert float(glog[5, 2]) == 0.0 and float(glog[9, 0]) == 0.0
    for name, got in (("loss", loss), ("glog", glog), ("demb", demb)):
        fraction(got, ref[name], ref["b_" + name], name)
    layer = kl.Embedding(V, 64, device=dev)
    with pytest.raises(IndexError, match="embedding id out of range"):
        kl.SampledItemCrossentropy()(layer, emb.reshape(1, 37, 64), ids[:, 0].reshape(1, 37), ids[:, 1:].reshape(1, 37, 3))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layer_equals_the_stored_composition_which_is_the_former_example_loss(dtype):
    b, length, d = 6, 25, 50
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    layer = kl.Embedding(V, d, device=dev, dtype="mixed_bfloat16" if dtype == BF16 else "float32")
    emb = (torch.randn(b, length, d, generator=g) * 0.3).to(dtype).to(dev).requires_grad_()
    pos = torch.randint(0, V, (b, length), generator=g, dtype=torch.int32).to(dev)
    neg = torch.randint(0, V, (b, length), generator=g, dtype=torch.int32).to(dev)
    mask = (torch.rand(b, length, generator=g) > 0.3).to(dev)

    fused = kl.SampledItemCrossentropy()(layer, emb, pos, neg, mask)
    fused.backward()
    got = (fused.detach(), emb.grad.clone(), layer.embeddings.grad.clone())
    emb.grad = layer.embeddings.grad = None
    stored = sampled_item_crossentropy_stored(layer, emb, pos, neg, mask)
    stored.backward()

    # the example's compute_loss as it stood before the layer, restated: the stored composition is that arithmetic
    e32, p32, n32 = emb.detach().float(), layer(pos).float(), layer(neg).float()
    logits = torch.cat([(p32 * e32).sum(-1), (n32 * e32).sum(-1)], dim=1)
    labels = torch.cat([torch.ones_like(logits[:, :length]), torch.zeros_like(logits[:, length:])], dim=1)
    weight = torch.cat([mask, mask], dim=1).float()
    total = weight.sum()
    former = (torch.nn.functional.binary_cross_entropy_with_logits(logits, labels, reduction="none") * weight).sum() / total
    assert torch.equal(former, stored.detach())

    ids_h = torch.stack([pos.cpu(), neg.cpu()], -1).reshape(-1, 2)
    ref = reference(emb.detach().cpu().reshape(-1, d), layer.embeddings.detach().cpu(), ids_h,
                    mask.cpu().float().reshape(-1), 1.0, 8)
    # (under mixed_bfloat16 the composition's lookups round every gathered row to bf16 and the fused loss reads the
    #  fp32 rows -- the deviation the layer's docstring states --, so only the all-fp32 policy is held to the bound)
    if dtype == F32:
        assert abs(float(got[0]) - float(stored.detach())) <= float(ref["b_loss"])
    fraction(got[0], ref["loss"], ref["b_loss"], "layer loss")
    fraction(got[1].reshape(-1, d), ref["demb"], ref["b_demb"], "layer demb")
    fraction(got[2], ref["dtable"], ref["b_dtable"], "layer dtable")

