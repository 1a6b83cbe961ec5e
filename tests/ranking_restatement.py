"""float64 restatement of the five keras_rs.losses ranking losses (written from their formulas, used by the K9
tests): unreduced losses, Keras 3 reductions, and per-element magnitudes for the fp32 error bounds."""

import torch

EPS_LISTMLE = 1e-10
U32 = 2.0 ** -24          # fp32 unit roundoff


def _valid(y, mask):
    v = y >= 0
    return v if mask is None else v & mask.bool()


def pairwise(kind, s, y, mask=None, temperature=1.0):
    """[B, L] per-item losses: sum_j w_ij phi(x_ij) (autodiff-able in s)."""
    valid = _valid(y, mask)
    vp = valid[:, :, None] & valid[:, None, :]
    if kind == "mse":
        eye = torch.eye(s.shape[1], dtype=torch.bool, device=s.device)
        d = (y[:, :, None] - y[:, None, :]) - (s[:, :, None] - s[:, None, :])
        return (d * d * (vp & ~eye)).sum(-1)
    x = (s[:, :, None] - s[:, None, :]) / temperature
    w = (y[:, :, None] > y[:, None, :]) & vp
    if kind == "hinge":
        phi = torch.relu(1.0 - x)
    elif kind == "logistic":
        phi = torch.relu(-x) + torch.log(1.0 + torch.exp(-torch.abs(x)))
    else:
        phi = torch.where(x > 0, 1.0 - torch.sigmoid(x), torch.sigmoid(-x))
    return (phi * w).sum(-1)


def listmle(s, y, mask=None, temperature=1.0):
    """[B] per-list losses in the order label descending, index ascending (autodiff-able in s)."""
    valid = _valid(y, mask)
    has = valid.sum(1, keepdim=True) > 0
    lab = torch.where(valid, y, torch.full_like(y, -1e9))
    order = torch.sort(lab, dim=1, descending=True, stable=True).indices
    sl = torch.gather(torch.where(valid, s, torch.full_like(s, -1e9)), 1, order) / temperature
    sv = torch.gather(valid, 1, order)
    mx = torch.where(sv, sl, torch.full_like(sl, -1e9)).amax(1, keepdim=True)
    mx = torch.where(has, mx, torch.zeros_like(mx))
    sl = torch.where(sv, sl - mx, torch.full_like(sl, -1e9))
    cs = torch.flip(torch.cumsum(torch.flip(torch.exp(sl), [1]), 1), [1])
    lp = torch.where(sv, sl - torch.log(cs + EPS_LISTMLE), torch.zeros_like(sl))
    return torch.where(has[:, 0], -lp.sum(1), torch.zeros_like(lp[:, 0]))


def unreduced(kind, s, y, mask=None, temperature=1.0):
    if kind == "listmle":
        return listmle(s, y, mask, temperature)
    return pairwise(kind, s, y, mask, 1.0 if kind == "mse" else temperature)


def reduce(v, w, reduction):
    """Keras 3 Loss reduction of the unreduced v with sample weight w (None, or broadcastable to v)."""
    vw = v if w is None else v * w
    if reduction in (None, "none"):
        return vw
    total = vw.sum()
    if reduction == "sum":
        return total
    if reduction == "mean_with_sample_weight" and w is not None:
        div = torch.broadcast_to(w, v.shape).sum()
    else:
        div = torch.tensor(float(v.numel()), dtype=v.dtype, device=v.device)
    return torch.where(div != 0, total / torch.where(div != 0, div, torch.ones_like(div)), torch.zeros_like(total))


def magnitudes(kind, s, y, mask=None, temperature=1.0, g=None):
    """(loss magnitude, gradient magnitude): for each output element the float64 sum of the absolute values of the
    terms fp32 adds up to form it, each term counted with its argument's size (so a rounding of x = (s_i - s_j) / T
    is covered).  g: the per-item (pairwise) / per-list (ListMLE) weight of the gradient, default 1."""
    s = s.detach().double()
    if kind == "listmle":
        valid = _valid(y, mask)
        t = temperature
        lab = torch.where(valid, y, torch.full_like(y, -1e9))
        order = torch.sort(lab, dim=1, descending=True, stable=True).indices
        sl = torch.gather(s, 1, order) / t
        sv = torch.gather(valid, 1, order)
        mx = torch.where(sv, sl, torch.full_like(sl, -1e300)).amax(1, keepdim=True)
        z = torch.where(sv, sl - mx, torch.full_like(sl, -1e300))
        e = torch.exp(z)
        cs = torch.flip(torch.cumsum(torch.flip(e, [1]), 1), [1])
        terms = torch.where(sv, torch.abs(torch.log(cs + EPS_LISTMLE)) + torch.abs(z) + 1.0, torch.zeros_like(z))
        inv = torch.where(sv, 1.0 / (cs + EPS_LISTMLE), torch.zeros_like(z))
        q = torch.cumsum(inv, 1)
        gs = torch.where(sv, e * q + 1.0 + (torch.abs(sl) + torch.abs(mx)) * 1.0, torch.zeros_like(z))
        gm = torch.zeros_like(s).scatter(1, order, gs) / t
        gl = torch.ones(s.shape[0], dtype=s.dtype, device=s.device) if g is None else torch.broadcast_to(g, (s.shape[0],))
        return terms.sum(1), gm * gl[:, None].abs()
    valid = _valid(y, mask)
    vp = valid[:, :, None] & valid[:, None, :]
    gi = torch.ones_like(s) if g is None else torch.broadcast_to(g, s.shape).double()
    if kind == "mse":
        d = ((y[:, :, None] - y[:, None, :]).abs() + (s[:, :, None] - s[:, None, :]).abs()
             + y.abs()[:, :, None] + y.abs()[:, None, :] + s.abs()[:, :, None] + s.abs()[:, None, :])
        lm = (d * d * vp).sum(-1)
        gm = 2 * (d * vp * (gi.abs()[:, :, None] + gi.abs()[:, None, :])).sum(-1)
        return lm, gm
    t = temperature
    x = (s[:, :, None] - s[:, None, :]) / t
    ax = x.abs() + (s.abs()[:, :, None] + s.abs()[:, None, :]) / t
    w = ((y[:, :, None] > y[:, None, :]) & vp).double()
    lm = ((1.0 + ax) * w).sum(-1)                 # |phi| <= 1 + |x| for all three; |phi'| <= 1
    gm = ((gi.abs()[:, :, None] * w + gi.abs()[:, None, :] * w.transpose(1, 2)) * (1.0 + ax)).sum(-1) / t
    return lm, gm
