"""Float64 restatement of K13 (csrc/retrieval_xent.hip), written from the formulas of include/krs.h: the in-batch
softmax cross-entropy computed from query [B, D] and candidates [N, D], its gradients by autograd, and the error
bounds the tests hold the kernels to.  Plain torch on whatever device the inputs are on.

Bounds, with u = 2^-24, kappa = 4 (N + 16) u, delta_i = max_j 4 (D + 16) u (sum_k |q_ik c_jk| + |bias_j|), p the
float64 softmax and P = g (p - y'):
    |loss_i - ref|  <= sum_j y'_ij (2 delta_i + kappa (|lse_i - s_ij| + 1))
    E_ij             = |g_i| p_ij (2 delta_i + kappa) + (2^-8 + kappa) |P_ij|
    |dq - ref|      <= E |c| + 2^-8 |ref|          |dc - ref| <= E^T |q| + 2^-8 |ref|
(2 delta: the score error moves s_ij and lse_i; kappa: the fp32 sums over N terms; 2^-8: P is rounded to bf16 before
the gradient products, and a bf16 output is rounded once more).  A computation that keeps P and the outputs in fp32
drops the two 2^-8 terms; one that keeps P in fp32 and rounds only the outputs to bf16 drops the first."""

import torch

from tests import retrieval_loss_restatement as R

U32 = R.U32


def scores(q, c, pos=None, bias=None, ids=None, hit_value=0.0):
    """(s [B, N], positives [B] int64) in the dtype of q: q c^T + bias + hit_value on the accidental hits."""
    b, n = q.shape[0], c.shape[0]
    pos = torch.arange(b, device=q.device) if pos is None else pos.to(torch.int64)
    s = q @ c.T
    if bias is not None:
        s = s + bias.to(s.dtype)[None, :]
    if ids is not None:
        ok = (pos >= 0) & (pos < n)
        id_pos = ids[pos.clamp(0, n - 1)]
        j = torch.arange(n, device=q.device)
        hit = (ids[None, :] == id_pos[:, None]) & (j[None, :] != pos[:, None]) & ok[:, None]
        s = s + hit.to(s.dtype) * hit_value
    return s, pos


def row_loss(q, c, pos=None, bias=None, ids=None, hit_value=0.0, ls=0.0):
    """The unreduced loss [B] (autodiff-able in q and c); a positive outside [0, N) has an all-zero label row here."""
    s, pos = scores(q, c, pos, bias, ids, hit_value)
    return R.row_loss(s, R.one_hot(pos, c.shape[0], s.dtype), ls)


def reference(q, c, pos=None, bias=None, ids=None, hit_value=0.0, ls=0.0, g=None, p_bf16=True, out_bf16=True):
    """float64 loss [B], lse [B], dq, dc (autograd of sum_i g_i loss_i) and the three bounds, as a dict."""
    q64 = q.detach().double().requires_grad_(True)
    c64 = c.detach().double().requires_grad_(True)
    b, d = q64.shape
    n = c64.shape[0]
    bias64 = None if bias is None else bias.detach().double()
    g64 = torch.ones(b, dtype=torch.float64, device=q.device) if g is None else g.detach().double()
    s, pos = scores(q64, c64, pos, bias64, ids, hit_value)
    yp = R.smooth(R.one_hot(pos, n, torch.float64), ls)
    loss = R.row_loss(s, R.one_hot(pos, n, torch.float64), ls)
    (loss * g64).sum().backward()
    s = s.detach()
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[:, None])
    big_p = g64[:, None] * (p - yp)
    kappa = 4 * (n + 16) * U32
    mag = q64.detach().abs() @ c64.detach().abs().T
    if bias64 is not None:
        mag = mag + bias64.abs()[None, :]
    delta = 4 * (d + 16) * U32 * mag.amax(-1)
    loss_tol = (yp * (2 * delta[:, None] + kappa * ((lse[:, None] - s).abs() + 1))).sum(-1)
    e = g64.abs()[:, None] * p * (2 * delta[:, None] + kappa) + ((2.0 ** -8 if p_bf16 else 0.0) + kappa) * big_p.abs()
    out = 2.0 ** -8 if out_bf16 else 0.0
    dq_tol = e @ c64.detach().abs() + out * q64.grad.abs()
    dc_tol = e.T @ q64.detach().abs() + out * c64.grad.abs()
    return {"loss": loss.detach(), "lse": lse, "dq": q64.grad, "dc": c64.grad, "loss_tol": loss_tol, "dq_tol": dq_tol,
            "dc_tol": dc_tol}
