"""Float64 restatement of K14 (hard-negative mining in front of the in-batch softmax loss), written from the formulas of
include/krs.h on top of tests/retrieval_xent_restatement.py: the corrected scores, the selection of each row's k
hardest negatives in the one total order (score descending, then index ascending, -0.0 as +0.0), the cross-entropy over
the k + 1 kept logits, its gradients by autograd through the gather, and the error bounds the tests hold the kernels to.
Plain torch on whatever device the inputs are on.

Bounds: those of retrieval_xent_restatement.reference with its p_bf16=False (P stays in fp32 on this path), restated
for the k + 1 kept logits.  With u = 2^-24, delta_i = max_j 4 (D + 16) u (sum_d |q_id c_jd| + |bias_j| + |hit_ij|) the
score bound, kappa = 4 (k + 1 + 16) u for the sums over the k + 1 logits (softmax, loss, dq), and
kappa_c = 4 (B + 16) u for dc_j, whose fp32 sum runs over the up to B queries that mined candidate j:
    |loss_i - ref| <= sum_m y'_im (2 delta_i + kappa (|lse_i - s_im| + 1))
    E_im            = |g_i| p_im (2 delta_i + kappa) + kappa   |P_im|        (for dq)
    F_im            = |g_i| p_im (2 delta_i + kappa) + kappa_c |P_im|        (for dc)
    |dq - ref|     <= sum_m E_im |c[idx_im]| + 2^-8 |ref| [bf16 output]
    |dc_j - ref|   <= sum_{(i,m): idx_im = j} F_im |q_i| + 2^-8 |ref| [bf16 output]
They hold where the kernel and float64 select the same set; `gap` says where that is guaranteed."""

import torch

from tests import retrieval_loss_restatement as R
from tests import retrieval_xent_restatement as X

U32 = X.U32


def select(s, pos, k):
    """int64 [B, k]: per row of the scores s [B, N] the k columns other than pos that come first in the total order
    (value descending, then index ascending; -0.0 counts as +0.0).  A pos outside [0, N) excludes nothing."""
    n = s.shape[1]
    key = -(s.detach().clone() + 0.0)                     # ascending sort of -s; + 0.0 turns -0.0 into +0.0
    ok = (pos >= 0) & (pos < n)
    rows = torch.nonzero(ok)[:, 0]
    key[rows, pos[rows]] = float("inf")                   # the positive goes last: never among the first k <= N - 1
    return torch.sort(key, dim=-1, stable=True).indices[:, :k]


def mined_logits(q, c, k, pos=None, bias=None, ids=None, hit_value=0.0):
    """(logits [B, k + 1] with the positive first -- NaN where there is none --, the selection int64 [B, k], the full
    scores [B, N], the positives int64 [B], ok [B]) in the dtype of q; differentiable through the gather."""
    s, pos = X.scores(q, c, pos, bias, ids, hit_value)
    n = s.shape[1]
    ok = (pos >= 0) & (pos < n)
    idx = select(s, pos, k)
    pos_score = s.gather(1, pos.clamp(0, n - 1)[:, None])[:, 0]
    pos_score = torch.where(ok, pos_score, torch.full_like(pos_score, float("nan")))
    return torch.cat((pos_score[:, None], s.gather(1, idx)), dim=1), idx, s, pos, ok


def row_loss(q, c, k, pos=None, bias=None, ids=None, hit_value=0.0, ls=0.0):
    """The unreduced loss [B]: NaN for a row without a positive."""
    logits = mined_logits(q, c, k, pos, bias, ids, hit_value)[0]
    zero = torch.zeros(logits.shape[0], dtype=torch.int64, device=logits.device)
    return R.row_loss(logits, R.one_hot(zero, k + 1, logits.dtype), ls)


def reference(q, c, k, pos=None, bias=None, ids=None, hit_value=0.0, ls=0.0, g=None, out_bf16=True):
    """float64 results and bounds as a dict: loss [B] (NaN for a row without a positive), idx [B, k], scores [B, k],
    pos_score [B], dq, dc (autograd of sum_i g_i loss_i over the rows that have a positive), loss_tol, dq_tol, dc_tol,
    delta [B] (the score bound), gap [B] (k-th minus (k+1)-th negative score; inf when there are only k negatives),
    ok [B], and nan_dc [N]: the candidates mined by a row without a positive, whose dc rows are NaN."""
    q64 = q.detach().double().requires_grad_(True)
    c64 = c.detach().double().requires_grad_(True)
    b, d = q64.shape
    n = c64.shape[0]
    bias64 = None if bias is None else bias.detach().double()
    g64 = torch.ones(b, dtype=torch.float64, device=q.device) if g is None else g.detach().double()
    logits, idx, s, pos, ok = mined_logits(q64, c64, k, pos, bias64, ids, hit_value)
    zero = torch.zeros(b, dtype=torch.int64, device=q.device)
    y = R.one_hot(zero, k + 1, torch.float64)
    yp = R.smooth(y, ls)
    loss = R.row_loss(logits, y, ls)
    (R.row_loss(logits[ok], y[ok], ls) * g64[ok]).sum().backward()     # (a NaN row stays out of the graph)
    x = logits.detach()
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[:, None])
    big_p = g64[:, None] * (p - yp)
    kappa, kappa_c = 4 * (k + 1 + 16) * U32, 4 * (b + 16) * U32
    mag = q64.detach().abs() @ c64.detach().abs().T
    if bias64 is not None:
        mag = mag + bias64.abs()[None, :]
    if ids is not None:
        plain = X.scores(q64.detach(), c64.detach(), pos, bias64, None, 0.0)[0]
        mag = mag + (s.detach() - plain).abs()
    delta = 4 * (d + 16) * U32 * mag.amax(-1)
    loss_tol = (yp * (2 * delta[:, None] + kappa * ((lse[:, None] - x).abs() + 1))).sum(-1)
    common = g64.abs()[:, None] * p * (2 * delta[:, None] + kappa)
    index = torch.cat((pos.clamp(0, n - 1)[:, None], idx), dim=1)

    def dense(t):
        t = torch.where(ok[:, None], t, torch.zeros_like(t))
        return torch.zeros((b, n), dtype=torch.float64, device=q.device).scatter_add_(1, index, t)

    out = 2.0 ** -8 if out_bf16 else 0.0
    dq_tol = dense(common + kappa * big_p.abs()) @ c64.detach().abs() + out * q64.grad.abs()
    dc_tol = dense(common + kappa_c * big_p.abs()).T @ q64.detach().abs() + out * c64.grad.abs()
    masked = s.detach().clone() + 0.0
    rows = torch.nonzero(ok)[:, 0]
    masked[rows, pos[rows]] = float("-inf")
    top = torch.sort(masked, dim=-1, descending=True).values
    negatives = n - ok.to(torch.int64)
    gap = torch.where(negatives > k, top[:, k - 1] - top[:, min(k, n - 1)], torch.full_like(delta, float("inf")))
    nan_dc = torch.zeros(n, dtype=torch.bool, device=q.device)
    nan_dc[idx[~ok].reshape(-1)] = True
    return {"loss": loss.detach(), "idx": idx, "scores": x[:, 1:], "pos_score": x[:, 0], "dq": q64.grad, "dc": c64.grad,
            "loss_tol": loss_tol, "dq_tol": dq_tol, "dc_tol": dc_tol, "delta": delta, "gap": gap, "ok": ok,
            "nan_dc": nan_dc}
