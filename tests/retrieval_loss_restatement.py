"""Float64 restatement of K11 (csrc/softmax_xent.hip), written from the formulas of include/krs.h: the smoothed row
softmax cross-entropy with its Keras reductions, the term magnitudes its tolerances are built from, the two logit
corrections, and the assembled retrieval head.  Everything is differentiable torch in the dtype of its inputs."""

import numpy as np
import torch

U32 = 2.0 ** -24          # fp32 unit roundoff


def smooth(y, ls):
    """y' = y (1 - ls) + ls / N over the last axis."""
    return y * (1.0 - ls) + ls / y.shape[-1]


def one_hot(index, n, dtype=torch.float64):
    return (index[..., None] == torch.arange(n, device=index.device)).to(dtype)


def row_loss(x, y, ls=0.0):
    """sum_j y'_j ((m - x_j) + log Z) per row of x [..., N] (autodiff-able in x)."""
    yp = smooth(y, ls)
    m = x.amax(-1, keepdim=True)
    log_z = torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    return (yp * ((m - x) + log_z)).sum(-1)


def row_grad(x, y, ls=0.0, g=None):
    """g_r (S exp(x_j - m) / Z - y'_j) per element, g [...] or None (= 1)."""
    yp = smooth(y, ls)
    p = torch.softmax(x, -1)
    d = yp.sum(-1, keepdim=True) * p - yp
    return d if g is None else d * g[..., None]


def reduce(v, w, reduction):
    """keras.losses.Loss reduction of the unreduced v with sample weight w (None, or broadcastable to v)."""
    vw = v if w is None else v * w
    if reduction in (None, "none"):
        return vw
    if reduction == "sum":
        return vw.sum()
    if reduction == "mean_with_sample_weight" and w is not None:
        div = torch.broadcast_to(w, v.shape).sum()
        return vw.sum() / div if float(div) != 0.0 else vw.sum() * 0.0
    return vw.sum() / v.numel()


def magnitudes(x, y, ls=0.0):
    """(loss magnitude [...], gradient magnitude [..., N]) in float64:
        sum_j |y'_j| (|m - x_j| + |log Z| + 1)     and     S p_j (1 + |m - x_j|) + |y'_j|   (for g = 1)."""
    x, yp = x.detach().double(), smooth(y.detach().double(), ls)
    m = x.amax(-1, keepdim=True)
    z = torch.exp(x - m).sum(-1, keepdim=True)
    p = torch.exp(x - m) / z
    lm = (yp.abs() * ((m - x).abs() + torch.log(z).abs() + 1.0)).sum(-1)
    gm = yp.sum(-1, keepdim=True) * p * (1.0 + (m - x).abs()) + yp.abs()
    return lm, gm


def sampling_correction(x, p, eps=1e-6):
    """x - log(clip(p, eps, 1)); p broadcasts from the last axes."""
    return x - torch.log(torch.clamp(p, eps, 1.0))


def remove_accidental_hits_f32(logits, labels, ids, value):
    """The fp32 numpy expression logits + (dup - labels) * value, every operation rounded to fp32 on its own; the
    positive of a row is the first index of its largest label.  Inputs are numpy arrays; ids broadcasts from the last
    axes of labels."""
    logits, labels = np.asarray(logits, np.float32), np.asarray(labels, np.float32)
    ids = np.broadcast_to(np.asarray(ids), labels.shape)
    pos = np.argmax(labels, axis=-1)[..., None]
    dup = (np.take_along_axis(ids, pos, -1) == ids).astype(np.float32)
    return (logits + ((dup - labels) * np.float32(value)).astype(np.float32)).astype(np.float32)


def mine_hard_negatives(scores, labels, num_hard_negatives):
    """The positive and the `num_hard_negatives` highest-scoring negatives of each row: top-k of the key
    scores + labels * (float32 max / 100), gathered from scores and labels (differentiable through the gather)."""
    k = min(num_hard_negatives + 1, scores.shape[-1])
    key = scores.detach() + labels * (float(np.finfo(np.float32).max) / 100.0)
    idx = torch.topk(key, k, dim=-1).indices
    return torch.gather(scores, -1, idx), torch.gather(labels, -1, idx)


def retrieval_head(q, c, cand_ids=None, cand_prob=None, num_hard_negatives=None, value=None):
    """The in-batch softmax loss of q [B, D] against c [N, D] in their dtype, stage by stage: scores, sampling
    correction, accidental hits (with `value`), hard-negative mining, mean of the row losses.  Returns the loss and
    the (scores, labels) that entered the softmax."""
    scores = q @ c.T
    labels = torch.eye(scores.shape[0], scores.shape[1], dtype=scores.dtype, device=scores.device)
    if cand_prob is not None:
        scores = sampling_correction(scores, cand_prob.to(scores.dtype))
    if cand_ids is not None:
        pos = labels.argmax(-1, keepdim=True)
        ids = cand_ids[None, :].expand(labels.shape)
        dup = (torch.gather(ids, -1, pos) == ids).to(scores.dtype)
        scores = scores + (dup - labels) * value
    if num_hard_negatives is not None:
        scores, labels = mine_hard_negatives(scores, labels, num_hard_negatives)
    return row_loss(scores, labels).mean(), scores, labels
