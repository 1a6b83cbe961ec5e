"""Float64 numpy restatement of the dense elementwise kernels (csrc/cross_epilogue.hip, dense_aux.hip, loss.hip), written
from the formulas of their header comments in include/krs.h and from the autodiff of feature_cross.py's
`y = x0 * (act(z) + diag * x) + x`:

    cross_fwd        y   = x0 * (u + diag * x) + x
    cross_bwd        dz  = g * x0 * act'(u)                 act' through the OUTPUT u: relu u > 0, sigmoid u (1 - u),
                     dx0 = [init +] g * (u + diag * x)      tanh 1 - u^2, none 1
                     dxd = g + diag * g * x0                folded (x is x0): added into dx0, no dxd
                     dbias[c] = sum_i dz[i, c]
    dense_act_bwd    dz  = g * act'(y),  dbias[c] = sum_i dz[i, c]
    colsum           out[c] = sum_i a[i, c]
    bce              p = clip(pred, eps, 1 - eps);  loss = mean_i -(y_i log p_i + (1 - y_i) log(1 - p_i))
                     dpred_i = scale / n * ((1 - y_i) / (1 - p_i) - y_i / p_i), 0 where the clip is active

Next to every output comes its magnitude M: the float64 sum of the absolute values of the terms the output is a sum
of, which is what a rounding error of the fp32 evaluation is proportional to (tests/dense_walk_cases.py turns M into
the bound).  No kernel, no torch, no oracle: plain numpy on float64 arrays."""

import numpy as np

NONE, RELU, SIGMOID, TANH = 0, 1, 2, 3


def act_grad(act, u):
    """act'(z) written through the output u = act(z)."""
    if act == RELU:
        return (u > 0).astype(np.float64)
    if act == SIGMOID:
        return u * (1.0 - u)
    if act == TANH:
        return 1.0 - u * u
    return np.ones_like(u)


def act_grad_magnitude(act, u):
    """D of M_dz = |g x0| D: the absolute values of the terms of act' (u - u^2, 1 - u^2; 1 for none and relu)."""
    if act == SIGMOID:
        return np.abs(u) + u * u
    if act == TANH:
        return 1.0 + u * u
    return np.ones_like(u)


def cross_fwd(u, x0, x, diag):
    y = x0 * (u + diag * x) + x
    return {"y": y}, {"y": np.abs(x0) * (np.abs(u) + np.abs(diag * x)) + np.abs(x)}


def cross_bwd(g, u, x0, x, diag=0.0, act=NONE, init=None, fold=False, want=("dz", "dx0", "dxd", "dbias")):
    """u None: zeros (allowed without an activation and without dx0).  init: the running dL/dx0 of the layers above
    (dx0_accumulate).  fold: the direct term lands in dx0 and no dxd exists.  Returns (outputs, magnitudes)."""
    out, mag = {}, {}
    uu = np.zeros_like(g) if u is None else u
    gx0 = g * x0
    m_dz = np.abs(gx0) * act_grad_magnitude(act, uu)
    if "dz" in want or "dbias" in want:
        dz = gx0 * act_grad(act, uu)
        if "dz" in want:
            out["dz"], mag["dz"] = dz, m_dz
        if "dbias" in want:
            out["dbias"], mag["dbias"] = dz.sum(axis=0), m_dz.sum(axis=0)
    direct, m_direct = g + diag * gx0, np.abs(g) + np.abs(diag * gx0)
    if "dx0" in want:
        dx0 = g * (uu + diag * x)
        m = np.abs(g) * (np.abs(uu) + np.abs(diag * x))
        if init is not None:
            dx0, m = init + dx0, np.abs(init) + m
        if fold:
            dx0, m = dx0 + direct, m + m_direct
        out["dx0"], mag["dx0"] = dx0, m
    if "dxd" in want and not fold:
        out["dxd"], mag["dxd"] = direct, m_direct
    return out, mag


def dense_act_bwd(g, y, act=NONE, want=("dz", "dbias")):
    yy = np.zeros_like(g) if y is None else y
    dz, m_dz = g * act_grad(act, yy), np.abs(g) * act_grad_magnitude(act, yy)
    out, mag = {}, {}
    if "dz" in want:
        out["dz"], mag["dz"] = dz, m_dz
    if "dbias" in want:
        out["dbias"], mag["dbias"] = dz.sum(axis=0), m_dz.sum(axis=0)
    return out, mag


def colsum(a):
    return {"colsum": a.sum(axis=0)}, {"colsum": np.abs(a).sum(axis=0)}


def bce_bounds(eps):
    """The clip's bounds: fp32 numbers, as the loss is computed in fp32 (lo = eps, hi = 1 - eps rounded to fp32)."""
    lo = np.float32(eps)
    return float(lo), float(np.float32(1.0) - lo)


def bce(pred, labels, eps=1e-7, scale=1.0):
    """M of the loss: sum_i (|y_i log p_i| + |1 - y_i| (|log(1 - p_i)| + 1)) / n -- the 1 is the condition of
    log(1 - p) against the rounding of 1 - p (a relative delta in the argument moves the logarithm by delta)."""
    lo, hi = bce_bounds(eps)
    n = pred.size
    p = np.clip(pred, lo, hi)
    a, b = labels * np.log(p), (1.0 - labels) * np.log1p(-p)
    inside = (pred >= lo) & (pred <= hi)
    t1, t2 = (1.0 - labels) / (1.0 - p), labels / p
    out = {"loss": -(a + b).sum() / n, "dpred": np.where(inside, scale / n * (t1 - t2), 0.0)}
    mag = {"loss": (np.abs(a) + np.abs(1.0 - labels) * (np.abs(np.log1p(-p)) + 1.0)).sum() / n,
           "dpred": np.where(inside, abs(scale) / n * (np.abs(t1) + np.abs(t2)), 0.0)}
    return out, mag
