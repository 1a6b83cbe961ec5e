"""K20's arithmetic (include/krs.h) restated in float64 numpy: the forward and the hand-written backward of a GRU layer's
recurrence over projected inputs xz [B, L, 3U], gates in Keras' order z, r, h.

`bf16=True` rounds exactly where the fast path rounds: the A-operand copy of h, the reserve (z, r, c, q) and da to bf16,
and hs, because the backward reads h_{t-1} from the stored hs.  The carried state, the carried dh and the accumulators
are not rounded, and neither are the results that nothing reads back (the final state, dxz, dh0, the weight
gradients): their own half ulp is a term of the bound, not of this mode.  xz, the recurrent kernel, h0 and the
incoming gradients are expected to be bf16 values already.

`defect` names one deliberate error (tests/test_gru_host.py shows that the bounds reject each of them).
"""

import numpy as np

DEFECTS = ("swap_z", "torch_order", "rbh_outside", "mask_zero_state", "mask_out_state", "round_state", "drop_last")


def round_bf16(x):
    """float64 -> nearest-even bf16 value, as float64 (finite inputs)."""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def first_valid(valid, b, l):
    """[B]: the first valid step of every row (L when it has none)."""
    if valid is None:
        return np.zeros(b, dtype=np.int64)
    v = np.asarray(valid) != 0
    return np.where(v.any(axis=1), v.argmax(axis=1), l).astype(np.int64)


def forward(xz, rk, rb, valid, h0, *, bf16=False, defect=None):
    """hs [B, L, U] (the sequence output), h_last [B, U] (the final state), res [B, L, 4, U] (z, r, c, q as the reserve
    holds them)."""
    assert defect is None or defect in DEFECTS
    b, l, u3 = xz.shape
    u = u3 // 3
    rnd = round_bf16 if bf16 else (lambda x: x)
    rb = np.zeros(u3) if rb is None else np.asarray(rb, dtype=np.float64)
    sz, sr, sh = slice(0, u), slice(u, 2 * u), slice(2 * u, 3 * u)
    if defect == "torch_order":
        sz, sr = sr, sz
    h = np.zeros((b, u)) if h0 is None else np.array(h0, dtype=np.float64)
    out_prev = np.zeros((b, u))
    hs, res = np.zeros((b, l, u)), np.zeros((b, l, 4, u))
    for t in range(l):
        v = np.ones(b, dtype=bool) if valid is None else np.asarray(valid)[:, t] != 0
        if defect == "drop_last" and t == l - 1:
            v = np.zeros(b, dtype=bool)
        v = v[:, None]
        a = rnd(h) @ rk
        z = _sigmoid(xz[:, t, sz] + a[:, sz] + rb[sz])
        r = _sigmoid(xz[:, t, sr] + a[:, sr] + rb[sr])
        if defect == "rbh_outside":
            q = a[:, sh]
            c = np.tanh(xz[:, t, sh] + r * q + rb[sh])
        else:
            q = a[:, sh] + rb[sh]
            c = np.tanh(xz[:, t, sh] + r * q)
        hn = (1.0 - z) * h + z * c if defect == "swap_z" else z * h + (1.0 - z) * c
        out = np.where(v, hn, h if defect == "mask_out_state" else out_prev)
        h = np.where(v, hn, 0.0 if defect == "mask_zero_state" else h)
        if defect == "round_state":
            h = round_bf16(h)
        out_prev = out
        hs[:, t] = out
        res[:, t] = np.stack([z, r, c, q], axis=1)
    return {"hs": rnd(hs), "h_last": h, "res": rnd(res)}


def backward(rk, valid, h0, fwd, dhs, dh_last, *, bf16=False):
    """dxz [B, L, 3U], dh0 [B, U], drk [U, 3U], drb [3U] from the forward's stored hs and reserve.  dhs / dh_last: the
    gradients arriving at the sequence output and at the final state (None = zeros)."""
    hs, res = fwd["hs"], fwd["res"]
    b, l, u = hs.shape
    rnd = round_bf16 if bf16 else (lambda x: x)
    first = first_valid(valid, b, l)
    h0 = np.zeros((b, u)) if h0 is None else np.asarray(h0, dtype=np.float64)
    dh = np.zeros((b, u)) if dh_last is None else np.array(dh_last, dtype=np.float64)
    dxz, da, hprev = np.zeros((b, l, 3 * u)), np.zeros((b, l, 3 * u)), np.zeros((b, l, u))
    for t in range(l - 1, -1, -1):
        v = (np.ones(b, dtype=bool) if valid is None else np.asarray(valid)[:, t] != 0)[:, None]
        # h_{t-1}: the stored output from the first valid step on, the initial state before it
        hp = np.where((t - 1 >= first)[:, None], hs[:, t - 1] if t > 0 else 0.0, h0)
        g = dh if dhs is None else dh + np.where((t >= first)[:, None], dhs[:, t], 0.0)
        z, r, c, q = res[:, t, 0], res[:, t, 1], res[:, t, 2], res[:, t, 3]
        dc = np.where(v, g * (1.0 - z) * (1.0 - c * c), 0.0)
        dz = np.where(v, g * (hp - c) * z * (1.0 - z), 0.0)
        dq = dc * r
        dr = dc * q * r * (1.0 - r)
        dxz[:, t] = np.concatenate([dz, dr, dc], axis=1)
        da[:, t] = rnd(np.concatenate([dz, dr, dq], axis=1))
        hprev[:, t] = hp
        dh = np.where(v, g * z, g) + da[:, t] @ rk.T
    drk = hprev.reshape(b * l, u).T @ da.reshape(b * l, 3 * u)
    return {"dxz": dxz, "dh0": dh, "drk": drk, "drb": da.sum(axis=(0, 1))}


def layer(x, kernel, rk, bias, valid, h0, dhs, dh_last, *, bf16=False):
    """layers.GRU as a whole: x [B, L, D], kernel [D, 3U], rk [U, 3U], bias [2, 3U] or None.  Returns hs, h_last and the
    gradients dx, dkernel, drk, dbias, dh0.  bf16=True rounds where the mixed_bfloat16 layer rounds: x, the kernels and
    h0 on their way in, xz (the Dense output), what the recurrence rounds, and dxz, which the layer's own products read
    back.  dx and the other results are left unrounded, as in `backward`."""
    rnd = round_bf16 if bf16 else (lambda v: v)
    b, l, d = x.shape
    u = rk.shape[0]
    xr, kr, rkr = rnd(x), rnd(kernel), rnd(rk)
    h0r = None if h0 is None else rnd(h0)
    b0, b1 = (None, None) if bias is None else (bias[0], bias[1])
    xz = rnd(xr.reshape(b * l, d) @ kr + (0.0 if b0 is None else b0)).reshape(b, l, 3 * u)
    f = forward(xz, rkr, b1, valid, h0r, bf16=bf16)
    g = backward(rkr, valid, h0r, f, dhs, dh_last, bf16=bf16)
    dxz = rnd(g["dxz"]).reshape(b * l, 3 * u)
    out = {"hs": f["hs"], "h_last": f["h_last"], "dx": (dxz @ kr.T).reshape(b, l, d),
           "dkernel": xr.reshape(b * l, d).T @ dxz, "drk": g["drk"], "dh0": g["dh0"]}
    out["dbias"] = None if bias is None else np.stack([dxz.sum(axis=0), g["drb"]])
    return out


def torch_loop(t):
    """Keras' backend rnn over t's xz, rk, rb, h0, valid in float64 torch, one step at a time: torch.where on the state
    and on the output, zeros before the first valid step.  Returns (leaves, hs, h_last); torch autograd does the rest."""
    import torch

    b, l, u3 = t["xz"].shape
    u = u3 // 3
    leaves = {k: torch.from_numpy(t[k]).clone().requires_grad_(True) for k in ("xz", "rk")}
    leaves["rb"] = torch.from_numpy(np.zeros(u3) if t["rb"] is None else t["rb"]).clone().requires_grad_(True)
    leaves["h0"] = torch.from_numpy(np.zeros((b, u)) if t["h0"] is None else t["h0"]).clone().requires_grad_(True)
    h, prev, outs = leaves["h0"], torch.zeros(b, u, dtype=torch.float64), []
    for step in range(l):
        a = h @ leaves["rk"]
        x = leaves["xz"][:, step]
        z = torch.sigmoid(x[:, :u] + a[:, :u] + leaves["rb"][:u])
        r = torch.sigmoid(x[:, u:2 * u] + a[:, u:2 * u] + leaves["rb"][u:2 * u])
        c = torch.tanh(x[:, 2 * u:] + r * (a[:, 2 * u:] + leaves["rb"][2 * u:]))
        hn = z * h + (1 - z) * c
        v = torch.ones(b, 1, dtype=torch.bool) if t["valid"] is None else torch.from_numpy(t["valid"][:, step:step + 1] != 0)
        prev = torch.where(v, hn, prev)
        h = torch.where(v, hn, h)
        outs.append(prev)
    return leaves, torch.stack(outs, dim=1), h
