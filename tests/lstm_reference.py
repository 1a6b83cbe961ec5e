"""K25's arithmetic (include/krs.h) in float64 numpy, as plain loops over t: the forward and the hand-written backward of
an LSTM layer's recurrence over projected inputs xz [B, L, 4U], gates in Keras' order i, f, c, o, with the masked-step
rule (both states carried, the previous output repeated, zeros before the first valid step).

`bf16=True` rounds, to nearest even, what the fast route rounds: xz and the recurrent kernel (expected to be bf16 values
already), the A-operand copy of h, the stored hs, the reserve as the kernel stores it (i and g as bf16; f, o and the
carried c as fp32) and da, which is dxz.  The carried h, c, dh, dc and the accumulators are not rounded, and neither are
the results nothing reads back (the final states, dh0, dc0, d recurrent_kernel): their own half ulp is the second term
of the bound.  The bound of a bf16 case (the derivation is in tests/gru_cases.py): with E the largest distance between
the rounding form and the exact form of that case and output, a result must be within 2 E + 2^-8 |ref| of the exact one.
"""

import numpy as np

FP32_TOL = 1e-5
OUTPUTS = ("hs", "h", "c", "dxz", "dh0", "dc0", "drk")


def round_bf16(x):
    """float64 -> nearest-even bf16 value, as float64 (finite inputs)."""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _fp32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm(xz, rk, valid, h0, c0, dhs, dh_last, dc_last, *, bf16=False):
    """Every output of the recurrence: hs [B, L, U], the final h and c [B, U]; dxz [B, L, 4U], dh0, dc0 [B, U] and
    drk [U, 4U] for the gradients dhs / dh_last / dc_last arriving at hs, h and c (None = zeros)."""
    b, l, u4 = xz.shape
    u = u4 // 4
    r16 = round_bf16 if bf16 else (lambda x: x)
    r32 = _fp32 if bf16 else (lambda x: x)
    valid = np.ones((b, l), dtype=bool) if valid is None else np.asarray(valid) != 0
    first = np.where(valid.any(axis=1), valid.argmax(axis=1), l)
    h0 = np.zeros((b, u)) if h0 is None else np.asarray(h0, dtype=np.float64)
    c0 = np.zeros((b, u)) if c0 is None else np.asarray(c0, dtype=np.float64)
    h, c, out = h0.copy(), c0.copy(), np.zeros((b, u))
    hs = np.zeros((b, l, u))
    gi, gf, gg, go, cs = (np.zeros((b, l, u)) for _ in range(5))
    for t in range(l):
        v = valid[:, t, None]
        a = xz[:, t] + r16(h) @ rk
        i, f = _sigmoid(a[:, :u]), _sigmoid(a[:, u:2 * u])
        g, o = np.tanh(a[:, 2 * u:3 * u]), _sigmoid(a[:, 3 * u:])
        cn = f * c + i * g
        hn = o * np.tanh(cn)
        h, c, out = np.where(v, hn, h), np.where(v, cn, c), np.where(v, hn, out)
        hs[:, t] = r16(out)
        gi[:, t], gg[:, t], gf[:, t], go[:, t], cs[:, t] = r16(i), r16(g), r32(f), r32(o), r32(c)

    dh = np.zeros((b, u)) if dh_last is None else np.array(dh_last, dtype=np.float64)
    dc = np.zeros((b, u)) if dc_last is None else np.array(dc_last, dtype=np.float64)
    dxz, hprev = np.zeros((b, l, u4)), np.zeros((b, l, u))
    for t in range(l - 1, -1, -1):
        v = valid[:, t, None]
        # h_{t-1}: the stored output from the first valid step on, the initial state before it; c_{t-1} likewise carried
        hprev[:, t] = np.where((t - 1 >= first)[:, None], hs[:, t - 1] if t > 0 else 0.0, h0)
        cp = cs[:, t - 1] if t > 0 else c0
        gh = dh if dhs is None else dh + np.where((t >= first)[:, None], dhs[:, t], 0.0)
        i, f, g, o, tc = gi[:, t], gf[:, t], gg[:, t], go[:, t], np.tanh(cs[:, t])
        dct = dc + gh * o * (1.0 - tc * tc)
        da = np.concatenate([dct * g * i * (1.0 - i), dct * cp * f * (1.0 - f), dct * i * (1.0 - g * g),
                             gh * tc * o * (1.0 - o)], axis=1)
        dxz[:, t] = r16(np.where(v, da, 0.0))
        dc = np.where(v, dct * f, dc)
        dh = np.where(v, 0.0, gh) + dxz[:, t] @ rk.T
    drk = hprev.reshape(b * l, u).T @ dxz.reshape(b * l, u4)
    return {"hs": hs, "h": h, "c": c, "dxz": dxz, "dh0": dh, "dc0": dc, "drk": drk}


def layer(x, kernel, rk, bias, valid, h0, c0, dhs, dh_last, dc_last, *, bf16=False):
    """layers.LSTM as a whole: x [B, L, D], kernel [D, 4U], rk [U, 4U], bias [4U].  Adds dx, dkernel and dbias to
    lstm()'s outputs.  bf16=True also rounds where the mixed_bfloat16 layer rounds: x, the kernels and the initial
    states on their way in, and xz (the Dense output)."""
    rnd = round_bf16 if bf16 else (lambda v: v)
    b, l, d = x.shape
    xr, kr = rnd(x).reshape(b * l, d), rnd(kernel)
    xz = rnd(xr @ kr + bias).reshape(b, l, -1)
    out = lstm(xz, rnd(rk), valid, None if h0 is None else rnd(h0), None if c0 is None else rnd(c0), dhs, dh_last,
               dc_last, bf16=bf16)
    dxz = out["dxz"].reshape(b * l, -1)
    out.update(dx=(dxz @ kr.T).reshape(b, l, d), dkernel=xr.T @ dxz, dbias=dxz.sum(axis=0))
    return out


def bounds(ref, rounded, bf16):
    """Per-element bound of every output, and E per output (0 for an fp32 case)."""
    if not bf16:
        return {k: FP32_TOL + FP32_TOL * np.abs(ref[k]) for k in ref}, {k: 0.0 for k in ref}
    e = {k: float(np.abs(rounded[k] - ref[k]).max(initial=0.0)) for k in ref}
    return {k: 2.0 * e[k] + 2.0 ** -8 * np.abs(ref[k]) for k in ref}, e
