"""A numpy restatement of K24 (include/krs.h, krs_regression_fwd_bwd).  No torch, no GPU.

Two things are restated:
  * `gradient32`: dpred in the contract's fp32 operation order, one numpy float32 operation per contract operation, the
    final rounding to bf16 included, and under MEAN_WITH_SAMPLE_WEIGHT the sum W of the weights in the contract's
    summation order (`ordered_sum32`).  The kernel's dpred must equal it bit for bit.
  * `reference64`: the loss and the three batch sums in float64 from the same (already rounded) inputs, with the sum of
    the absolute values of the terms of every sum, from which `bounds` derives how far the kernel's fp32 sums may be.

pred, target: [B, C]; weight: [B] or None; g: [B] (the upstream gradient of reduction "none") or a scalar.
"""

import numpy as np

F32 = np.float32
U = 2.0 ** -24                   # unit round-off of fp32
THREADS, MAX_BLOCKS = 1024, 256  # KRS_REGRESSION_THREADS, KRS_REGRESSION_MAX_BLOCKS
KINDS = ("mse", "mae", "huber")
REDUCTIONS = ("none", "sum", "sum_over_batch_size", "mean_with_sample_weight")


def round_bf16(x):
    """float32 -> the nearest-even bf16 value as float32; NaN stays NaN, +-inf stay."""
    f = np.asarray(x, dtype=F32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    return np.where(np.isnan(f), F32(np.nan), r.view(F32))


def blocks_for(items):
    return int(min(MAX_BLOCKS, max(1, -(-items // THREADS))))


def vec_rows(dtype):
    return 8 if dtype == "bf16" else 4


def ordered_sum32(x):
    """sum of the fp32 vector x in the element route's order: thread t of workgroup j of G adds x[j T + t], + G T, ..;
    a halving tree over the T threads; the G partials in order."""
    x = np.asarray(x, dtype=F32)
    n, g = len(x), blocks_for(len(x))
    rounds = max(1, -(-n // (g * THREADS)))
    padded = np.zeros(rounds * g * THREADS, dtype=F32)     # (+0 leaves every partial sum as it is)
    padded[:n] = x
    steps = padded.reshape(rounds, g, THREADS)
    acc = np.zeros((g, THREADS), dtype=F32)
    for i in range(rounds):
        acc = acc + steps[i]
    o = THREADS // 2
    while o:
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
        o //= 2
    s = F32(0)
    for j in range(g):
        s = F32(s + acc[j, 0])
    return s


def sign32(e):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(e), e, (e > 0).astype(F32) - (e < 0).astype(F32)).astype(F32)


def derivative32(e, kind, delta):
    """f'(e) in the contract's operations (fp32 in, fp32 out)."""
    e = np.asarray(e, dtype=F32)
    if kind == "mse":
        return e + e
    if kind == "mae":
        return sign32(e)
    d = F32(delta)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(e) <= d, e, d * sign32(e)).astype(F32)


def term64(e, kind, delta):
    e = np.asarray(e, dtype=np.float64)
    if kind == "mse":
        return e * e
    if kind == "mae":
        return np.abs(e)
    d = float(F32(delta))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.abs(e) <= d, 0.5 * e * e, d * np.abs(e) - 0.5 * d * d)


def shares32(weight, b, reduction):
    """s_b [B] fp32 of the contract."""
    phi = F32(1) / F32(b) if b else F32(0)
    if weight is None:
        s = phi if reduction in ("sum_over_batch_size", "mean_with_sample_weight") else F32(1)
        return np.full(b, s, dtype=F32)
    w = np.asarray(weight, dtype=F32)
    if reduction == "mean_with_sample_weight":
        W = ordered_sum32(w)
        with np.errstate(all="ignore"):
            return (w / W).astype(F32) if W != 0 else np.zeros(b, dtype=F32)
    if reduction == "sum_over_batch_size":
        return (w * phi).astype(F32)
    return w.copy()


def gradient32(pred, target, weight, kind, delta, reduction, g=1.0, dtype="fp32"):
    """dpred [B, C] as float32 values (bf16 values when dtype == "bf16"), bit for bit what the kernel stores."""
    pred, target = np.asarray(pred, dtype=F32), np.asarray(target, dtype=F32)
    b, c = pred.shape
    with np.errstate(all="ignore"):
        e = pred - target
        d = derivative32(e, kind, delta)
        gb = np.broadcast_to(np.asarray(g, dtype=F32), (b,))
        k = ((gb * shares32(weight, b, reduction)).astype(F32) / F32(c)).astype(F32)
        out = (k[:, None] * d).astype(F32)
    return round_bf16(out) if dtype == "bf16" else out


def reference64(pred, target, weight, kind, delta, reduction):
    """{"loss": float64 scalar or [B], "sums": [3], "abs_loss": sum |terms| of the loss's sum (or per row),
    "abs_sums": [3] likewise, "abs_w": sum |w|} from the inputs as the kernel reads them."""
    p, y = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    b, c = p.shape
    with np.errstate(all="ignore"):
        e = p - y
        v = term64(e, kind, delta).sum(axis=1) / c
        absv = np.abs(term64(e, kind, delta)).sum(axis=1) / c
        q, a = (e * e).sum(axis=1), np.abs(e).sum(axis=1)
        if weight is None:
            w = np.ones(b)
            sums = np.array([q.sum(), a.sum(), float(b * c)])
            abs_sums = np.array([q.sum(), a.sum(), 0.0])
        else:
            w = np.asarray(weight, dtype=np.float64)
            sums = np.array([(w * q / c).sum(), (w * a / c).sum(), w.sum()])
            abs_sums = np.array([(np.abs(w) * q / c).sum(), (np.abs(w) * a / c).sum(), np.abs(w).sum()])
        t = w * v
        abs_t = np.abs(w) * absv
        total, W = t.sum(), w.sum()
        if reduction == "none":
            loss, abs_loss = t, abs_t
        elif reduction == "sum":
            loss, abs_loss = total, abs_t.sum()
        elif reduction == "sum_over_batch_size" or weight is None:
            loss, abs_loss = (total / b if b else 0.0), (abs_t.sum() / b if b else 0.0)
        else:
            loss, abs_loss = (total / W if float(F32(W)) != 0 and W != 0 else 0.0), abs_t.sum()
    return {"loss": loss, "sums": sums, "abs_loss": abs_loss, "abs_sums": abs_sums, "abs_w": float(np.abs(w).sum()),
            "W": float(W), "total": float(total)}


def depth(b, c, dtype, vec):
    """the longest chain of fp32 additions behind a sum of the main pass: a thread's items (rows of an item, columns of
    a row), the tail row of the vector route, the tree over 1024 threads, the partials in workgroup order."""
    v = vec_rows(dtype) if vec else 1
    items = b // v
    g = blocks_for(items)
    per_thread = -(-items // (g * THREADS)) * v if items else 0
    return per_thread + (1 if vec and b % v else 0) + c + 10 + g


# fp32 operations on a term before it enters a sum (e, the square or product, the Huber branch's two, / c, * w), and
# on a sum after it (* phi or / W): each at most one unit round-off relative to the term
TERM_OPS = 6


def bounds(ref, b, c, dtype, vec, reduction, weighted):
    """(loss bound, sums bounds [3]): depth x unit round-off x sum |terms| (first order in U, with 1.01 for the higher
    orders), from the summation order alone.  Under a weighted MEAN_WITH_SAMPLE_WEIGHT the quotient T / W adds the
    error of W (its own pass, in the element route's depth over b) scaled by |T| / W^2."""
    n = depth(b, c, dtype, vec) + TERM_OPS
    sums = 1.01 * n * U * np.asarray(ref["abs_sums"])
    if reduction == "none":
        return 1.01 * (c + TERM_OPS) * U * np.asarray(ref["abs_loss"]), sums
    loss = 1.01 * n * U * ref["abs_loss"]
    if reduction == "mean_with_sample_weight" and weighted and ref["W"] != 0:
        n_w = depth(b, 1, "fp32", False)
        loss = loss / abs(ref["W"]) + 1.01 * n_w * U * ref["abs_w"] * abs(ref["total"]) / ref["W"] ** 2
    return loss, sums
