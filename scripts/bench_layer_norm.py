"""K22 fused residual + dropout + layer norm: forward + backward of two implementations in one process, device events,
every shape warmed up first, the implementations alternating over several repeats, every timed window at least
--window seconds long (development aid):
  krs      norm_ops.residual_layer_norm (K22: one launch forward, one or two backward);
  torch    the composition the sequence layers ran before K22: F.dropout, an add, and F.layer_norm on a float() copy
           cast back.
Per-op: the forms norm, add-norm (y and the sum) and add, bf16 and fp32, p in {0, 0.2}, rows x d at (4096*50, 50),
(4096*200, 64), (4096*200, 128), (1024*200, 256), (65536, 1024).  Whole block: one pre-norm and one post-norm
TransformerDecoder training step (forward, loss, every gradient) with layers.sequence.FUSE_NORM on against off, at
B = 1024, L = 200, d = 128 and at examples/sas_rec.py's B = 64, L = 50, d = 50.
One JSON line per point with the median and the fastest repeat's time per call and the peak memory of each side, and
the bytes the algorithm has to move (per-op); --out FILE also writes them there.

Kernel times and launch counts come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats -d DIR -o k22 -- python scripts/bench_layer_norm.py --trace --plan PLAN.json
    python scripts/bench_layer_norm.py --parse DIR/.../k22_results.db --plan PLAN.json [--out FILE]
--trace runs every point once (a warm-up) and then three times, each behind a marker (six tiny K22 forward launches
in a row, which no point produces), and writes the order of the sections to PLAN.json; --parse splits the trace at the markers and reports, per
point, the K22 kernel time per call, the needed bytes over it as a share of 8 TB/s, and the launches per call."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import layers as kl
from keras_rs_amd import norm_ops
from keras_rs_amd.layers import sequence

SHAPES = [(4096 * 50, 50), (4096 * 200, 64), (4096 * 200, 128), (1024 * 200, 256), (65536, 1024)]
FORMS = [("norm", 0.0), ("addnorm", 0.0), ("addnorm", 0.2), ("add", 0.0), ("add", 0.2)]
BLOCKS = [(1024, 200, 128, 2), (64, 50, 50, 1)]          # B, L, d, heads
PEAK_TBS = 8.0
MARKER = 6


def needed_bytes(form, p, n, d, esize):
    """What forward + backward have to move at the least: every operand read once, every result written once."""
    m = n * d * esize
    if form == "norm":
        return 5 * m + 4 * 4 * n                  # x, y | x, dy, dx; mean and rstd written and read
    if form == "addnorm":
        return (9 if p > 0 else 8) * m + 4 * 4 * n    # x, res, y, sum | sum, dy, dsum, dx (and dres under dropout)
    return 3 * m + (2 * m if p > 0 else 0)        # x, res, sum | dsum, dx under dropout (none without)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def peak_of(fn):
    """Peak bytes of one call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - m0


def op_pair(form, p, n, d, dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(n + d)
    mk = lambda: torch.randn(n, d, generator=g).to(dtype).to(dev)
    x, res, dy, dsum = mk().requires_grad_(True), mk().requires_grad_(True), mk(), mk()
    gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(d, generator=g)).to(dev).requires_grad_(True)
    draw = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = lambda t: torch.nn.functional.layer_norm(t.float(), (d,), gamma, beta, 1e-5).to(dtype)
    drop = lambda t: torch.nn.functional.dropout(t, p, True) if p > 0 else t

    if form == "norm":
        def krs():
            y = norm_ops.residual_layer_norm(x, None, gamma, beta, epsilon=1e-5)
            return torch.autograd.grad(y, (x, gamma, beta), dy)

        def ref():
            return torch.autograd.grad(ln(x), (x, gamma, beta), dy)
    elif form == "addnorm":
        def krs():
            y, s = norm_ops.residual_layer_norm(x, res, gamma, beta, epsilon=1e-5, dropout_p=p, seed=3, draw=draw,
                                                return_sum=True)
            return torch.autograd.grad((y, s), (x, res, gamma, beta), (dy, dsum))

        def ref():
            s = drop(x) + res
            return torch.autograd.grad((ln(s), s), (x, res, gamma, beta), (dy, dsum))
    else:
        def krs():
            s = norm_ops.residual_layer_norm(x, res, epsilon=0.0, dropout_p=p, seed=3, draw=draw, norm=False)
            return torch.autograd.grad(s, (x, res), dsum)

        def ref():
            return torch.autograd.grad(drop(x) + res, (x, res), dsum)
    return krs, ref


def block_step(b, l, d, heads, normalize_first, dev):
    torch.manual_seed(b + d)
    layer = kl.TransformerDecoder(d, num_heads=heads, dropout=0.2, normalize_first=normalize_first, seed=5,
                                  dtype="mixed_bfloat16", device=dev)
    x = torch.randn(b, l, d, device=dev).requires_grad_(True)
    target = torch.randn(b, l, d, device=dev)
    mask = (torch.arange(l, device=dev)[None, :] >= (torch.arange(b, device=dev) % (l // 2))[:, None])
    layer(x, decoder_padding_mask=mask)

    def step(fused):
        sequence.FUSE_NORM = fused
        out = layer(x, decoder_padding_mask=mask, training=True)
        loss = (out.float() - target).square().mean()
        return torch.autograd.grad(loss, [x] + layer.weights)

    return (lambda: step(True)), (lambda: step(False))


def points(dev, only_ops=False):
    for n, d in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            for form, p in FORMS:
                label = dict(kind="op", form=form, p=p, n=n, d=d, dtype=str(dtype).split(".")[-1],
                             needed_bytes=needed_bytes(form, p, n, d, 2 if dtype == torch.bfloat16 else 4))
                yield label, op_pair(form, p, n, d, dtype, dev)
    if only_ops:
        return
    for b, l, d, heads in BLOCKS:
        for first in (True, False):
            label = dict(kind="block", norm="pre" if first else "post", b=b, l=l, d=d, heads=heads, dtype="bfloat16")
            yield label, block_step(b, l, d, heads, first, dev)


def run_timed(args, dev):
    lines = []
    for label, (krs, ref) in points(dev):
        fns = {"krs": krs, "torch": ref}
        rec = dict(label)
        calls = {}
        for name, fn in fns.items():
            for _ in range(args.warmup):
                fn()
            trial = timed(fn, 3)
            calls[name] = max(args.steps, int(args.window * 1e6 / max(trial, 1.0)) + 1)
        times = {name: [] for name in fns}
        for _ in range(args.repeats):
            for name, fn in fns.items():
                times[name].append(timed(fn, calls[name]))
        for name, fn in fns.items():
            rec[name] = dict(median_us=round(statistics.median(times[name]), 1), best_us=round(min(times[name]), 1),
                             calls=calls[name], peak_bytes=peak_of(fn))
        rec["speedup"] = round(rec["torch"]["median_us"] / rec["krs"]["median_us"], 3)
        if label["kind"] == "op":
            rec["krs"]["wall_share_of_8tbs"] = round(label["needed_bytes"] / (rec["krs"]["median_us"] * 1e-6) / (PEAK_TBS * 1e12), 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del fns, krs, ref
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def marker(dev):
    t = torch.zeros(1, 8, dtype=torch.bfloat16, device=dev)
    for _ in range(MARKER):
        norm_ops.residual_layer_norm(t, t, epsilon=0.0, norm=False)


def run_trace(args, dev):
    plan = []
    for label, (krs, ref) in points(dev):
        sides = {"krs": krs} if label["kind"] == "op" else {"krs": krs, "torch": ref}
        for side, fn in sides.items():
            marker(dev)
            fn()                                   # (a warm-up in a section of its own, which --parse drops)
            torch.cuda.synchronize()
            plan.append(dict(label, side=side, calls=1, warmup=True))
            marker(dev)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            plan.append(dict(label, side=side, calls=3))
        del sides, krs, ref
        torch.cuda.empty_cache()
    marker(dev)
    torch.cuda.synchronize()
    with open(args.plan, "w") as f:
        json.dump(plan, f)


def run_parse(args):
    db = sqlite3.connect(args.parse)
    cur = db.cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = cur.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    plan = json.load(open(args.plan))
    # split at the markers: MARKER consecutive ln_fwd_kernel dispatches
    sections, current, run = [], None, 0
    for name, start, end in rows:
        run = run + 1 if "ln_fwd_kernel" in name else 0
        if run == MARKER:
            if current is not None:
                sections.append(current[:-(MARKER - 1)])
            current = []
            continue
        if current is not None:
            current.append((name, end - start))
    assert len(sections) == len(plan), (len(sections), len(plan))
    lines = []
    for label, sec in zip(plan, sections):
        if label.get("warmup"):
            continue
        calls = label["calls"]
        ln_ns = sum(t for name, t in sec if "ln_" in name and "kernel" in name and "krs" in name)
        rec = dict(label, launches_per_call=round(len(sec) / calls, 2), kernel_us_all=round(sum(t for _, t in sec) / calls / 1e3, 1),
                   k22_kernel_us=round(ln_ns / calls / 1e3, 1))
        if label["kind"] == "op" and ln_ns:
            rec["k22_share_of_8tbs"] = round(label["needed_bytes"] / (ln_ns / calls * 1e-9) / (PEAK_TBS * 1e12), 3)
        lines.append(json.dumps(rec))
        print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="fewest calls in a timed window")
    ap.add_argument("--window", type=float, default=0.5, help="fewest seconds in a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--plan", default="k22_plan.json")
    ap.add_argument("--parse", default=None)
    args = ap.parse_args()
    if args.parse:
        return run_parse(args)
    dev = torch.device("cuda:0")
    old = sequence.FUSE_NORM
    try:
        run_trace(args, dev) if args.trace else run_timed(args, dev)
    finally:
        sequence.FUSE_NORM = old


if __name__ == "__main__":
    main()
