"""K8 retrieval: the fused score + top-k (krs_retrieval_topk) against the two-step baseline -- dense_ops.gemm into
fp32 slab chunks of at most 1 GiB, then torch.topk -- at the three shapes of DESIGN.md section 4 (K8), in one process,
device events, warm-up first (development aid).  One JSON line per shape; --out FILE also writes them there.

Bounds: S1 reads the candidate matrix once (HBM 6.29 TB/s, the measured copy bandwidth of MI355X); S2 / S3 are
MFMA-bound (2.5 PFLOP/s dense bf16, 157 TFLOP/s fp32 matrix: spec figures)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from keras_rs_amd import dense_ops as D
from keras_rs_amd import retrieval_ops as R

HBM = 6.29e12
SHAPES = [  # name, dtype, B, N, D, k, bound
    ("S1", torch.bfloat16, 64, 1 << 20, 128, 100, "bytes"),
    ("S2", torch.bfloat16, 8192, 1 << 20, 128, 100, "flops"),
    ("S3", torch.float32, 1024, 1 << 20, 64, 10, "flops"),
]
PEAK = {torch.bfloat16: 2.5e15, torch.float32: 157e12}


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def two_step(q, c, k):
    rows = max(1, min(q.shape[0], (1 << 30) // (c.shape[0] * 4)))
    slab = torch.empty((rows, c.shape[0]), dtype=torch.float32, device=q.device)
    outs = []
    for r0 in range(0, q.shape[0], rows):
        qc = q[r0:r0 + rows]
        s = slab[:qc.shape[0]]
        D.gemm(qc, c, b_is_nk=True, out_dtype=torch.float32, out=s)
        outs.append(torch.topk(s, k, dim=1))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="S1,S2,S3", help="comma-separated subset of S1,S2,S3")
    ap.add_argument("--no-baseline", action="store_true", help="time the fused path only (profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, dt, b, n, d, k, bound in SHAPES:
        if name not in args.shapes.split(","):
            continue
        q = torch.randn((b, d), device=dev, generator=g).to(dt)
        c = torch.randn((n, d), device=dev, generator=g).to(dt)
        us_f = timed(lambda: R.retrieval_topk(q, c, k), args.steps, args.warmup)
        us_b = float("nan") if args.no_baseline else timed(lambda: two_step(q, c, k), max(1, args.steps // 5), 1)
        flops = 2.0 * b * n * d
        nbytes = float(n * d * c.element_size() + b * d * q.element_size())
        if bound == "bytes":
            achieved, limit, unit = nbytes / (us_f * 1e-6), HBM, "B/s"
        else:
            achieved, limit, unit = flops / (us_f * 1e-6), PEAK[dt], "FLOP/s"
        rec = {"shape": name, "dtype": str(dt).split(".")[-1], "B": b, "N": n, "D": d, "k": k,
               "fused_us": round(us_f, 1), "two_step_us": round(us_b, 1), "speedup": round(us_b / us_f, 2),
               "bound": bound, "achieved": f"{achieved:.3e} {unit}", "fraction_of_bound": round(achieved / limit, 3),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, c
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
