"""K15, the positive's rank among all candidates: three ways to the top-k accuracy of a two-tower model in one process,
device events, warm-up first (development aid):
  fused   retrieval_ops.retrieval_rank(path="fused"): krs_retrieval_rank, scores never stored, every k at once;
  topk    layers.BruteForceRetrieval(k=100, return_scores=False) and the membership test `pos in ids`: K8, one k only;
  slab    retrieval_ops.retrieval_rank(path="slab"): krs_gemm into fp32 slabs of query rows and the count with torch ops.
bf16, D = 128, at B = 64 and B = 8192 against N = 2^20 (K8's serving shapes) and at B = N = 32768.  One JSON line per
shape with the time and the peak memory of each (or why it did not run); --out FILE also writes them there.

The fused path is reported against the 2 B N D flops of its one score product (the short first launch adds 2 B D) over
the 2.5 PF/s bf16 matrix peak, as `fused_tflops` and `fused_of_peak`: a whole-call rate, not a kernel's.  A timed
window is at least --window seconds of calls."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import layers, retrieval_ops

SHAPES = [(64, 2**20), (8192, 2**20), (32768, 32768)]
D = 128
K = 100
PEAK_FLOPS = 2.5e15


def timed(fn, steps, warm, window):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(steps, min(500, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, n


def measure(fn, steps, warm, window):
    """(microseconds per call, calls timed, peak bytes above what was allocated before), or (None, 0, reason)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    try:
        us, n = timed(fn, steps, warm, window)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None, 0, "cannot allocate"
    return round(us, 1), n, torch.cuda.max_memory_allocated() - m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", default="fused,topk,slab")
    ap.add_argument("--shapes", default=None, help="BxN,BxN,... instead of the three of the table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_retrieval_rank: needs an MI355X")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    paths = args.paths.split(",")
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    lines = []
    for b, n in shapes:
        q = (torch.randn((b, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16)
        c = (torch.randn((n, D), device=dev, generator=gen) * 0.5).to(torch.bfloat16)
        pos = torch.randint(0, n, (b,), device=dev, generator=gen, dtype=torch.int32)
        k = min(K, n)
        brute = layers.BruteForceRetrieval(c, k=k, return_scores=False)

        def topk():
            return (brute(q) == pos[:, None]).any(dim=1)

        def rank(path):
            return lambda: retrieval_ops.retrieval_rank(q, c, pos, path=path)[0] < k

        rec = {"B": b, "N": n, "D": D, "k": k, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0),
               "score_matrix_fp32_bytes": b * n * 4,
               "fused_workspace_bytes": retrieval_ops.retrieval_rank_workspace_bytes(b, n, D)}
        if "fused" in paths and "topk" in paths:
            rec["fused_equals_topk"] = bool(torch.equal(rank("fused")(), topk()))
        for name, fn in (("fused", rank("fused")), ("topk", topk), ("slab", rank("slab"))):
            if name in paths:
                rec[f"{name}_us"], rec[f"{name}_calls"], rec[f"{name}_peak_bytes"] = \
                    measure(fn, args.steps, args.warmup, args.window)
        if rec.get("fused_us"):
            flops = 2.0 * b * n * D
            rec["fused_tflops"] = round(flops / rec["fused_us"] / 1e6, 1)
            rec["fused_of_peak"] = round(flops / (rec["fused_us"] * 1e-6) / PEAK_FLOPS, 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, c, pos, brute
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
