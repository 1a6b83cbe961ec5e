"""K12 binary metrics: one BinaryMetricGroup update of BinaryAccuracy and AUC(200) on the HIP path against the same
update composed from torch ops as keras composes it (metrics_utils.update_confusion_matrix_variables with evenly
spaced thresholds: clip, multiply, ceil, relu, two segment sums, two flips and cumsums, the subtractions; and
Mean.update_state of `y_true == (y_pred > 0.5)`), and the per-step cost of `metrics=` in
examples/dlrm_dcn_v2.train_step (development aid).

One (path, size) per process, so that a `rocprofv3 --kernel-trace --stats -- python scripts/bench_binary_metrics.py
--path k12 --n 65536` run sees the kernels of that path alone; without the profiler the script times every update with
device events and prints one JSON line (median, minimum, 90th percentile in microseconds).

    --path k12 | torch          one update at --n samples (65 536 = the C3 batch, 4 194 304 = an evaluation slab)
    --path step | step-metrics  one training step of the example's model at --n = the batch (8192), without / with
                                metrics=BinaryMetricGroup([BinaryAccuracy(), AUC()])

Bound: at n = 65 536 the update reads 0.5 MB and is launch-bound (two launches); at 4 M it is bound by the walk of
the staged samples in LDS (n * 256 bin comparisons), not by the 34 MB it reads."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import keras_rs_amd.layers as kl

T = 200


class TorchComposition:
    """keras' update of AUC(200) and BinaryAccuracy() in torch ops, state on the device."""

    def __init__(self, device):
        self.state = torch.zeros((4, T), device=device)
        self.mean = torch.zeros(2, device=device)

    def update_state(self, y_true, y_pred):
        y_pred = torch.clip(y_pred.float().reshape(-1), 0.0, 1.0)
        y_true = y_true.reshape(-1)
        true_labels = (y_true != 0).float()
        false_labels = 1.0 - true_labels
        bucket = torch.relu(torch.ceil(y_pred * (T - 1)) - 1).to(torch.int64)
        tp_bucket = torch.zeros(T, device=y_pred.device).index_add_(0, bucket, true_labels)     # segment_sum
        fp_bucket = torch.zeros(T, device=y_pred.device).index_add_(0, bucket, false_labels)
        tp = torch.flip(torch.cumsum(torch.flip(tp_bucket, [0]), 0), [0])
        fp = torch.flip(torch.cumsum(torch.flip(fp_bucket, [0]), 0), [0])
        self.state[0] += tp
        self.state[1] += fp
        self.state[2] += false_labels.sum() - fp
        self.state[3] += true_labels.sum() - tp
        match = ((y_pred > 0.5).float() == y_true).float()
        self.mean[0] += match.sum()
        self.mean[1] += match.numel()

    def result(self):
        return {"binary_accuracy": self.mean[0] / self.mean[1], "auc": kl.auc_from_confusion(*self.state)}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in events:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(us[0], 1),
            "p90_us": round(us[int(0.9 * (len(us) - 1))], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["k12", "torch", "step", "step-metrics"], required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"path": args.path, "n": args.n, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    if args.path in ("k12", "torch"):
        gen = torch.Generator(device=dev).manual_seed(0)
        y = (torch.rand(args.n, 1, device=dev, generator=gen) < 0.3).float()
        p = torch.clip(0.35 + 0.25 * y + 0.2 * torch.randn(args.n, 1, device=dev, generator=gen), 0.0, 1.0)
        metrics = (kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()]) if args.path == "k12"
                   else TorchComposition(dev))
        rec.update(timed(lambda: metrics.update_state(y, p), args.steps, args.warmup))
        rec.update({k: round(float(v), 6) for k, v in metrics.result().items()})
    else:
        spec = importlib.util.spec_from_file_location("dlrm_dcn_v2", os.path.join(ROOT, "examples", "dlrm_dcn_v2.py"))
        ex = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ex)
        hots = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]
        model = ex.build_model(args.n, 100_000, hots)
        x, y = ex.synthetic_batch(args.n, 13, 100_000, hots, dev, seed=0)
        box = [None]
        metrics = kl.BinaryMetricGroup([kl.BinaryAccuracy(), kl.AUC()]) if args.path == "step-metrics" else None
        rec.update(timed(lambda: ex.train_step(model, box, x, y, metrics), args.steps, args.warmup))
        if metrics is not None:
            rec.update({k: round(float(v), 6) for k, v in metrics.result().items()})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
