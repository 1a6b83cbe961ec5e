"""K18 against the bf16 krs_gemm: the int8 product (activation quantizer + krs_gemm_q8) and the bf16 product on the same
shape in the same process, at the C3 serving shapes of DESIGN.md section 4 -- the two FeatureCross products (the second
with the cross epilogue) and the four wide top-MLP products, B = 65 536 -- and the whole served model
(examples/dlrm_dcn_v2.py forward, unquantized bf16 tables on both sides) float against int8 Dense / FeatureCross.  Both sides are warmed up first,
then timed in alternating rounds with device events, so that clocks and cache state drift over both alike; the figure of a
side is the median of its rounds, the rounds themselves are reported (development aid).  The int8 time INCLUDES the
activation quantizer.  One JSON line per shape; --out FILE also writes them there."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import dense_ops as D
from keras_rs_amd import embedding_ops as E

B = 65536
SHAPES = [  # name, M, K, N, epilogue: "linear" | "cross" | "relu"
    ("cross_down", B, 3456, 512, "linear"),       # h = x U
    ("cross_up", B, 512, 3456, "cross"),          # x0 * (h K + b) + x
    ("top_3456_1024", B, 3456, 1024, "relu"),
    ("top_1024_1024", B, 1024, 1024, "relu"),
    ("top_1024_512", B, 1024, 512, "relu"),
    ("top_512_256", B, 512, 256, "relu"),
]


def run(fn, n):
    """microseconds per call of n back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(calls, args):
    for fn in calls.values():
        run(fn, args.warmup)
    rounds = {key: [] for key in calls}
    for _ in range(args.rounds):
        for key, fn in calls.items():
            rounds[key].append(run(fn, args.steps))
    return {key: statistics.median(v) for key, v in rounds.items()}, rounds


def product(name, m, k, n, form, args, dev, g):
    x = torch.randn((m, k), device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn((n, k), device=dev, generator=g) / k ** 0.5).to(torch.bfloat16)       # [N, K]: K-contiguous, as served
    bias = torch.randn(n, device=dev, generator=g) * 0.1
    wq, wstep = E.quantize_rows(w)
    kw = {}
    if form == "cross":
        x0 = torch.randn((m, n), device=dev, generator=g).to(torch.bfloat16)
        xr = torch.randn((m, n), device=dev, generator=g).to(torch.bfloat16)
        kw = dict(bias=bias, x0=x0, diag_scale=0.0)
    elif form == "relu":
        kw = dict(bias=bias, act=L.ACT_RELU)
    aq, astep = E.quantize_rows(x)

    def bf16():
        D.gemm(x, w, b_is_nk=True, **(dict(kw, x=xr) if form == "cross" else kw))

    def int8():
        D.gemm_q8(x, wq, wstep, out_dtype=torch.bfloat16, **(dict(kw, x_res=xr) if form == "cross" else kw))

    def int8_product_only():
        D.gemm_q8_prequantized(aq, astep, wq, wstep, out_dtype=torch.bfloat16, **(dict(kw, x_res=xr) if form == "cross" else kw))

    us, rounds = alternate({"bf16": bf16, "int8": int8, "int8_product_only": int8_product_only}, args)
    bf16()
    route_bf16 = D.last_gemm_route()["kernel"]
    int8()
    route_q8 = D.last_gemm_q8_route()["kernel"]
    return {"shape": name, "M": m, "K": k, "N": n, "epilogue": form, "bf16_kernel": route_bf16, "int8_kernel": route_q8,
            "bf16_us": round(us["bf16"], 1), "int8_us": round(us["int8"], 1),
            "int8_product_only_us": round(us["int8_product_only"], 1),
            "bf16_over_int8": round(us["bf16"] / us["int8"], 3),
            "bf16_tflops": round(2.0 * m * n * k / us["bf16"] * 1e-6, 1),
            "int8_tops_product_only": round(2.0 * m * n * k / us["int8_product_only"] * 1e-6, 1),
            **{key + "_rounds_us": [round(v, 1) for v in r] for key, r in rounds.items()}}


def served_model(args, dev):
    """The example's forward, float against int8 Dense / FeatureCross (unquantized bf16 tables on both sides).  The two models are built
    from the same seeds, so they hold the same weights."""
    import keras_rs_amd.layers as kl

    spec = importlib.util.spec_from_file_location("dlrm_dcn_v2", os.path.join(ROOT, "examples", "dlrm_dcn_v2.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    hots = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]
    batch = args.model_batch
    models = [ex.build_model(batch, 100_000, hots) for _ in range(2)]
    x, _ = ex.synthetic_batch(batch, 13, 100_000, hots, dev, seed=99)
    with torch.no_grad():
        for m in models:
            m(x)
        for m in models[1].modules():
            if isinstance(m, (kl.Dense, kl.FeatureCross)):
                m.quantize("int8")
        before, after = models[0](x).float(), models[1](x).float()

        def forward(model):
            def go():
                with torch.no_grad():
                    model(x)
            return go

        us, rounds = alternate({"float": forward(models[0]), "int8": forward(models[1])}, args)
    return {"shape": "served_model", "batch": batch, "float_us": round(us["float"], 1), "int8_us": round(us["int8"], 1),
            "float_over_int8": round(us["float"] / us["int8"], 3),
            "max_abs_prediction_difference": float((before - after).abs().max()),
            **{key + "_rounds_us": [round(v, 1) for v in r] for key, r in rounds.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per side")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-batch", type=int, default=B)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES) + ",served_model")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gemm_q8 needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    wanted = args.shapes.split(",")
    lines = []
    for name, m, k, n, form in SHAPES:
        if name in wanted:
            lines.append(product(name, m, k, n, form, args, dev, g))
            lines[-1].update(steps=args.steps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    if "served_model" in wanted:
        lines.append(served_model(args, dev))
        lines[-1].update(steps=args.steps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
