"""K26 vocabulary lookup: krs_vocab_lookup against the torch composition a user writes without it, in one process,
device events, every point warmed up first, the implementations alternating over --repeats repeats, every timed window
at least --window seconds long (development aid):
  krs      vocab_ops.lookup on the table of the vocabulary (the planner's route, or a forced route / ids per lane);
  torch    torch.searchsorted on the sorted vocabulary, the equality test and the remap through the sort permutation.
Sections (one JSON line per point; --out FILE also writes them there):
  main       vocabularies 2^10 (it would fit the LDS route), 2^20 and 40 M (the largest Criteo vocabulary of bench.py) x 2^16 and 2^22
             int64 ids, drawn uniformly and with bench.py's skew (token of row floor(V u^4));
  ipl        the global route at 1, 2, 4 and 8 ids per lane (vocabularies 2^20 and 40 M, 2^22 uniform ids);
  crossover  vocabulary 2^10, the LDS route against the global route at 2^8 .. 2^16 and 2^22 ids.
Each line carries the median and the fastest repeat's time per call, the bytes the lookup has to move (8 B id read,
8 B index written, one 16 B probe) over the median, and the table's bytes per token."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from keras_rs_amd import _lib as L
from keras_rs_amd import vocab_ops as V

MULT, ADD = 0x9E3779B97F4A7C15 - (1 << 64), 12345      # raw token of row r: r * MULT + ADD modulo 2^64 (MULT is odd)
CRITEO_MAX = 40_000_000


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def measure(fns, args):
    calls = {}
    for name, fn in fns.items():
        for _ in range(args.warmup):
            fn()
        calls[name] = max(args.steps, int(args.window * 1e6 / max(timed(fn, 3), 1.0)) + 1)
    times = {name: [] for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            times[name].append(timed(fn, calls[name]))
    return {name: dict(median_us=round(statistics.median(t), 2), best_us=round(min(t), 2), calls=calls[name])
            for name, t in times.items()}


def make_vocab(v, dev):
    raw = torch.arange(v, device=dev, dtype=torch.int64) * MULT + ADD
    table = V.build_table(raw)
    ordered, perm = torch.sort(raw)
    return raw, table, ordered, perm


def make_ids(raw, n, skew, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    v = raw.numel()
    if skew > 0:
        rows = (torch.rand(n, device=dev, generator=g, dtype=torch.float64).pow(skew) * v).long().clamp_(max=v - 1)
    else:
        rows = torch.randint(0, v, (n,), device=dev, generator=g)
    ids = raw[rows]
    ids[::16] += 1      # one id in 16 is out of the vocabulary
    return ids


def torch_lookup(ordered, perm, ids):
    pos = torch.searchsorted(ordered, ids).clamp_(max=ordered.numel() - 1)
    return torch.where(ordered[pos] == ids, perm[pos] + 1, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--sections", default="main,ipl,crossover")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    sections = args.sections.split(",")
    lines = []

    def emit(rec, n, table, v):
        rec["needed_bytes"] = n * 32
        rec["table_bytes_per_token"] = round((128 + 16 * table.slots) / v, 2)
        for name in rec["times"]:
            rec["times"][name]["needed_gbs"] = round(n * 32 / rec["times"][name]["median_us"] / 1e3, 1)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for v in (1 << 10, 1 << 20, CRITEO_MAX):
        raw, table, ordered, perm = make_vocab(v, dev)
        for n in (1 << 16, 1 << 22):
            for skew in (0.0, 4.0):
                ids = make_ids(raw, n, skew, dev, v + n)
                want = torch_lookup(ordered, perm, ids)
                assert torch.equal(V.lookup(table, ids), want), "krs and torch disagree"
                route = V.last_route()
                if "main" in sections:
                    times = measure({"krs": lambda: V.lookup(table, ids), "torch": lambda: torch_lookup(ordered, perm, ids)},
                                    args)
                    emit(dict(section="main", vocab=v, n=n, skew=skew, route=route.route, ids_per_lane=route.ids_per_lane,
                              blocks=route.blocks, times=times,
                              speedup=round(times["torch"]["median_us"] / times["krs"]["median_us"], 3)), n, table, v)
                if "ipl" in sections and v >= 1 << 20 and n == 1 << 22 and skew == 0.0:
                    fns = {f"ipl{k}": (lambda k=k: V.lookup(table, ids, route_hint=L.VOCAB_GLOBAL, ids_per_lane=k))
                           for k in (1, 2, 4, 8)}
                    emit(dict(section="ipl", vocab=v, n=n, skew=skew, times=measure(fns, args)), n, table, v)
        if "crossover" in sections and v == 1 << 10:
            for n in (1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 22):
                ids = make_ids(raw, n, 0.0, dev, n)
                fns = {"lds": lambda: V.lookup(table, ids, route_hint=L.VOCAB_LDS),
                       "global": lambda: V.lookup(table, ids, route_hint=L.VOCAB_GLOBAL)}
                emit(dict(section="crossover", vocab=v, n=n, times=measure(fns, args)), n, table, v)
        del raw, table, ordered, perm
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
