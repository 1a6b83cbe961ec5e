# kernel trace of the C5 shape (Criteo vocabularies, power-law ids) with L = 1 as the primary leg; the multi-hot leg of the
# same --full run is reported under `also`.  Usage: c5prof.sh OUTDIR
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:?usage: c5prof.sh OUTDIR}
mkdir -p "$OUT"
T=$(mktemp -d)
rocprofv3 --kernel-trace --stats -d "$T" -o b -- python "$R/bench.py" --full --criteo-vocab 40000000 --id-skew 4 --hotness 1 --no-cpu-baseline --steps 10 --warmup 3 > "$OUT/c5_l1_profiled.json" 2>/dev/null
python "$R/scripts/rocpd_stats.py" $(ls "$T"/*/*.db "$T"/*.db 2>/dev/null | head -1) 30 > "$OUT/c5_l1_kernel_stats.md"
head -24 "$OUT/c5_l1_kernel_stats.md" | cut -c1-140
python -c "
import json, sys; d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['ms_per_step'], d['also']['ms_per_step'])" "$OUT/c5_l1_profiled.json"
rm -rf "$T"
