#!/bin/bash
# Per-kernel times of one short bench with every leg (rocprofv3 kernel trace + stats).
# Results go to $OUT (default: bench_out).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/kprof" -o run -- \
    python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > "$OUT/kprof.log" 2>&1 || exit $?
f=$(find "$OUT/kprof" -name "*kernel_stats.csv" | head -1)
cp "$f" "$OUT/kernel_stats.csv"
python - "$OUT/kernel_stats.csv" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    print(f'{r["Name"].split("(")[0][:48]:48s} calls={r["Calls"]:>4s} avg_ms={float(r["AverageNs"])/1e6:9.4f}')
PY
