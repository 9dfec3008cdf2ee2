#!/bin/bash
# End-of-round pass: the whole GPU suite, the bench line with every leg (--full), the
# rocprofv3 kernel stats and the FETCH/WRITE PMC passes of the bench (gpu_round3.sh steps).
# Logs go to $OUT (default: bench_out).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
V=${V:-final}
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider \
    > "$OUT/pytest_gpu_$V.log" 2>&1 || { tail -20 "$OUT/pytest_gpu_$V.log"; exit 1; }
tail -2 "$OUT/pytest_gpu_$V.log"
timeout -k 10 400 python -u bench.py --full > "$OUT/bench_$V.log" 2>&1 || { tail -20 "$OUT/bench_$V.log"; exit 1; }
tail -c 600 "$OUT/bench_$V.log"
STEPS=rocprof,pmc bash scripts/gpu_round3.sh > "$OUT/prof_$V.log" 2>&1 || { tail -20 "$OUT/prof_$V.log"; exit 1; }
grep "rc=" "$OUT/prof_$V.log"
