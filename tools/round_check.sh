#!/bin/bash
# GPU: the whole check of a tree (pytest -m gpu, smoke, bench --full) + a rocprofv3 summary of the bench.
# Outputs under $OUT (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/.."; export OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -1 "$OUT/pytest_gpu.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -1 "$OUT/smoke.log"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.log" 2>&1 || { tail -20 "$OUT/bench.log"; exit 1; }
grep "\[bench\] 10" "$OUT/bench.log"; tail -1 "$OUT/bench.log" > "$OUT/bench.json"
bash tools/bench_prof.sh > "$OUT/bench_prof_summary.txt" 2>&1 || { tail -5 "$OUT/bench_prof_summary.txt"; exit 1; }
head -3 "$OUT/bench_prof_summary.txt"
