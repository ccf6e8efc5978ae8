#!/bin/bash
# One GPU-box session: parity tests -> bench --full -> rocprofv3 kernel trace of the bench.
# Every GPU step has its own time limit and the chain stops at the first failure.
# Outputs under $OUT (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS=${STEPS:-10}
timeout -k 10 900 python -u -m pytest tests -q -m gpu -x --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { echo "pytest failed"; tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -3 "$OUT/pytest_gpu.log"
if [ "${BENCH:-1}" = "1" ]; then
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 3 --out "$OUT/bench.json" > "$OUT/bench.log" 2>&1 || { echo "bench failed"; tail -30 "$OUT/bench.log"; exit 1; }
tail -4 "$OUT/bench.log"
fi
if [ "${SMOKE:-0}" = "1" ]; then
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo "smoke failed"; tail -30 "$OUT/smoke.log"; exit 1; }
  tail -2 "$OUT/smoke.log"
fi
if [ "${PROFILE:-1}" = "1" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --cpu-baseline 0 > "$OUT/prof.log" 2>&1 || { echo "rocprof failed"; tail -20 "$OUT/prof.log"; exit 1; }
  find "$OUT/prof" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/kernel_stats.csv"
  head -15 "$OUT/kernel_stats.csv"
fi
