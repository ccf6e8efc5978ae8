#!/bin/bash
# GPU: bench --full under rocprofv3 kernel trace -> $OUT/bench_kernel_stats.csv (+ the bench JSON line);
# $OUT defaults to bench_out/
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/benchprof" -o bench --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --out "$OUT/bench_prof.json" > "$OUT/bench_prof.log" 2>&1 || { tail -20 "$OUT/bench_prof.log"; exit 1; }
grep "\[bench\]" "$OUT/bench_prof.log" | tail -3
f=$(find "$OUT/benchprof" -name '*kernel_stats.csv' | head -1); cp "$f" "$OUT/bench_kernel_stats.csv"
python3 - "$OUT/bench_kernel_stats.csv" <<'PY'
import csv
import sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: -float(r['TotalDurationNs']))
for r in rows[:40]:
    print(f"{r['Name'][:80]:80s} calls={r['Calls']:>5s} avg_us={float(r['AverageNs'])/1e3:9.1f} tot_ms={float(r['TotalDurationNs'])/1e6:8.2f}")
PY
