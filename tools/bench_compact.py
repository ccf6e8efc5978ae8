"""GPU: time DenseIndex.compact() on a store with deleted rows, split by HIP events into its three
device phases (rank, move, plane rebuild + tail -- the pairs cm_dense_timing records around them),
next to a device-to-device hipMemcpyAsync of as many bytes as the move reads, in the same process.

The move reads every row from the first dead row on twice and writes it twice (gather into staging,
copy staging to its place), the memcpy reads and writes its bytes once: both rates count bytes read
+ written.  Prints one JSON line.
  python tools/bench_compact.py --rows 1000000 --dim 768 --dead 0.25 --reps 3
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "classmate-rag_amd"))


def build(engine, torch, rows, dim, dead_frac, seed):
    idx = engine.DenseIndex(dim, capacity=rows)
    g = torch.Generator(device="cuda").manual_seed(seed)
    per = 125_000
    for r0 in range(0, rows, per):
        x = torch.randn(min(per, rows - r0), dim, device="cuda", generator=g)
        x /= x.norm(dim=1, keepdim=True)
        idx.upsert_dev(x, r0)
        torch.cuda.synchronize()
        del x
    dead = np.nonzero(np.random.default_rng(seed).random(rows) < dead_frac)[0].astype(np.int64)
    idx.delete(dead)
    return idx, dead


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dead", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    from classmate_hip import engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_compact needs a GPU")

    warm, _ = build(engine, torch, 4096, a.dim, 0.25, a.seed)      # loads the kernels
    warm.compact()
    warm.close()

    ld = -(-a.dim // 128) * 128
    row_b = ld * 4 + 4                                             # an fp32 row and its norm
    runs = []
    for rep in range(a.reps):
        idx, dead = build(engine, torch, a.rows, a.dim, a.dead, a.seed + rep)
        n_live = a.rows - dead.shape[0]
        moved = n_live - int(dead[0]) if dead.shape[0] else 0      # new rows from the first dead row on
        bytes0 = idx.mem_stats()["bytes"]
        idx.timing(True)
        t0 = time.perf_counter()
        m = idx.compact(expect_live=n_live)
        wall = time.perf_counter() - t0
        ms = idx.timing_drain()
        idx.timing(False)
        assert m.shape[0] == n_live == idx.size and len(ms) == 3, (m.shape, n_live, idx.size, ms)
        idx.close()
        # the copy the move is compared with: as many bytes as the move reads, device to device
        nbytes = 2 * moved * row_b
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        dst.copy_(src)
        torch.cuda.synchronize()
        cp = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)                                         # contiguous, same device: hipMemcpyAsync
            e1.record()
            torch.cuda.synchronize()
            cp.append(e0.elapsed_time(e1))
        del src, dst
        cp_ms = statistics.median(cp)
        runs.append(dict(rank_ms=ms[0], move_ms=ms[1], planes_ms=ms[2], wall_ms=wall * 1e3, moved_rows=moved,
                         move_GBps=4 * moved * row_b / (ms[1] * 1e6), memcpy_ms=cp_ms,
                         memcpy_GBps=2 * nbytes / (cp_ms * 1e6), bytes_before=bytes0))
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    print(json.dumps(dict(bench="compact", device=torch.cuda.get_device_name(0), rows=a.rows, dim=a.dim,
                          dead_frac=a.dead, reps=a.reps, median=med,
                          move_over_memcpy=med["move_GBps"] / med["memcpy_GBps"], runs=runs)))


if __name__ == "__main__":
    main()
