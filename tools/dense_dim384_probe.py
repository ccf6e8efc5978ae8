#!/usr/bin/env python3
"""The ld-384 int8 route (K1q-s with 3 chunks per tile, cm_dense.hip dense_kind / coarse_config)
against the f16 routes the same store ran before it existed, on one MI355X -> profiles/dense_dim384.txt.

Shape: --rows x 384 Gaussian unit rows (generated on the device in seeded chunks), Gaussian queries,
k = 24.  Batches of 1, 16 and 32 queries: the int8 route (automatic) against K1s (set_path(4)).
Batches of 64 and 256: a forced K1q-s (set_path(6), one stream pass per 32 queries) against K1c
(automatic there).

Method: one index, one process.  Per batch size the two routes are first compared with each other
(rows equal up to ties within 1e-5 of the k-th distance, distances within 1e-4); then, after a
warm-up, the two alternate, every call through the device entry with a caller workspace and ended by
a synchronise inside a host clock; --runs series of --reps repetitions, the median of each series,
and over the series the median and max - min of those medians (the f16 route's max - min is the
spread a difference has to exceed).  The counters (band rows, wide re-ranks, exact re-runs) are read
from the int8 route's workspace outside the clock; the scan kernels' own time comes from the index's
event timer (cm_dense_timing: the events span every pass's scan launch of a search) in a separate
series per route, and its fraction of the 8 TB/s HBM peak counts the bytes that route's scan reads:
int8 passes x rows x (384 + 8), K1s rows x 768, K1c ceil(B / 256) x rows x 768.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "classmate-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIM, K, CHUNK, HBM_PEAK = 384, 24, 1 << 18, 8.0e12
STREAM, COARSE, Q8S, SQ = 4, 3, 6, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16, 32, 64, 256])
    ap.add_argument("--out", default="bench_out/dense_dim384.txt")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from classmate_hip import engine

    dev = torch.device("cuda", 0)
    idx = engine.DenseIndex(DIM, capacity=a.rows)
    for c, r0 in enumerate(range(0, a.rows, CHUNK)):
        g = torch.Generator(device=dev).manual_seed(1_000_003 + c)
        x = torch.randn(min(CHUNK, a.rows - r0), DIM, device=dev, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        idx.upsert_dev(x.contiguous(), r0)
        del x
    torch.cuda.synchronize()
    gq = torch.Generator(device=dev).manual_seed(99)
    Q = torch.randn(max(a.batches), DIM, device=dev, generator=gq)
    mem = idx.mem_stats()["bytes"]
    lines = [f"{a.tag}rows {a.rows} x {DIM}, k {K}, reps {a.reps}, runs {a.runs}; row arrays {mem / 1e9:.2f} GB "
             f"(fp32 {a.rows * DIM * 4 / 1e9:.2f}, f16 {a.rows * DIM * 2 / 1e9:.2f}, int8 {a.rows * DIM / 1e9:.2f}, "
             f"the rest metadata)"]

    def run(B, kind, ws, out):
        idx.set_path(kind)
        try:
            return idx.search_dev(Q[:B].contiguous(), K, out=out, workspace=ws)
        finally:
            idx.set_path(0)

    for B in a.batches:
        small = B <= SQ
        # (forced kind, the kind it must resolve to): the int8 route, and the route of the parent commit
        kinds = {"int8": (0 if small else Q8S, Q8S), "f16": (STREAM, STREAM) if small else (0, COARSE)}
        f16_name = "K1s" if small else "K1c"
        ws, outb, res = {}, {}, {}
        for n, (kind, want) in kinds.items():
            idx.set_path(kind)
            assert idx.search_kind(B, K) == want, (B, n, idx.search_kind(B, K))
            ws[n] = torch.empty(idx.workspace_bytes(B, K), dtype=torch.uint8, device=dev)
            idx.set_path(0)
            outb[n] = (torch.empty((B, K), dtype=torch.float32, device=dev),
                       torch.empty((B, K), dtype=torch.int64, device=dev))
            for _ in range(3):                          # correctness first (also the warm-up)
                run(B, kind, ws[n], outb[n])
            torch.cuda.synchronize()
            res[n] = (outb[n][0].cpu().numpy().copy(), outb[n][1].cpu().numpy().copy())
        idx.set_path(kinds["int8"][0])                  # the counters sit where that kind's workspace layout puts them
        stats = (idx.workspace_band_rows(B, K, ws["int8"]), idx.workspace_wide_reranks(B, K, ws["int8"]),
                 idx.workspace_fallbacks(B, K, ws["int8"]))
        idx.set_path(0)
        (d8, r8), (d1, r1) = res["int8"], res["f16"]
        assert np.abs(d8 - d1).max() <= 1e-4, float(np.abs(d8 - d1).max())
        for j in range(B):
            diff = set(r8[j].tolist()) ^ set(r1[j].tolist())
            near = {int(r) for dd, rr in ((d8, r8), (d1, r1)) for r, x in zip(rr[j], dd[j]) if abs(x - d1[j, K - 1]) < 1e-5}
            assert diff <= near, (B, j, diff)
        meds = {n: [] for n in kinds}
        for _ in range(a.runs):
            ts = {n: [] for n in kinds}
            for _ in range(a.reps):                     # alternating
                for n, (kind, _w) in kinds.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(B, kind, ws[n], outb[n])
                    torch.cuda.synchronize()
                    ts[n].append((time.perf_counter() - t0) * 1e3)
            for n in kinds:
                meds[n].append(statistics.median(ts[n]))
        scan_ms = {}
        for n, (kind, _w) in kinds.items():             # the scan launches' own time, a series of its own
            idx.timing(True)
            for _ in range(a.reps):
                run(B, kind, ws[n], outb[n])
            scan = idx.timing_drain()
            idx.timing(False)
            scan_ms[n] = statistics.median(scan) if scan else float("nan")
        passes = -(-B // SQ)
        byts = {"int8": passes * a.rows * (DIM + 8), "f16": (1 if small else -(-B // 256)) * a.rows * DIM * 2}
        frac = {n: byts[n] / (scan_ms[n] * 1e-3) / HBM_PEAK for n in kinds}
        m8, m1 = statistics.median(meds["int8"]), statistics.median(meds["f16"])
        spread = max(meds["f16"]) - min(meds["f16"])
        verdict = "int8 ahead by more than the spread" if m1 - m8 > spread else "int8 NOT ahead by more than the spread"
        fmt = lambda v: " / ".join(f"{x:.3f}" for x in v)
        lines.append(f"{a.tag}B {B:3d}  int8 {m8:7.3f} ms (runs {fmt(meds['int8'])})  {f16_name} {m1:7.3f} ms "
                     f"(runs {fmt(meds['f16'])}; max - min {spread:.3f})  {f16_name} / int8 {m1 / m8:5.2f}x: {verdict}")
        lines.append(f"{a.tag}       passes {passes}  int8 scan {scan_ms['int8']:.3f} ms = {frac['int8']:.2f} of HBM peak on its "
                     f"{byts['int8'] / 1e6:.0f} MB  {f16_name} scan {scan_ms['f16']:.3f} ms = {frac['f16']:.2f} on its "
                     f"{byts['f16'] / 1e6:.0f} MB  band rows {stats[0] / B:.0f}/query  wide re-ranks {stats[1]}  "
                     f"exact re-runs {stats[2]}  workspace {ws['int8'].numel() / 1e6:.0f} MB")
        del ws, outb
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    idx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
