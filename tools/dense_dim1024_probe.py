#!/usr/bin/env python3
"""The ld-1024 int8 route (K1q-s in passes of 32 queries, cm_dense.hip dense_kind / coarse_config)
against the exact fp32 scan on the same store, on one MI355X -> profiles/dense_dim1024.txt.

Shape: --rows x 1024 Gaussian unit rows (generated on the device in seeded chunks), Gaussian queries,
k = 24, batches of 1, 16, 32, 64 and 256 queries.

Method: one index, one process.  Per batch size the automatic kind (the int8 stream) and the forced
fp32 kind (set_path(1), what every ld-1024 search ran before the route existed) are first compared
with each other (rows equal up to ties within 1e-5 of the k-th distance, distances within 1e-4);
then, after a warm-up, the two alternate, every call through the device entry with a caller workspace
and ended by a synchronise inside a host clock; medians of --reps repetitions.  The counters (band
rows, wide re-ranks, exact re-runs) are read from the workspace outside the clock; the scan kernels'
own time comes from the index's event timer (cm_dense_timing: the events span every pass's scan
launch of a search) in a separate series, and its fraction of the 8 TB/s HBM peak counts the int8
plane and its row metadata once per pass: passes x rows x (1024 + 8) bytes.
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

DIM, K, CHUNK, HBM_PEAK = 1024, 24, 1 << 18, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16, 32, 64, 256])
    ap.add_argument("--out", default="bench_out/dense_dim1024.txt")
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
    lines = [f"{a.tag}rows {a.rows} x {DIM}, k {K}, reps {a.reps}; row arrays {mem / 1e9:.2f} GB "
             f"(fp32 {a.rows * DIM * 4 / 1e9:.2f}, int8 {a.rows * DIM / 1e9:.2f}, the rest f16 prefix + metadata)"]

    def run(B, kind, ws, out):
        idx.set_path(kind)
        try:
            return idx.search_dev(Q[:B].contiguous(), K, out=out, workspace=ws)
        finally:
            idx.set_path(0)

    for B in a.batches:
        kinds = {"int8": 0, "fp32": 1}
        assert idx.search_kind(B, K) == 6, idx.search_kind(B, K)
        ws, outb, res = {}, {}, {}
        for n, kind in kinds.items():
            idx.set_path(kind)
            ws[n] = torch.empty(idx.workspace_bytes(B, K), dtype=torch.uint8, device=dev)
            idx.set_path(0)
            outb[n] = (torch.empty((B, K), dtype=torch.float32, device=dev),
                       torch.empty((B, K), dtype=torch.int64, device=dev))
            for _ in range(3):                          # correctness first (also the warm-up)
                run(B, kind, ws[n], outb[n])
            torch.cuda.synchronize()
            res[n] = (outb[n][0].cpu().numpy().copy(), outb[n][1].cpu().numpy().copy())
        stats = (idx.workspace_band_rows(B, K, ws["int8"]), idx.workspace_wide_reranks(B, K, ws["int8"]),
                 idx.workspace_fallbacks(B, K, ws["int8"]))
        (d8, r8), (d1, r1) = res["int8"], res["fp32"]
        assert np.abs(d8 - d1).max() <= 1e-4, float(np.abs(d8 - d1).max())
        for j in range(B):
            diff = set(r8[j].tolist()) ^ set(r1[j].tolist())
            near = {int(r) for dd, rr in ((d8, r8), (d1, r1)) for r, x in zip(rr[j], dd[j]) if abs(x - d1[j, K - 1]) < 1e-5}
            assert diff <= near, (B, j, diff)
        ts = {n: [] for n in kinds}
        for _ in range(a.reps):                         # alternating
            for n, kind in kinds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(B, kind, ws[n], outb[n])
                torch.cuda.synchronize()
                ts[n].append((time.perf_counter() - t0) * 1e3)
        idx.timing(True)                                # the scan launches' own time, a series of its own
        for _ in range(a.reps):
            run(B, 0, ws["int8"], outb["int8"])
        scan = idx.timing_drain()
        idx.timing(False)
        scan_ms = statistics.median(scan) if scan else float("nan")
        passes = -(-B // 32)
        frac = passes * a.rows * (DIM + 8) / (scan_ms * 1e-3) / HBM_PEAK
        m8, m1 = statistics.median(ts["int8"]), statistics.median(ts["fp32"])
        lines.append(f"{a.tag}B {B:3d}  int8 route {m8:8.3f} ms (min {min(ts['int8']):.3f})  exact fp32 {m1:8.3f} ms "
                     f"(min {min(ts['fp32']):.3f})  ratio {m1 / m8:5.2f}x  passes {passes}  scan {scan_ms:.3f} ms "
                     f"= {frac:.2f} of HBM peak on the int8 bytes  band rows {stats[0] / B:.0f}/query  "
                     f"wide re-ranks {stats[1]}  exact re-runs {stats[2]}  workspace {ws['int8'].numel() / 1e6:.0f} MB")
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
