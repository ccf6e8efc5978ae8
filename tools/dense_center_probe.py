#!/usr/bin/env python3
"""Centred int8 plane on one MI355X: what the centre (cm_dense_set_center) does to the K1q / K1q-s
search on anisotropic rows, in time, band rows and fallbacks -> profiles/dense_center.txt.

Rows: normalize(sqrt(a) m + sqrt(1 - a) u_i), u_i uniform unit vectors, pairwise cosine ~ a (the
generator of tools/int8_band_center.py, here on the device in seeded chunks); queries drawn the same
way.  Cells: rows x a, each with B = 256 (K1q) and B = 16 (K1q-s), k = 24.

Method: one process per cell holds a plain and a centred index of the same rows.  Both are checked
against an fp64 oracle (torch GEMMs over the regenerated chunks) first; then, after a warm-up, plain
and centred searches alternate, every call through the device entry with a caller workspace and
ended by a synchronise inside a host clock; medians of --reps repetitions.  The counters
(band rows, wide re-ranks, exact fallbacks) are read from the workspace outside the clock.
mean() and set_center() are timed the same way on the centred index.

Without --cell the tool runs every cell in a child process of its own under a time limit and stops
at the first that fails.
"""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "classmate-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIM, K, CHUNK = 768, 24, 1 << 18


def chunk_rows(torch, dev, m_dir, a, seed, c, n):
    g = torch.Generator(device=dev).manual_seed(seed * 100_003 + c)
    u = torch.randn(n, DIM, device=dev, generator=g)
    u /= u.norm(dim=1, keepdim=True)
    x = (a ** 0.5) * m_dir + ((1.0 - a) ** 0.5) * u
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def cell(rows: int, a: float, reps: int, out: Path):
    import numpy as np
    import torch
    from classmate_hip import engine

    dev = torch.device("cuda", 0)
    gm = torch.Generator(device=dev).manual_seed(7)
    m_dir = torch.randn(DIM, device=dev, generator=gm)
    m_dir /= m_dir.norm()
    Q = chunk_rows(torch, dev, m_dir, a, 991, 0, 256)
    plain, cent = engine.DenseIndex(DIM, capacity=rows), engine.DenseIndex(DIM, capacity=rows)
    best_d = torch.empty((256, 0), dtype=torch.float64, device=dev)
    best_r = torch.empty((256, 0), dtype=torch.int64, device=dev)
    Qd = Q.double()
    Qd /= Qd.norm(dim=1, keepdim=True)
    for c, r0 in enumerate(range(0, rows, CHUNK)):
        x = chunk_rows(torch, dev, m_dir, a, 17, c, min(CHUNK, rows - r0))
        plain.upsert_dev(x, r0)
        cent.upsert_dev(x, r0)
        xd = x.double()
        d = 1.0 - (Qd @ xd.T) / xd.norm(dim=1)[None, :]
        v, ix = torch.topk(d, K + 16, dim=1, largest=False)
        best_d, best_r = torch.cat([best_d, v], 1), torch.cat([best_r, ix + r0], 1)
        o = torch.sort(best_d, dim=1, stable=True).indices[:, :K + 16]
        best_d, best_r = torch.gather(best_d, 1, o), torch.gather(best_r, 1, o)
        del x, xd, d
    torch.cuda.synchronize()
    o_d, o_r = best_d.cpu().numpy(), best_r.cpu().numpy()

    def timed(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    cent.mean()
    t_mean = timed(cent.mean, 5)
    mu = cent.mean()
    cent.set_center(mu)
    t_set = timed(lambda: cent.set_center(mu), 5)
    alloc = -(-rows // 128) * 128
    moved = alloc * (DIM * 4 + 4 + DIM + 8)          # fp32 row + invc read, codes + rmeta written
    lines = [f"rows {rows} a {a}: |mean| {float(np.linalg.norm(mu)):.4f}; mean() {t_mean:.2f} ms "
             f"({rows * DIM * 4 / t_mean / 1e6:.0f} GB/s of fp32 rows); set_center {t_set:.2f} ms, "
             f"{moved / 1e9:.2f} GB moved ({moved / t_set / 1e6:.0f} GB/s)"]

    for B in (256, 16):
        q = Q[:B].contiguous()
        ws = {n: torch.empty(i.workspace_bytes(B, K), dtype=torch.uint8, device=dev)
              for n, i in (("plain", plain), ("centred", cent))}
        idx = {"plain": plain, "centred": cent}
        outb = {n: (torch.empty((B, K), dtype=torch.float32, device=dev),
                    torch.empty((B, K), dtype=torch.int64, device=dev)) for n in idx}
        stats = {}
        for n, i in idx.items():                      # correctness first (also the warm-up)
            for _ in range(3):
                d, r = i.search_dev(q, K, out=outb[n], workspace=ws[n])
            torch.cuda.synchronize()
            d, r = d.cpu().numpy(), r.cpu().numpy()
            assert np.abs(d - o_d[:B, :K]).max() <= 1e-4, (n, B, float(np.abs(d - o_d[:B, :K]).max()))
            for j in range(B):                        # the set, up to ties within 1e-5 of the k-th distance
                unsure = set(o_r[j][np.abs(o_d[j] - o_d[j, K - 1]) < 1e-5].tolist())
                assert set(r[j].tolist()) ^ set(o_r[j, :K].tolist()) <= unsure, (n, B, j)
            stats[n] = (i.workspace_band_rows(B, K, ws[n]), i.workspace_wide_reranks(B, K, ws[n]),
                        i.workspace_fallbacks(B, K, ws[n]))
        ts = {n: [] for n in idx}
        for _ in range(reps):                         # alternating
            for n, i in idx.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                i.search_dev(q, K, out=outb[n], workspace=ws[n])
                torch.cuda.synchronize()
                ts[n].append((time.perf_counter() - t0) * 1e3)
        for n in idx:
            b, w, fb = stats[n]
            lines.append(f"rows {rows} a {a} B {B:3d} {n:8s} search {statistics.median(ts[n]):8.3f} ms "
                         f"(min {min(ts[n]):.3f})  band rows {b} ({b / B:.0f}/query)  wide re-ranks {w}  "
                         f"exact fallbacks {fb}  kind {i.search_kind(B, K)}")
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    plain.close()
    cent.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--a", type=float, nargs="*", default=[0.0, 0.5, 0.8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="bench_out/dense_center.txt")
    ap.add_argument("--cell", action="store_true", help="run the one (rows, a) cell given, in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per cell")
    a = ap.parse_args()
    if a.cell:
        cell(a.rows[0], a.a[0], a.reps, Path(a.out))
        return 0
    for rows in a.rows:
        for al in a.a:
            cmd = [sys.executable, __file__, "--cell", "--rows", str(rows), "--a", str(al), "--reps", str(a.reps),
                   "--out", a.out]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print(f"cell rows {rows} a {al}: over its {a.limit} s limit; stopping", flush=True)
                return 124
            if rc != 0:
                print(f"cell rows {rows} a {al}: exit {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
