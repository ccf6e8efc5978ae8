#!/usr/bin/env python3
"""CPU model (numpy, no GPU) of K1q's certified band on anisotropic rows, with and without a centre
for the int8 plane (cm_dense_set_center; DESIGN "Centred int8 plane").  Beside tools/int8_band.py,
which asked the same question for isotropic rows on the GPU.

The model is not the kernels.  It follows their arithmetic where the band depends on it:
  * rows xn = fp32-normalised, y = fl32(xn - mu) (mu = 0: the plain plane);
  * the real scale-group geometry (q8_group_row: group G = rows 64 (G >> 2) + 16 (i >> 2) +
    4 (G & 3) + (i & 3)): one scale S per group, codes rint(y / S), e_r = ||y - S q8|| per row,
    and the scans' per-row bound taken with the group's largest e_r, as their epilogues do;
  * queries quantised with their own scale, a_q = max||x~|| e_q + 4e-6 (+ 5e-7 with a centre),
    b_q = ||qn||, coarse distance d~ = (1 - mu.qn) - q~.x~, bound E_r = a_q + b_q e_r;
  * seed = the k-th exact distance of the first 1 / sample rows + 2e-3 (the f16 sample pass's
    bound is ~1e-3: a stand-in, not its arithmetic);
  * candidates = rows with lo <= seed; kth_up = the k-th smallest up among them; the band from
    kth_up = rows with lo <= kth_up; the pilot bound = the k-th exact distance of the k rows with the
    smallest up, band = rows with lo <= it.
It asserts |d - d~| <= E_r for every (row, query) pair with the row's own e_r.

`model()` is importable (tests/test_gpu_dense_center.py runs it on its own arrays before it asks the
GPU); the command line prints the table of profiles/dense_center_model.txt.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

DIM = 768


def aniso_rows(n, dim, a, seed, m_seed=7):
    """normalize(sqrt(a) m + sqrt(1 - a) u_i), u_i uniform unit vectors, m one fixed unit vector:
    pairwise cosine ~ a.  fp32."""
    rng = np.random.default_rng([seed, int(round(a * 1000))])
    m = np.random.default_rng(m_seed).standard_normal(dim)
    m /= np.linalg.norm(m)
    out = np.empty((n, dim), np.float32)
    for r0 in range(0, n, 1 << 15):
        u = rng.standard_normal((min(1 << 15, n - r0), dim))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x = np.sqrt(a) * m + np.sqrt(1.0 - a) * u
        out[r0:r0 + u.shape[0]] = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return out


def group_of(rows):
    return (rows >> 6) * 4 + ((rows >> 2) & 3)


def quantise_rows(C, mu):
    """-> (x~ fp32 (n, dim), e_r (n,), group E per row (n,), max ||x~||) under the group geometry.
    Every row is live."""
    n, dim = C.shape
    c = C.astype(np.float32)
    inv = (1.0 / (np.sqrt((c.astype(np.float64) ** 2).sum(1)) + 1e-30)).astype(np.float32)
    xn = c * inv[:, None]
    centred = mu is not None
    y = xn - mu.astype(np.float32)[None, :] if centred else xn
    zero = (np.abs(xn).max(1) == 0) if centred else np.zeros(n, bool)
    rows = np.arange(n, dtype=np.int64)
    G = group_of(rows)
    nG = int(G.max()) + 1
    amax = np.abs(y).max(1)
    amax[zero] = 0.0
    gmax = np.zeros(nG, np.float32)
    np.maximum.at(gmax, G, amax)
    S = np.where(gmax > 0, gmax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    q8 = np.clip(np.rint(y / S[G][:, None]), -127, 127)
    q8[zero] = 0
    xt = (S[G][:, None].astype(np.float64) * q8)
    err = np.where(zero[:, None], np.broadcast_to(mu if centred else 0.0, y.shape), y.astype(np.float64) - xt)
    e_r = np.sqrt((err ** 2).sum(1)) * (1 + 1e-6)
    gE = np.zeros(nG)
    np.maximum.at(gE, G, e_r)     # (a cut tile's never-written rows are dead: e_r = 0, dense_q8_group_kernel)
    nmax = float(np.sqrt((xt ** 2).sum(1)).max()) * (1 + 1e-6)
    return xt.astype(np.float32), e_r, gE[G], nmax, xn


def model(C, Q, k, mu=None, sample=16, range_rows=192, seed_margin=2e-3, check=True):
    """Per query: candidates, their largest count in one `range_rows` range (the 128-slot buffers),
    the band from kth_up and the band at the pilot bound."""
    n = C.shape[0]
    xt, e_r, gE, nmax, xn = quantise_rows(C, mu)
    q = Q.astype(np.float32)
    qinv = (1.0 / (np.sqrt((q * q).sum(1, dtype=np.float32)) + np.float32(1e-30))).astype(np.float32)
    qn = q * qinv[:, None]
    sq = np.abs(qn).max(1) / np.float32(127.0)
    qt = (np.clip(np.rint(qn / sq[:, None]), -127, 127) * sq[:, None]).astype(np.float64)
    e_q = np.sqrt(((qn.astype(np.float64) - qt) ** 2).sum(1)) * (1 + 1e-6)
    a_q = nmax * e_q * (1 + 1e-6) + (4e-6 + 5e-7 if mu is not None else 4e-6)
    b_q = np.sqrt((qn.astype(np.float64) ** 2).sum(1)) * (1 + 1e-6)
    base = 1.0 - (qn.astype(np.float64) @ mu.astype(np.float64) if mu is not None else 0.0)
    # exact distances as the fp64 re-rank forms them
    Cn = C.astype(np.float64)
    Cn /= np.maximum(np.linalg.norm(Cn, axis=1, keepdims=True), 1e-300)
    Qn = Q.astype(np.float64)
    Qn /= np.linalg.norm(Qn, axis=1, keepdims=True)
    out = {"cand": [], "cand_range_max": [], "band_kth_up": [], "band_pilot": []}
    xt64 = xt.astype(np.float64)
    for i in range(Q.shape[0]):
        d = 1.0 - Cn @ Qn[i]
        dc = base[i] - xt64 @ qt[i] if mu is not None else 1.0 - xt64 @ qt[i]
        if check:
            worst = np.abs(d - dc) - (a_q[i] + b_q[i] * e_r)
            assert worst.max() <= 0, ("bound violated", i, float(worst.max()))
        E = a_q[i] + b_q[i] * gE
        lo, up = dc - E, dc + E + 1e-6
        seed = np.partition(d[:max(n // sample, k)], k - 1)[k - 1] + seed_margin
        cand = lo <= seed
        nc = int(cand.sum())
        out["cand"].append(nc)
        per = np.add.reduceat(cand.astype(np.int64), np.arange(0, n, range_rows))
        out["cand_range_max"].append(int(per.max()))
        kth_up = np.partition(up[cand], k - 1)[k - 1] if nc >= k else np.inf
        out["band_kth_up"].append(int((lo[cand] <= kth_up).sum()))
        idx = np.nonzero(cand)[0]
        best = idx[np.argsort(up[idx], kind="stable")[:k]]
        pilot = np.sort(d[best])[min(k, best.size) - 1] if best.size >= k else np.inf
        out["band_pilot"].append(int((lo[cand] <= min(pilot, kth_up)).sum()))
    return {key: np.asarray(v) for key, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[40_000, 200_000])
    ap.add_argument("--a", type=float, nargs="*", default=[0.0, 0.5, 0.8, 0.9])
    ap.add_argument("--nq", type=int, default=16)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# tools/int8_band_center.py: CPU model of K1q's band, real scale-group geometry (q8_group_row)",
             f"# dim {DIM}, k {a.k}, {a.nq} queries drawn like the rows; mean (max) per query; ranges of 192 rows",
             "# rows    a    plane    candidates        per-range max   band from kth_up   band at the pilot bound"]
    for n in a.rows:
        for al in a.a:
            C = aniso_rows(n + a.nq, DIM, al, seed=n)
            C, Q = C[:n], C[n:]
            Cn = C.astype(np.float64)
            mu = Cn.mean(0).astype(np.float32)
            for name, m in (("plain", None), ("centred", mu)):
                r = model(C, Q, a.k, m)
                lines.append(f"{n:7d}  {al:.1f}  {name:8s} {r['cand'].mean():9.0f} ({r['cand'].max():6d})  "
                             f"{r['cand_range_max'].max():6d}  {r['band_kth_up'].mean():9.0f} ({r['band_kth_up'].max():6d})  "
                             f"{r['band_pilot'].mean():9.0f} ({r['band_pilot'].max():6d})")
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
