"""What a batch with per-question where clauses costs the dense index: the row-list search against
one ordinary filtered search per distinct clause (not a test).

python tools/dense_lists_probe.py [--rows N] [--nq B] [--k K] [--budget-s S]

A store of N unit Gaussian rows of dim 768 and a batch of B Gaussian questions.  For 1, 16 and B
distinct clauses (the questions dealt evenly over them), each allowing about N/1024, N/64, N/8 and
N/4 rows, as a contiguous run and as a scattered (Bernoulli) set:
  * lists  DenseIndex.search_lists over the whole batch, split like GpuVectorStore.query_batch at
           LIST_PAIR_BUDGET (query, allowed row) pairs per call;
  * scans  DenseIndex.search once per distinct clause with the questions that use it: the only way
           a caller had before.
Both run in this process, alternating, after one warm-up each; every figure is a host clock around
calls that end in a device synchronise, median and minimum over the repetitions that fit the
per-configuration time budget (at least 3).  Before timing, the two outputs are compared at the
project's bars: distances within 1e-4, and a differing row only where the two distances are within
1e-5 of each other.  The byte columns are what each route has to read: allowed rows x 4 ld per tile
of 8 questions against N x ld of the int8 plane per scan.  The crossover is the allowed share at
which the two medians meet (log-linear between the measured shares).
"""
import argparse
import math
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "classmate-rag_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from classmate_hip import engine  # noqa: E402
from classmate_hip.retrieval.vector_store import LIST_PAIR_BUDGET, route_clauses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=256)
ap.add_argument("--k", type=int, default=24)
ap.add_argument("--budget-s", type=float, default=1.5, help="timed seconds per route and configuration")
a = ap.parse_args()

D, N, B, K = 768, a.rows // 32 * 32, a.nq, a.k
dev = torch.device("cuda", 0)
idx = engine.DenseIndex(D, capacity=N)
g = torch.Generator(device=dev).manual_seed(1700)
for r0 in range(0, N, 1 << 16):
    x = torch.randn((min(1 << 16, N - r0), D), generator=g, device=dev)
    idx.upsert_dev((x / x.norm(dim=1, keepdim=True)).contiguous(), r0)
torch.cuda.synchronize()
Q = torch.randn((B, D), generator=g, device=dev).cpu().numpy()
print(f"{torch.cuda.get_device_name(0)}: {N} rows x {D}, {B} questions, k = {K}, "
      f"scan kind {idx.search_kind(B, K)} at nq = {B}, {idx.search_kind(16, K)} at 16, {idx.search_kind(1, K)} at 1",
      flush=True)

POW = (1 << torch.arange(32, device=dev, dtype=torch.int64))


def pack(mask):
    """(nc, N) bool on the device -> (nc, N / 32) int32 allow words."""
    w = (mask.view(mask.shape[0], N // 32, 32).to(torch.int64) * POW).sum(dim=2)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).contiguous()   # two's complement words


def clauses(nc, frac, shape, seed):
    m = max(1, int(N * frac))
    if shape == "run":
        start = (torch.arange(nc, device=dev) * 7919 * 131) % (N - m)
        r = torch.arange(N, device=dev)[None, :]
        mask = (r >= start[:, None]) & (r < start[:, None] + m)
    else:
        gg = torch.Generator(device=dev).manual_seed(seed)
        mask = torch.rand((nc, N), generator=gg, device=dev) < frac
    words = pack(mask)
    counts = mask.sum(dim=1).cpu().numpy()
    torch.cuda.synchronize()
    return words, counts


def run_lists(words, counts, filter_of):
    dist = np.zeros((B, K), np.float32)
    rows = np.full((B, K), -1, np.int64)
    plan = route_clauses(filter_of.tolist(), counts.tolist(), N, K, 256, True, 1.0, LIST_PAIR_BUDGET, 0.0)
    assert not plan["scan"] and not plan["empty"] and not plan["plain"]      # every question on the list route
    for call in plan["lists"]:
        sel = [i for _, qs in call for i in qs]
        fo = np.concatenate([np.full(len(qs), f, np.int32) for f, (_, qs) in enumerate(call)])
        gs = [c for c, _ in call]
        d, r = idx.search_lists(Q[sel], K, words[gs] if len(gs) < words.shape[0] else words, fo)
        dist[sel], rows[sel] = d, r
    return dist, rows, len(plan["lists"])


def run_scans(words, filter_of):
    dist = np.empty((B, K), np.float32)
    rows = np.empty((B, K), np.int64)
    for c in range(words.shape[0]):
        sel = np.nonzero(filter_of == c)[0]
        d, r = idx.search(Q[sel], K, words[c])
        dist[sel], rows[sel] = d, r
    return dist, rows


def timed(fn, budget):
    ts = []
    t_end = time.perf_counter() + budget
    while len(ts) < 3 or (time.perf_counter() < t_end and len(ts) < 50):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


print(f"{'clauses':>7} {'share':>7} {'shape':>7} {'rows/cl':>8} {'calls':>5} | {'lists ms med':>12} {'min':>8} {'GB':>7} | "
      f"{'scans ms med':>12} {'min':>8} {'GB':>7} | {'scans/lists':>11} {'max|dd|':>8} {'reps':>9}", flush=True)
FRACS = (1 / 1024, 1 / 64, 1 / 8, 1 / 4)
cross = {}
for nc in (1, 16, B):
    filter_of = (np.arange(B) % nc).astype(np.int32)
    for shape in ("run", "scatter"):
        ratios = []
        for fi, frac in enumerate(FRACS):
            words, counts = clauses(nc, frac, shape, 1800 + fi)
            dl, rl, n_calls = run_lists(words, counts, filter_of)          # warm-up of both, and the comparison
            ds, rs = run_scans(words, filter_of)
            assert ((rl >= 0) == (rs >= 0)).all()
            dd = np.abs(dl - ds)
            assert dd.max() <= 1e-4, dd.max()
            diff = rl != rs
            assert (dd[diff] <= 1e-5).all(), "rows differ beyond a tie"
            tl, tsn = [], []
            for _ in range(2):                                             # two alternating windows per route
                tl += timed(lambda: run_lists(words, counts, filter_of), a.budget_s / 2)
                tsn += timed(lambda: run_scans(words, filter_of), a.budget_s / 2)
            tiles = sum(math.ceil((filter_of == c).sum() / 8) * int(counts[c]) for c in range(nc))
            gb_l, gb_s = tiles * D * 4 / 1e9, nc * N * D / 1e9
            ml, ms_ = np.median(tl), np.median(tsn)
            ratios.append(ms_ / ml)
            print(f"{nc:>7} {frac:>7.5f} {shape:>7} {int(counts.mean()):>8} {n_calls:>5} | {1e3 * ml:>12.3f} "
                  f"{1e3 * min(tl):>8.3f} {gb_l:>7.2f} | {1e3 * ms_:>12.3f} {1e3 * min(tsn):>8.3f} {gb_s:>7.2f} | "
                  f"{ms_ / ml:>11.2f} {dd.max():>8.1e} {len(tl):>4}/{len(tsn):<4}", flush=True)
            del words
        # the share at which the medians meet
        x = None
        if ratios[0] < 1:
            x = "below 1/1024"
        elif ratios[-1] >= 1:
            x = "above 1/4"
        else:
            for j in range(len(FRACS) - 1):
                if ratios[j] >= 1 > ratios[j + 1]:
                    t = math.log(ratios[j]) / (math.log(ratios[j]) - math.log(ratios[j + 1]))
                    f = math.exp(math.log(FRACS[j]) + t * (math.log(FRACS[j + 1]) - math.log(FRACS[j])))
                    x = f"1/{1 / f:.1f}"
                    break
        cross[(nc, shape)] = x
        print(f"  crossover ({nc} clauses, {shape}): allowed share {x}", flush=True)
print("crossovers:", {f"{k[0]}/{k[1]}": v for k, v in cross.items()})
