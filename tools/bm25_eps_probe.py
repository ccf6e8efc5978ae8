"""What the epsilon floors of a batch's clauses cost: BM25Index.filter_eps_multi (up to 32 clauses a
postings pass) against a loop of BM25Index.filter_eps (one pass per clause) (not a test).

timeout -k 10 600 python tools/bm25_eps_probe.py [--docs N] [--reps R] [--filters 1,32,256] [--shares 1024,64]

bench.py's BM25 corpus (gen_tokens: Zipf 1.07 over 2^20 terms, Poisson(120) tokens per document) of
N documents; scattered (Bernoulli) clauses that allow about N/share rows, as device words.  Both run
in this process, alternating repetition by repetition after one warm-up each; every figure is a host
clock around calls that end in a device synchronise, the median (and minimum) over R repetitions.
Before timing, the two outputs are compared for bit equality.
"""
import argparse
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "classmate-rag_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from classmate_hip import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--filters", default="1,32,256")
ap.add_argument("--shares", default="1024,64", help="allowed rows = docs / share")
a = ap.parse_args()

N, V = a.docs // 32 * 32, 1 << 20
dev = torch.device("cuda", 0)
tokens, doc_off = bench.gen_tokens(N, V, 1.07, 120.0, seed=500)
idx = engine.BM25Index(device=0)
idx.build_dev(tokens, doc_off, V)
del tokens, doc_off
torch.cuda.synchronize()
print(f"{torch.cuda.get_device_name(0)}: {N} documents, {idx.num_postings} postings, {a.reps} repetitions", flush=True)

POW = (1 << torch.arange(32, device=dev, dtype=torch.int64))


def clauses(nc, frac, seed):
    gg = torch.Generator(device=dev).manual_seed(seed)
    words = []
    for c0 in range(0, nc, 16):
        mask = torch.rand((min(16, nc - c0), N), generator=gg, device=dev) < frac
        w = (mask.view(mask.shape[0], N // 32, 32).to(torch.int64) * POW).sum(dim=2)
        words.append(torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32))   # two's complement words
    torch.cuda.synchronize()
    return torch.cat(words).contiguous()


print(f"{'filters':>7} {'share':>7} {'passes':>6} | {'multi ms med':>12} {'min':>9} | {'loop ms med':>11} {'min':>9} | "
      f"{'loop/multi':>10} | {'loop ms/filter':>14}", flush=True)
for nf in [int(x) for x in a.filters.split(",")]:
    for share in [int(x) for x in a.shares.split(",")]:
        words = clauses(nf, 1.0 / share, 1800 + share)
        got = idx.filter_eps_multi(words)                                    # warm-up of both, and the comparison
        passes = idx.last_eps_passes()
        want = np.asarray([idx.filter_eps(w) for w in words])
        assert (got == want).all(), "the epsilons differ"
        tm, tl = [], []
        for _ in range(a.reps):                                              # alternating
            t0 = time.perf_counter()
            idx.filter_eps_multi(words)
            t1 = time.perf_counter()
            for w in words:
                idx.filter_eps(w)
            t2 = time.perf_counter()
            tm.append(t1 - t0)
            tl.append(t2 - t1)
        mm, ml = np.median(tm), np.median(tl)
        print(f"{nf:>7} {'1/' + str(share):>7} {passes:>6} | {1e3 * mm:>12.3f} {1e3 * min(tm):>9.3f} | "
              f"{1e3 * ml:>11.3f} {1e3 * min(tl):>9.3f} | {ml / mm:>10.2f} | {1e3 * ml / nf:>14.3f}", flush=True)
        del words
