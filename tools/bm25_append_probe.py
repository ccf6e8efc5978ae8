"""What one ingested file costs the BM25 device index: a rebuild against an append (not a test).

python tools/bm25_append_probe.py [--docs N] [--new M] [--reps R] [--build-reps R]

A synthetic index with bench.py's BM25 generator (vocabulary 2^20, Zipf 1.07, Poisson(120) chunk
lengths).  Timed on one GPU, each figure a host clock around a call that ends in a device
synchronise:
  * BM25Index.build (host arrays) over N + M documents -- what the next search after an
    upsert_many cost before the append existed;
  * BM25Index.append of the last M documents (host arrays) to an index of the first N, with the
    merge kernel's own time from HIP events (BM25Index.timing) and its achieved bytes/s against
    the 2 x 10 B x postings it has to move.
The first repetition of each is reported apart (code-object load, allocator warm-up).  The
appended index is compared with the built one at the timed size: statistics, posting and head
counts, and a batch of searches, bit for bit.
"""
import argparse
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "classmate-rag_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import gen_tokens, sample_query_terms  # noqa: E402
from classmate_hip import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=10_000_000, help="documents already in the index (N)")
ap.add_argument("--new", type=int, default=4096, help="documents of the ingested file (M)")
ap.add_argument("--reps", type=int, default=4, help="appends timed (the first is the warm-up)")
ap.add_argument("--build-reps", type=int, default=2, help="rebuilds timed (the first is the warm-up)")
ap.add_argument("--vocab", type=int, default=1 << 20)
a = ap.parse_args()
HBM_ACHIEVABLE = 6.3e12   # bytes/s a float4 copy reaches on an MI355X (8.0e12 is the specification)


def ms(xs):
    return "[" + ", ".join(f"{1e3 * x:.1f}" for x in xs) + "] ms"


N, M, V = a.docs, a.new, a.vocab
tok, off = gen_tokens(N + M, V, 1.07, 120.0, seed=1500)
tok_h, off_h = tok.cpu().numpy(), off.cpu().numpy()
cut = int(off_h[N])
new_t, new_o = np.ascontiguousarray(tok_h[cut:]), np.ascontiguousarray(off_h[N:] - cut)
print(f"{torch.cuda.get_device_name(0)}: N = {N} documents + M = {M} new, {tok_h.shape[0]} tokens "
      f"({new_t.shape[0]} new), vocabulary {V}", flush=True)

# ---- the rebuild: BM25Index.build over all N + M documents
full = engine.BM25Index()
t_build = []
for _ in range(a.build_reps):
    t0 = time.perf_counter()
    full.build(tok_h, off_h, V)
    t_build.append(time.perf_counter() - t0)
print(f"rebuild  BM25Index.build(N + M): {ms(t_build)}  ({full.num_postings} postings, "
      f"{full.num_head_terms} head terms)", flush=True)

# ---- the append: M documents to an index of N (built on the device each time: a starting state, untimed)
t_app, t_merge, b = [], [], None
for _ in range(a.reps):
    if b is not None:
        b.close()
    b = engine.BM25Index()
    b.build_dev(tok[:cut], off[:N + 1].contiguous(), V)
    b.timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.append(new_t, new_o, V)
    t_app.append(time.perf_counter() - t0)
    t_merge.append(b.timing_drain()[0] * 1e-3)
    b.timing(False)
print(f"append   BM25Index.append(M):    {ms(t_app)}", flush=True)
moved = 20 * b.num_postings
best = min(t_merge[1:] or t_merge)
print(f"merge kernel alone (HIP events): {ms(t_merge)}; {moved / 1e9:.2f} GB to move (2 x 10 B x {b.num_postings} "
      f"postings): {moved / best / 1e12:.2f} TB/s at the best warm launch = {100 * moved / best / HBM_ACHIEVABLE:.0f} % of "
      f"the {HBM_ACHIEVABLE / 1e12:.1f} TB/s a copy reaches", flush=True)
warm_b, warm_a = t_build[1:] or t_build, t_app[1:] or t_app
print(f"warm medians: rebuild {1e3 * float(np.median(warm_b)):.1f} ms, append {1e3 * float(np.median(warm_a)):.1f} ms "
      f"(x{float(np.median(warm_b)) / float(np.median(warm_a)):.1f}); the append's remainder beside the merge is the "
      f"delta sort, the head-tile recompute and the first-key sort on the host", flush=True)

# ---- same index?  (at the size that was timed)
same = (b.stats() == full.stats() and b.num_postings == full.num_postings and b.num_docs == full.num_docs
        and b.num_head_terms == full.num_head_terms)
qt = sample_query_terms(tok, off, 64, 8, seed=10)
q_terms = qt.reshape(-1).contiguous()
q_off = (torch.arange(65, device="cuda", dtype=torch.int32) * 8).contiguous()
for path in (engine.BM25Index.PATH_PRUNED, engine.BM25Index.PATH_FULL):
    full.set_path(path)
    b.set_path(path)
    s1, r1 = full.search_dev(q_terms, q_off, 10)
    s2, r2 = b.search_dev(q_terms, q_off, 10)
    torch.cuda.synchronize()
    same = same and bool((s1 == s2).all()) and bool((r1 == r2).all())
print(f"appended index == built index (statistics, counts, 64 searches x 2 paths, bit for bit): {same}", flush=True)
sys.exit(0 if same else 1)
