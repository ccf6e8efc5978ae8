"""What a batch with per-question where clauses costs the BM25 index: the row-list search against
one ordinary filtered search per distinct clause (not a test).

timeout -k 10 900 python tools/bm25_lists_probe.py [--docs N] [--nq B] [--k K] [--reps R]
                                                   [--clauses 256,16,1] [--shares 1024,64,8]

bench.py's BM25 corpus (gen_tokens: Zipf 1.07 over 2^20 terms, Poisson(120) tokens per document) of
N documents and B questions of 8 terms sampled from documents (sample_query_terms).  For 256, 16
and 1 distinct clauses (the questions dealt evenly over them), each allowing about N/1024, N/64 and
N/8 rows as a scattered (Bernoulli) set:
  * lists       BM25Index.search_lists over the whole batch, split like BM25Store.search_batch at
                BM25_LIST_PAIR_BUDGET (query, allowed row) pairs per call;
  * per clause  BM25Index.search once per distinct clause with the questions that use it: what
                search_batch did before, and still does for unselective clauses.
Both run in this process, alternating repetition by repetition after one warm-up each; every figure
is a host clock around calls that end in a device synchronise, the median (and minimum) over R
repetitions.  Before timing, the two outputs are compared for bit equality.  "eps" is the number of
clauses of the batch that had a negative idf and took the epsilon pass over all postings
(filtered_eps): both routes pay it, once per such clause.  One cell group per invocation
(--clauses / --shares) gives each GPU step a time limit of its own.
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
from classmate_hip.retrieval.bm25 import BM25_LIST_PAIR_BUDGET  # noqa: E402
from classmate_hip.retrieval.vector_store import route_clauses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=256)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--clauses", default="256,16,1")
ap.add_argument("--shares", default="1024,64,8", help="allowed rows = docs / share")
a = ap.parse_args()

N, B, K, V, QT = a.docs // 32 * 32, a.nq, a.k, 1 << 20, 8
dev = torch.device("cuda", 0)
tokens, doc_off = bench.gen_tokens(N, V, 1.07, 120.0, seed=500)
idx = engine.BM25Index(device=0)
idx.build_dev(tokens, doc_off, V)
queries = bench.sample_query_terms(tokens, doc_off, B, QT, seed=3).cpu().numpy().tolist()
del tokens, doc_off
torch.cuda.synchronize()
print(f"{torch.cuda.get_device_name(0)}: {N} documents, {idx.num_postings} postings, {idx.num_head_terms} head tiles, "
      f"{B} questions x {QT} terms, k = {K}, {a.reps} repetitions", flush=True)

POW = (1 << torch.arange(32, device=dev, dtype=torch.int64))


def clauses(nc, frac, seed):
    """nc scattered clauses -> (nc, N / 32) int32 allow words on the device, and their row counts."""
    gg = torch.Generator(device=dev).manual_seed(seed)
    words, counts = [], []
    for c0 in range(0, nc, 16):
        mask = torch.rand((min(16, nc - c0), N), generator=gg, device=dev) < frac
        w = (mask.view(mask.shape[0], N // 32, 32).to(torch.int64) * POW).sum(dim=2)
        words.append(torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32))   # two's complement words
        counts.append(mask.sum(dim=1).cpu().numpy())
    torch.cuda.synchronize()
    return torch.cat(words).contiguous(), np.concatenate(counts)


def run_lists(words, counts, filter_of):
    scores = np.zeros((B, K))
    rows = np.full((B, K), -1, np.int64)
    nvalid = np.zeros(B, np.int32)
    plan = route_clauses(filter_of.tolist(), counts.tolist(), N, K, 1 << 62, True, 1.0, BM25_LIST_PAIR_BUDGET, 0.0)
    assert not plan["scan"] and not plan["empty"] and not plan["plain"]      # every question on the list route
    eps = 0
    for call in plan["lists"]:
        sel = [i for _, qs in call for i in qs]
        fo = np.concatenate([np.full(len(qs), f, np.int32) for f, (_, qs) in enumerate(call)])
        gs = [c for c, _ in call]
        s, r, n = idx.search_lists([queries[i] for i in sel], K, words[gs] if len(gs) < words.shape[0] else words, fo)
        scores[sel], rows[sel], nvalid[sel] = s, r, n
        eps += idx.last_eps_filters()
    return scores, rows, nvalid, len(plan["lists"]), eps


def run_per_clause(words, filter_of):
    scores = np.empty((B, K))
    rows = np.empty((B, K), np.int64)
    nvalid = np.empty(B, np.int32)
    for c in range(words.shape[0]):
        sel = np.nonzero(filter_of == c)[0]
        s, r, n = idx.search([queries[i] for i in sel], K, words[c])
        scores[sel], rows[sel], nvalid[sel] = s, r, n
    return scores, rows, nvalid


print(f"{'clauses':>7} {'q/clause':>8} {'share':>7} {'rows/cl':>8} {'calls':>5} {'eps':>4} | {'lists ms med':>12} {'min':>9} | "
      f"{'per-clause ms med':>17} {'min':>9} | {'per-clause/lists':>16}", flush=True)
for nc in [int(x) for x in a.clauses.split(",")]:
    filter_of = (np.arange(B) % nc).astype(np.int32)
    for share in [int(x) for x in a.shares.split(",")]:
        words, counts = clauses(nc, 1.0 / share, 1800 + share)
        sl, rl, nl, n_calls, eps = run_lists(words, counts, filter_of)       # warm-up of both, and the comparison
        sp, rp, npc = run_per_clause(words, filter_of)
        assert np.array_equal(nl, npc) and np.array_equal(rl, rp) and (sl == sp).all(), "the routes differ"
        tl, tp = [], []
        for _ in range(a.reps):                                              # alternating
            t0 = time.perf_counter()
            run_lists(words, counts, filter_of)
            t1 = time.perf_counter()
            run_per_clause(words, filter_of)
            t2 = time.perf_counter()
            tl.append(t1 - t0)
            tp.append(t2 - t1)
        ml, mp = np.median(tl), np.median(tp)
        print(f"{nc:>7} {B // nc:>8} {'1/' + str(share):>7} {int(counts.mean()):>8} {n_calls:>5} {eps:>4} | "
              f"{1e3 * ml:>12.3f} {1e3 * min(tl):>9.3f} | {1e3 * mp:>17.3f} {1e3 * min(tp):>9.3f} | {mp / ml:>16.2f}",
              flush=True)
        del words
