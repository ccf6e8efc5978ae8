"""What the host detour costs HybridRetriever.retrieve_batch(filters=[one per question]): the device
chain (device_batch.retrieve_batch_clauses) against the host per-stage path (CM_RETRIEVE_DEVICE=0,
what every such batch took before) on the same stores (not a test).

timeout -k 10 1100 python tools/hybrid_lists_probe.py [--docs N] [--nq B] [--reps R] [--cells 0,1,...]
                                                      [--out profiles/hybrid_lists.txt]

One MI355X.  bench.py's BM25 corpus (gen_tokens: Zipf 1.07 over 2^20 terms, Poisson(120) tokens per
document) of N documents beside N x 768 random unit rows, in a BM25Store and a GpuVectorStore that
hold the same ids; B questions of 8 terms sampled from documents (sample_query_terms), written as
words; k_vector = k_bm25 = 10, MMR pool 24, top_k 10.  The embedder is a preset table that offers
encode_queries and encode_queries_dev: the encode costs the same on both routes and is not what is
compared.  (The BM25 device index is built from the token ids and the store's catalog filled in
beside it: tokenising 120M words on the host is not what is measured either.)

Metadata: course = i mod 1024 (~N/1024 rows a value), unit / doc_type / author / semester = 64 values
each (~N/64 rows a value), language en / it by halves.  Cells: 256, 16 and 1 distinct clauses (the
questions dealt evenly over them) of ~1k rows (a course) or ~16k rows (a unit, doc_type, author or
semester value), and one mixed batch: a third of the questions without a clause, a third under
{"language": "en"} (half the corpus: the scans), a third under a course each.

Both routes run in this process, alternating repetition by repetition after a warm-up of each; every
figure is a host clock around a call followed by a device synchronise: median (and minimum) over R
repetitions.  Before timing the two outputs are compared with ==.  "first" is the device chain's
first call on a cold epsilon cache (one call, after the warm-up, with the cache emptied); "eps" the
floors that call computed: on the list route / by per-clause filtered searches.  The host path computes them on every call.
"""
import argparse
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "classmate-rag_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from classmate_hip import engine  # noqa: E402
from classmate_hip.retrieval import BM25Store, GpuVectorStore, HybridRetriever, device_batch  # noqa: E402
from classmate_hip.retrieval.bm25 import _Entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=256)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--cells", default="0,1,2,3,4,5,6")
ap.add_argument("--out", default=str(REPO / "profiles" / "hybrid_lists.txt"))
a = ap.parse_args()

N, B, D, V, QT, K = a.docs // 32 * 32, a.nq, 768, 1 << 20, 8, 10
dev = torch.device("cuda", 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


def word(t):
    s = "zq"
    for _ in range(5):
        s += chr(97 + t % 26)
        t //= 26
    return s


t_setup = time.perf_counter()
ids = [f"c{i}" for i in range(N)]
metas = [{"course": f"c{i % 1024}", "unit": f"u{i % 64}", "doc_type": f"t{(i // 64) % 64}", "author": f"a{(i // 7) % 64}",
          "semester": f"s{(i // 13) % 64}", "language": "en" if i % 2 else "it"} for i in range(N)]
vs = GpuVectorStore(persist_dir=None, device=0)
g = torch.Generator(device="cuda").manual_seed(77)
for i in range(0, N, 1 << 18):
    n = min(N, i + (1 << 18)) - i
    emb = torch.randn(n, D, device=dev, generator=g)
    emb /= emb.norm(dim=1, keepdim=True)
    vs.upsert(ids=ids[i:i + n], documents=[""] * n, metadatas=metas[i:i + n], embeddings=emb.cpu().numpy())
tokens, doc_off = bench.gen_tokens(N, V, 1.07, 120.0, seed=500)
qterms = bench.sample_query_terms(tokens, doc_off, B, QT, seed=3).cpu().numpy().tolist()
bm = BM25Store(index_dir=None, device=0)
for i, m in zip(ids, metas):
    bm._entries[i] = _Entry(id=i, text="", tokens=[], metadata=m)
bm._id_list = list(ids)
bm._version += 1
bm._vocab.update({word(t): t for q in qterms for t in q})
bm._index = engine.BM25Index(device=0)
bm._index.build_dev(tokens, doc_off, V)
bm._dirty, bm._meta_dirty = False, True
del tokens, doc_off
questions = [" ".join(word(t) for t in q) for q in qterms]
assert all(bm._query_ids(q) == t for q, t in zip(questions, qterms))
qv = torch.randn(B, D, device=dev, generator=g)
qv /= qv.norm(dim=1, keepdim=True)


class Preset:
    def __init__(self):
        self.dev = {q: i for i, q in enumerate(questions)}
        self.host = qv.cpu().numpy()

    def encode_queries(self, qs):
        return self.host[[self.dev[q] for q in qs]]

    def encode_queries_dev(self, qs):
        return qv[torch.tensor([self.dev[q] for q in qs], device=dev)]


retr = HybridRetriever(vector_store=vs, bm25_store=bm, embedder=Preset(), k_vector=K, k_bm25=K, mmr_max_pool=24)
torch.cuda.synchronize()
say(f"{torch.cuda.get_device_name(0)}: {N} documents ({bm._index.num_postings} postings) beside {N} x {D} unit rows, "
    f"{B} questions x {QT} terms, k_vector = k_bm25 = {K}, pool 24, top_k {K}, {a.reps} repetitions "
    f"(setup {time.perf_counter() - t_setup:.0f} s)")

WIDE = [("unit", "u"), ("doc_type", "t"), ("author", "a"), ("semester", "s")]


def cell_filters(nc, wide):
    if wide:
        cl = [{WIDE[c // 64][0]: f"{WIDE[c // 64][1]}{c % 64}"} for c in range(nc)]
    else:
        cl = [{"course": f"c{c}"} for c in range(nc)]
    return [cl[i % nc] for i in range(B)]


CELLS = [("256 x 1", "1k", cell_filters(256, False)), ("16 x 16", "1k", cell_filters(16, False)),
         ("1 x 256", "1k", cell_filters(1, False)), ("256 x 1", "16k", cell_filters(256, True)),
         ("16 x 16", "16k", cell_filters(16, True)), ("1 x 256", "16k", cell_filters(1, True)),
         ("mixed", "-", [None if i % 3 == 0 else {"language": "en"} if i % 3 == 1 else {"course": f"c{i}"}
                         for i in range(B)])]


eps_seen = [0, 0]          # floors computed by search_lists calls / by _bm25_filtered's per-clause recovery
_lists, _feps = engine.BM25Index.search_lists, engine.BM25Index.filter_eps


def _spy_lists(self, *args, **kw):
    out = _lists(self, *args, **kw)
    eps_seen[0] += self.last_eps_filters()
    return out


def _spy_feps(self, allow):
    eps_seen[1] += 1
    return _feps(self, allow)


engine.BM25Index.search_lists, engine.BM25Index.filter_eps = _spy_lists, _spy_feps


def run(fs, device):
    os.environ["CM_RETRIEVE_DEVICE"] = "1" if device else "0"
    out = retr.retrieve_batch(questions=questions, filters=fs, top_k=K)
    torch.cuda.synchronize()
    return out


say(f"{'clauses x q':>11} {'rows/cl':>7} {'eps':>7} | {'host ms med':>11} {'min':>8} | {'device ms med':>13} {'min':>8} "
    f"{'first':>8} | {'host/device':>11} {'host/first':>10} | equal")
for c in [int(x) for x in a.cells.split(",")]:
    name, rows, fs = CELLS[c]
    got, want = run(fs, True), run(fs, False)             # warm-up of both, and the comparison
    equal = got == want
    assert equal, f"cell {name} {rows}: the routes differ"
    device_batch._EPS_CACHE.clear()
    eps_seen[:] = [0, 0]
    t0 = time.perf_counter()
    run(fs, True)
    first = time.perf_counter() - t0
    n_eps = f"{eps_seen[0]}/{eps_seen[1]}"
    th, td = [], []
    for _ in range(a.reps):                               # alternating
        t0 = time.perf_counter()
        run(fs, True)
        t1 = time.perf_counter()
        run(fs, False)
        t2 = time.perf_counter()
        td.append(t1 - t0)
        th.append(t2 - t1)
    mh, md = np.median(th), np.median(td)
    say(f"{name:>11} {rows:>7} {n_eps:>7} | {1e3 * mh:>11.1f} {1e3 * min(th):>8.1f} | {1e3 * md:>13.1f} {1e3 * min(td):>8.1f} "
        f"{1e3 * first:>8.1f} | {mh / md:>11.2f} {mh / first:>10.2f} | {equal}")
