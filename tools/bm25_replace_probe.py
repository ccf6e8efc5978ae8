"""What replacing documents in place costs the BM25 device index: a rebuild against a replace (not a test).

python tools/bm25_replace_probe.py [--docs N] [--set file|uniform|both] [--reps R] [--build-reps R]

A synthetic index with bench.py's BM25 generator (vocabulary 2^20, Zipf 1.07, Poisson(120) chunk
lengths) of N documents, and two sets of rows to replace, each with freshly drawn text of the same
kind: 4096 consecutive rows from the middle (one file's chunks) and a seeded uniform 1 % of the
rows.  Timed on one GPU, each figure a host clock around a call that ends in a device synchronise:
  * BM25Index.build (host arrays) over the documents with those rows substituted -- what the next
    search after such an upsert_many cost before the replace existed;
  * BM25Index.replace of the rows (host arrays) on an index of all N, with the two timed pass
    groups from HIP events (BM25Index.timing: the flag pass with its scan, the two scatters) and
    their achieved bytes/s against the bytes they have to move: postings x (4 + 10 + 10 s) B
    (s = the surviving share of the old postings) plus the delta, read and written (20 B a posting);
  * BM25Index.remove of the same rows from such an index, for comparison (it moves the same bytes
    but the delta);
  * a device-to-device copy in the same process.
The first repetition of each is reported apart (code-object load, allocator warm-up).  The index
after the replace is compared with the built one: statistics, posting and head counts, every
exported array, and a batch of searches, bit for bit.  One (N, set) per process lets a caller put
each under a time limit of its own.
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
ap.add_argument("--docs", type=int, default=10_000_000, help="documents in the index (N)")
ap.add_argument("--set", choices=("file", "uniform", "both"), default="both")
ap.add_argument("--reps", type=int, default=3, help="replaces timed per set (the first is the warm-up)")
ap.add_argument("--build-reps", type=int, default=2, help="rebuilds timed per set (the first is the warm-up)")
ap.add_argument("--vocab", type=int, default=1 << 20)
a = ap.parse_args()


def ms(xs):
    return "[" + ", ".join(f"{1e3 * x:.1f}" for x in xs) + "] ms"


N, V = a.docs, a.vocab
tok, off = gen_tokens(N, V, 1.07, 120.0, seed=1500)
tok_h, off_h = tok.cpu().numpy(), off.cpu().numpy()
lens = np.diff(off_h)
print(f"{torch.cuda.get_device_name(0)}: N = {N} documents, {tok_h.shape[0]} tokens, vocabulary {V}", flush=True)

# ---- a device-to-device copy in this process (read + write of a buffer the size of the token ids)
dst = torch.empty_like(tok)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
t_copy = []
for _ in range(3):
    ev[0].record()
    dst.copy_(tok)
    ev[1].record()
    torch.cuda.synchronize()
    t_copy.append(ev[0].elapsed_time(ev[1]) * 1e-3)
copy_rate = 2 * tok.numel() * 4 / min(t_copy[1:])
print(f"device-to-device copy of {tok.numel() * 4 / 1e9:.2f} GB: {ms(t_copy)}; {copy_rate / 1e12:.2f} TB/s read + write "
      f"at the best warm copy", flush=True)
del dst

sets = {"file": ("4096 consecutive rows from the middle",
                 np.arange(N // 2, N // 2 + min(4096, N // 2), dtype=np.int64)),
        "uniform": ("a seeded uniform 1 % of the rows",
                    np.sort(np.random.default_rng(1501).choice(N, size=N // 100, replace=False)))}
qt = sample_query_terms(tok, off, 64, 8, seed=10)
q_terms = qt.reshape(-1).contiguous()
q_off = (torch.arange(65, device="cuda", dtype=torch.int32) * 8).contiguous()
all_same = True
for key, (name, rows) in sets.items():
    if a.set not in (key, "both"):
        continue
    print(f"-- replace {rows.shape[0]} documents: {name}", flush=True)
    new_t, new_o = gen_tokens(int(rows.shape[0]), V, 1.07, 120.0, seed=1502)
    new_t, new_o = new_t.cpu().numpy(), new_o.cpu().numpy()
    torch.cuda.empty_cache()
    repl = np.zeros(N, bool)
    repl[rows] = True
    sub_lens = lens.copy()
    sub_lens[rows] = np.diff(new_o)
    sub_o = np.zeros(N + 1, np.int64)
    sub_o[1:] = np.cumsum(sub_lens)
    sub_t = np.empty(int(sub_o[-1]), np.int32)
    sub_t[np.repeat(~repl, sub_lens)] = tok_h[np.repeat(~repl, lens)]
    sub_t[np.repeat(repl, sub_lens)] = new_t

    # ---- the rebuild: BM25Index.build over the substituted documents
    full = engine.BM25Index()
    t_build = []
    for _ in range(a.build_reps):
        t0 = time.perf_counter()
        full.build(sub_t, sub_o, V)
        t_build.append(time.perf_counter() - t0)
    print(f"rebuild  BM25Index.build(substituted): {ms(t_build)}  ({full.num_postings} postings, "
          f"{full.num_head_terms} head terms)", flush=True)
    del sub_t

    # ---- the replace, on an index of all N (built on the device each time: a starting state, untimed)
    t_rp, t_a, t_b, b = [], [], [], None
    for _ in range(a.reps):
        if b is not None:
            b.close()
        b = engine.BM25Index()
        b.build_dev(tok, off, V)
        p0 = b.num_postings
        b.timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.replace(rows, new_t, new_o, V)
        t_rp.append(time.perf_counter() - t0)
        pa, pb = b.timing_drain()[:2]
        t_a.append(pa * 1e-3)
        t_b.append(pb * 1e-3)
        b.timing(False)
    print(f"replace  BM25Index.replace(rows):      {ms(t_rp)}", flush=True)

    # ---- the removal of the same rows, from the same starting state
    t_rm, t_ra, t_rb = [], [], []
    for _ in range(max(2, a.reps - 1)):
        r = engine.BM25Index()
        r.build_dev(tok, off, V)
        r.timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.remove(rows)
        t_rm.append(time.perf_counter() - t0)
        pa, pb = r.timing_drain()[:2]
        t_ra.append(pa * 1e-3)
        t_rb.append(pb * 1e-3)
        p_surv = r.num_postings
        r.close()
    print(f"remove   BM25Index.remove(rows):       {ms(t_rm)}; its passes: A + scan {ms(t_ra)}, B {ms(t_rb)}", flush=True)

    s = p_surv / p0
    dp = b.num_postings - p_surv
    moved = p0 * (4 + 10 + 10 * s) + 20 * dp
    t_ab = [x + y for x, y in zip(t_a, t_b)]
    best = min(t_ab[1:] or t_ab)
    print(f"timed passes alone (HIP events): flag + scan {ms(t_a)}, scatters {ms(t_b)}; {moved / 1e9:.2f} GB to move "
          f"({p0} postings x (4 + 10 + 10 x {s:.4f}) B + {dp} delta postings x 20 B): {moved / best / 1e12:.2f} TB/s at "
          f"the best warm pair = {100 * moved / best / copy_rate:.0f} % of the copy's rate", flush=True)
    warm_b, warm_r, warm_m = t_build[1:] or t_build, t_rp[1:] or t_rp, t_rm[1:] or t_rm
    mb, mr, mm = float(np.median(warm_b)), float(np.median(warm_r)), float(np.median(warm_m))
    print(f"warm medians: rebuild {1e3 * mb:.1f} ms, replace {1e3 * mr:.1f} ms (x{mb / mr:.1f}), remove {1e3 * mm:.1f} ms "
          f"(x{mb / mm:.1f}); the replace's remainder beside the passes is the delta's upload and sort, the "
          f"head-tile recompute and the first-key sort on the host", flush=True)

    # ---- same index?
    same = (b.stats() == full.stats() and b.num_postings == full.num_postings and b.num_docs == full.num_docs
            and b.num_head_terms == full.num_head_terms)
    e1, e2 = full.export(), b.export()
    same = same and all(bool((e1[k] == e2[k]).all()) for k in e1)
    del e1, e2
    for path in (engine.BM25Index.PATH_PRUNED, engine.BM25Index.PATH_FULL):
        full.set_path(path)
        b.set_path(path)
        s1, r1 = full.search_dev(q_terms, q_off, 10)
        s2, r2 = b.search_dev(q_terms, q_off, 10)
        torch.cuda.synchronize()
        same = same and bool((s1 == s2).all()) and bool((r1 == r2).all())
    print(f"replaced index == built index (statistics, counts, exported arrays, 64 searches x 2 paths, bit for bit): "
          f"{same}", flush=True)
    all_same = all_same and same
    b.close()
    full.close()
sys.exit(0 if all_same else 1)
