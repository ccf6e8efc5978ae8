"""What deleting documents costs the BM25 device index: a rebuild against a removal (not a test).

python tools/bm25_remove_probe.py [--docs N] [--reps R] [--build-reps R]

A synthetic index with bench.py's BM25 generator (vocabulary 2^20, Zipf 1.07, Poisson(120) chunk
lengths) of N documents, and two removal sets: 4096 consecutive rows from the middle (one file's
chunks) and a seeded uniform 1 % of the rows.  Timed on one GPU, each figure a host clock around a
call that ends in a device synchronise:
  * BM25Index.build (host arrays) over the surviving documents -- what the next search after a
    delete_many cost before the removal existed;
  * BM25Index.remove of the rows (host array) from an index of all N, with the two compaction
    passes' own time from HIP events (BM25Index.timing: pass A with its scan, pass B) and their
    achieved bytes/s against the postings x (4 + 10 + 10 s) bytes they have to move (s = the
    surviving share of the postings);
  * a device-to-device copy in the same process, for comparison.
The first repetition of each is reported apart (code-object load, allocator warm-up).  The index
after the removal is compared with the built one: statistics, posting and head counts, and a batch
of searches, bit for bit.
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
ap.add_argument("--reps", type=int, default=3, help="removals timed per set (the first is the warm-up)")
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

sets = {"4096 consecutive rows from the middle": np.arange(N // 2, N // 2 + min(4096, N // 2), dtype=np.int64),
        "a seeded uniform 1 % of the rows": np.sort(np.random.default_rng(1501).choice(N, size=N // 100, replace=False))}
qt = sample_query_terms(tok, off, 64, 8, seed=10)
q_terms = qt.reshape(-1).contiguous()
q_off = (torch.arange(65, device="cuda", dtype=torch.int32) * 8).contiguous()
all_same = True
for name, rows in sets.items():
    print(f"-- remove {rows.shape[0]} documents: {name}", flush=True)
    keep = np.ones(N, bool)
    keep[rows] = False
    surv_t = np.ascontiguousarray(tok_h[np.repeat(keep, lens)])
    surv_o = np.zeros(int(keep.sum()) + 1, np.int64)
    surv_o[1:] = np.cumsum(lens[keep])

    # ---- the rebuild: BM25Index.build over the surviving documents
    full = engine.BM25Index()
    t_build = []
    for _ in range(a.build_reps):
        t0 = time.perf_counter()
        full.build(surv_t, surv_o, V)
        t_build.append(time.perf_counter() - t0)
    print(f"rebuild  BM25Index.build(survivors): {ms(t_build)}  ({full.num_postings} postings, "
          f"{full.num_head_terms} head terms)", flush=True)
    del surv_t

    # ---- the removal, from an index of all N (built on the device each time: a starting state, untimed)
    t_rm, t_a, t_b, b = [], [], [], None
    for _ in range(a.reps):
        if b is not None:
            b.close()
        b = engine.BM25Index()
        b.build_dev(tok, off, V)
        p0 = b.num_postings
        b.timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.remove(rows)
        t_rm.append(time.perf_counter() - t0)
        pa, pb = b.timing_drain()[:2]
        t_a.append(pa * 1e-3)
        t_b.append(pb * 1e-3)
        b.timing(False)
    print(f"remove   BM25Index.remove(rows):     {ms(t_rm)}", flush=True)
    s = b.num_postings / p0
    moved = p0 * (4 + 10 + 10 * s)
    t_ab = [x + y for x, y in zip(t_a, t_b)]
    best = min(t_ab[1:] or t_ab)
    print(f"passes A + B alone (HIP events): A + scan {ms(t_a)}, B {ms(t_b)}; {moved / 1e9:.2f} GB to move "
          f"({p0} postings x (4 + 10 + 10 x {s:.4f}) B): {moved / best / 1e12:.2f} TB/s at the best warm pair = "
          f"{100 * moved / best / copy_rate:.0f} % of the copy's rate", flush=True)
    warm_b, warm_r = t_build[1:] or t_build, t_rm[1:] or t_rm
    print(f"warm medians: rebuild {1e3 * float(np.median(warm_b)):.1f} ms, remove {1e3 * float(np.median(warm_r)):.1f} ms "
          f"(x{float(np.median(warm_b)) / float(np.median(warm_r)):.1f}); the removal's remainder beside the passes is "
          f"the head-tile recompute and the first-key sort on the host", flush=True)

    # ---- same index?
    same = (b.stats() == full.stats() and b.num_postings == full.num_postings and b.num_docs == full.num_docs
            and b.num_head_terms == full.num_head_terms)
    for path in (engine.BM25Index.PATH_PRUNED, engine.BM25Index.PATH_FULL):
        full.set_path(path)
        b.set_path(path)
        s1, r1 = full.search_dev(q_terms, q_off, 10)
        s2, r2 = b.search_dev(q_terms, q_off, 10)
        torch.cuda.synchronize()
        same = same and bool((s1 == s2).all()) and bool((r1 == r2).all())
    print(f"removed index == built index (statistics, counts, 64 searches x 2 paths, bit for bit): {same}", flush=True)
    all_same = all_same and same
    b.close()
    full.close()
sys.exit(0 if all_same else 1)
