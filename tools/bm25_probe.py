"""Ablation/profiling probe for the BM25 kernels at the bench's 10M shape (not a test).

python tools/bm25_probe.py [--docs N] [--batch B] [--reps R] [--k2a-trace FILE]
--k2a-trace needs a -DK2A_TRACE=1 variant library (tools/build_variant.sh, $CLASSMATE_HIP_LIB): the per-unit
start / end clocks of the last pruned search's K2a launch, summarised into FILE.
Env CM_BM25_DEBUG=1 (skip scoring) / 2 (skip range top-k) for ablations.
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
from bench import gen_tokens, sample_query_terms  # noqa: E402
from classmate_hip import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=10_000_000)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--head-frac", type=float, default=1.0 / 128)
ap.add_argument("--head-bytes", type=int, default=8 << 30)
ap.add_argument("--paths", default="1,2", help="search strategies to time (1 full K2 scan, 2 pruned)")
ap.add_argument("--dbg", default="", help="comma list of CM_BM25_DEBUG values to sweep (ablation builds only)")
ap.add_argument("--k2a-trace", default="", help="write the K2a occupancy / tail summary here (K2A_TRACE builds)")
a = ap.parse_args()


def k2a_trace_summary(path_out, nq, nr):
    """Occupancy over time and per-unit duration against postings of the last K2a launch."""
    import ctypes as C
    import heapq
    from classmate_hip import _lib as L
    fn = L.lib.cm_bm25_k2a_trace
    fn.restype, fn.argtypes = C.c_int64, (C.c_void_p, C.c_void_p, C.c_int64)
    n = 1 << 22
    buf = np.zeros((n, 4), dtype=np.uint64)
    n = int(fn(b._h, buf.ctypes.data, n))
    rec = buf[:n]
    rec = rec[rec[:, 0] != 0]
    unit = (rec[:, 0] & np.uint64(0xffffffff)).astype(np.int64) - 1
    xcc = (rec[:, 0] >> np.uint64(32)).astype(np.int64)
    t0 = rec[:, 1].astype(np.int64)
    t1 = rec[:, 2].astype(np.int64)
    post = rec[:, 3].astype(np.int64)
    base = t0.min()
    t0, t1 = t0 - base, t1 - base
    span = int(t1.max())
    dur = t1 - t0
    # resident waves over time (ticks of 10 ns): +1 at a start, -1 at an end
    ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    act = np.cumsum(ev[:, 1])
    seg = np.diff(np.append(ev[:, 0], span))            # time each level holds
    simds = 1024
    lines = [f"K2a trace: {len(rec)} units run of {n} slots, nq {nq} nr {nr}, span {span / 100:.1f} us "
             f"(first start -> last end), sum of unit durations {dur.sum() / 100:.0f} us = "
             f"{dur.sum() / span / simds:.2f} resident waves per SIMD on average"]
    for lim in (4, 2, 1):
        below = seg[act < lim * simds].sum()
        # the tail: from the last time the level was at or above lim to the end
        above = np.nonzero(act >= lim * simds)[0]
        tail_from = int(ev[above[-1] + 1, 0]) if len(above) and above[-1] + 1 < len(ev) else 0
        head_to = int(ev[above[0], 0]) if len(above) else span
        lines.append(f"below {lim} waves/SIMD: {100.0 * below / span:.1f} % of the span; ramp-up until {head_to / 100:.1f} us, "
                     f"never again at or above after {tail_from / 100:.1f} us (tail {100.0 * (span - tail_from) / span:.1f} %)")
    lines.append("resident waves per SIMD at each tenth of the span: " + " ".join(
        f"{act[max(np.searchsorted(ev[:, 0], span * i // 10, side='right') - 1, 0)] / simds:.2f}" for i in range(10)))
    lines.append(f"unit duration us: mean {dur.mean() / 100:.2f} p50 {np.percentile(dur, 50) / 100:.2f} p90 "
                 f"{np.percentile(dur, 90) / 100:.2f} p99 {np.percentile(dur, 99) / 100:.2f} max {dur.max() / 100:.2f}")
    lines.append(f"unit postings: mean {post.mean():.0f} p50 {np.percentile(post, 50):.0f} p90 {np.percentile(post, 90):.0f} "
                 f"p99 {np.percentile(post, 99):.0f} max {post.max()}; correlation(duration, postings) "
                 f"{np.corrcoef(dur, post)[0, 1]:.3f}")
    order = np.argsort(post)
    lines.append("by postings decile: postings mean | duration us mean / max | start us mean")
    for i in range(10):
        ix = order[len(order) * i // 10:len(order) * (i + 1) // 10]
        lines.append(f"  d{i}: {post[ix].mean():9.0f} | {dur[ix].mean() / 100:8.2f} / {dur[ix].max() / 100:8.2f} | {t0[ix].mean() / 100:8.1f}")
    last = np.argsort(-t1)[:8]
    lines.append("last units to end: " + "; ".join(
        f"unit {unit[i]} (qg {unit[i] % ((nq + 3) // 4)}) xcc {xcc[i]} {t0[i] / 100:.0f}->{t1[i] / 100:.0f} us post {post[i]}" for i in last))
    # what a heaviest-first list schedule of the same durations on the same wave slots would take
    hp = [0] * (5 * simds)
    for d in np.sort(dur)[::-1]:
        heapq.heappush(hp, heapq.heappop(hp) + int(d))
    lines.append(f"same durations, heaviest first on {5 * simds} wave slots: {max(hp) / 100:.1f} us; perfectly even: "
                 f"{dur.sum() / (5 * simds) / 100:.1f} us")
    per_x = [int((xcc == x).sum()) for x in range(8)]
    lines.append(f"units per XCC: {per_x}; duration sum per XCC us: {[int(dur[xcc == x].sum() / 100) for x in range(8)]}")
    Path(path_out).parent.mkdir(parents=True, exist_ok=True)
    Path(path_out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


tok, off = gen_tokens(a.docs, 1 << 20, 1.07, 120.0, seed=1500)
b = engine.BM25Index()
b.build_dev(tok, off, 1 << 20)
b.set_head_policy(a.head_frac, a.head_bytes)
qt = sample_query_terms(tok, off, a.batch, 8, seed=10)
q_terms = qt.reshape(-1).contiguous()
q_off = (torch.arange(a.batch + 1, device="cuda", dtype=torch.int32) * 8).contiguous()
df, _ = b.term_stats()
qh = qt.cpu().numpy()
qdf = df[qh].astype("int64")                                  # (B, 8)
head = qdf > a.docs * a.head_frac
print(f"workload: mean head terms/query {head.sum(1).mean():.2f}, mean head df sum/query {(qdf * head).sum(1).mean():.4g}, "
      f"mean tail df sum/query {(qdf * ~head).sum(1).mean():.4g}, distinct head terms in batch "
      f"{len(set(qh[head].tolist()))}, head tiles {b.num_head_terms}", flush=True)
ref = None
runs = [(int(p), None) for p in a.paths.split(",")]
if a.dbg:
    runs = [(int(a.paths.split(",")[-1]), d) for d in a.dbg.split(",")]
for path, dbgv in runs:
    if dbgv is not None:
        os.environ["CM_BM25_DEBUG"] = dbgv
    b.set_path(path)
    ws = torch.empty(b.workspace_bytes(a.batch, q_terms.numel(), 10), dtype=torch.uint8, device="cuda")
    out = b.search_dev(q_terms, q_off, 10, workspace=ws)
    torch.cuda.synchronize()
    ts = []
    b.timing(True)
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.search_dev(q_terms, q_off, 10, out=out, workspace=ws)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    kt = b.timing_drain()
    b.timing(False)
    if a.k2a_trace and path == 2:
        k2a_trace_summary(a.k2a_trace, a.batch, (a.docs + 1023) // 1024)
    res = (out[0].cpu(), out[1].cpu())
    same = "" if ref is None else f" identical_to_path{ref[2]}={bool(torch.equal(ref[0], res[0]) and torch.equal(ref[1], res[1]))}"
    if ref is None:
        ref = (res[0], res[1], path)
    nr = (a.docs + 1023) // 1024
    resc = b.workspace_rescored(a.batch, q_terms.numel(), 10, ws)
    if path == 2 and os.environ.get("BM25_ITEMS"):
        # K2b work: mirror bm_ws_layout (cm_bm25.hip) to read the planned items (diagnostic only)
        ru = lambda x: (x + 255) // 256 * 256
        nq, tt, k = a.batch, q_terms.numel(), 10
        off = ru(nq * 8) + ru(128 * 16 * 8) + ru(tt * 8) + ru(tt * (nr + 1) * 8) + ru(nq * nr * k * 8) + ru(nq * nr * k * 4)
        off_need = off
        off += ru(((nq + 3) // 4) * nr)
        off_items = off
        off += ru(nq * nr * 8)
        n_items = int(ws[off:off + 4].view(torch.int32).item())
        items = ws[off_items:off_items + 8 * n_items].view(torch.int64).cpu().numpy()
        masks = (items & 0xffff).astype(np.uint64)
        nblk = int(sum(bin(int(m)).count("1") for m in masks))
        need = ws[off_need:off_need + ((nq + 3) // 4) * nr].cpu().numpy()
        print(f"K2b items={n_items} blocks={nblk} ({nblk * 64} docs scored); K2 need pairs="
              f"{int(sum(bin(int(x)).count('1') for x in need))}", flush=True)
    print(f"docs={a.docs} B={a.batch} head_terms={b.num_head_terms} path={path} dbg={os.environ.get('CM_BM25_DEBUG', '0')} "
          f"search_ms={sorted(ts)[len(ts) // 2]:.3f} kernel_ms={sorted(kt)[len(kt) // 2]:.3f} rescored={resc}/{a.batch * nr}{same} "
          f"all={['%.2f' % t for t in ts]}", flush=True)
