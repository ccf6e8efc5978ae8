"""Selective allow bitmaps on every scan kind of the dense index.

A real `where` filter selects one course: a small, often contiguous run of rows.  On the coarse
kinds (K1c 3, K1s 4, K1q 5, K1q-s 6) that reaches what the dense bitmaps of the other tests never
do: a seed of +inf (fewer than k sample groups hold an allowed live row, dense_seed_kernel),
(range, query) candidate buffers that a contiguous allowed run overflows, lists shorter than k, and
the clamped read of the last allow word.  Every case runs every kind through the host entry (the
bitmap as a host array and as a device tensor) and the two device entries -- search_dev, and
search_dev(defer_exact=True) + exact_fallback_dev, what device_batch.py runs -- and must equal the
exact fp64 oracle over the live and allowed rows (check_lists of test_gpu_dense_mutations.py: the
project's bars, pads equal to the fp32 kind's, every list ascending in (distance, row)).

Candidate-buffer capacities (cm_dense.hip, cm_dense_q8.inc): kCBufCap = 64 slots per (range, query)
on K1c and K1s, kQCap = 128 on K1q and K1q-s; the certified band is kRerankCap = 1 024 rows on K1c /
K1s and kQBand = 4 096 on K1q / K1q-s.  A range is rows_per_wg of coarse_config: the store's 64-row
tiles dealt over max(64, CUs / passes) workgroups on the batched kinds and over 4 x CUs waves on the
stream kinds (rows_per_range below restates it).  With a seed of +inf every allowed live row of a
range is appended, so a range the allowed run covers overflows when it holds more rows than slots.
"""
import numpy as np
import pytest

from test_gpu_dense_mutations import (COARSE, D, F32, KINDS, KS, N, Q8, Q8S, SLACK_CAP, STREAM, Model, _bits,
                                      base_store, check_lists, host_lists, near, near_tie_free, pick_queries,
                                      queries_of, sharded_case, sharded_lists, tie_slack_share, verify)

pytestmark = pytest.mark.gpu

CAP = {COARSE: 64, STREAM: 64, Q8: 128, Q8S: 128}          # kCBufCap, kCBufCap, kQCap, kQCap


def rows_per_range(kind, size, nq):
    """coarse_config's rows_per_wg for `kind` at `size` rows and nq queries on this device."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-size // 128) * 128 // 64
    n_pass = -(-nq // 256)
    groups = cus * 4 if kind in (STREAM, Q8S) else max(64, max(1, cus // n_pass))
    return -(-tiles // min(groups, tiles)) * 64


@pytest.fixture(scope="module")
def store():
    """The 20 480-row store of this module (read-only: a case that deletes rows puts them back)."""
    from classmate_hip import engine
    C, Q = base_store(N, 701)
    idx = engine.DenseIndex(D)
    model = Model(D)
    idx.upsert(C, np.arange(N, dtype=np.int64))
    model.upsert(C, np.arange(N))
    yield dict(idx=idx, model=model, C=C, Q=Q)
    idx.close()


def planted_queries(store, rows, seed, among=None):
    """The store's queries -- or, under a filter that allows thousands of rows, queries picked
    tie-free among the allowed rows `among` (pick_queries) -- with query j near row rows[j]."""
    Q = store["Q"].copy() if among is None else pick_queries(store["C"][among], 64, seed + 1)
    Q[:len(rows)] = near(store["C"][np.asarray(rows)], np.random.default_rng(seed))
    return Q


def mask_of(rows, n=N):
    allow = np.zeros(n, bool)
    allow[np.asarray(rows)] = True
    return allow


def test_nothing_allowed_inside_any_sample(store):
    """Case 1: 2 000 scattered rows, all >= 4 096 (outside every seed sample): no sample group holds an
    allowed row, the seed is +inf, every allowed row is a candidate."""
    rng = np.random.default_rng(710)
    rows = np.sort(rng.choice(np.arange(4096, N), 2000, replace=False))
    Q = planted_queries(store, rows[[0, 1, 500, 1000, 1500, 1999]], 711, among=rows)
    res = verify("filter: outside every sample", store["idx"], store["model"], Q, allow=mask_of(rows))
    for (kind, k), (d, r, _, _) in res.items():
        assert (r[:6, 0] == rows[[0, 1, 500, 1000, 1500, 1999]]).all() and (d[:6, 0] < 1e-3).all(), (kind, k)
        assert np.isin(r, rows).all(), (kind, k)


def test_contiguous_course_inside_the_sample(store):
    """Case 2: rows 100..139 only -- at least k rows, but two 64-row sample groups (fewer than k): the
    seed is +inf and all 40 rows are considered; at k = 24 the list is the exact top 24 of the 40."""
    rows = np.arange(100, 140)
    Q = planted_queries(store, [100, 139, 127, 128], 721)
    res = verify("filter: course inside the sample", store["idx"], store["model"], Q, allow=mask_of(rows))
    for (kind, k), (d, r, _, _) in res.items():
        assert (r[:4, 0] == [100, 139, 127, 128]).all() and (d[:4, 0] < 1e-3).all(), (kind, k)
        assert ((r >= 100) & (r < 140)).all(), (kind, k)            # k allowed rows: no pad, nothing else
    # all 40 are considered: the exact order of the whole course, 24 at a time
    idx, model = store["idx"], store["model"]
    for kind in KINDS:
        Qk = queries_of(kind, Q)
        d, r, _, _ = host_lists(idx, kind, Qk, 24, _bits(mask_of(rows)))
        rest = mask_of(rows)
        rest[r[0]] = False                                          # query 0's remaining 16 rows
        d2, r2, _, _ = host_lists(idx, kind, Qk, 24, _bits(rest))
        d1 = host_lists(idx, F32, Qk, 24, _bits(rest))[0]
        check_lists(d2, r2, model, Qk, 24, rest, pad_ref=d1)
        assert set(r[0].tolist()) | set(r2[0, :16].tolist()) == set(rows.tolist()) and (r2[0, 16:] == -1).all(), kind
        assert d2[0, 0] >= d[0, 23], kind


def test_contiguous_course_outside_the_sample(store):
    """Case 3: rows 6 000..8 999 only.  The seed is +inf, so a range inside the run appends every one
    of its rows: where rows_per_range exceeds the kind's slots (K1c: 128-row ranges against kCBufCap =
    64) the buffers overflow and the exact pass or the wide re-rank has to finish the query."""
    rows = np.arange(6000, 9000)
    Q = planted_queries(store, [6000, 8999, 6063, 6064, 7500], 731, among=rows)
    res = verify("filter: course outside the sample", store["idx"], store["model"], Q, allow=mask_of(rows))
    for (kind, k), (d, r, fb, wide) in res.items():
        assert (r[:5, 0] == [6000, 8999, 6063, 6064, 7500]).all() and (d[:5, 0] < 1e-3).all(), (kind, k)
        assert ((r >= 6000) & (r < 9000)).all(), (kind, k)
        if kind != F32:
            per = rows_per_range(kind, N, 64)
            print(f"\n[filter: course outside the sample] kind {kind}: {per} rows per range, {CAP[kind]} slots", end="")
            if per > CAP[kind]:
                assert fb + max(wide, 0) > 0, (kind, k, per)


def test_fewer_allowed_rows_than_k(store):
    """Case 4: five allowed rows (row 0, 31, 32, size - 1, one mid row), then the same with two of
    them dead: the lists hold exactly the live allowed rows in order, then pads."""
    idx, model, C = store["idx"], store["model"], store["C"]
    rows = np.array([0, 31, 32, N - 1, 10000])
    Q = planted_queries(store, rows, 741)
    res = verify("filter: 5 allowed rows", idx, model, Q, allow=mask_of(rows))
    for (kind, k), (d, r, _, _) in res.items():
        assert (r[:5, 0] == rows).all() and (r[:, 5:] == -1).all(), (kind, k)
        assert (np.sort(r[:, :5], axis=1) == np.sort(rows)).all(), (kind, k)
    dead = np.array([31, 10000])
    idx.delete(dead)
    model.delete(dead)
    try:
        res = verify("filter: 5 allowed rows, 2 dead", idx, model, Q, allow=mask_of(rows))
        for (kind, k), (d, r, _, _) in res.items():
            assert (np.sort(r[:, :3], axis=1) == [0, 32, N - 1]).all() and (r[:, 3:] == -1).all(), (kind, k)
            assert (r[[0, 2, 3], 0] == [0, 32, N - 1]).all(), (kind, k)
    finally:
        idx.upsert(C[dead], dead.astype(np.int64))           # restore the module store
        model.upsert(C[dead], dead)


def test_nothing_allowed(store):
    """Case 5: an all-zero bitmap, and a bitmap whose only set bits are dead rows: all pads on every
    kind and entry, and the fallback counter never negative (host_lists asserts it)."""
    idx, model, C, Q = store["idx"], store["model"], store["C"], store["Q"]
    res = verify("filter: nothing allowed", idx, model, Q, allow=np.zeros(N, bool))
    for (kind, k), (d, r, _, _) in res.items():
        assert (r == -1).all(), (kind, k)
    dead = np.array([7, 4100, 20000])
    idx.delete(dead)
    model.delete(dead)
    try:
        res = verify("filter: only dead rows allowed", idx, model, Q, allow=mask_of(dead))
        for (kind, k), (d, r, _, _) in res.items():
            assert (r == -1).all(), (kind, k)
    finally:
        idx.upsert(C[dead], dead.astype(np.int64))
        model.upsert(C[dead], dead)


def test_ragged_size_and_bits_past_the_end(store):
    """Case 6: 20 467 rows (size % 32 == 19, size % 64 != 0); the bitmap's last word has its bits past
    `size` set and only the last 40 real rows are allowed: no row >= size comes back, the 40 are
    ranked exactly."""
    from classmate_hip import engine
    n = 20467
    assert n % 32 == 19 and n % 64 != 0
    C = store["C"][:n]
    idx, model = engine.DenseIndex(D), Model(D)
    try:
        idx.upsert(C, np.arange(n, dtype=np.int64))
        model.upsert(C, np.arange(n))
        allow = np.zeros(-(-n // 32) * 32, bool)
        allow[n - 40:] = True                                  # the 40 rows and the 13 bits past the end
        assert _bits(allow).shape[0] == -(-n // 32) and allow[n:].all()
        Q = planted_queries(store, [n - 1, n - 40, n - 19, n - 20], 761)
        res = verify("filter: ragged size", idx, model, Q, allow=allow)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:4, 0] == [n - 1, n - 40, n - 19, n - 20]).all() and (d[:4, 0] < 1e-3).all(), (kind, k)
            assert ((r >= n - 40) & (r < n)).all(), (kind, k)
    finally:
        idx.close()


def test_one_filter_two_passes(store):
    """Case 7: 300 queries (two passes of 256) under one contiguous filter outside the sample, on K1c
    and K1q: the lists of query i of the first pass and of the same query placed in the second pass
    are identical.  Two passes halve the workgroups per pass, so K1q's ranges (192 rows) outgrow its
    128 slots as well and all 300 queries leave the LDS re-rank.

    On K1q "identical" holds for the rows; the distances are held to 1e-6 (the coarse kinds' bar
    against a fresh index), by design: the wide re-rank finishes the first kWideSlots = 16 failing
    queries of a search (fp64 distances rounded to fp32) and the exact fp32 pass the other 284, so
    query i < 16 and its copy at 256 + i take different routes and their distances differ in the last
    bit (measured: at most 6e-8).  K1c sends all 300 to the one exact pass: bit-equal, as on the fp32
    kind.  (Which 16 queries get the slots is by query index; they were handed out in the order the
    workgroups arrived, and two runs of this search then differed in those bits -- fixed with this
    test.)"""
    rows = np.arange(6000, 9000)
    Q = pick_queries(store["C"][rows], 300, 770)
    Q[:5] = near_tie_free(store["C"][rows], [0, 2999, 63, 64, 1500], 771)     # rows 6000, 8999, 6063, 6064, 7500
    Q[256:] = Q[:44]
    res = verify("filter: 300 queries", store["idx"], store["model"], Q, kinds=[COARSE, Q8], allow=mask_of(rows))
    for (kind, k), (d, r, fb, wide) in res.items():
        bad = np.nonzero((r[256:] != r[:44]).any(axis=1))[0]
        assert bad.size == 0, (kind, k, bad, r[bad[0]], r[256 + bad[0]], d[bad[0]], d[256 + bad[0]])
        diff = float(np.abs(d[256:].astype(np.float64) - d[:44]).max())
        print(f"\n[filter: 300 queries] kind {kind} k {k}: max |d(i) - d(256 + i)| = {diff:.3g}", end="")
        assert diff <= 1e-6 if kind == Q8 else np.array_equal(d[256:], d[:44]), (kind, k, diff)
        assert (r[:5, 0] == [6000, 8999, 6063, 6064, 7500]).all(), (kind, k)
        if kind != F32 and rows_per_range(kind, N, 300) > CAP[kind]:
            assert fb + max(wide, 0) > 0, (kind, k)


def test_sharded_filters():
    """Case 8: cases 3 and 4 on the 3-shard index of test_gpu_dense_mutations.py's case 10, the
    allowed run entirely in one shard's blocks (a contiguous local run there, nothing allowed on the
    other two): lists equal to the single index's and to the oracle."""
    import torch
    sh, one, model, Q, planted, stay, back = sharded_case()
    try:
        B, G = sh.map.B, sh.map.G
        blocks = np.arange(100 * G + 1, 160 * G + 1, G)        # 60 blocks of shard 1: 3 840 rows, local rows 6400..10239
        run = (blocks[:, None] * B + np.arange(B)[None, :]).ravel()
        assert (sh.map.owner_local(run)[0] == 1).all() and np.ptp(sh.map.owner_local(run)[1]) == run.shape[0] - 1
        few = np.array([0, 31, 32, model.size - 1, 10000, int(stay[3])])       # stay[3] is dead
        live_run = run[model.live[run]]
        Q = pick_queries(model.vecs[live_run], 64, 782)
        Q[:3] = near(model.vecs[live_run[[0, 1000, -1]]], np.random.default_rng(781))
        for name, rows in (("run in one shard", run), ("5 allowed rows + 1 dead", few)):
            allow = np.zeros(model.size, bool)
            allow[rows] = True
            words = _bits(allow)
            wdev = torch.from_numpy(words.view(np.int32).copy()).cuda()
            for k in KS:
                assert tie_slack_share(model, Q, k, allow) <= SLACK_CAP
                d1 = sharded_lists(sh, F32, Q, k, words)[0]
                for kind in KINDS:
                    d, r = sharded_lists(sh, kind, Q, k, words)
                    check_lists(d, r, model, Q, k, allow, pad_ref=d1)
                    dw, rw, fb, wide = host_lists(one, kind, Q, k, words)
                    print(f"\n[sharded filter: {name}] kind {kind} k {k}: single index fallbacks {fb}, "
                          f"wide re-ranks {wide}", end="")
                    assert np.array_equal(r, rw), (name, kind, k)
                    assert float(np.abs(d.astype(np.float64) - dw).max()) <= 1e-6, (name, kind, k)
                    if rows is run:
                        assert (r[:3, 0] == live_run[[0, 1000, -1]]).all() and np.isin(r, run).all(), (kind, k)
                    else:
                        assert (r[:, 5:] == -1).all() and not np.isin(r, stay).any(), (kind, k)
                dd, rd = sh.search_dev(torch.from_numpy(Q).cuda(), k, allow=wdev)
                torch.cuda.synchronize()
                d, r = sh.search(Q, k, words)
                assert np.array_equal(rd.cpu().numpy(), r) and np.array_equal(dd.cpu().numpy(), d), (name, k)
                d, r = sh.search(Q, k, wdev)                   # the device bitmap through the host entry
                assert np.array_equal(rd.cpu().numpy(), r), (name, k)
    finally:
        sh.close()
        one.close()
