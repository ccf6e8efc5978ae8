"""cm_dense_search_lists: a batch whose queries carry different where clauses, answered from row
lists without a scan (engine.DenseIndex.search_lists).

Every case checks the lists against the exact fp64 oracle of a numpy model at the project's bars
(test_gpu_dense_mutations.check_lists: distances within DIST_TOL, sets equal except rows within TIE
of the k-th exact distance, order strict where exact neighbours differ by more than TIE, lists
ascending in (distance, row), pads byte-equal to the fp32 kind's output for the same query under the
same single bitmap).  The 2 % cap on tie slack is a condition on the inputs: the queries of a clause
are chosen tie-free among the rows that clause allows (pick_queries over those rows) or planted next
to one of them, and every (clause, k) asserts tie_slack_share <= SLACK_CAP from the oracle alone.
"""
import numpy as np
import pytest

from test_gpu_dense_mutations import (F32, KS, SLACK_CAP, Model, _bits, base_store, check_lists, exact_dist, gauss,
                                      host_lists, near, pick_queries, tie_slack_share)
from test_gpu_scale import DIST_TOL, TIE, unit_rows

pytestmark = pytest.mark.gpu

D, N = 768, 20480
LIST_CHUNK = 256            # kListChunk of cm_dense_lists.inc: rows of one list per workgroup
QUERY_TILE = 8              # kListQT: queries per workgroup


def mask_of(n, rows):
    m = np.zeros(n, bool)
    m[np.asarray(rows, np.int64)] = True
    return m


def clause_queries(C, rows, nq, seed, planted=()):
    """nq queries for the clause that allows `rows`: random directions whose exact top-(k + 1) among
    those rows is tie-free (pick_queries over C[rows]; plain Gaussian directions for a clause with
    fewer rows than k + 2), the first len(planted) replaced by a vector next to row planted[j]."""
    rows = np.asarray(rows, np.int64)
    if rows.shape[0] >= max(KS) + 16:
        Q = pick_queries(C[rows], nq, seed)
    else:
        Q = gauss(nq, C.shape[1], seed)
    rng = np.random.default_rng(seed + 1)
    for j, r in enumerate(planted[:nq]):
        Q[j] = near(C[r], rng)
    return Q


def mixed_clauses(n):
    """The six bitmaps of the mixed batch, as row sets."""
    scattered = 4096 + np.random.default_rng(11).choice(n - 4096, 2000, replace=False)
    few = np.array([5, 640, 4097, 9999, 12345, 16384, n - 1])
    return [np.arange(100, 140), np.sort(scattered), np.array([7777]), np.zeros(0, np.int64), few,
            np.arange(6000, 9000)]


def mixed_batch(C, nq=64):
    """(clauses, Q, filter_of, planted): six clauses dealt round-robin over nq queries; planted[i] is
    the row query i sits next to (-1: none)."""
    clauses = mixed_clauses(C.shape[0])
    filter_of = np.arange(nq, dtype=np.int32) % len(clauses)
    Q = np.zeros((nq, C.shape[1]), np.float32)
    planted = np.full(nq, -1, np.int64)
    plant = {0: [100, 139, 120], 1: [int(clauses[1][0]), int(clauses[1][-1])], 2: [7777], 4: [int(clauses[4][-1])],
             5: [6000, 8999, 7000]}
    for f, rows in enumerate(clauses):
        sel = np.nonzero(filter_of == f)[0]
        p = plant.get(f, [])[:sel.shape[0]]
        Q[sel] = clause_queries(C, rows if rows.shape[0] else np.arange(C.shape[0]), sel.shape[0], 700 + 10 * f, p)
        planted[sel[:len(p)]] = p
    return clauses, Q, filter_of, planted


def assert_slack(model, Q, filter_of, masks, ks=KS):
    """The condition on the inputs: per (clause, k) the oracle's tie slack stays under the cap."""
    for f, m in enumerate(masks):
        sel = np.nonzero(filter_of == f)[0]
        for k in ks:
            if sel.shape[0]:
                assert tie_slack_share(model, Q[sel], k, m) <= SLACK_CAP, (f, k)


def check_batch(idx, model, Q, filter_of, masks, ks=KS):
    """search_lists over the whole batch, every query checked under its own clause's mask."""
    assert_slack(model, Q, filter_of, masks, ks)
    words = [_bits(m) for m in masks]
    out = {}
    for k in ks:
        dist, rows = idx.search_lists(Q, k, words, filter_of)
        assert dist.shape == rows.shape == (Q.shape[0], k)
        for f, m in enumerate(masks):
            sel = np.nonzero(filter_of == f)[0]
            if not sel.shape[0]:
                continue
            pad_ref = host_lists(idx, F32, np.ascontiguousarray(Q[sel]), k, words[f])[0]
            check_lists(dist[sel], rows[sel], model, np.ascontiguousarray(Q[sel]), k, m, pad_ref)
        out[k] = (dist, rows)
    return out


@pytest.fixture(scope="module")
def store():
    from classmate_hip import engine
    C, _ = base_store(N, 901, nq=32)
    idx = engine.DenseIndex(D)
    model = Model(D)
    rows = np.arange(N, dtype=np.int64)
    idx.upsert(C, rows)
    model.upsert(C, rows)
    yield dict(C=C, idx=idx, model=model)
    idx.close()


def test_mixed_batch(store):
    C, idx, model = store["C"], store["idx"], store["model"]
    clauses, Q, filter_of, planted = mixed_batch(C)
    masks = [mask_of(N, r) for r in clauses]
    res = check_batch(idx, model, Q, filter_of, masks)
    has = np.nonzero(planted >= 0)[0]
    assert has.shape[0] >= 10
    for k, (dist, rows) in res.items():
        assert (rows[has, 0] == planted[has]).all() and (dist[has, 0] < 1e-3).all(), k
        empty = np.nonzero(filter_of == 3)[0]
        assert (rows[empty] == -1).all()
        assert ((rows[filter_of == 2] >= 0).sum(axis=1) == 1).all()          # the single row 7777
        assert ((rows[filter_of == 4] >= 0).sum(axis=1) == 7).all()          # 7 rows, fewer than k


def test_dead_rows(store):
    C, idx, model = store["C"], store["idx"], store["model"]
    clauses, Q, filter_of, _ = mixed_batch(C)
    masks = [mask_of(N, r) for r in clauses]
    rng = np.random.default_rng(31)
    gone = np.concatenate([rng.choice(clauses[0], 10, replace=False), rng.choice(clauses[1], 100, replace=False)])
    idx.delete(gone)
    model.delete(gone)
    try:
        res = check_batch(idx, model, Q, filter_of, masks)
        for k, (dist, rows) in res.items():
            assert not np.isin(rows, gone).any(), k
            assert ((rows[filter_of == 0] >= 0).sum(axis=1) == min(k, 30)).all()
    finally:
        idx.upsert(C[gone], gone)
        model.upsert(C[gone], gone)
    check_batch(idx, model, Q, filter_of, masks, ks=(10,))                    # the rows are back


def test_ties(store):
    C, idx, model = store["C"], store["idx"], store["model"]
    rows = np.concatenate([[300, 9000], np.arange(6000, 9000)])
    old = C[9000:9001].copy()
    idx.upsert(C[300:301], np.array([9000]))
    try:
        q = np.ascontiguousarray(C[300:301])
        for k in KS:
            dist, got = idx.search_lists(q, k, [_bits(mask_of(N, rows))], np.zeros(1, np.int32))
            assert got[0, :2].tolist() == [300, 9000], (k, got[0, :4])
            assert dist[0, 0].tobytes() == dist[0, 1].tobytes() and abs(float(dist[0, 0])) < 1e-6
            assert (got[0] >= 0).all() and dist[0, 2] > 0.5
    finally:
        idx.upsert(old, np.array([9000]))


def check_short(dist, rows, model, Q, mask, pad_ref):
    """A list shorter than k, beyond check_lists' oracle depth: every allowed live row, in exact order
    where the exact distances differ by more than TIE, then pads as the fp32 kind writes them."""
    d = exact_dist(model, Q, mask)
    for i in range(Q.shape[0]):
        want = np.nonzero(np.isfinite(d[i]))[0]
        want = want[np.lexsort((want, d[i, want]))]
        m = want.shape[0]
        assert m < rows.shape[1] and (rows[i, m:] == -1).all() and (rows[i, :m] >= 0).all()
        assert dist[i, m:].tobytes() == pad_ref[i, m:].tobytes()
        assert sorted(rows[i, :m].tolist()) == sorted(want.tolist())
        np.testing.assert_allclose(dist[i, :m], d[i, rows[i, :m]], rtol=0, atol=DIST_TOL)
        dd, rr = dist[i, :m], rows[i, :m]
        assert not ((dd[1:] < dd[:-1]) | ((dd[1:] == dd[:-1]) & (rr[1:] <= rr[:-1]))).any()
        for j in np.nonzero(np.diff(d[i, want]) > TIE)[0]:
            assert rows[i, j] == want[j] or abs(dist[i, j] - d[i, want[j]]) < TIE, (i, j)


@pytest.mark.parametrize("dim,n", [(100, 300), (384, 1000)])
def test_other_shapes(dim, n):
    """Below the coarse kinds' 16 384 rows; dim 100 pads to ld 128, 300 rows end inside a word."""
    from classmate_hip import engine
    C = unit_rows(n, dim, seed=77)
    idx = engine.DenseIndex(dim)
    model = Model(dim)
    idx.upsert(C, np.arange(n, dtype=np.int64))
    model.upsert(C, np.arange(n, dtype=np.int64))
    try:
        rng = np.random.default_rng(5)
        clauses = [np.arange(n - 100, n),                                     # ends at the last row
                   np.sort(rng.choice(n, 150, replace=False)),
                   np.array([0, 31, 32, n - 1])]
        masks = [mask_of(n, r) for r in clauses]
        nq = 18
        filter_of = np.arange(nq, dtype=np.int32) % 3
        Q = np.zeros((nq, dim), np.float32)
        for f, r in enumerate(clauses):
            sel = np.nonzero(filter_of == f)[0]
            Q[sel] = clause_queries(C, r, sel.shape[0], 40 + f, planted=[int(r[-1])])
        assert_slack(model, Q, filter_of, masks, ks=(10,))
        words = [_bits(m) for m in masks]
        if n % 32:
            for w in words:
                w[-1] |= np.uint32(0xffffffff) << np.uint32(n % 32)          # bits at and above size: ignored
        dist, rows = idx.search_lists(Q, 10, np.stack(words), filter_of)
        for f, m in enumerate(masks):
            sel = np.nonzero(filter_of == f)[0]
            qs = np.ascontiguousarray(Q[sel])
            pad_ref = host_lists(idx, F32, qs, 10, words[f])[0]
            check_lists(dist[sel], rows[sel], model, qs, 10, m, pad_ref)
            assert (rows[sel[0], 0] == clauses[f][-1]) and dist[sel[0], 0] < 1e-3
        assert rows.max() == n - 1
        # k = 256 against lists of 100, 150 and 4 rows
        dist, rows = idx.search_lists(Q, 256, np.stack(words), filter_of)
        for f, m in enumerate(masks):
            sel = np.nonzero(filter_of == f)[0]
            qs = np.ascontiguousarray(Q[sel])
            check_short(dist[sel], rows[sel], model, qs, m, host_lists(idx, F32, qs, 256, words[f])[0])
    finally:
        idx.close()


def test_many_tiles_and_chunk_edges(store):
    """300 queries on one 3 000-row clause (38 query tiles x 12 chunks), and clauses of exactly one
    chunk and one chunk + 1 rows."""
    C, idx, model = store["C"], store["idx"], store["model"]
    rng = np.random.default_rng(9)
    clauses = [np.arange(6000, 9000), np.sort(rng.choice(N, LIST_CHUNK, replace=False)),
               np.sort(rng.choice(N, LIST_CHUNK + 1, replace=False))]
    masks = [mask_of(N, r) for r in clauses]
    nqs = (300, QUERY_TILE + 1, QUERY_TILE + 1)
    filter_of = np.concatenate([np.full(n, f, np.int32) for f, n in enumerate(nqs)])
    Q = np.concatenate([clause_queries(C, r, n, 60 + f, planted=[int(r[0]), int(r[-1])])
                        for f, (r, n) in enumerate(zip(clauses, nqs))])
    perm = rng.permutation(Q.shape[0])                                      # the clauses interleaved
    Q, filter_of = np.ascontiguousarray(Q[perm]), filter_of[perm]
    res = check_batch(idx, model, Q, filter_of, masks)
    for f, r in enumerate(clauses):
        first = int(np.nonzero(perm == sum(nqs[:f]))[0][0])
        last = int(np.nonzero(perm == sum(nqs[:f]) + 1)[0][0])
        for k, (dist, rows) in res.items():
            assert rows[first, 0] == r[0] and rows[last, 0] == r[-1], (f, k)


def test_return_vectors(store):
    C, idx = store["C"], store["idx"]
    clauses, Q, filter_of, _ = mixed_batch(C, nq=12)
    words = [_bits(mask_of(N, r)) for r in clauses]
    dist, rows, vecs = idx.search_lists(Q, 10, words, filter_of, return_vectors=True)
    d2, r2 = idx.search_lists(Q, 10, words, filter_of)
    assert dist.tobytes() == d2.tobytes() and rows.tobytes() == r2.tobytes()
    assert vecs.shape == (12, 10, D)
    live = rows >= 0
    assert live.any() and (~live).any()
    assert np.array_equal(vecs[live], C[rows[live]])
    assert not vecs[~live].any()


def test_argument_errors(store):
    idx = store["idx"]
    q = np.zeros((2, D), np.float32)
    w = np.zeros((1, N // 32), np.uint32)
    with pytest.raises(ValueError):
        idx.search_lists(q, 10, w, np.array([0, 1], np.int32))               # filter_of out of range
    with pytest.raises(ValueError):
        idx.search_lists(q, 10, w[:, :-1], np.zeros(2, np.int32))            # bitmap too short
    with pytest.raises(ValueError):
        idx.search_lists(q, 10, w, np.zeros(3, np.int32))                    # one entry per query
    with pytest.raises(RuntimeError):
        idx.search_lists(q, 257, w, np.zeros(2, np.int32))                   # above cm_max_topk: unsupported
