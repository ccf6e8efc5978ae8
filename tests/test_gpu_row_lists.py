"""The row-list builder that cm_dense_search_lists and cm_bm25_search_lists share (cm_row_lists.h), at
its edges, against numpy alone: a single partial word, exactly one 256-word block, a second block of
one partial word; an empty bitmap, bits at and above N, words past the end, deleted rows, a bitmap no
query uses, and a filter_of that is not grouped by filter.  k is at least every list's length, so
the rows that come back are the list itself: no tolerance on the sets.  Host and dev=True forms."""
import types

import numpy as np
import pytest

from test_gpu_scale import DIST_TOL

pytestmark = pytest.mark.gpu

SIZES = (31, 8192, 8197)      # words: 1 (partial); 256 = one count block, no partial; 257 = a block of one partial word
D = 64
K_DENSE, K_BM25 = 256, 300    # cm_max_topk; beyond every list
V = 40                        # BM25 vocabulary: small, so that every query hits
FILTER_OF = np.asarray([1, 0, 2, 1, 2], np.int32)   # not grouped by filter; bitmap 3 is used by no query
EXTRA_WORDS = 3


def _words(n, rows):
    w = np.zeros((n + 31) // 32, np.uint32)
    rows = np.asarray(rows, np.int64)
    np.bitwise_or.at(w, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return w


def _make(n):
    rng = np.random.default_rng(1000 + n)
    inner = np.arange(1, n - 1)
    dead = np.sort(rng.choice(inner, size=max(3, n // 10), replace=False))
    live = np.ones(n, bool)
    live[dead] = False
    must = [0, n - 1] + [r for r in (255 * 32, 255 * 32 + 31, 256 * 32, 256 * 32 + 3) if r < n]
    f1 = np.union1d(rng.choice(n, size=20 if n < 64 else 200, replace=False), must)
    f2 = np.union1d(rng.choice(np.nonzero(live)[0], size=min(256, n // 3), replace=False), dead[::2])
    f3 = rng.choice(n, size=min(100, n // 2), replace=False)
    clauses = [np.zeros(0, np.int64), f1, f2, np.sort(f3)]
    words = [_words(n, c) for c in clauses]
    if n % 32:
        words[1][-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)        # every bit at or above n
    words[1] = np.concatenate([words[1], np.full(EXTRA_WORDS, 0xFFFFFFFF, np.uint32)])   # and words past the end
    assert (live[f2]).sum() <= 256 and (~live[f2]).any() and live[f2].any() and len(f1) < K_DENSE
    want = []
    for f in FILTER_OF:
        m = np.zeros(n, bool)
        m[clauses[f]] = True
        want.append(np.nonzero(m & live)[0])
    return types.SimpleNamespace(n=n, rng=rng, dead=dead, live=live, words=words, want=want)


def _forms(words, dev, device):
    if not dev:
        return words
    import torch
    return [torch.from_numpy(w.view(np.int32)).to(device) for w in words]


@pytest.fixture(scope="module", params=SIZES)
def dense(request):
    import torch
    from classmate_hip import engine
    w = _make(request.param)
    C = w.rng.standard_normal((w.n, D)).astype(np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    Q = w.rng.standard_normal((len(FILTER_OF), D)).astype(np.float32)
    idx = engine.DenseIndex(D)
    idx.upsert(C, np.arange(w.n, dtype=np.int64))
    idx.delete(w.dead)
    C64, Q64 = C.astype(np.float64), Q.astype(np.float64)
    w.exact = 1.0 - (Q64 @ C64.T) / (np.linalg.norm(Q64, axis=1)[:, None] * np.linalg.norm(C64, axis=1)[None, :])
    w.idx, w.Q, w.device = idx, Q, torch.device("cuda", idx.device)
    yield w
    idx.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_dense_lists_are_the_allowed_live_rows(dense, dev):
    import torch
    w = dense
    q = torch.from_numpy(w.Q).to(w.device) if dev else w.Q
    dist, rows = w.idx.search_lists(q, K_DENSE, _forms(w.words, dev, w.device), FILTER_OF, dev=dev)
    if dev:
        dist, rows = dist.cpu().numpy(), rows.cpu().numpy()
    assert dist.shape == rows.shape == (len(FILTER_OF), K_DENSE)
    for i, want in enumerate(w.want):
        m = want.shape[0]
        assert np.array_equal(np.sort(rows[i, :m]), want), i
        assert (rows[i, m:] == -1).all() and (dist[i, m:] == 0.0).all(), i
        np.testing.assert_allclose(dist[i, :m], w.exact[i, rows[i, :m]], atol=DIST_TOL, rtol=0)
        d, r = dist[i, :m], rows[i, :m]
        assert ((d[:-1] < d[1:]) | ((d[:-1] == d[1:]) & (r[:-1] < r[1:]))).all(), i


@pytest.fixture(scope="module", params=SIZES)
def bm25(request):
    import torch
    from classmate_hip import engine
    w = _make(request.param)
    docs = [w.rng.integers(0, V, size=int(w.rng.integers(3, 12))).astype(np.int32) for _ in range(w.n)]
    off = np.zeros(w.n + 1, np.int64)
    off[1:] = np.cumsum([d.shape[0] for d in docs])
    idx = engine.BM25Index()
    idx.build(np.concatenate(docs), off, V, live=w.live.astype(np.uint8))
    w.queries = [w.rng.choice(V, size=3, replace=False).tolist() for _ in FILTER_OF]
    w.ref = [idx.search([q], K_BM25, w.words[f]) for q, f in zip(w.queries, FILTER_OF)]   # one query, one bitmap
    w.idx, w.device = idx, torch.device("cuda", idx.device)
    yield w
    idx.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_bm25_lists_are_the_allowed_live_rows(bm25, dev):
    w = bm25
    scores, rows, nvalid = w.idx.search_lists(w.queries, K_BM25, _forms(w.words, dev, w.device), FILTER_OF, dev=dev)
    if dev:
        scores, rows = scores.cpu().numpy(), rows.cpu().numpy()
    assert scores.shape == rows.shape == (len(FILTER_OF), K_BM25)
    for i, want in enumerate(w.want):
        m = want.shape[0]
        assert nvalid[i] == m, i
        assert np.array_equal(np.sort(rows[i, :m]), want), i
        assert (rows[i, m:] == -1).all() and (scores[i, m:] == 0.0).all(), i
        r_scores, r_rows, r_n = w.ref[i]
        assert r_n[0] == m and np.array_equal(rows[i], r_rows[0]) and np.array_equal(scores[i], r_scores[0]), i
