"""K2a (the pruned BM25 search's tail pass) runs one work unit (query group, run of ranges) per
one-wave block, in whatever order the device starts them: the order only decides how early each
query's running threshold tightens, so the pruned search must return the bits of the full K2 scan
(set_path(1)) and of the C oracle whatever the unit count and shape.

Shapes are the smallest that reach every branch of the unit mapping: 5 000 docs (5 ranges: one or
two units per query group, fewer blocks than the 8 XCD shares of the grid) and 70 000 docs (69
ranges: not a multiple of the 4-range run or super-range), batches of 1, 5, 64 and 257 queries (a
partial query group; 65 groups), k = 1 and 10.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB = 4096
HEAVY = 7            # a term planted in ~45 % of the documents of one range: its list overflows K2a's LDS slice
DOCS = [5_000, 70_000]


def _bits(mask: np.ndarray) -> np.ndarray:
    n = mask.shape[0]
    words = np.zeros((n + 31) // 32, np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def _corpus(nd):
    rng = np.random.default_rng(1000 + nd)
    lens = np.maximum(rng.poisson(24, nd), 2)
    off = np.zeros(nd + 1, np.int64)
    off[1:] = np.cumsum(lens)
    p = 1.0 / np.arange(1, VOCAB + 1) ** 1.07
    toks = rng.choice(VOCAB, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    toks[toks == HEAVY] = HEAVY + 1
    r0 = 2048 if nd > 4096 else 1024           # the heavy term lives in one 1024-doc range only
    docs = r0 + np.nonzero(rng.random(1024) < 0.45)[0]
    toks[off[docs]] = HEAVY
    return toks, off, lens


def _queries(toks, off, lens, nq, seed):
    """8-term queries drawn from documents (Zipf draws: head and tail terms mixed), plus the special ones."""
    rng = np.random.default_rng(seed)
    nd = lens.shape[0]
    qs = [[int(toks[off[d] + rng.integers(0, lens[d])]) for _ in range(8)] for d in rng.integers(0, nd, nq)]
    special = [[-1, -1],                                            # no known term
               [int(x) for x in rng.integers(0, VOCAB, 23)],        # > 16 terms: the re-score path
               [HEAVY, int(toks[off[3]])],                          # a range that overflows K2A_CAP
               [HEAVY]]
    for i, q in enumerate(special[:nq]):
        qs[(i * 5) % nq] = q
    return qs


@pytest.fixture(scope="module")
def eng():
    from classmate_hip import engine
    return engine


_INDEX = {}


def _index(eng, nd):
    """One index and one oracle CSR per corpus size, shared by every case (never modified)."""
    if nd not in _INDEX:
        from oracle import corc
        toks, off, lens = _corpus(nd)
        b = eng.BM25Index()
        b.build(toks, off, VOCAB)
        b.set_head_policy(1.0 / 128, 8 << 30)
        assert b.num_head_terms > 0
        csr = corc.build_csr(toks, off, VOCAB)
        idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], nd)
        _INDEX[nd] = dict(b=b, toks=toks, off=off, lens=lens, nd=nd, csr=csr, idf=idf, avgdl=float(lens.sum()) / nd)
    return _INDEX[nd]


@pytest.fixture(params=DOCS)
def index(request, eng):
    return _index(eng, request.param)


def _both_paths(b, qs, k, allow=None):
    b.set_path(1)
    s1, r1, n1 = b.search(qs, k, allow)
    b.set_path(2)
    s2, r2, n2 = b.search(qs, k, allow)
    assert np.array_equal(r1, r2) and np.array_equal(s1, s2) and np.array_equal(n1, n2)
    return s2, r2


def _check_oracle(ix, qs, k, s, r):
    from oracle import corc
    o_sc, o_rw = corc.bm25_topk(ix["csr"], ix["idf"], ix["avgdl"], qs, k)
    for i in range(len(qs)):
        assert r[i].tolist() == o_rw[i].tolist(), i
        assert s[i].tolist() == o_sc[i].tolist(), i


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [1, 5, 64, 257])
def test_pruned_equals_full_scan_and_oracle(index, nq, k):
    qs = _queries(index["toks"], index["off"], index["lens"], nq, seed=nq)
    s, r = _both_paths(index["b"], qs, k)
    _check_oracle(index, qs, k, s, r)
    if nq >= 5:
        assert index["b"].last_rescored() > 0      # the > 16-term query and the overflowing range were re-scored


def test_with_allow_mask(index):
    qs = _queries(index["toks"], index["off"], index["lens"], 64, seed=3)
    mask = np.zeros(index["nd"], bool)
    mask[::3] = True
    s, r = _both_paths(index["b"], qs, 10, _bits(mask))
    assert all(int(x) % 3 == 0 for x in r.ravel() if x >= 0)


def test_after_deletes(eng, index):
    """Every fifth document deleted (live mask) on a handle of its own: their postings are still
    walked and must be dropped by the tail pass as by the full scan."""
    nd = index["nd"]
    live = np.ones(nd, np.uint8)
    live[::5] = 0
    b = eng.BM25Index()
    b.build(index["toks"], index["off"], VOCAB, live)
    b.set_head_policy(1.0 / 128, 8 << 30)
    qs = _queries(index["toks"], index["off"], index["lens"], 64, seed=4)
    s, r = _both_paths(b, qs, 10)
    assert all(int(x) % 5 != 0 for x in r.ravel() if x >= 0)


def test_few_units_and_all_cost_in_one_unit(eng):
    """One query on the 5-range corpus: 2 units, so six of the grid's eight XCD shares are empty; the
    heavy term's query has all its cost in the one unit that holds its range."""
    ix = _index(eng, 5_000)
    for q in ([HEAVY], [HEAVY, HEAVY + 1], [int(ix["toks"][ix["off"][4100]])]):
        s, r = _both_paths(ix["b"], [q], 10)
        _check_oracle(ix, [q], 10, s, r)


def test_two_searches_one_handle_different_batches(index):
    """Back-to-back searches on one handle and one (grow-only) workspace with different batch sizes:
    nothing of the earlier search's unit count or lists may leak into the later one."""
    b = index["b"]
    b.set_path(2)
    for nq in (257, 5, 64, 1, 257):
        qs = _queries(index["toks"], index["off"], index["lens"], nq, seed=50 + nq)
        s, r, _ = b.search(qs, 10)
        _check_oracle(index, qs, 10, s, r)
