"""cm_bm25_replace: documents replaced in place on the device index without a rebuild.

The bar is equality with ``BM25Index.build`` over the documents with the replaced rows substituted
(code the replacement does not touch): every exported array, the statistics, df and first keys, the
head-term count, the vocabulary, and scores and rows of every search entry point on both paths, all
with ``==``.  Unfiltered searches are also held against the C oracle over the substituted documents.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 5000                                 # the old index's vocabulary
V2 = V + 2                               # ... and the one the replacement brings (NEW = V)
SAT = 0                                  # tf 300 in document 0
# planted terms (make_docs)
GONE, KEEP, BEFORE, BETWEEN, AFTER, ALLREPL, GROW, SHRINK = (V - 1 - i for i in range(8))
NEW = V
N_DRAWN = V - 8                          # the Zipf draw uses ids below the planted ones
PLANTS = (GONE, KEEP, BEFORE, BETWEEN, AFTER, ALLREPL, GROW, SHRINK, NEW)
K = 10


def _seeded(n, share, seed, also=()):
    rng = np.random.default_rng(seed)
    return sorted(set(rng.choice(n, size=int(n * share), replace=False).tolist()) | set(also))


CASES = {
    "1-all": (1, [0]),
    "64-last": (64, [63]),
    "65-first-word": (65, list(range(32))),
    "1025-one-untouched": (1025, list(range(1024))),
    "2049-one-row": (2049, [1024]),
    "3000-seeded-5pct": (3000, _seeded(3000, 0.05, 77, also=(0, 31, 32, 2999))),
    "3000-contiguous-file": (3000, list(range(1500, 2524))),
    "1000-none": (1000, []),
}
# the cases at which every planted property can hold at once (asserted in make_docs)
ALL_PLANTED = {"3000-seeded-5pct", "3000-contiguous-file"}


@pytest.fixture(scope="module")
def eng():
    from classmate_hip import engine
    return engine


def _bits(mask: np.ndarray) -> np.ndarray:
    words = np.zeros(max((mask.shape[0] + 31) // 32, 1), np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def _csr(docs):
    off = np.zeros(len(docs) + 1, np.int64)
    if docs:
        off[1:] = np.cumsum([d.shape[0] for d in docs])
    flat = np.concatenate(docs).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return flat, off


def _df(docs):
    df = np.zeros(V2, np.int64)
    for t in docs:
        df[np.unique(t)] += 1
    return df


def _draw(rng, p, n, empty_mod=5):
    docs = []
    for d in range(n):
        ln = 0 if d % 17 == empty_mod else int(rng.poisson(100))
        t = rng.choice(N_DRAWN, size=ln, p=p).astype(np.int32)
        if d % 11 == 3 and ln:
            t = np.concatenate([t, np.repeat(t[:1], 5)])
        docs.append(t)
    return docs


def _zipf():
    p = 1.0 / np.arange(1, N_DRAWN + 1) ** 1.1
    return p / p.sum()


def _rows_with(docs, term):
    return [d for d in range(len(docs)) if (docs[d] == term).any()]


def make_docs(n: int, replaced=(), seed: int = 7, require_all: bool = False):
    """Seeded Zipf text as term ids: lengths ~ Poisson(100), every 17th document empty, some that
    repeat a token, SAT with tf 300 in document 0; a fresh draw of the same kind for every replaced
    row; and -- where the replaced set leaves room -- terms planted around it (R = the replaced rows,
    ascending; "kept" = the others):
      * GONE: only in replaced documents' old text; its df goes to 0;
      * NEW (id >= the old vocabulary): only in the new text; the vocabulary grows in the call;
      * KEEP: old and new text of R[0] (tf 1 at the end, then tf 2 from the front) and in kept
        documents on both sides where there are any: the new posting lands at the old one's rank;
      * BEFORE / BETWEEN / AFTER: old postings in kept documents only, the new one in a replaced row
        before the first / between two / after the last of them;
      * ALLREPL: old postings in replaced documents only, new postings in (other) replaced documents;
      * GROW: at most n / 128 documents before, above it after: becomes a head term;
      * SHRINK: above n / 128 documents before, at most that after: stops being one;
      * a replaced document that goes from empty to non-empty, and one the other way.
    Returns (old documents, {row: new document}, the set of planted properties); every planted
    property is checked here, on the host, for the seed in use."""
    rng = np.random.default_rng(seed)
    p = _zipf()
    old = _draw(rng, p, n)
    old[0] = np.concatenate([old[0], np.full(300, SAT, np.int32)])
    R = sorted(set(replaced))
    fresh = _draw(np.random.default_rng(seed + 1000), p, len(R), empty_mod=9)
    new = {r: fresh[i] for i, r in enumerate(R)}
    rset = set(R)
    kept = [d for d in range(n) if d not in rset]

    def plant(docs, term, rows, front=0):
        for d in rows:
            add = np.array([term], np.int32)
            docs[int(d)] = np.concatenate([np.repeat(add, front), docs[int(d)], add] if front else [docs[int(d)], add])

    planted = set()
    if R:
        plant(new, NEW, R[:2])
        planted.add(NEW)
        plant(old, GONE, R[:3])
        planted.add(GONE)
        r0 = R[0]
        plant(old, KEEP, [r0])
        plant(new, KEEP, [r0], front=1)                      # tf 2, first at position 0
        plant(old, KEEP, [d for d in kept if d < r0][-2:] + [d for d in kept if d > r0][:2])
        planted.add(KEEP)
        behind = [d for d in kept if d > r0]
        if behind:
            plant(old, BEFORE, behind[:: max(1, len(behind) // 4)])
            plant(new, BEFORE, [r0])
            planted.add(BEFORE)
        mid = [r for r in R if kept and kept[0] < r < kept[-1]]
        if mid:
            r = mid[len(mid) // 2]
            plant(old, BETWEEN, [d for d in kept if d < r][-3:] + [d for d in kept if d > r][:3])
            plant(new, BETWEEN, [r])
            planted.add(BETWEEN)
        ahead = [d for d in kept if d < R[-1]]
        if ahead:
            plant(old, AFTER, ahead[:: max(1, len(ahead) // 4)])
            plant(new, AFTER, [R[-1]])
            planted.add(AFTER)
    if len(R) >= 4:
        plant(old, ALLREPL, R[:2])
        plant(new, ALLREPL, R[-2:])
        planted.add(ALLREPL)
    g = n // 128
    if R and g <= len(kept):
        plant(old, GROW, rng.choice(kept, size=g, replace=False) if g else [])
        plant(new, GROW, R[-1:])
        planted.add(GROW)
        plant(old, SHRINK, list(rng.choice(kept, size=g, replace=False) if g else []) + R[-1:])
        planted.add(SHRINK)
    if len(R) >= 6:                                      # (rows without a plant of their own above)
        e_in, e_out = R[3], R[4]
        old[e_in] = np.zeros(0, np.int32)
        assert new[e_in].shape[0]
        new[e_out] = np.zeros(0, np.int32)
        assert old[e_out].shape[0]
        planted.add("empty")
    if 0 in new and not new[0].shape[0]:                 # (a corpus of one document keeps a token)
        new[0] = np.array([NEW, 3, 3], np.int32)
    sub = [new.get(d, old[d]) for d in range(n)]
    # -- the planted properties
    before, after = _df(old), _df(sub)
    assert np.bincount(old[0])[SAT] >= 300
    assert all(int(t.max()) < V for t in old if t.shape[0]) and all(int(t.max()) < V2 for t in sub if t.shape[0])
    if n >= 18:
        assert any(t.shape[0] == 0 for t in old)
        assert any(t.shape[0] and np.bincount(t).max() > 1 for t in old[1:])
    if NEW in planted:
        assert before[NEW] == 0 and after[NEW] > 0 and NEW >= V
    if GONE in planted:
        assert before[GONE] > 0 and after[GONE] == 0
    if KEEP in planted:
        r0 = R[0]
        rank_old, rank_new = _rows_with(old, KEEP).index(r0), _rows_with(sub, KEEP).index(r0)
        assert rank_old == rank_new
        assert (np.bincount(old[r0])[KEEP], np.bincount(sub[r0])[KEEP]) == (1, 2)
        assert int(np.nonzero(old[r0] == KEEP)[0][0]) != 0 and int(np.nonzero(sub[r0] == KEEP)[0][0]) == 0
    if BEFORE in planted:
        assert _rows_with(sub, BEFORE)[0] == R[0] < _rows_with(old, BEFORE)[0]
    if BETWEEN in planted:
        o, s = _rows_with(old, BETWEEN), _rows_with(sub, BETWEEN)
        added = sorted(set(s) - set(o))
        assert len(added) == 1 and o[0] < added[0] < o[-1] and set(o) <= set(s)
    if AFTER in planted:
        assert _rows_with(sub, AFTER)[-1] == R[-1] > _rows_with(old, AFTER)[-1]
    if ALLREPL in planted:
        assert set(_rows_with(old, ALLREPL)) <= rset and set(_rows_with(sub, ALLREPL)) <= rset and after[ALLREPL] > 0
        assert set(_rows_with(old, ALLREPL)) != set(_rows_with(sub, ALLREPL))
    if GROW in planted:
        assert before[GROW] <= n / 128.0 < after[GROW]
        assert after[SHRINK] <= n / 128.0 < before[SHRINK]
    if "empty" in planted:
        assert not old[R[3]].shape[0] and sub[R[3]].shape[0] and old[R[4]].shape[0] and not sub[R[4]].shape[0]
    if require_all:
        assert planted == {NEW, GONE, KEEP, BEFORE, BETWEEN, AFTER, ALLREPL, GROW, SHRINK, "empty"}
    return old, new, planted


def make_queries(seed: int = 8, plants=PLANTS):
    """16 queries of 8 tokens: frequent and rare terms, the planted ones, one duplicated token and
    one unknown (-1) each."""
    rng = np.random.default_rng(seed)
    qs = []
    for i in range(16):
        q = [int(x) for x in rng.integers(0, 60, 3)] + [int(x) for x in rng.integers(0, V, 2)]
        q.append(([SAT] + list(plants))[i % (len(plants) + 1)])
        q += [q[0], -1]
        qs.append(q)
    return qs


def _dev_queries(qs):
    import torch
    off = np.zeros(len(qs) + 1, np.int32)
    off[1:] = np.cumsum([len(q) for q in qs])
    return torch.from_numpy(np.concatenate([np.asarray(q, np.int32) for q in qs])).cuda(), torch.from_numpy(off).cuda()


def _state(b):
    e = b.export()
    df, fk = b.term_stats()
    return dict(e, df=df, fk=fk, stats=b.stats(), nd=b.num_docs, npost=b.num_postings, nhead=b.num_head_terms,
                vocab=b.vocab)


def _same_state(got, want):
    for k in ("term_off", "post_doc", "post_tf", "post_pos", "dl", "df", "fk"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert (got[k] == want[k]).all(), k
    for k in ("stats", "nd", "npost", "nhead", "vocab"):
        assert got[k] == want[k], (k, got[k], want[k])       # stats: eps and avgdl bit for bit


def _searches(b, qs, allow_mask):
    """Every entry point's (scores, rows) on both paths."""
    import torch
    out = {}
    qt, qo = _dev_queries(qs)
    words = _bits(allow_mask)
    allow = torch.from_numpy(words.view(np.int32)).cuda()
    for path in (b.PATH_PRUNED, b.PATH_FULL):
        b.set_path(path)
        out[path, "host"] = b.search(qs, K)
        sd, rd = b.search_dev(qt, qo, K)
        torch.cuda.synchronize()
        out[path, "dev"] = (sd.cpu().numpy(), rd.cpu().numpy())
        out[path, "host_filtered"] = b.search(qs, K, words)
        sf, rf = b.search_filtered(qt, qo, K, allow)     # raises on a status bit other than 'eps missing'
        out[path, "dev_filtered"] = (sf.cpu().numpy(), rf.cpu().numpy())
    b.set_path(b.PATH_AUTO)
    return out


def _same_searches(got, want):
    assert got.keys() == want.keys()
    for key in want:
        for a, w in zip(got[key], want[key]):
            assert (np.asarray(a) == np.asarray(w)).all(), key


def _check_oracle(res, docs, qs, vocab):
    from oracle import corc
    flat, off = _csr(docs)
    csr = corc.build_csr(flat, off, vocab)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], len(docs))
    o_sc, o_rw = corc.bm25_topk(csr, idf, float(off[-1]) / len(docs), qs, K)
    for path in (1, 2):
        s, r, n = res[path, "host"]
        for i in range(len(qs)):
            assert r[i][: n[i]].tolist() == o_rw[i][o_rw[i] >= 0].tolist(), (path, i)
            assert s[i][: n[i]].tolist() == o_sc[i][o_rw[i] >= 0].tolist(), (path, i)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _replace_dev(b, rows, docs, vocab):
    flat, off = _csr(docs)
    b.replace_dev(_dev(rows, np.int64), _dev(flat, np.int32), _dev(off, np.int64), vocab)


@pytest.fixture(scope="module")
def queries():
    return make_queries()


@pytest.mark.parametrize("case", list(CASES))
def test_replace_equals_build(eng, queries, case):
    n, rows = CASES[case]
    old, new, planted = make_docs(n, rows, require_all=case in ALL_PLANTED)
    sub = [new.get(d, old[d]) for d in range(n)]
    v2 = V2 if rows else V                           # (an empty replace changes nothing, the vocabulary included)
    qs = queries if rows else make_queries(plants=PLANTS[:-1])
    allow_mask = (np.arange(n) % 3 != 1)
    ref = eng.BM25Index()
    ref.build(*_csr(sub), v2)
    ref.prepare_filtered()
    want, want_s = _state(ref), _searches(ref, qs, allow_mask)
    _check_oracle(want_s, sub, qs, v2)

    b = eng.BM25Index()
    b.build(*_csr(old), V)
    b.prepare_filtered()
    was = _state(b)
    order = list(reversed(rows))                     # the host form takes the rows in any order
    order = order[1::2] + order[::2]
    b.replace(np.asarray(order, np.int64) if len(order) % 2 else order, *_csr([new[r] for r in order]), V2)
    assert b.vocab == v2 and b.num_docs == n
    _same_state(_state(b), want)
    _same_searches(_searches(b, qs, allow_mask), want_s)

    b2 = eng.BM25Index()                             # the device form: ascending rows
    b2.build(*_csr(old), V)
    b2.prepare_filtered()
    _replace_dev(b2, rows, [new[r] for r in rows], V2)
    assert b2.vocab == v2 and b2.num_docs == n
    _same_state(_state(b2), want)
    _same_searches(_searches(b2, qs, allow_mask), want_s)

    if NEW in planted:
        assert want["df"][NEW] > 0 and was["vocab"] == V <= NEW < want["vocab"]
    if GONE in planted:
        assert want["df"][GONE] == 0 and was["df"][GONE] > 0
    if KEEP in planted:                              # same rank in the term's run, another tf and position
        r0 = rows[0]
        po = was["term_off"][KEEP] + was["post_doc"][was["term_off"][KEEP]: was["term_off"][KEEP + 1]].tolist().index(r0)
        pn = want["term_off"][KEEP] + want["post_doc"][want["term_off"][KEEP]: want["term_off"][KEEP + 1]].tolist().index(r0)
        assert po - was["term_off"][KEEP] == pn - want["term_off"][KEEP]
        assert (was["post_tf"][po], want["post_tf"][pn]) == (1, 2) and was["post_pos"][po] != want["post_pos"][pn] == 0
    if BEFORE in planted:                            # first key: (row << 32 | position) of the first posting
        assert (int(want["fk"][BEFORE]) >> 32) == rows[0] < (int(was["fk"][BEFORE]) >> 32)
    if GROW in planted:
        assert was["df"][GROW] <= n / 128.0 < want["df"][GROW]
        assert want["df"][SHRINK] <= n / 128.0 < was["df"][SHRINK]


def test_chained_replaces_appends_and_removes_equal_one_build(eng, queries):
    """Replacements (host rows on an index built with tombstones, a device replace across the
    old/appended border that brings new terms, once more after cm_bm25_set_stats) around an append,
    then a removal."""
    docs, _, _ = make_docs(1000, seed=21)
    fresh = _draw(np.random.default_rng(99), _zipf(), 60, empty_mod=4)
    fresh[7] = np.concatenate([fresh[7], np.array([NEW, NEW, V + 1], np.int32)])
    it = iter(fresh)
    live = np.ones(700, np.uint8)
    live[[3, 31, 32, 333, 640]] = 0
    cur = [(docs[d], int(live[d])) for d in range(700)]      # (document, live flag), in row order
    b = eng.BM25Index()
    b.build(*_csr(docs[:700]), V, live)

    def put(rows):
        new = [next(it) for _ in rows]
        for r, t in zip(rows, new):
            cur[r] = (t, 1)
        return new

    rows = [699, 31, 0, 100, 333, 450]               # 31 and 333 are tombstones: live afterwards
    b.replace(rows, *_csr(put(rows)), V)
    assert b.vocab == V and b.stats()["n_live"] == 697
    b.append(*_csr(docs[700:]), V)
    cur += [(t, 1) for t in docs[700:]]
    rows = list(range(692, 708)) + [999]             # across the border between old and appended rows
    _replace_dev(b, rows, put(rows), V2)             # (fresh[7] is among them: the vocabulary grows)
    assert b.vocab == V2 and b.num_docs == 1000
    b.set_stats(np.full(b.vocab, 0.5), 123456, 9999999, 0.125)   # foreign statistics give way
    rows = [5, 0, 999, 32]
    b.replace(rows, *_csr(put(rows)), V2)
    b.replace([], np.zeros(0, np.int32), np.zeros(1, np.int64), V2)   # no row: nothing changes
    gone = [1, 700, 333]
    b.remove(gone)
    cur[:] = [x for r, x in enumerate(cur) if r not in gone]

    ref = eng.BM25Index()
    ref.build(*_csr([t for t, _ in cur]), V2, np.array([f for _, f in cur], np.uint8))
    assert b.num_docs == len(cur) == 997
    _same_state(_state(b), _state(ref))
    allow_mask = (np.arange(len(cur)) % 4 != 2)
    ref.prepare_filtered()
    b.prepare_filtered()
    _same_searches(_searches(b, queries, allow_mask), _searches(ref, queries, allow_mask))


def test_replace_errors_leave_the_index_unchanged(eng):
    import torch
    qs = make_queries(plants=PLANTS[:-1])            # (terms of the old vocabulary only)
    docs, _, _ = make_docs(300, seed=5)
    fresh = _draw(np.random.default_rng(6), _zipf(), 4, empty_mod=16)
    b = eng.BM25Index()
    b.build(*_csr(docs), V)
    b.prepare_filtered()
    allow_mask = np.arange(300) % 2 == 0
    before, before_s = _state(b), _searches(b, qs, allow_mask)
    two = _csr(fresh[:2])
    for rows in ([4, 300], [-1, 4], [4, 4]):         # a row == num_docs, a negative row, a duplicate
        with pytest.raises(ValueError):
            b.replace(rows, *two, V)
    bad = (np.array([1, V, 2], np.int32), np.array([0, 2, 3], np.int64))
    with pytest.raises(ValueError):
        b.replace([4, 5], *bad, V)                   # a term id >= vocab
    with pytest.raises(ValueError):
        b.replace_dev(_dev([4, 5], np.int64), _dev(bad[0], np.int32), _dev(bad[1], np.int64), V)
    with pytest.raises(ValueError):
        b.replace([4, 5], *two, V - 1)               # vocab below the index's
    for rows in ([5, 4], [4, 4], [4, 300]):          # rows_dev: not strictly ascending, or out of range
        with pytest.raises(ValueError):
            _replace_dev(b, rows, fresh[:2], V)
    torch.cuda.synchronize()
    _same_state(_state(b), before)
    _same_searches(_searches(b, qs, allow_mask), before_s)
    b.replace([299, 4], *two, V)                     # and the handle still takes a replace
    sub = list(docs)
    sub[299], sub[4] = fresh[0], fresh[1]
    ref = eng.BM25Index()
    ref.build(*_csr(sub), V)
    _same_state(_state(b), _state(ref))


def test_replacing_every_text_by_an_empty_one_raises_with_that_state(eng):
    docs, _, _ = make_docs(300, seed=5)
    b = eng.BM25Index()
    b.build(*_csr(docs), V)
    full = [d for d in range(300) if docs[d].shape[0]]
    assert 2 <= 300 - len(full)
    with pytest.raises(ZeroDivisionError):
        b.replace(full, np.zeros(0, np.int32), np.zeros(len(full) + 1, np.int64), V)
    ref = eng.BM25Index()
    with pytest.raises(ZeroDivisionError):
        ref.build(np.zeros(0, np.int32), np.zeros(301, np.int64), V)
    assert b.num_docs == ref.num_docs == 300 and b.num_postings == ref.num_postings == 0
    assert b.stats() == ref.stats()
    assert (b.export()["dl"] == 0).all()             # (ref's wrapper never learnt its vocabulary: not exported)


# ---- the edges of what append, remove and replace share (offsets kernel, survivor pass, install) ----
# These cases exercise cm_bm25_remove and cm_bm25_append as well as the replace; they live here because
# this file's helpers already cover all three calls (tests/test_gpu_bm25_remove.py and _append.py hold
# each call's own cases).
VS, VS2 = 300, 320                       # a small vocabulary, so that one term's run crosses a 64-group
# old posting counts: a multiple of 64 below one workgroup's 2048, then one either side of 2048
EDGE_POSTINGS = (1984, 2047, 2048, 2049)
EDGE_ROWS = [0, 13, 38, 39]              # the first and the last document among them


def _edge_docs(p0: int, seed: int = 3):
    """40 documents of distinct terms below VS (one posting per token) with exactly p0 postings, and
    replacement texts for EDGE_ROWS that use terms at and beyond VS.  Checked here for the seed in
    use: some term behind the first starts its postings at the first slot of a 64-group."""
    rng = np.random.default_rng(seed)
    docs = [rng.choice(VS, size=k, replace=False).astype(np.int32) for k in [50] * 39 + [p0 - 39 * 50]]
    fresh = [rng.choice(VS2, size=60, replace=False).astype(np.int32) for _ in EDGE_ROWS]
    fresh[0] = np.union1d(fresh[0], [VS, VS2 - 1]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(np.concatenate(docs), minlength=VS))])
    assert off[-1] == p0
    assert any(off[t] % 64 == 0 and off[t] < off[t + 1] for t in range(1, VS))
    return docs, fresh


def _edge_queries():
    rng = np.random.default_rng(4)
    return [[int(x) for x in rng.integers(0, VS2, 6)] + [VS, -1] for _ in range(8)]


@pytest.mark.parametrize("p0", EDGE_POSTINGS)
def test_posting_count_edges_equal_build(eng, p0):
    docs, fresh = _edge_docs(p0)
    allow_mask = np.arange(40) % 3 != 1
    qs = _edge_queries()

    def built(texts, vocab):
        ref = eng.BM25Index()
        ref.build(*_csr(texts), vocab)
        ref.prepare_filtered()
        return ref

    b = built(docs, VS2)
    assert b.num_postings == p0
    b.remove(EDGE_ROWS)
    ref = built([t for d, t in enumerate(docs) if d not in EDGE_ROWS], VS2)
    _same_state(_state(b), _state(ref))
    _same_searches(_searches(b, qs, allow_mask[:36]), _searches(ref, qs, allow_mask[:36]))

    b = built(docs, VS)                              # the replacement brings the terms from VS on
    assert b.num_postings == p0
    b.replace(EDGE_ROWS, *_csr(fresh), VS2)
    sub = list(docs)
    for r, t in zip(EDGE_ROWS, fresh):
        sub[r] = t
    ref = built(sub, VS2)
    _same_state(_state(b), _state(ref))
    _same_searches(_searches(b, qs, allow_mask), _searches(ref, qs, allow_mask))


def test_mutations_of_a_tombstoned_index_without_postings(eng):
    """Documents present, none live: no posting to flag, scan or move (all-zero offsets)."""
    docs, fresh = _edge_docs(1984)
    b = eng.BM25Index()
    b.build(*_csr(docs), VS, np.zeros(40, np.uint8))
    assert b.num_docs == 40 and b.num_postings == 0
    b.remove([0, 31, 32, 39])
    kept = [t for d, t in enumerate(docs) if d not in (0, 31, 32, 39)]
    ref = eng.BM25Index()
    ref.build(*_csr(kept), VS, np.zeros(36, np.uint8))
    assert b.num_docs == 36 and b.num_postings == 0
    _same_state(_state(b), _state(ref))
    b.replace([5], *_csr(fresh[:1]), VS2)            # ... and a replacement makes its row live
    kept[5] = fresh[0]
    live = np.zeros(36, np.uint8)
    live[5] = 1
    ref.build(*_csr(kept), VS2, live)
    assert b.num_postings == fresh[0].shape[0]
    _same_state(_state(b), _state(ref))


def test_chained_mutations_with_filtered_searches_between(eng, queries):
    """Append, remove, replace and append again on one handle whose filtered-search table was
    prepared once, before the first: every search entry point after each step, against a build."""
    docs, _, _ = make_docs(420, seed=33)
    fresh = _draw(np.random.default_rng(34), _zipf(), 8, empty_mod=6)
    fresh[0] = np.concatenate([fresh[0], np.array([NEW, V + 1], np.int32)])
    b = eng.BM25Index()
    b.build(*_csr(docs[:300]), V)
    b.prepare_filtered()                             # the log table is for 300 documents
    cur = list(docs[:300])

    def check():
        ref = eng.BM25Index()
        ref.build(*_csr(cur), V2)
        ref.prepare_filtered()
        allow_mask = np.arange(len(cur)) % 3 != 1
        _same_state(_state(b), _state(ref))
        _same_searches(_searches(b, queries, allow_mask), _searches(ref, queries, allow_mask))

    b.append(*_csr(docs[300:400]), V2)               # 400 documents: the table has to grow
    cur += docs[300:400]
    check()
    gone = [0, 64, 299, 300, 399]
    b.remove(gone)
    cur[:] = [t for r, t in enumerate(cur) if r not in gone]
    check()
    rows = [0, 1, 63, 64, 200, 297, 298, 394]
    b.replace(rows, *_csr(fresh), V2)
    for r, t in zip(rows, fresh):
        cur[r] = t
    check()
    b.append(*_csr(docs[400:]), V2)                  # 415 documents: beyond the table once more
    cur += docs[400:]
    check()


# ---- BM25Store -------------------------------------------------------------------------------
def _store_corpus():
    from synth import make_corpus, make_queries
    ids, texts, metas, emb = make_corpus(360, 8, seed=31)
    qtexts, _, _ = make_queries(texts, emb, nq=6, seed=32)
    return ids, texts, metas, qtexts + ["the of and", "nosuchtoken"]


def _record_calls(monkeypatch, eng):
    """('build' | 'append' | 'remove' | 'replace', documents) of every BM25Index call, in order."""
    log = []
    counts = {"build": lambda a: int(np.asarray(a[1]).shape[0]) - 1,
              "append": lambda a: int(np.asarray(a[1]).shape[0]) - 1,
              "remove": lambda a: len(a[0]),
              "replace": lambda a: len(a[0])}
    for name, count in counts.items():
        def patched(self, *a, _real=getattr(eng.BM25Index, name), _name=name, _count=count, **kw):
            log.append((_name, _count(a)))
            return _real(self, *a, **kw)
        monkeypatch.setattr(eng.BM25Index, name, patched)
    return log


def _results(store, queries, where=None):
    return [[(r["id"], r["score"]) for r in rs] for rs in store.search_batch(queries=queries, where=where, top_k=8)]


def _fresh_results(ids, texts, metas, keep, qs, where=None):
    from classmate_hip.retrieval import BM25Store
    one = BM25Store(index_dir=None)
    one.upsert_many(ids=[ids[i] for i in keep], texts=[texts[i] for i in keep], metadatas=[metas[i] for i in keep])
    return _results(one, qs, where)


def test_store_replace_uses_the_device_index(eng, monkeypatch):
    from classmate_hip.retrieval import BM25Store
    ids, texts, metas, qs = _store_corpus()
    texts, metas = list(texts), [dict(m) for m in metas]
    where = {"course": "cs101"}
    log = _record_calls(monkeypatch, eng)
    st = BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:300], texts=texts[:300], metadatas=metas[:300])
    assert any(_results(st, qs)) and any(_results(st, qs, where))
    handle = st._index
    # three documents replaced, one of them moving into the filtered course
    assert metas[31].get("course") != "cs101" and metas[0].get("course") == "cs101"
    for i, j in ((0, 340), (31, 341), (299, 342)):
        texts[i] = texts[j]
    metas[31] = dict(metas[31], course="cs101")
    st.upsert_many(ids=[ids[i] for i in (299, 0, 31)], texts=[texts[i] for i in (299, 0, 31)],
                   metadatas=[metas[i] for i in (299, 0, 31)])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert log == [("build", 300), ("replace", 3)]
    assert st._index is handle and handle.num_docs == 300 and not st._meta_dirty
    keep = list(range(300))
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    assert any(r[0] == ids[31] for rs in _results(st, [texts[31]], where) for r in rs)
    del log[:]
    # one call mixing 2 existing ids with 5 new ones
    texts[7], texts[150] = texts[343], texts[344]
    mix = [300, 7, 301, 302, 150, 303, 304]
    st.upsert_many(ids=[ids[i] for i in mix], texts=[texts[i] for i in mix], metadatas=[metas[i] for i in mix])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert log == [("replace", 2), ("append", 5)]
    assert st._index is handle and handle.num_docs == 305 and not st._meta_dirty
    keep = list(range(305))
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    del log[:]
    # a delete, then a replace, then a new-id upsert without a search between; one id given twice
    st.delete_many([ids[5], ids[200]])
    texts[9] = texts[345]
    st.upsert_many(ids=[ids[9], ids[9]], texts=[texts[346], texts[9]], metadatas=[metas[9], metas[9]])
    st.upsert_many(ids=ids[305:320], texts=texts[305:320], metadatas=metas[305:320])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert log == [("remove", 2), ("replace", 1), ("append", 15)]
    assert st._index is handle and handle.num_docs == 318
    keep = [i for i in range(320) if i not in (5, 200)]
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    assert _results(st, [texts[9]])[0] == _fresh_results(ids, texts, metas, keep, [texts[9]])[0]


def test_store_reopened_from_sidecar_rebuilds_once_then_replaces(eng, monkeypatch, tmp_path):
    """A store opened from its sidecar keeps the rebuild at its first replace (which parses the
    catalog, as tests/test_gpu_dropin.py requires of it); from then on replaces go to the device.
    The results equal a fresh store's, with and without ``where``, at every step."""
    from classmate_hip.retrieval import BM25Store
    from classmate_hip.retrieval import bm25 as bm25_mod
    ids, texts, metas, qs = _store_corpus()
    texts = list(texts)
    where = {"course": "cs101"}
    keep = list(range(300))
    st = BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:300], texts=texts[:300], metadatas=metas[:300])
    st.save()
    del st
    bm25_mod.release_all()                           # a fresh process: open from the files
    log = _record_calls(monkeypatch, eng)
    re = BM25Store(index_dir=tmp_path)
    re.load()
    assert re._entries.pending
    assert any(_results(re, qs))                     # builds from the persisted CSR
    texts[3], texts[150] = texts[340], texts[341]
    re.upsert_many(ids=[ids[150], ids[3]], texts=[texts[150], texts[3]], metadatas=[metas[150], metas[3]])
    got, got_w = _results(re, qs), _results(re, qs, where)
    assert log == [("build", 300), ("build", 300)] and not re._entries.pending and re._csr is None
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    del log[:]
    handle = re._index
    texts[7] = texts[342]
    re.upsert_many(ids=[ids[7]], texts=[texts[7]], metadatas=[metas[7]])
    got, got_w = _results(re, qs), _results(re, qs, where)
    assert log == [("replace", 1)] and re._index is handle and handle.num_docs == 300
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    bm25_mod.release_all()
