"""cm_bm25_remove: documents removed from the device index without a rebuild.

The bar is equality with ``BM25Index.build`` over the surviving documents (code the removal does
not touch): every exported array, the statistics, df and first keys, the head-term count, and
scores and rows of every search entry point, all with ``==``.  Unfiltered searches are also held
against the C oracle over the survivors, the way tests/test_gpu_bm25_append.py does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 5000
SAT = 0                                  # tf 300 in document 0: a head candidate by df that the tiles drop
GONE, FIRST, GROW, SHRINK = V - 1, V - 2, V - 3, V - 4    # planted terms (make_docs)
N_DRAWN = V - 4                          # the Zipf draw uses ids below the planted ones
K = 10


def _seeded(n, share, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n, size=int(n * share), replace=False)).tolist()


CASES = {
    "1-all": (1, [0]),
    "64-last": (64, [63]),
    "65-first-word": (65, list(range(32))),
    "1000-every-third": (1000, list(range(0, 1000, 3))),
    "1025-one-survivor": (1025, list(range(1024))),
    "2049-one-row": (2049, [1024]),
    "3000-seeded-5pct": (3000, _seeded(3000, 0.05, 77)),
    "3000-contiguous-file": (3000, list(range(1500, 2524))),
    "1000-none": (1000, []),
}
# the cases at which every planted property can hold at once (asserted in make_docs)
ALL_PLANTED = {"1000-every-third", "3000-seeded-5pct", "3000-contiguous-file"}


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
    df = np.zeros(V, np.int64)
    for t in docs:
        df[np.unique(t)] += 1
    return df


def make_docs(n: int, removed=(), seed: int = 7, require_all: bool = False):
    """Seeded Zipf text as term ids: lengths ~ Poisson(100), every 17th document empty, some that
    repeat a token, SAT with tf 300 in document 0, and -- where the removal set leaves room -- four
    terms planted around it (n' = the survivors' number):
      * GONE: only in removed documents; its df goes to 0 and it leaves the first-occurrence order;
      * FIRST: in the first removed document and in survivors behind it only; its first key changes;
      * GROW: in floor(n / 128) survivors, at most n / 128 before and above n' / 128 after: a head
        term of the new index that was none of the old one;
      * SHRINK: in floor(n' / 128) survivors and enough removed documents to lie above n / 128
        before: a head term of the old index that is none of the new one.
    Returns (docs, the set of planted terms); the planted properties are checked here, on the
    host, for the seed in use."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, N_DRAWN + 1) ** 1.1
    p /= p.sum()
    docs = []
    for d in range(n):
        ln = 0 if d % 17 == 5 else int(rng.poisson(100))
        t = rng.choice(N_DRAWN, size=ln, p=p).astype(np.int32)
        if d % 11 == 3 and ln:
            t = np.concatenate([t, np.repeat(t[:1], 5)])
        docs.append(t)
    docs[0] = np.concatenate([docs[0], np.full(300, SAT, np.int32)])
    gone = sorted(set(removed))
    gone_set = set(gone)
    kept = [d for d in range(n) if d not in gone_set]
    n1 = len(kept)

    def plant(term, rows):
        for d in rows:
            docs[int(d)] = np.concatenate([docs[int(d)], np.array([term], np.int32)])

    planted = set()
    if gone:
        plant(GONE, gone[:3])
        planted.add(GONE)
        behind = [d for d in kept if d > gone[0]]
        if behind:
            plant(FIRST, [gone[0]] + behind[:: max(1, len(behind) // 5)])
            planted.add(FIRST)
    g = n // 128
    if 1 <= g <= n1 and g > n1 / 128.0:
        plant(GROW, rng.choice(kept, size=g, replace=False))
        planted.add(GROW)
    m = n1 // 128
    k = n // 128 + 1 - m
    if 1 <= k <= len(gone) and m <= n1:
        plant(SHRINK, list(rng.choice(kept, size=m, replace=False)) + list(rng.choice(gone, size=k, replace=False)))
        planted.add(SHRINK)
    # -- the planted properties
    before, after = _df(docs), _df([docs[d] for d in kept])
    assert np.bincount(docs[0])[SAT] >= 300 and before[SAT] > n / 128.0
    assert all(int(t.max()) < V for t in docs if t.shape[0])
    if n >= 18:
        assert any(t.shape[0] == 0 for t in docs)
        assert any(t.shape[0] and np.bincount(t).max() > 1 for t in docs[1:])
    if GONE in planted:
        assert before[GONE] > 0 and after[GONE] == 0
    if FIRST in planted:
        first = min(d for d in range(n) if (docs[d] == FIRST).any())
        assert first == gone[0] and after[FIRST] > 0
    if GROW in planted:
        assert 0 < before[GROW] <= n / 128.0 and after[GROW] > n1 / 128.0
    if SHRINK in planted:
        assert before[SHRINK] > n / 128.0 and after[SHRINK] <= n1 / 128.0
    if require_all:
        assert planted == {GONE, FIRST, GROW, SHRINK}
    return docs, planted


def make_queries(seed: int = 8):
    """16 queries of 8 tokens: frequent and rare terms, the planted ones, one duplicated token and
    one unknown (-1) each."""
    rng = np.random.default_rng(seed)
    qs = []
    for i in range(16):
        q = [int(x) for x in rng.integers(0, 60, 3)] + [int(x) for x in rng.integers(0, V, 2)]
        q.append([SAT, GONE, FIRST, GROW, SHRINK][i % 5])
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
    """Every entry point's (scores, rows) on both paths.  An index without documents answers the
    host search with no result and refuses the device forms (ValueError), whoever made it."""
    import torch
    out = {}
    qt, qo = _dev_queries(qs)
    words = _bits(allow_mask)
    allow = torch.from_numpy(words.view(np.int32)).cuda()
    for path in (b.PATH_PRUNED, b.PATH_FULL):
        b.set_path(path)
        out[path, "host"] = b.search(qs, K)
        if b.num_docs == 0:
            with pytest.raises(ValueError):
                b.search_dev(qt, qo, K)
            continue
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


def _check_oracle(res, docs, qs):
    from oracle import corc
    flat, off = _csr(docs)
    csr = corc.build_csr(flat, off, V)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], len(docs))
    o_sc, o_rw = corc.bm25_topk(csr, idf, float(off[-1]) / len(docs), qs, K)
    for path in (1, 2):
        s, r, n = res[path, "host"]
        for i in range(len(qs)):
            assert r[i][: n[i]].tolist() == o_rw[i][o_rw[i] >= 0].tolist(), (path, i)
            assert s[i][: n[i]].tolist() == o_sc[i][o_rw[i] >= 0].tolist(), (path, i)


@pytest.fixture(scope="module")
def queries():
    return make_queries()


@pytest.mark.parametrize("case", list(CASES))
def test_remove_equals_build(eng, queries, case):
    n, removed = CASES[case]
    docs, planted = make_docs(n, removed, require_all=case in ALL_PLANTED)
    gone = set(removed)
    kept = [docs[d] for d in range(n) if d not in gone]
    n1 = len(kept)
    allow_mask = (np.arange(n1) % 3 != 1)
    ref = eng.BM25Index()
    ref.build(*_csr(kept), V)
    ref.prepare_filtered()
    want, want_s = _state(ref), _searches(ref, queries, allow_mask)
    if n1:
        _check_oracle(want_s, kept, queries)

    b = eng.BM25Index()
    b.build(*_csr(docs), V)
    b.prepare_filtered()                             # the log table is for n documents
    old = _state(b)
    if SHRINK in planted:
        assert old["df"][SHRINK] > n / 128.0 and old["nhead"] > 0
    # any order, duplicates allowed
    rows = list(reversed(removed)) + removed[:2]
    b.remove(np.asarray(rows, np.int64) if len(rows) % 2 else rows)
    assert b.vocab == V and b.num_docs == n1
    _same_state(_state(b), want)
    _same_searches(_searches(b, queries, allow_mask), want_s)
    if GONE in planted:
        assert want["df"][GONE] == 0 and old["df"][GONE] > 0
    if FIRST in planted:                             # first key: (row << 32 | position) of the first posting
        assert want["fk"][FIRST] != old["fk"][FIRST] and (int(old["fk"][FIRST]) >> 32) == removed[0]
    if GROW in planted:
        assert old["df"][GROW] <= n / 128.0 and want["df"][GROW] > n1 / 128.0
    if SHRINK in planted:
        assert want["df"][SHRINK] <= n1 / 128.0


def test_chained_removes_and_appends_equal_one_build(eng, queries):
    """Removals (host rows, then a device bitmap across the old/new border, then once more after
    cm_bm25_set_stats) around an append, on an index built with tombstones."""
    import torch
    docs, _ = make_docs(1000, seed=21)
    live = np.ones(700, np.uint8)
    live[[3, 31, 32, 333, 640]] = 0
    surv = [(docs[d], int(live[d])) for d in range(700)]      # (document, live flag), in row order
    b = eng.BM25Index()
    b.build(*_csr(docs[:700]), V, live)

    def drop(rows):
        gone = set(rows)
        surv[:] = [x for r, x in enumerate(surv) if r not in gone]

    rows = [699, 31, 0, 100, 101, 450]               # 31 is a tombstone
    b.remove(rows)
    drop(rows)
    assert b.num_docs == len(surv) == 694
    b.append(*_csr(docs[700:]), V)
    surv += [(t, 1) for t in docs[700:]]
    assert b.num_docs == 994
    rows = list(range(688, 700)) + [2, 993]          # across the border between old and appended rows
    mask = np.zeros(994, bool)
    mask[rows] = True
    words = _bits(mask)
    words[-1] |= np.uint32(1) << np.uint32(31)       # a bit at or above num_docs: ignored
    b.remove_dev(torch.from_numpy(words.view(np.int32)).cuda())
    drop(rows)
    assert b.num_docs == len(surv) == 980
    b.set_stats(np.full(b.vocab, 0.5), 123456, 9999999, 0.125)   # foreign statistics give way
    rows = [0, 5, 979]
    b.remove(rows)
    drop(rows)
    b.remove_dev(torch.zeros((977 + 31) // 32, dtype=torch.int32).cuda())   # no bit: nothing changes
    b.remove([])

    ref = eng.BM25Index()
    ref.build(*_csr([t for t, _ in surv]), V, np.array([f for _, f in surv], np.uint8))
    assert b.num_docs == len(surv) == 977
    _same_state(_state(b), _state(ref))
    allow_mask = (np.arange(len(surv)) % 4 != 2)
    ref.prepare_filtered()
    b.prepare_filtered()
    _same_searches(_searches(b, queries, allow_mask), _searches(ref, queries, allow_mask))


def test_remove_errors_leave_the_index_unchanged(eng, queries):
    docs, _ = make_docs(300, seed=5)
    b = eng.BM25Index()
    b.build(*_csr(docs), V)
    b.prepare_filtered()
    allow_mask = np.arange(300) % 2 == 0
    before, before_s = _state(b), _searches(b, queries, allow_mask)
    with pytest.raises(ValueError):
        b.remove([4, 300])                           # a row == num_docs
    with pytest.raises(ValueError):
        b.remove([-1])
    _same_state(_state(b), before)
    _same_searches(_searches(b, queries, allow_mask), before_s)
    b.remove([4, 299])                               # and the handle still takes a removal
    kept = [docs[d] for d in range(300) if d not in (4, 299)]
    ref = eng.BM25Index()
    ref.build(*_csr(kept), V)
    _same_state(_state(b), _state(ref))
    # only empty documents remain: the error a build of them gives, with their state installed
    empty = [d for d in range(298) if kept[d].shape[0] == 0]
    assert len(empty) >= 2
    with pytest.raises(ZeroDivisionError):
        b.remove([d for d in range(298) if kept[d].shape[0]])
    ref = eng.BM25Index()
    with pytest.raises(ZeroDivisionError):
        ref.build(*_csr([kept[d] for d in empty]), V)
    assert b.num_docs == ref.num_docs == len(empty) and b.num_postings == ref.num_postings == 0
    assert b.stats() == ref.stats()


# ---- BM25Store -------------------------------------------------------------------------------
def _store_corpus():
    from synth import make_corpus, make_queries
    ids, texts, metas, emb = make_corpus(360, 8, seed=31)
    qtexts, _, _ = make_queries(texts, emb, nq=6, seed=32)
    return ids, texts, metas, qtexts + ["the of and", "nosuchtoken"]


def _record_calls(monkeypatch, eng):
    """('build' | 'append' | 'remove', documents) of every BM25Index call, in order."""
    log = []
    counts = {"build": lambda a: int(np.asarray(a[1]).shape[0]) - 1,
              "append": lambda a: int(np.asarray(a[1]).shape[0]) - 1,
              "remove": lambda a: len(a[0])}
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


def test_store_delete_uses_the_device_index(eng, monkeypatch):
    from classmate_hip.retrieval import BM25Store
    ids, texts, metas, qs = _store_corpus()
    where = {"course": "cs101"}
    log = _record_calls(monkeypatch, eng)
    st = BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:300], texts=texts[:300], metadatas=metas[:300])
    assert any(_results(st, qs)) and any(_results(st, qs, where))
    handle = st._index
    gone = [0, 17, 31, 32, 150, 298, 299]
    st.delete_many([ids[i] for i in gone[:4]] + ["no-such-id"] + [ids[i] for i in gone[4:]])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert log == [("build", 300), ("remove", 7)]
    assert st._index is handle and handle.num_docs == 293 and not st._meta_dirty
    keep = [i for i in range(300) if i not in gone]
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    del log[:]
    # deletes and new-id upserts without a search between: one remove, then one append
    st.delete_many([ids[5], ids[200]])
    st.upsert_many(ids=ids[300:340], texts=texts[300:340], metadatas=metas[300:340])
    st.delete_many([ids[305], ids[100]])
    st.upsert_many(ids=ids[340:], texts=texts[340:], metadatas=metas[340:])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert log == [("remove", 3), ("append", 59)]
    assert st._index is handle and handle.num_docs == 349
    keep = [i for i in range(360) if i not in gone + [5, 200, 305, 100]]
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    assert got_w == _fresh_results(ids, texts, metas, keep, qs, where) and any(got_w)
    del log[:]
    # a replace in place followed by a delete rebuilds, as before
    st.upsert_many(ids=[ids[7]], texts=[texts[300]], metadatas=[metas[7]])
    st.delete_many([ids[11]])
    got = _results(st, qs)
    assert log == [("build", 348)] and st._index.num_docs == 348
    keep = [i for i in keep if i != 11]
    t2 = list(texts)
    t2[7] = texts[300]
    assert got == _fresh_results(ids, t2, metas, keep, qs)


def test_store_reopened_from_sidecar_deletes_without_parsing(eng, monkeypatch, tmp_path):
    from classmate_hip.retrieval import BM25Store
    from classmate_hip.retrieval import bm25 as bm25_mod
    ids, texts, metas, qs = _store_corpus()
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
    re.delete_many([ids[3], ids[150], ids[299]])
    got = _results(re, qs)
    assert re._entries.pending                       # no surviving record was materialised
    assert log == [("build", 300), ("remove", 3)] and re._index.num_docs == 297
    keep = [i for i in range(300) if i not in (3, 150, 299)]
    assert got == _fresh_results(ids, texts, metas, keep, qs) and any(got)
    where = {"course": "cs101"}
    assert _results(re, qs, where) == _fresh_results(ids, texts, metas, keep, qs, where) and re._entries.pending
