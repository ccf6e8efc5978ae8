"""cm_bm25_append: documents appended to the device index without a rebuild.

The bar is equality with ``BM25Index.build`` over the concatenation (code the append does not
touch): every exported array, the statistics, df and first keys, the head-term count, and scores
and rows of every search entry point, all with ``==``.  Unfiltered searches are also held against
the C oracle over the concatenation, the way tests/test_gpu_engine.py does.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V_OLD, V_NEW = 5000, 5040      # the delta brings term ids >= the old vocabulary
SAT, FADE = 0, V_OLD - 1       # planted terms (below)
K = 10
SHAPES = [(1, 1), (63, 1), (1000, 24), (1024, 1), (1023, 1061), (3000, 25), (0, 500)]
# shapes at which FADE's df, just above n_old / 128, is at most (n_old + n_new) / 128 afterwards
FADES = {(1000, 24), (1023, 1061)}


@pytest.fixture(scope="module")
def eng():
    from classmate_hip import engine
    return engine


def _bits(mask: np.ndarray) -> np.ndarray:
    words = np.zeros((mask.shape[0] + 31) // 32, np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def _csr(docs):
    off = np.zeros(len(docs) + 1, np.int64)
    if docs:
        off[1:] = np.cumsum([d.shape[0] for d in docs])
    flat = np.concatenate(docs).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return flat, off


def make_docs(n_old: int, n_new: int, seed: int = 7):
    """Seeded Zipf text as term ids: lengths ~ Poisson(100), some empty documents, some that repeat
    a token, and
      * SAT: a frequent term with tf 300 in document 0 -- a head candidate by df whose tf does not
        fit the head tiles' byte, so build_head_tiles drops it;
      * FADE: in floor(n_old / 128) + 1 old documents and in no new one -- a head term of the old
        index that (at the FADES shapes) is none of the new one;
      * term ids >= V_OLD in the new documents only.
    The planted properties are checked here, on the host, for the seed in use."""
    rng = np.random.default_rng(seed)
    n = n_old + n_new
    p = 1.0 / np.arange(1, V_OLD) ** 1.1        # ids [0, V_OLD - 1): FADE is planted, not drawn
    p /= p.sum()
    docs = []
    for d in range(n):
        ln = 0 if d % 17 == 5 else int(rng.poisson(100))
        t = rng.choice(V_OLD - 1, size=ln, p=p).astype(np.int32)
        if d >= n_old and ln:
            new = rng.random(ln) < 0.03
            t[new] = rng.integers(V_OLD, V_NEW, int(new.sum()))
        if d % 11 == 3 and ln:
            t = np.concatenate([t, np.repeat(t[:1], 5)])
        docs.append(t)
    docs[0] = np.concatenate([docs[0], np.full(300, SAT, np.int32)])
    if n_new:
        docs[n_old] = np.concatenate([docs[n_old], np.array([V_OLD + 1], np.int32)])
    n_fade = n_old // 128 + 1 if n_old else 0
    for d in rng.choice(n_old, size=min(n_fade, n_old), replace=False) if n_old else []:
        docs[int(d)] = np.concatenate([docs[int(d)], np.array([FADE], np.int32)])
    # -- the planted properties
    df = np.zeros(V_NEW, np.int64)
    for t in docs:
        df[np.unique(t)] += 1
    assert np.bincount(docs[0], minlength=1)[SAT] >= 300 and df[SAT] > n / 128.0
    if n >= 18:
        assert any(t.shape[0] == 0 for t in docs)
        assert any(t.shape[0] and np.bincount(t).max() > 1 for t in docs[1:])
    if n_new:
        assert max(int(t.max()) for t in docs[n_old:] if t.shape[0]) >= V_OLD
        assert not any((t == FADE).any() for t in docs[n_old:])
    if n_old:
        assert max(int(t.max()) for t in docs[:n_old] if t.shape[0]) < V_OLD
        assert df[FADE] == n_fade and df[FADE] > n_old / 128.0
    if (n_old, n_new) in FADES:
        assert df[FADE] <= n / 128.0
    return docs


def make_queries(seed: int = 8):
    """16 queries of 8 tokens: frequent and rare terms, the planted ones, new-vocabulary ids, one
    duplicated token and one unknown (-1) each."""
    rng = np.random.default_rng(seed)
    qs = []
    for i in range(16):
        q = [int(x) for x in rng.integers(0, 60, 3)] + [int(x) for x in rng.integers(0, V_OLD, 2)]
        q.append([SAT, FADE, V_OLD + 1, int(rng.integers(V_OLD, V_NEW))][i % 4])
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
        s, r, n = b.search(qs, K)
        out[path, "host"] = (s, r, n)
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
    csr = corc.build_csr(flat, off, V_NEW)
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


@pytest.mark.parametrize("n_old,n_new", SHAPES)
def test_append_equals_build(eng, queries, n_old, n_new):
    docs = make_docs(n_old, n_new)
    n = n_old + n_new
    allow_mask = (np.arange(n) % 3 != 1)
    ref = eng.BM25Index()
    ref.build(*_csr(docs), V_NEW)
    ref.prepare_filtered()
    want, want_s = _state(ref), _searches(ref, queries, allow_mask)
    _check_oracle(want_s, docs, queries)

    b = eng.BM25Index()
    if n_old:
        b.build(*_csr(docs[:n_old]), V_OLD)
        assert b.num_head_terms > 0
        df_old, _ = b.term_stats()
        assert df_old[FADE] > n_old / 128.0          # a head term of the old index by df
    b.prepare_filtered()                             # the log table is for n_old documents
    b.append(*_csr(docs[n_old:]), V_NEW)
    assert b.vocab == V_NEW
    _same_state(_state(b), want)
    _same_searches(_searches(b, queries, allow_mask), want_s)
    if (n_old, n_new) in FADES:                      # ... and none of the new one
        assert want["df"][FADE] <= n / 128.0


def test_chained_appends_equal_one_build(eng, queries):
    """Five uneven appends -- one with an unchanged vocabulary, one from device tensors, one after
    cm_bm25_set_stats -- to an index built with tombstones."""
    import torch
    docs = make_docs(700, 650, seed=21)
    cuts = [700, 701, 764, 765, 1100, 1350]
    live = np.ones(700, np.uint8)
    live[[0, 5, 31, 32, 333, 699]] = 0
    live_all = np.concatenate([live, np.ones(650, np.uint8)])
    ref = eng.BM25Index()
    ref.build(*_csr(docs), V_NEW, live_all)
    b = eng.BM25Index()
    b.build(*_csr(docs[:700]), V_OLD, live)
    vocabs = [V_NEW, V_NEW, V_NEW, V_NEW, V_NEW]     # grows with the first append, then stays
    for i in range(5):
        flat, off = _csr(docs[cuts[i]:cuts[i + 1]])
        if i == 2:   # statistics a sharded caller installed give way to the index's own, as after a build
            b.set_stats(np.full(b.vocab, 0.5), 123456, 9999999, 0.125)
        if i == 3:
            b.append_dev(torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), vocabs[i])
        else:
            b.append(flat, off, vocabs[i])
        assert b.num_docs == cuts[i + 1]
    b.append(np.zeros(0, np.int32), np.zeros(1, np.int64), V_NEW + 7)   # no document: nothing changes
    assert b.vocab == V_NEW
    _same_state(_state(b), _state(ref))
    allow_mask = (np.arange(1350) % 4 != 2)
    ref.prepare_filtered()
    b.prepare_filtered()
    _same_searches(_searches(b, queries, allow_mask), _searches(ref, queries, allow_mask))


def test_append_errors_leave_the_index_unchanged(eng, queries):
    docs = make_docs(300, 40, seed=5)
    b = eng.BM25Index()
    b.build(*_csr(docs[:300]), V_OLD)
    b.prepare_filtered()
    allow_mask = np.arange(300) % 2 == 0
    before, before_s = _state(b), _searches(b, queries, allow_mask)
    flat, off = _csr(docs[300:])

    bad = flat.copy()
    bad[3] = V_NEW                                   # term id == vocab
    with pytest.raises(ValueError):
        b.append(bad, off, V_NEW)
    with pytest.raises(ValueError):                  # vocab below the handle's
        b.append(np.minimum(flat, V_OLD - 2), off, V_OLD - 1)
    dec = off.copy()
    dec[5] = dec[4] - 1                              # decreasing offsets
    with pytest.raises(ValueError):
        b.append(flat, dec, V_NEW)
    with pytest.raises(RuntimeError, match="65535"):  # CM_EUNSUPPORTED: a tf of 65536
        b.append(np.full(65536, 3, np.int32), np.array([0, 65536], np.int64), V_NEW)
    import torch                                     # the device form finds the bad id in its key kernel
    with pytest.raises(ValueError):
        b.append_dev(torch.from_numpy(bad).cuda(), torch.from_numpy(off).cuda(), V_NEW)

    assert b.vocab == V_OLD
    _same_state(_state(b), before)
    _same_searches(_searches(b, queries, allow_mask), before_s)
    b.append(flat, off, V_NEW)                       # and the handle still takes the append
    ref = eng.BM25Index()
    ref.build(*_csr(docs), V_NEW)
    _same_state(_state(b), _state(ref))


def test_sharded_append_equals_build(queries):
    import torch
    from classmate_hip.multidev import ShardedBM25Index
    docs = make_docs(200, 301, seed=9)
    ref = ShardedBM25Index([0, 0, 0], block=64)
    ref.build(*_csr(docs), V_NEW)
    b = ShardedBM25Index([0, 0, 0], block=64)
    b.build(*_csr(docs[:200]), V_OLD)
    b.append(*_csr(docs[200:201]), V_NEW)            # row 200: shard 0 alone; 1 and 2 keep V_OLD
    assert [sh.vocab for sh in b.shards] == [V_NEW, V_OLD, V_OLD]
    mid = ShardedBM25Index([0, 0, 0], block=64)
    mid.build(*_csr(docs[:201]), V_NEW)
    assert b.stats() == mid.stats() and (b.idf == mid.idf).all()
    for al in (None, _bits(np.arange(201) % 3 != 1)):
        assert all((x == y).all() for x, y in zip(b.search(queries, K, al), mid.search(queries, K, al)))
    b.append(*_csr(docs[201:]), V_NEW)
    assert b.num_docs == ref.num_docs == 501
    assert [sh.num_docs for sh in b.shards] == [sh.num_docs for sh in ref.shards]
    assert b.stats() == ref.stats() and b.eps == ref.eps and (b.idf == ref.idf).all()
    eb, er = b.export(), ref.export()
    assert all((eb[k] == er[k]).all() for k in er)
    allow = _bits(np.arange(501) % 3 != 1)
    for al in (None, allow):
        for x, y in zip(b.search(queries, K, al), ref.search(queries, K, al)):
            assert (x == y).all()
    qt, qo = _dev_queries(queries)
    for x, y in zip(b.search_dev(qt, qo, K), ref.search_dev(qt, qo, K)):
        assert (x == y).all()
    al = torch.from_numpy(allow.view(np.int32)).cuda()
    for x, y in zip(b.search_filtered(qt, qo, K, al), ref.search_filtered(qt, qo, K, al)):
        assert (x == y).all()


# ---- BM25Store -------------------------------------------------------------------------------
def _store_corpus():
    from synth import make_corpus, make_queries
    ids, texts, metas, emb = make_corpus(360, 8, seed=31)
    qtexts, _, _ = make_queries(texts, emb, nq=6, seed=32)
    return ids, texts, metas, qtexts + ["the of and", "nosuchtoken"]


def _count_builds(monkeypatch, eng):
    calls = []
    real = eng.BM25Index.build

    def build(self, *a, **kw):
        calls.append(int(np.asarray(a[1]).shape[0]) - 1)
        return real(self, *a, **kw)
    monkeypatch.setattr(eng.BM25Index, "build", build)
    return calls


def _results(store, queries, where=None):
    return [[(r["id"], r["score"]) for r in rs] for rs in store.search_batch(queries=queries, where=where, top_k=8)]


def test_store_upserts_append_to_the_device_index(eng, monkeypatch):
    from classmate_hip.retrieval import BM25Store
    ids, texts, metas, qs = _store_corpus()
    where = {"course": "cs101"}
    calls = _count_builds(monkeypatch, eng)
    st = BM25Store(index_dir=None)
    cuts = [0, 200, 203, 360]
    handle = None
    for i in range(3):
        a, e = cuts[i], cuts[i + 1]
        st.upsert_many(ids=ids[a:e], texts=texts[a:e], metadatas=metas[a:e])
        got = _results(st, qs, where if i == 1 else None)
        assert calls == [200]                        # one build; the later upserts are appended
        one = BM25Store(index_dir=None)
        one.upsert_many(ids=ids[:e], texts=texts[:e], metadatas=metas[:e])
        assert got == _results(one, qs, where if i == 1 else None) and any(got)
        del calls[1:]                                # (the comparison store's own build)
        if handle is None:
            handle = st._index
        assert st._index is handle and handle.num_docs == e
    # a replace in place and a delete rebuild, as before
    st.upsert_many(ids=[ids[7]], texts=[texts[300]], metadatas=[metas[7]])
    st.delete_many([ids[11]])
    got, got_w = _results(st, qs), _results(st, qs, where)
    assert calls == [200, 359] and st._index.num_docs == 359
    keep = [i for i in range(360) if i != 11]
    one = BM25Store(index_dir=None)
    one.upsert_many(ids=[ids[i] for i in keep], texts=[texts[300] if i == 7 else texts[i] for i in keep],
                    metadatas=[metas[i] for i in keep])
    assert got == _results(one, qs) and got_w == _results(one, qs, where)


def test_store_reopened_from_sidecar_appends_without_parsing(eng, monkeypatch, tmp_path):
    from classmate_hip.retrieval import BM25Store
    from classmate_hip.retrieval import bm25 as bm25_mod
    ids, texts, metas, qs = _store_corpus()
    st = BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:300], texts=texts[:300], metadatas=metas[:300])
    st.save()
    del st
    bm25_mod.release_all()                           # a fresh process: open from the files
    calls = _count_builds(monkeypatch, eng)
    re = BM25Store(index_dir=tmp_path)
    re.load()
    assert re._entries.pending
    re.upsert_many(ids=ids[300:], texts=texts[300:], metadatas=metas[300:])
    got = _results(re, qs)
    assert re._entries.pending                       # no old record was materialised
    assert calls == [300] and re._index.num_docs == 360   # built from the persisted CSR, then appended
    one = BM25Store(index_dir=None)
    one.upsert_many(ids=ids, texts=texts, metadatas=metas)
    assert got == _results(one, qs) and any(got)
    re.upsert_many(ids=["extra"], texts=[texts[5] + " gradient"], metadatas=[metas[5]])
    one.upsert_many(ids=["extra"], texts=[texts[5] + " gradient"], metadatas=[metas[5]])
    assert _results(re, qs) == _results(one, qs) and re._entries.pending
    assert calls[:2] == [300, 360] and len(calls) == 2     # (the second is the comparison store's)
