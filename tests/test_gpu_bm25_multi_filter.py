"""BM25Store.search_batch(where=[...]) on the row-list route (engine.BM25Index.search_lists), on the
golden 1k corpus: every question equals BM25Store.search with its own clause -- (id, score) with ==
-- with every clause forced to the lists, none of them, and at the default constants; through
HybridRetriever.retrieve_batch; after an append, a replace and a delete; and on a sharded index,
which keeps one filtered search per clause."""
import numpy as np
import pytest

from test_gpu_scale import DIST_TOL

pytestmark = pytest.mark.gpu

# per-question filters (tests/test_gpu_multi_filter.py's list)
FILTERS = [{"course": "cs101"}, {"unit": "u1"}, None, {"doc_type": "pptx"}, {"course": "nope"},
           {"unit": "u2", "course": "math201"}, {"course": "cs101"}, {}, {"course": "math201", "unit": "u2"}]


def filters_for(n):
    return [FILTERS[i % len(FILTERS)] for i in range(n)]


class _Preset:
    def __init__(self, qtexts, qvecs):
        self.by = {q: v for q, v in zip(qtexts, qvecs)}

    def encode_queries(self, qs):
        return np.stack([self.by[q] for q in qs])


def make_stores(corpus):
    from classmate_hip.retrieval import BM25Store, GpuVectorStore
    vs = GpuVectorStore(persist_dir=None)
    vs.upsert(ids=corpus["ids"], documents=corpus["texts"], metadatas=corpus["metas"], embeddings=corpus["emb"])
    bm = BM25Store(index_dir=None)
    bm.upsert_many(ids=corpus["ids"], texts=corpus["texts"], metadatas=corpus["metas"])
    return vs, bm


@pytest.fixture(scope="module")
def stores(corpus):
    return make_stores(corpus)


@pytest.fixture
def list_calls(monkeypatch):
    """Counts engine.BM25Index.search_lists calls (AttributeError where the method does not exist)."""
    from classmate_hip import engine
    calls = []
    real = engine.BM25Index.search_lists
    monkeypatch.setattr(engine.BM25Index, "search_lists", lambda self, *a, **kw: calls.append(1) or real(self, *a, **kw))
    return calls


def _force(monkeypatch, cutoff):
    if cutoff is None:
        monkeypatch.delenv("CM_BM25_LIST_CUTOFF_DIV", raising=False)
    else:
        monkeypatch.setenv("CM_BM25_LIST_CUTOFF_DIV", cutoff)


def assert_search_batch(bm, qs, top_k=10):
    fs = filters_for(len(qs))
    got = bm.search_batch(queries=qs, where=fs, top_k=top_k)
    assert len(got) == len(qs)
    for i, f in enumerate(fs):
        want = bm.search(query=qs[i], where=f, top_k=top_k)
        assert [(r["id"], r["score"]) for r in got[i]] == [(r["id"], r["score"]) for r in want], (i, f)
        for a, b in zip(got[i], want):
            assert a["document"] == b["document"] and a["metadata"] == b["metadata"]
    assert any(got) and not all(got)
    return got


@pytest.mark.parametrize("cutoff", ["1", "1e9", None])
def test_search_batch_equals_one_search_per_question(stores, corpus, monkeypatch, list_calls, cutoff):
    """Every clause through the list route, none of them, and the default constants."""
    _, bm = stores
    _force(monkeypatch, cutoff)
    qs = list(corpus["qtexts"])
    qs[4] = "   "                                       # a blank question gives []
    got = assert_search_batch(bm, qs)
    assert got[4] == []
    if cutoff == "1":
        assert list_calls
    if cutoff == "1e9":
        assert not list_calls
    # top_k beyond the fused lists, beyond every clause's candidates, and python's negative slice
    del list_calls[:]
    assert_search_batch(bm, qs, top_k=400)
    if cutoff is not None:
        assert bool(list_calls) == (cutoff == "1")      # any k >= 1 stays on the list route
    del list_calls[:]
    assert_search_batch(bm, qs, top_k=-3)
    assert not list_calls
    with pytest.raises(ValueError):
        bm.search_batch(queries=qs, where=filters_for(len(qs))[:-1], top_k=10)


def assert_retrieve_batch(vs, bm, corpus):
    from classmate_hip.retrieval import HybridRetriever
    retr = HybridRetriever(vector_store=vs, bm25_store=bm, embedder=_Preset(corpus["qtexts"], corpus["qvecs"]),
                           k_vector=10, k_bm25=10)
    qs = corpus["qtexts"]
    fs = filters_for(len(qs))
    got = retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    for i, f in enumerate(fs):
        want = retr.retrieve(question=qs[i], filters=f, top_k=10)
        assert [r["id"] for r in got[i]] == [r["id"] for r in want], (i, f)
        for a, b in zip(got[i], want):
            assert a["scores"]["fused"] == b["scores"]["fused"] and a["scores"]["bm25_score"] == b["scores"]["bm25_score"]
            da, db = a["scores"]["vector_distance"], b["scores"]["vector_distance"]
            assert (da is None) == (db is None) and (da is None or abs(da - db) <= DIST_TOL)


def test_hybrid_retrieve_batch_takes_the_list_route(stores, corpus, monkeypatch, list_calls):
    monkeypatch.setenv("CM_LIST_CUTOFF_DIV", "1")
    _force(monkeypatch, "1")
    assert_retrieve_batch(stores[0], stores[1], corpus)
    assert list_calls


def test_lists_follow_append_replace_and_delete(corpus, monkeypatch, list_calls):
    """The lists come from the mutated index's live bits and postings."""
    from classmate_hip.retrieval import BM25Store
    _force(monkeypatch, "1")
    n = 400
    ids, texts, metas = corpus["ids"], corpus["texts"], corpus["metas"]
    bm = BM25Store(index_dir=None)
    bm.upsert_many(ids=ids[:n], texts=texts[:n], metadatas=metas[:n])
    qs = corpus["qtexts"][:18]
    assert_search_batch(bm, qs)
    bm.upsert_many(ids=ids[n:n + 150], texts=texts[n:n + 150], metadatas=metas[n:n + 150])          # append
    assert_search_batch(bm, qs)
    held = ids[3:n:7]
    bm.upsert_many(ids=held, texts=[texts[(i * 13 + 500) % len(texts)] for i in range(len(held))],    # replace
                   metadatas=[metas[(i * 5 + 1) % len(metas)] for i in range(len(held))])
    assert_search_batch(bm, qs)
    bm.delete_many(ids[1:n:5])                                                                       # delete
    assert_search_batch(bm, qs)
    assert len(list_calls) >= 4


def test_sharded_index_keeps_the_per_clause_route(corpus, monkeypatch, list_calls):
    from classmate_hip import multidev
    from classmate_hip.retrieval import bm25 as bm25_mod, vector_store as vs_mod
    monkeypatch.setenv("CM_DEVICES", "0,0")
    monkeypatch.setenv("CM_SHARD_BLOCK", "64")
    _force(monkeypatch, "1")
    try:
        vs, bm = make_stores(corpus)
        assert_search_batch(bm, corpus["qtexts"])
        assert isinstance(bm._index, multidev.ShardedBM25Index) and not hasattr(bm._index, "search_lists")
        assert_retrieve_batch(vs, bm, corpus)
        assert not list_calls
    finally:
        bm25_mod.release_all()
        vs_mod.release_all()
