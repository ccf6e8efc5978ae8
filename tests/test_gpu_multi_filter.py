"""One where clause per question in a batch, at store and retriever level, on the golden 1k corpus:
GpuVectorStore.query_batch(where=[...]), BM25Store.search_batch(where=[...]) and
HybridRetriever.retrieve_batch(filters=[...]) against the same stores asked one question at a time."""
import numpy as np
import pytest

from test_gpu_scale import DIST_TOL

pytestmark = pytest.mark.gpu

# per-question filters, in ask_question's form (build_where_filter turns them into Chroma clauses)
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


def assert_query_batch(vs, corpus, top_k=24):
    from classmate_hip.retrieval import build_where_filter
    qv = corpus["qvecs"]
    wheres = [build_where_filter(f) if f else f for f in filters_for(len(qv))]
    got = vs.query_batch(query_embeddings=qv, where=wheres, top_k=top_k, include_embeddings=True)
    assert len(got) == len(qv)
    n_empty = 0
    for i, w in enumerate(wheres):
        want = vs.query(query_embeddings=qv[i], where=w, top_k=top_k, include_embeddings=True)
        assert [r["id"] for r in got[i]] == [r["id"] for r in want], (i, w)
        np.testing.assert_allclose([r["distance"] for r in got[i]], [r["distance"] for r in want], rtol=0,
                                   atol=DIST_TOL)
        for a, b in zip(got[i], want):
            assert a["metadata"] == b["metadata"] and a["document"] == b["document"]
            assert np.array_equal(a["embedding"], b["embedding"])
        n_empty += not want
    assert 0 < n_empty < len(qv)
    return got


@pytest.mark.parametrize("cutoff", ["1", "1e9", None])
def test_vector_store_query_batch(stores, corpus, monkeypatch, cutoff):
    """Every clause through the list route, none of them, and the default cutoff."""
    from classmate_hip import engine
    vs, _ = stores
    if cutoff is None:
        monkeypatch.delenv("CM_LIST_CUTOFF_DIV", raising=False)
    else:
        monkeypatch.setenv("CM_LIST_CUTOFF_DIV", cutoff)
    calls = []
    real = engine.DenseIndex.search_lists
    monkeypatch.setattr(engine.DenseIndex, "search_lists", lambda self, *a, **kw: calls.append(1) or real(self, *a, **kw))
    assert_query_batch(vs, corpus)
    assert bool(calls) == (cutoff != "1e9")      # at the default, course + unit allows 1/9 of the rows
    with pytest.raises(ValueError):
        vs.query_batch(query_embeddings=corpus["qvecs"], where=[None], top_k=5)


def test_bm25_search_batch(stores, corpus):
    _, bm = stores
    qs = corpus["qtexts"]
    fs = filters_for(len(qs))
    got = bm.search_batch(queries=qs, where=fs, top_k=10)
    for i, f in enumerate(fs):
        want = bm.search(query=qs[i], where=f, top_k=10)
        assert [(r["id"], r["score"]) for r in got[i]] == [(r["id"], r["score"]) for r in want], (i, f)
    assert any(got) and not all(got)
    with pytest.raises(ValueError):
        bm.search_batch(queries=qs, where=fs[:-1], top_k=10)


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
    with pytest.raises(ValueError):
        retr.retrieve_batch(questions=qs, filters=fs[:2], top_k=10)


def test_hybrid_retrieve_batch(stores, corpus):
    assert_retrieve_batch(stores[0], stores[1], corpus)


def test_sharded_store_takes_the_per_clause_route(corpus, monkeypatch):
    """Two shards on one card: the sharded index has no search_lists, every clause falls back to one
    ordinary filtered search, with the same answers."""
    from classmate_hip import multidev
    from classmate_hip.retrieval import bm25 as bm25_mod, vector_store as vs_mod
    monkeypatch.setenv("CM_DEVICES", "0,0")
    monkeypatch.setenv("CM_SHARD_BLOCK", "64")
    try:
        vs, bm = make_stores(corpus)
        assert isinstance(vs._index, multidev.ShardedDenseIndex) and not hasattr(vs._index, "search_lists")
        assert_query_batch(vs, corpus)
        assert_retrieve_batch(vs, bm, corpus)
    finally:
        bm25_mod.release_all()
        vs_mod.release_all()
