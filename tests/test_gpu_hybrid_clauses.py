"""HybridRetriever.retrieve_batch(filters=[one per question]) on the device chain
(device_batch.retrieve_batch_clauses) against the host path (CM_RETRIEVE_DEVICE=0) on the same
stores: whole result dicts with ==, under every routing of the clauses, on stores that hold different
documents, with pools shorter than the MMR pool, after mutations, and with the BM25 epsilon floors
cached per (BM25 version, clause)."""
import numpy as np
import pytest

from test_gpu_multi_filter import _Preset, filters_for, make_stores

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls device_batch.retrieve_batch_clauses answers."""
    from classmate_hip.retrieval import device_batch
    calls = []
    real = device_batch.retrieve_batch_clauses
    monkeypatch.setattr(device_batch, "retrieve_batch_clauses", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    return calls


def both_paths(retr, monkeypatch, spy, **kw):
    """(device chain's result, host path's result) of one retrieve_batch call."""
    monkeypatch.delenv("CM_RETRIEVE_DEVICE", raising=False)
    n = len(spy)
    got = retr.retrieve_batch(**kw)
    assert len(spy) == n + 1, "the device chain did not answer"
    monkeypatch.setenv("CM_RETRIEVE_DEVICE", "0")
    want = retr.retrieve_batch(**kw)
    assert len(spy) == n + 1
    monkeypatch.delenv("CM_RETRIEVE_DEVICE")
    return got, want


def force(monkeypatch, cutoff):
    for name in ("CM_LIST_CUTOFF_DIV", "CM_BM25_LIST_CUTOFF_DIV"):
        if cutoff is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, cutoff)


@pytest.fixture(scope="module")
def stores(corpus):
    return make_stores(corpus)


@pytest.mark.parametrize("cutoff", ["1", "1e9", None])
def test_equals_the_host_path(stores, corpus, monkeypatch, spy, cutoff):
    """Every clause on the list routes, none of them, and the default constants."""
    from classmate_hip.retrieval import HybridRetriever
    retr = HybridRetriever(vector_store=stores[0], bm25_store=stores[1],
                           embedder=_Preset(corpus["qtexts"], corpus["qvecs"]), k_vector=10, k_bm25=10)
    qs = list(corpus["qtexts"])
    fs = filters_for(len(qs))
    force(monkeypatch, cutoff)
    for top_k in (10, 3, 0, -4):
        got, want = both_paths(retr, monkeypatch, spy, questions=qs, filters=fs, top_k=top_k)
        assert got == want, top_k
        if top_k == 10:
            assert any(got) and any(len(g) < 10 for g in got)
            assert any(r["scores"]["vector_distance"] is not None and r["scores"]["bm25_score"] is not None
                       for g in got for r in g)
    assert got == retr.retrieve_batch(questions=qs, filters=tuple(fs), top_k=-4)      # a tuple is a sequence too
    with pytest.raises(ValueError):
        retr.retrieve_batch(questions=qs, filters=fs[:2], top_k=10)


def disjoint_stores(corpus):
    from classmate_hip.retrieval import BM25Store, GpuVectorStore
    ids, texts, metas, emb = corpus["ids"], corpus["texts"], corpus["metas"], corpus["emb"]
    vs = GpuVectorStore(persist_dir=None)
    vs.upsert(ids=ids[:250], documents=[t if i % 7 else "" for i, t in enumerate(texts[:250])],
              metadatas=[m if i % 5 else {} for i, m in enumerate(metas[:250])], embeddings=emb[:250])
    vs.delete([ids[3], ids[120]])
    bm = BM25Store(index_dir=None)
    bm.upsert_many(ids=list(ids[40:]) + ["lexical-only"], texts=list(texts[40:]) + [texts[41] + " " + texts[42]],
                   metadatas=list(metas[40:]) + [{"course": "bm-only", "language": "en"}])
    return vs, bm


def test_disjoint_stores_short_pools_and_mutations(corpus, monkeypatch, spy):
    from classmate_hip.retrieval import HybridRetriever
    vs, bm = disjoint_stores(corpus)
    ids, texts, metas = corpus["ids"], corpus["texts"], corpus["metas"]
    qtexts = list(corpus["qtexts"]) + ["   "]
    qvecs = np.concatenate([corpus["qvecs"], corpus["qvecs"][:1]])
    retr = HybridRetriever(vector_store=vs, bm25_store=bm, embedder=_Preset(qtexts, qvecs), k_vector=8, k_bm25=8)
    pool = max(retr.k_vector, retr.mmr_max_pool)
    short = {"course": "math201", "unit": "u2"}
    held = [i for i in range(250) if i % 5 and i not in (3, 120)]                      # rows with their metadata
    n_short = sum(1 for i in held if metas[i].get("course") == "math201" and metas[i].get("unit") == "u2")
    assert 0 < n_short < pool                                                         # a pool shorter than the MMR pool
    assert not any(metas[i].get("course") == "bm-only" for i in range(250))           # no vector, one BM25 document
    menu = [short, {"course": "bm-only"}, None, {"course": "cs101"}, {"doc_type": "pdf"}, {"course": "nope"}, {}]
    fs = [menu[i % len(menu)] for i in range(len(qtexts))]
    fs[-1] = short                                                                    # the blank question, under a clause
    for cutoff in ("1", None):
        force(monkeypatch, cutoff)
        for top_k in (-4, 10):
            got, want = both_paths(retr, monkeypatch, spy, questions=qtexts, filters=fs, top_k=top_k)
            assert got == want, (cutoff, top_k)
    i_short, i_bm = fs.index(short), fs.index({"course": "bm-only"})
    assert 0 < sum(r["scores"]["vector_distance"] is not None for r in got[i_short]) <= n_short
    assert got[i_bm] and all(r["scores"]["vector_distance"] is None for r in got[i_bm])
    assert all(r["scores"]["bm25_score"] is None for r in got[-1])                    # whitespace only: no BM25 list
    # after a BM25 upsert and a vector delete: the key map and the caches follow the version counters
    bm.upsert_many(ids=[ids[0]], texts=["an extra lexical document " + texts[1]], metadatas=[{"course": "cs101"}])
    gone = next(r["id"] for r in got[i_short] if r["scores"]["vector_distance"] is not None)
    vs.delete([gone])
    got2, want2 = both_paths(retr, monkeypatch, spy, questions=qtexts, filters=fs, top_k=10)
    assert got2 == want2 and got2[i_short] != got[i_short]
    assert gone not in [r["id"] for r in got2[i_short] if r["scores"]["vector_distance"] is not None]


def test_eps_floors_are_cached_per_bm25_version(corpus, monkeypatch, spy):
    from classmate_hip.retrieval import HybridRetriever
    vs, bm = make_stores(corpus)
    retr = HybridRetriever(vector_store=vs, bm25_store=bm, embedder=_Preset(corpus["qtexts"], corpus["qvecs"]),
                           k_vector=10, k_bm25=10)
    qs = list(corpus["qtexts"])
    fs = filters_for(len(qs))
    force(monkeypatch, "1")                       # every clause on the list routes: one BM25 list call per batch
    monkeypatch.delenv("CM_RETRIEVE_DEVICE", raising=False)
    first = retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    assert bm._index.last_eps_filters() > 0       # some clause has a negative idf: its floor is computed
    again = retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    assert bm._index.last_eps_filters() == 0 and bm._index.last_eps_passes() == 0 and again == first
    monkeypatch.setenv("CM_RETRIEVE_DEVICE", "0")
    assert first == retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    monkeypatch.delenv("CM_RETRIEVE_DEVICE")
    bm.upsert_many(ids=["one-more"], texts=[corpus["texts"][5]], metadatas=[dict(corpus["metas"][5])])
    cold = retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    assert bm._index.last_eps_filters() > 0       # a new BM25 version: computed again
    warm = retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
    assert bm._index.last_eps_filters() == 0 and warm == cold
    assert len(spy) == 4
    monkeypatch.setenv("CM_RETRIEVE_DEVICE", "0")
    assert warm == retr.retrieve_batch(questions=qs, filters=fs, top_k=10)
