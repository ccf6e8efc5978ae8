"""The device chain for per-question where clauses, the parts that need no GPU: the two _dev symbols
in the header and the binding table, their argument checks that run before any device call, the
stores' planning helpers (the plan the host routes execute, under the default constants and both env
overrides, against stand-ins for the device indexes) and device_batch.applicable_clauses."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from test_bm25_lists_host import _ListIndex

REPO = Path(__file__).resolve().parents[1]


# ---- symbols ----
def test_symbols_in_header_and_binding_table():
    from classmate_hip import _lib
    header = (REPO / "include" / "classmate_hip.h").read_text()
    assert "cm_dense_search_lists_dev(cm_dense *h" in header and "cm_bm25_search_lists_dev(cm_bm25 *h" in header
    for name in ("cm_dense_search_lists_dev", "cm_bm25_search_lists_dev"):
        assert name in _lib.SIGNATURES and callable(_lib.fn[name])
    assert len(_lib.SIGNATURES["cm_dense_search_lists_dev"]) == 11      # the return type and ten arguments
    assert len(_lib.SIGNATURES["cm_bm25_search_lists_dev"]) == 14       # the return type and thirteen arguments
    # the host functions are what they were
    assert len(_lib.SIGNATURES["cm_dense_search_lists"]) == 11 and len(_lib.SIGNATURES["cm_bm25_search_lists"]) == 12
    assert "float *out_vec);" in header.split("int cm_dense_search_lists(cm_dense *h")[1].split(";")[0] + ";"


# ---- argument checks (host memory stands in for device memory: nothing is dereferenced) ----
def _dense(h, nq=1, k=1, n_filters=1, filter_of=(0,), null=None):
    from classmate_hip import _lib
    n = max(nq, 1)
    a = dict(q=np.zeros((n, 4), np.float32), allow=np.zeros(max(n_filters, 1), np.uint32),
             filter_of=np.asarray(filter_of, np.int32), dist=np.zeros((n, max(k, 1)), np.float32),
             row=np.zeros((n, max(k, 1)), np.int64))
    p = {name: None if name == null else _lib.ptr(v) for name, v in a.items()}
    return _lib.fn["cm_dense_search_lists_dev"](h, p["q"], nq, k, p["allow"], n_filters, p["filter_of"], p["dist"],
                                                p["row"], None)


def _bm25(h, nq=1, k=1, n_filters=1, filter_of=(0,), q_off=None, null=None, eps=False):
    from classmate_hip import _lib
    n = max(nq, 1)
    a = dict(q_terms=np.zeros(4, np.int32), q_off=np.asarray(q_off if q_off is not None else [0] * (n + 1), np.int32),
             allow=np.zeros(max(n_filters, 1), np.uint32), filter_of=np.asarray(filter_of, np.int32),
             eps=np.full(max(n_filters, 1), np.nan), score=np.zeros((n, max(k, 1))),
             row=np.zeros((n, max(k, 1)), np.int64), n=np.zeros(n, np.int32))
    p = {name: None if name == null else _lib.ptr(v) for name, v in a.items()}
    return _lib.fn["cm_bm25_search_lists_dev"](h, p["q_terms"], p["q_off"], nq, k, p["allow"], n_filters, p["filter_of"],
                                               p["eps"] if eps else None, p["score"], p["row"], p["n"], None)


def _fake():
    # the checks read only the arguments: a handle that is never dereferenced
    return ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))


def test_dense_dev_argument_checks_run_before_any_device_call():
    from classmate_hip import _lib
    assert _dense(None) == _lib.CM_EINVAL and "handle" in _lib.last_error()
    fake = _fake()
    cases = [(dict(nq=0), "nq"), (dict(k=0), "k must"), (dict(n_filters=0), "n_filters"),
             (dict(filter_of=(1,)), "filter_of"), (dict(filter_of=(-1,)), "filter_of"),
             (dict(nq=2, filter_of=(0, 3), n_filters=3), "filter_of[1]")]
    cases += [(dict(null=name), "NULL") for name in ("q", "allow", "filter_of", "dist", "row")]
    for kw, word in cases:
        assert _dense(fake, **kw) == _lib.CM_EINVAL, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert "cm_dense_search_lists_dev" in _lib.last_error() or "NULL" in _lib.last_error()
    assert _dense(fake, nq=0) == _lib.CM_EINVAL and "cm_dense_search_lists_dev: nq" in _lib.last_error()
    assert _dense(fake, k=_lib.max_topk() + 1) == _lib.CM_EUNSUPPORTED
    assert "cm_max_topk" in _lib.last_error()


def test_bm25_dev_argument_checks_run_before_any_device_call():
    from classmate_hip import _lib
    assert _bm25(None) == _lib.CM_EINVAL and "handle" in _lib.last_error()
    fake = _fake()
    cases = [(dict(nq=0), "nq"), (dict(k=0), "k must"), (dict(n_filters=0), "n_filters"),
             (dict(filter_of=(1,)), "filter_of"), (dict(filter_of=(-1,)), "filter_of"),
             (dict(nq=2, filter_of=(0, 3), n_filters=3), "filter_of[1]"),
             (dict(nq=2, filter_of=(0, 0), q_off=[0, 2, 1]), "non-decreasing"), (dict(q_off=[-1, 0]), "q_off")]
    cases += [(dict(null=name), "NULL") for name in ("q_terms", "q_off", "allow", "filter_of", "score", "row", "n")]
    for eps in (False, True):               # a null eps_io is accepted: the check after the NULL test still answers
        for kw, word in cases:
            assert _bm25(fake, eps=eps, **kw) == _lib.CM_EINVAL, kw
            assert word in _lib.last_error(), (kw, eps, _lib.last_error())
    assert _bm25(fake, nq=0) == _lib.CM_EINVAL and "cm_bm25_search_lists_dev: nq" in _lib.last_error()


def test_host_functions_keep_their_messages():
    from classmate_hip import _lib
    from test_bm25_lists_host import _call as bm25_call
    from test_multi_filter_host import _call as dense_call
    fake = _fake()
    assert dense_call(fake, nq=0) == _lib.CM_EINVAL and _lib.last_error() == "cm_dense_search_lists: nq must be >= 1"
    assert bm25_call(fake, k=0) == _lib.CM_EINVAL and _lib.last_error() == "cm_bm25_search_lists: k must be >= 1"


# ---- planning: the plan the host route executes ----
class _DenseStandIn:
    """A stand-in for engine.DenseIndex that records what it is asked."""
    device = 0

    def __init__(self, dim):
        self.dim, self.size, self.scans, self.lists = dim, 0, [], []

    def upsert(self, vecs, rows):
        self.size = max(self.size, int(np.max(rows)) + 1)

    def live_count(self):
        return self.size

    def _out(self, nq, k, vec):
        out = (np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64))
        return out + (np.zeros((nq, k, self.dim), np.float32),) if vec else out

    def search(self, q, k, allow_bits=None, return_vectors=False):
        self.scans.append((len(q), k, None if allow_bits is None else int(np.asarray(allow_bits).sum())))
        return self._out(len(q), k, return_vectors)

    def search_lists(self, q, k, allow_words, filter_of, return_vectors=False):
        self.lists.append((len(q), k, [int(np.asarray(w).sum()) for w in allow_words], np.asarray(filter_of).tolist()))
        return self._out(len(q), k, return_vectors)


def _where_bits(meta, where, semantics, device=None):
    """The filter as a host mask (the device evaluation needs a GPU): (mask, candidates)."""
    m = meta.chroma_mask(where) if semantics == "chroma" else meta.bm25_mask(where)
    return m, int(m.sum())


N_DOCS = 2048        # a course holds 4 documents, a half 1024
METAS = [{"language": "en", "course": "c%d" % (i % 512), "half": "h%d" % (i % 2)} for i in range(N_DOCS)]
WHERES = [{"course": "c1"}, {"half": "h0"}, {"course": "c1"}, None, {"course": "c2"}, {"course": "nope"}, {}]


@pytest.fixture
def vstore(monkeypatch):
    from classmate_hip.retrieval import vector_store as vsm
    monkeypatch.setattr(vsm.multidev, "new_dense_index", lambda dim, device=None, capacity=0: _DenseStandIn(dim))
    monkeypatch.setattr(vsm.engine, "where_bits", _where_bits)
    st = vsm.GpuVectorStore(persist_dir=None)
    st.upsert(ids=[f"d{i}" for i in range(N_DOCS)], documents=["x"] * N_DOCS, metadatas=METAS,
              embeddings=np.zeros((N_DOCS, 8), np.float32))
    return st


def _summary(plan, count=lambda w: int(np.asarray(w).sum())):
    return {"plain": list(plan["plain"]),
            "scan": [(list(e[0]), e[1] if len(e) == 3 else e[3], count(e[2] if len(e) == 3 else e[2][0]))
                     for e in plan["scan"]],
            "lists": [(list(e[0]), e[1], [count(w) for w in e[2]], np.asarray(e[3]).tolist()) for e in plan["lists"]]}


@pytest.mark.parametrize("env,want", [
    ("1", {"plain": [3, 6], "scan": [], "lists": [([0, 2, 1, 4], 24, [4, 1024, 4], [0, 0, 1, 2])]}),
    ("1e9", {"plain": [3, 6], "scan": [([0, 2], 4, 4), ([1], 24, 1024), ([4], 4, 4)], "lists": []}),
    (None, {"plain": [3, 6], "scan": [([1], 24, 1024)], "lists": [([0, 2, 4], 4, [4, 4], [0, 0, 1])]}),
])
def test_vector_store_plan_is_what_the_host_route_executes(vstore, monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("CM_LIST_CUTOFF_DIV", raising=False)
    else:
        monkeypatch.setenv("CM_LIST_CUTOFF_DIV", env)
    wheres = WHERES                               # (Chroma's form of these clauses is the same mapping)
    assert _summary(vstore._plan_clauses(wheres, 24)) == want
    idx = vstore._index
    got = vstore.query_batch(query_embeddings=np.zeros((len(wheres), 8), np.float32), where=wheres, top_k=24,
                             include_embeddings=True)
    assert got == [[] for _ in wheres]
    assert idx.lists == [(len(sel), k, counts, fo) for sel, k, counts, fo in want["lists"]]
    assert idx.scans == [(len(want["plain"]), 24, None)] + [(len(sel), k, n) for sel, k, n in want["scan"]]


@pytest.fixture
def bstore(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _ListIndex())
    monkeypatch.setattr(bm25.engine, "where_bits", _where_bits)
    bm25.release_all()
    st = bm25.BM25Store(index_dir=None)
    st.upsert_many(ids=[f"d{i}" for i in range(N_DOCS)], texts=[f"alpha beta w{i % 7}" for i in range(N_DOCS)],
                   metadatas=METAS)
    yield st
    bm25.release_all()


QUERIES = ["alpha", "beta w1", "", "alpha w3", "beta", "alpha", "beta"]


@pytest.mark.parametrize("env,want", [
    # (the blank question 2 shares c1's clause: planned with it, not sent to the list call; "half" is no filter
    # field of BM25Store's _matches_filter, quirk Q4: that clause allows every document)
    ("1", {"plain": [3, 6], "scan": [], "lists": [([0, 1, 4], 5, [4, 2048, 4], [0, 1, 2])]}),
    ("1e9", {"plain": [3, 6], "scan": [([0, 2], 4, 4), ([1], 5, 2048), ([4], 4, 4)], "lists": []}),
    (None, {"plain": [3, 6], "scan": [([1], 5, 2048)], "lists": [([0, 4], 4, [4, 4], [0, 1])]}),
])
def test_bm25_store_plan_is_what_the_host_route_executes(bstore, monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("CM_BM25_LIST_CUTOFF_DIV", raising=False)
    else:
        monkeypatch.setenv("CM_BM25_LIST_CUTOFF_DIV", env)
    plan = bstore._plan_clauses(QUERIES, WHERES, 5)
    assert _summary(plan) == want
    for sel, _, words, filter_of, clauses in plan["lists"]:       # the clause of every bitmap, for the eps cache's key
        assert len(clauses) == len(words)
        assert [clauses[f] for f in filter_of] == [WHERES[i] for i in sel]
    idx = bstore._index
    del idx.lists[:], idx.searches[:]
    got = bstore.search_batch(queries=QUERIES, where=WHERES, top_k=5)
    assert len(got) == len(QUERIES) and got[2] == [] and got[5] == []
    assert idx.lists == [(len(sel), len(counts), fo) for sel, _, counts, fo in want["lists"]]
    blank = {i for i, q in enumerate(QUERIES) if not q.strip()}
    assert sorted(idx.searches) == sorted([len(want["plain"])] + [len(set(sel) - blank) for sel, _, _ in want["scan"]])
    # a negative top_k has no list route: every clause is planned as a scan the store evaluates itself
    monkeypatch.setenv("CM_BM25_LIST_CUTOFF_DIV", "1")
    plan = bstore._plan_clauses(QUERIES, WHERES, -1)
    assert plan["lists"] == [] and all(bits is None and k is None for _, _, bits, k in plan["scan"])


# ---- applicability ----
def _retriever(vs, bm, **kw):
    from classmate_hip.retrieval import HybridRetriever
    return HybridRetriever(vector_store=vs, bm25_store=bm, embedder=None, k_vector=8, k_bm25=8, **kw)


def test_applicable_clauses(vstore, bstore):
    from classmate_hip.retrieval import device_batch
    fs = [{"course": "c1"}, None]
    retr = _retriever(vstore, bstore)
    assert device_batch.applicable_clauses(retr, fs, True) is True
    assert device_batch.applicable_clauses(retr, tuple(fs), True) is True
    for single in (None, {}, {"course": "c1"}):
        assert device_batch.applicable_clauses(retr, single, True) is False          # not a sequence
    assert device_batch.applicable_clauses(retr, fs, False) is False                 # hybrid=False
    assert device_batch.applicable_clauses(_retriever(vstore, bstore, use_mmr=False), fs, True) is False
    # ``applicable`` keeps declining a sequence, and keeps accepting one filter
    assert device_batch.applicable(retr, fs, True) is False and device_batch.applicable(retr, tuple(fs), True) is False
    assert device_batch.applicable(retr, {"course": "c1"}, True) is True
    # an index without search_lists (the sharded ones): the host path
    for store in (vstore, bstore):
        real = store._index

        class _NoLists:
            def __getattr__(self, name):
                if name == "search_lists":
                    raise AttributeError(name)
                return getattr(real, name)
        store._index = _NoLists()
        try:
            assert device_batch.applicable_clauses(retr, fs, True) is False
            assert device_batch.applicable(retr, {"course": "c1"}, True) is True
        finally:
            store._index = real
    assert device_batch.applicable_clauses(retr, fs, True) is True


def test_fusion_tries_the_device_chain_first(vstore, bstore, monkeypatch):
    """The sequence branch: the length error first, then applicable_clauses / retrieve_batch_clauses,
    and CM_RETRIEVE_DEVICE=0 forces the host path."""
    from classmate_hip.retrieval import device_batch
    retr = _retriever(vstore, bstore)
    calls = []
    monkeypatch.setattr(device_batch, "retrieve_batch_clauses", lambda *a: calls.append(a[1:]) or "answered")
    monkeypatch.delenv("CM_RETRIEVE_DEVICE", raising=False)
    fs = [{"course": "c1"}, None]
    with pytest.raises(ValueError):
        retr.retrieve_batch(questions=["a", "b"], filters=fs[:1], top_k=5)
    assert not calls
    assert retr.retrieve_batch(questions=["a", "b"], filters=fs, top_k=5) == "answered"
    assert calls == [(["a", "b"], 5, fs)]
    monkeypatch.setenv("CM_RETRIEVE_DEVICE", "0")
    class _Host(Exception):
        pass

    def encode(qs):
        raise _Host()                            # the host path's first step
    retr.embedder = type("E", (), {"encode_queries": staticmethod(encode)})()
    with pytest.raises(_Host):
        retr.retrieve_batch(questions=["a", "b"], filters=fs, top_k=5)
    assert len(calls) == 1
