"""BM25 per-question where clauses, the parts that need no GPU: the routing of a batch's clauses
under BM25's own constants (vector_store.route_clauses), the env override, the sequence-length
error, cm_bm25_search_lists' argument checks that run before any device call, and the symbol in the
header and the binding table."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


def _route(group_of, counts, size=1000, top_k=10, has_lists=True, **kw):
    from classmate_hip.retrieval import bm25
    from classmate_hip.retrieval.vector_store import route_clauses
    args = dict(cutoff_div=bm25.BM25_LIST_CUTOFF_DIV, pair_budget=bm25.BM25_LIST_PAIR_BUDGET,
                pair_div=bm25.BM25_LIST_PAIR_DIV)
    args.update(kw)
    return route_clauses(group_of, counts, size, top_k, 1 << 62, has_lists, **args)


def test_constants_are_bm25s_own():
    from classmate_hip.retrieval import bm25
    assert bm25.BM25_LIST_CUTOFF_DIV > 0 and bm25.BM25_LIST_PAIR_DIV > 0
    # 24 bytes of sort keys and rows per pair: the budget stays within 1 GiB
    assert 0 < bm25.BM25_LIST_PAIR_BUDGET * 24 <= 1 << 30


def test_routing_with_bm25_constants():
    from classmate_hip.retrieval import bm25
    size = 1 << 16
    edge = int(size // bm25.BM25_LIST_CUTOFF_DIV)       # the largest selective clause, one question
    plan = _route([-1, 0, 1, 2, -1], [0, edge, edge + 1], size)
    assert plan == {"plain": [0, 4], "empty": [1], "scan": [(2, [3])], "lists": [[(1, [2])]]}
    # the pair rule: questions x allowed rows up to size / BM25_LIST_PAIR_DIV
    rows = max(1, edge // 4)
    most = int(size // (bm25.BM25_LIST_PAIR_DIV * rows))
    assert most >= 2
    assert _route([0] * most, [rows], size)["lists"] == [[(0, list(range(most)))]]
    assert _route([0] * (most + 1), [rows], size)["scan"] == [(0, list(range(most + 1)))]
    # any top_k stays on the list route (the row-list search returns a full order) ...
    assert _route([0], [rows], size, top_k=100000)["lists"] == [[(0, [0])]]
    # ... an index without search_lists (the sharded one) never takes it
    assert _route([0, 1], [rows, 0], size, has_lists=False) == {"plain": [], "empty": [1], "scan": [(0, [0])],
                                                                "lists": []}
    # forced: 1 sends every clause with a candidate to the lists, a huge value none
    assert _route([0, 0, 1], [size, size], size, cutoff_div=1.0, pair_div=0.0)["scan"] == []
    assert _route([0, 0, 1], [1, 1], size, cutoff_div=1e9, pair_div=0.0)["lists"] == []


def test_routing_splits_at_bm25s_pair_budget():
    plan = _route([0, 0, 0, 1], [5, 4], 10 ** 6, pair_budget=10)
    assert plan["lists"] == [[(0, [0, 1])], [(0, [2]), (1, [3])]]


class _ListIndex:
    """A stand-in for the device index that records which route it is asked through."""
    device = 0

    def __init__(self):
        self.n, self.lists, self.searches = 0, [], []

    def build(self, flat, off, vocab, live=None):
        self.n = len(off) - 1

    @property
    def num_docs(self):
        return self.n

    def _out(self, nq, k):
        return np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)

    def search(self, qids, k, allow=None):
        self.searches.append(len(qids))
        return self._out(len(qids), k)

    def search_lists(self, qids, k, allow_words, filter_of):
        self.lists.append((len(qids), len(allow_words), np.asarray(filter_of).tolist()))
        return self._out(len(qids), k)


@pytest.fixture
def store(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _ListIndex())
    monkeypatch.setattr(bm25.engine, "where_bits",
                        lambda meta, where, semantics, device=None: (lambda m: (m, int(m.sum())))(meta.bm25_mask(where)))
    bm25.release_all()
    st = bm25.BM25Store(index_dir=None)
    n = 2048        # a course holds 4 documents: selective at any cutoff up to n / 4
    st.upsert_many(ids=[f"d{i}" for i in range(n)], texts=[f"alpha beta w{i % 7}" for i in range(n)],
                   metadatas=[{"language": "en", "course": "c%d" % (i % 512), "half": "h%d" % (i % 2)} for i in range(n)])
    yield st
    bm25.release_all()


def test_search_batch_routes_by_the_env_override(store, monkeypatch):
    queries = ["alpha", "beta w1", "", "alpha w3", "beta", "alpha"]
    wheres = [{"course": "c1"}, {"half": "h0"}, {"course": "c1"}, None, {"course": "c2"}, {"course": "nope"}]
    idx = None
    for env, n_lists in (("1", 1), ("1e9", 0), (None, 1)):
        if env is None:
            monkeypatch.delenv("CM_BM25_LIST_CUTOFF_DIV", raising=False)
        else:
            monkeypatch.setenv("CM_BM25_LIST_CUTOFF_DIV", env)
        got = store.search_batch(queries=queries, where=wheres, top_k=5)
        idx = store._index
        assert got[2] == [] and got[5] == [] and len(got) == len(queries)
        assert len(idx.lists) == n_lists, env
        if env == "1":          # c1 (one non-blank question), h0, c2 in one call; the blank question is not sent
            assert idx.lists == [(3, 3, [0, 1, 2])] and idx.searches == [1]
        if env == "1e9":
            assert sorted(idx.searches) == [1, 1, 1, 1]
        if env is None:         # half of the rows is not selective: the ordinary search
            assert idx.lists == [(2, 2, [0, 1])] and sorted(idx.searches) == [1, 1]
        del idx.lists[:], idx.searches[:]
    # a negative top_k (python's slice semantics) keeps the per-clause route
    monkeypatch.setenv("CM_BM25_LIST_CUTOFF_DIV", "1")
    store.search_batch(queries=queries, where=wheres, top_k=-1)
    assert idx.lists == []


def test_where_length_error(store):
    for bad in ([], [None], [None] * 3):
        with pytest.raises(ValueError):
            store.search_batch(queries=["a", "b"], where=bad, top_k=5)


def test_symbol_in_header_and_binding_table():
    from classmate_hip import _lib
    header = (REPO / "include" / "classmate_hip.h").read_text()
    for name in ("cm_bm25_search_lists", "cm_bm25_last_eps_filters"):
        assert f"{name}(cm_bm25 *h" in header
        assert name in _lib.SIGNATURES and callable(_lib.fn[name])
    assert len(_lib.SIGNATURES["cm_bm25_search_lists"]) == 12      # the return type and eleven arguments


def _call(h, nq=1, k=1, n_filters=1, filter_of=(0,), q_off=None, null=None):
    from classmate_hip import _lib
    n = max(nq, 1)
    a = dict(q_terms=np.zeros(4, np.int32), q_off=np.asarray(q_off if q_off is not None else [0] * (n + 1), np.int32),
             allow=np.zeros(max(n_filters, 1), np.uint32), filter_of=np.asarray(filter_of, np.int32),
             score=np.zeros((n, max(k, 1))), row=np.zeros((n, max(k, 1)), np.int64), n=np.zeros(n, np.int32))
    p = {name: None if name == null else _lib.ptr(v) for name, v in a.items()}
    return _lib.fn["cm_bm25_search_lists"](h, p["q_terms"], p["q_off"], nq, k, p["allow"], n_filters, p["filter_of"],
                                           p["score"], p["row"], p["n"])


def test_argument_checks_run_before_any_device_call():
    from classmate_hip import _lib
    assert _call(None) == _lib.CM_EINVAL and "handle" in _lib.last_error()
    assert _lib.fn["cm_bm25_last_eps_filters"](None) == -1
    # the remaining checks read only the arguments: a handle that is never dereferenced
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    cases = [(dict(nq=0), "nq"), (dict(k=0), "k must"), (dict(n_filters=0), "n_filters"),
             (dict(filter_of=(1,)), "filter_of"), (dict(filter_of=(-1,)), "filter_of"),
             (dict(nq=2, filter_of=(0, 3), n_filters=3), "filter_of[1]"),
             (dict(nq=2, filter_of=(0, 0), q_off=[0, 2, 1]), "non-decreasing"), (dict(q_off=[-1, 0]), "q_off")]
    cases += [(dict(null=name), "NULL") for name in ("q_terms", "q_off", "allow", "filter_of", "score", "row", "n")]
    for kw, word in cases:
        assert _call(fake, **kw) == _lib.CM_EINVAL, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
