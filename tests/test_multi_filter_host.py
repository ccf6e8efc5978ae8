"""Per-question where clauses, the parts that need no GPU: cm_dense_search_lists' argument checks
that run before any device call, the routing of a batch's clauses (vector_store.route_clauses), the
grouping of equal clauses, the sequence-length errors, and BM25Store.search_batch's one filtered
search per distinct clause (against a stand-in for the device index that records what it is given)."""
import ctypes

import numpy as np
import pytest


# ---- the C ABI's argument checks ----
def _call(h, nq=1, k=1, n_filters=1, filter_of=(0,), q=True, allow=True):
    from classmate_hip import _lib
    qv = np.zeros((max(nq, 1), 4), np.float32)
    words = np.zeros(max(n_filters, 1), np.uint32)
    fo = np.asarray(filter_of, np.int32)
    dist = np.zeros((max(nq, 1), max(k, 1)), np.float32)
    rows = np.zeros((max(nq, 1), max(k, 1)), np.int64)
    return _lib.fn["cm_dense_search_lists"](h, _lib.ptr(qv) if q else None, nq, k, _lib.ptr(words) if allow else None,
                                            n_filters, _lib.ptr(fo), _lib.ptr(dist), _lib.ptr(rows), None)


def test_search_lists_argument_checks_run_before_any_device_call():
    from classmate_hip import _lib
    with pytest.raises(ValueError):
        _lib.check(_call(None), "cm_dense_search_lists")
    assert "handle" in _lib.last_error()
    # the remaining checks read only the arguments: a handle that is never dereferenced
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    for kw, word in ((dict(nq=0), "nq"), (dict(k=0), "k must"), (dict(n_filters=0), "n_filters"),
                     (dict(filter_of=(1,)), "filter_of"), (dict(filter_of=(-1,)), "filter_of"),
                     (dict(nq=2, filter_of=(0, 3), n_filters=3), "filter_of[1]"), (dict(q=False), "NULL"),
                     (dict(allow=False), "NULL")):
        rc = _call(fake, **kw)
        assert rc == _lib.CM_EINVAL, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert _call(fake, k=_lib.max_topk() + 1) == _lib.CM_EUNSUPPORTED
    assert "cm_max_topk" in _lib.last_error()


# ---- routing ----
def _route(group_of, counts, **kw):
    from classmate_hip.retrieval.vector_store import route_clauses
    args = dict(size=1000, top_k=10, max_topk=256, has_lists=True, cutoff_div=8, pair_budget=1 << 20, pair_div=0)
    args.update(kw)
    return route_clauses(group_of, counts, **args)


def test_routing_of_a_mixed_batch():
    #           none  empty  selective  unselective  selective again, same clause
    plan = _route([-1, 0, 1, 2, 1, -1, 2], [0, 100, 126])
    assert plan == {"plain": [0, 5], "empty": [1], "scan": [(2, [3, 6])], "lists": [[(1, [2, 4])]]}
    # exactly size / cutoff_div rows is still selective; one more is not
    assert _route([0], [125])["lists"] == [[(0, [0])]] and _route([0], [125])["scan"] == []
    assert _route([0], [126])["scan"] == [(0, [0])]


def test_routing_counts_the_questions_that_share_a_clause():
    # 100 allowed rows of 1000: selective for 5 questions (500 pairs = size / 2), not for 6
    five, six = [0] * 5, [0] * 6
    assert _route(five, [100], pair_div=2)["lists"] == [[(0, [0, 1, 2, 3, 4])]]
    assert _route(six, [100], pair_div=2) == {"plain": [], "empty": [], "scan": [(0, [0, 1, 2, 3, 4, 5])], "lists": []}
    # each clause on its own: many selective clauses with one question each all stay on the list route
    plan = _route(list(range(50)), [100] * 50, pair_div=2)
    assert plan["scan"] == [] and len(plan["lists"]) == 1 and len(plan["lists"][0]) == 50


def test_routing_without_the_list_route():
    for kw in (dict(top_k=257), dict(has_lists=False)):
        plan = _route([0, 1, 0, -1, 2], [5, 7, 0], **kw)
        assert plan == {"plain": [3], "empty": [4], "scan": [(0, [0, 2]), (1, [1])], "lists": []}
    assert _route([0, 1], [5, 7], top_k=256)["lists"] == [[(0, [0]), (1, [1])]]


def test_routing_splits_at_the_pair_budget():
    # 4 + 4 + 4 pairs fit a budget of 12; the next query starts a new call, inside a clause if need be
    plan = _route([0, 0, 0, 0, 1, 1], [4, 3], pair_budget=12)
    assert plan["lists"] == [[(0, [0, 1, 2])], [(0, [3]), (1, [4, 5])]]
    # a single query above the budget still gets a call of its own
    plan = _route([0, 1, 1], [100, 60], pair_budget=50)
    assert plan["lists"] == [[(0, [0])], [(1, [1])], [(1, [2])]]
    assert sum(len(qs) for call in plan["lists"] for _, qs in call) == 3


def test_cutoff_constants_and_override(monkeypatch):
    from classmate_hip.retrieval import vector_store as vs
    assert vs.LIST_PAIR_BUDGET == 64 << 20 and vs.LIST_CUTOFF_DIV > 0 and vs.LIST_PAIR_DIV > 0
    monkeypatch.delenv("CM_LIST_CUTOFF_DIV", raising=False)
    assert vs._list_cutoff_div() == vs.LIST_CUTOFF_DIV
    monkeypatch.setenv("CM_LIST_CUTOFF_DIV", "1")
    assert vs._list_cutoff_div() == 1.0
    monkeypatch.setenv("CM_LIST_CUTOFF_DIV", "1e9")
    assert vs._list_cutoff_div() == 1e9


# ---- grouping ----
def test_equal_clauses_share_a_group_typed():
    from classmate_hip.retrieval.vector_store import group_clauses
    a = {"course": "cs101", "unit": "u1"}
    b = {"unit": "u1", "course": "cs101"}                 # another key order: the same clause
    group_of, clauses = group_clauses([a, None, b, {}, {"flag": True}, {"flag": 1}, {"flag": "1"}, {"flag": 1.0},
                                       {"$and": [{"course": "cs101"}, {"unit": "u1"}]}, {"flag": True}])
    assert group_of == [0, -1, 0, -1, 1, 2, 3, 4, 5, 1]
    assert clauses == [a, {"flag": True}, {"flag": 1}, {"flag": "1"}, {"flag": 1.0},
                       {"$and": [{"course": "cs101"}, {"unit": "u1"}]}]
    # a value without a canonical form: a group of its own, every time
    odd = {"tag": {1, 2}}
    group_of, clauses = group_clauses([odd, a, odd])
    assert group_of == [0, 1, 2] and clauses[0] is odd and clauses[2] is odd


# ---- sequence-length errors ----
def test_query_batch_sequence_length_errors():
    from classmate_hip.retrieval import vector_store as vs_mod
    vs = vs_mod.GpuVectorStore(persist_dir=None)
    q = np.zeros((3, 8), np.float32)
    for bad in ([], [None], [None] * 4, ({"a": 1},) * 2):
        with pytest.raises(ValueError):
            vs.query_batch(query_embeddings=q, where=bad, top_k=5)
    with pytest.raises(ValueError):
        vs.query_batch(query_embeddings=q, where=[None] * 3, top_k=0)
    assert vs.query_batch(query_embeddings=q, where=[None, {"a": 1}, {}], top_k=5) == [[], [], []]   # an empty store


def test_device_batch_declines_a_sequence():
    from classmate_hip.retrieval import device_batch

    class _R:
        use_mmr = True
        vector_store = bm25_store = None
    assert device_batch.applicable(_R(), [{"course": "cs101"}, None], True) is False
    assert device_batch.applicable(_R(), ({"course": "cs101"},), True) is False


# ---- BM25Store.search_batch: one filtered search per distinct clause ----
class _RecordingIndex:
    device = 0

    def __init__(self):
        self.docs, self.searches = [], []

    def build(self, flat, off, vocab, live=None):
        self.docs = [np.asarray(flat[off[i]:off[i + 1]]).tolist() for i in range(len(off) - 1)]

    @property
    def num_docs(self):
        return len(self.docs)

    def search(self, qids, k, allow=None):
        """Every allowed document that shares a token with the query, score = shared tokens, ties by row."""
        self.searches.append((len(qids), None if allow is None else tuple(np.nonzero(allow)[0].tolist())))
        ok = np.ones(len(self.docs), bool) if allow is None else np.asarray(allow, bool)
        scores = np.zeros((len(qids), k))
        rows = np.full((len(qids), k), -1, np.int64)
        nvalid = np.zeros(len(qids), np.int32)
        for j, q in enumerate(qids):
            hit = sorted(((-len(set(q) & set(d)), r) for r, d in enumerate(self.docs) if ok[r] and set(q) & set(d)))[:k]
            nvalid[j] = len(hit)
            for i, (s, r) in enumerate(hit):
                scores[j, i], rows[j, i] = -s, r
        return scores, rows, nvalid


@pytest.fixture
def bm25_mod(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _RecordingIndex())
    # the filter as a host mask (the device evaluation needs a GPU): (mask, candidates)
    monkeypatch.setattr(bm25.engine, "where_bits",
                        lambda meta, where, semantics, device=None: (lambda m: (m, int(m.sum())))(meta.bm25_mask(where)))
    bm25.release_all()
    yield bm25
    bm25.release_all()


def test_bm25_search_batch_groups_by_clause(bm25_mod):
    n = 40
    ids = [f"d{i}" for i in range(n)]
    words = ["".join(chr(97 + (k * m) % 26) for m in (3, 5, 7, 11, 2)) for k in range(1, 24)]
    texts = [" ".join(words[(i * 7 + j * j) % 23] for j in range(3 + i % 5)) for i in range(n)]
    metas = [{"language": "en", "course": "c%d" % (i % 2), "unit": "u%d" % (i % 3)} for i in range(n)]
    st = bm25_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    queries = [texts[3], texts[8], "", texts[11], texts[20], texts[5], texts[30]]
    wheres = [{"course": "c0"}, None, {"course": "c0"}, {"unit": "u1", "course": "c1"}, {"course": "c0"},
              {"course": "c1", "unit": "u1"}, {"course": "nope"}]
    want = [st.search(query=q, where=w, top_k=5) for q, w in zip(queries, wheres)]
    idx = st._index
    del idx.searches[:]
    got = st.search_batch(queries=queries, where=wheres, top_k=5)
    assert got == want and any(got) and got[2] == [] and got[6] == []
    # one search per distinct clause with a candidate (none for the clause that matches nothing):
    # no clause, course c0 (two non-blank queries), course c1 + unit u1 in either key order
    assert sorted(s[0] for s in idx.searches) == [1, 2, 2] and len(idx.searches) == 3
    allowed = {s[1] for s in idx.searches}
    assert None in allowed and tuple(range(0, n, 2)) in allowed
    assert tuple(i for i in range(n) if i % 2 == 1 and i % 3 == 1) in allowed
    for r in got[0] + got[4]:
        assert r["metadata"]["course"] == "c0"
    for bad in ([], wheres[:-1], wheres + [None]):
        with pytest.raises(ValueError):
            st.search_batch(queries=queries, where=bad, top_k=5)
    # a mapping keeps today's meaning: one search for the whole batch
    del idx.searches[:]
    assert st.search_batch(queries=queries, where={"course": "c0"}, top_k=5)[0] == want[0]
    assert len(idx.searches) == 1
