"""BM25 remove, the parts that need no GPU: the C ABI's argument check that runs before any device
call, and BM25Store's choice between a removal on the device index and a rebuild (against a
stand-in for the device index that records what it is given)."""
import numpy as np
import pytest


def test_remove_null_handle_is_value_error():
    from classmate_hip import _lib
    rows = np.zeros(1, np.int64)
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_remove"](None, _lib.ptr(rows), 1), "cm_bm25_remove")
    assert "handle" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_remove_dev"](None, None, None), "cm_bm25_remove_dev")
    assert "handle" in _lib.last_error()


# ---- BM25Store's choice between remove and rebuild, against a recording stand-in for the index ----
class _FakeIndex:
    """tests/test_bm25_append_host.py's stand-in: build and append only."""
    device = 0

    def __init__(self):
        self.docs, self.calls = [], []

    @staticmethod
    def _split(flat, off):
        return [np.asarray(flat[off[i]:off[i + 1]]).tolist() for i in range(len(off) - 1)]

    def build(self, flat, off, vocab, live=None):
        self.docs = self._split(flat, off)
        self.calls.append(("build", len(self.docs), vocab))

    def append(self, flat, off, vocab):
        new = self._split(flat, off)
        self.docs += new
        self.calls.append(("append", len(new), vocab))

    @property
    def num_docs(self):
        return len(self.docs)


class _FakeRemovingIndex(_FakeIndex):
    """... that can also drop rows, as engine.BM25Index can."""

    def remove(self, rows):
        rows = [int(r) for r in rows]
        assert all(0 <= r < len(self.docs) for r in rows) and len(set(rows)) == len(rows)
        gone = set(rows)
        self.docs = [d for r, d in enumerate(self.docs) if r not in gone]
        self.calls.append(("remove", len(rows), sorted(rows)))

    def stats(self):
        return dict(n_live=len(self.docs), sum_len=sum(len(d) for d in self.docs))


@pytest.fixture
def store_mod(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _FakeRemovingIndex())
    bm25.release_all()
    yield bm25
    bm25.release_all()


def _corpus(n=40):
    ids = [f"d{i}" for i in range(n)]
    words = ["".join(chr(97 + (k * m) % 26) for m in (3, 5, 7, 11, 2)) for k in range(1, 24)]
    texts = [" ".join(words[(i * 7 + j * j) % 23] for j in range(3 + i % 5)) for i in range(n)]
    return ids, texts, [{"language": "en", "course": "c%d" % (i % 2)} for i in range(n)]


def _indexed(store):
    """The documents the index holds, as tokens (ids are private to a store's vocabulary)."""
    store._ensure_index()
    words = {i: t for t, i in store._vocab.items()}
    return [[words[t] for t in d] for d in store._index.docs]


def _fresh(bm25, ids, texts, metas, keep):
    one = bm25.BM25Store(index_dir=None)
    one.upsert_many(ids=[ids[i] for i in keep], texts=[texts[i] for i in keep], metadatas=[metas[i] for i in keep])
    return _indexed(one)


def _ops(index, start=0):
    return [c[:2] for c in index.calls[start:]]


def test_delete_on_a_current_index_removes(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    idx, v0 = st._index, st._version
    st.delete_many([ids[3], "unknown", ids[39], ids[0]])
    assert st._version == v0 + 1 and st._dirty and st._id_list == [ids[i] for i in range(1, 39) if i != 3]
    keep = [i for i in range(40) if i not in (0, 3, 39)]
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, keep)
    assert st._index is idx and _ops(idx) == [("build", 40), ("remove", 3)]
    assert idx.calls[-1][2] == [0, 3, 39]
    assert not st._dirty and st._pending_drop is None and st._pending_row is None
    st.delete_many(["unknown"])                      # nothing to drop: the index stays current
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, keep) and len(idx.calls) == 2


def test_delete_of_a_pending_appended_id_shrinks_the_append(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    _indexed(st)
    st.upsert_many(ids=ids[30:], texts=texts[30:], metadatas=metas[30:])
    st.delete_many([ids[33], ids[39]])               # the device does not hold them yet
    keep = [i for i in range(40) if i not in (33, 39)]
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, keep)
    assert _ops(st._index) == [("build", 30), ("append", 8)]


def test_two_deletes_around_an_upsert_are_one_remove_then_one_append(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    _indexed(st)
    st.delete_many([ids[5], ids[6], ids[20]])
    st.upsert_many(ids=ids[30:36], texts=texts[30:36], metadatas=metas[30:36])
    st.delete_many([ids[4], ids[7], ids[29], ids[31]])   # store rows 4, 5, 26 of the device's, one of the tail
    st.upsert_many(ids=ids[36:], texts=texts[36:], metadatas=metas[36:])
    st.delete_many([ids[37]])
    keep = [i for i in range(40) if i not in (4, 5, 6, 7, 20, 29, 31, 37)]
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, keep)
    assert _ops(st._index) == [("build", 30), ("remove", 6), ("append", 8)]
    assert st._index.calls[1][2] == [4, 5, 6, 7, 20, 29]
    # the filter columns followed the rows
    st._ensure_meta()
    assert not st._meta_dirty and [m["course"] for m in st._meta.metas] == [metas[i]["course"] for i in keep]


def test_delete_on_an_index_without_remove_rebuilds(store_mod, monkeypatch):
    monkeypatch.setattr(store_mod.multidev, "new_bm25_index", lambda device=None: _FakeIndex())
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    st.delete_many([ids[9]])
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, [i for i in range(40) if i != 9])
    assert _ops(st._index) == [("build", 40), ("build", 39)]


def test_delete_after_a_replace_in_place_rebuilds(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    st.upsert_many(ids=[ids[4]], texts=[texts[9]], metadatas=[metas[4]])
    st.delete_many([ids[0]])
    want = _fresh(store_mod, ids, texts[:4] + [texts[9]] + texts[5:], metas, list(range(1, 40)))
    assert _indexed(st) == want
    assert _ops(st._index) == [("build", 40), ("build", 39)]
    st.delete_many([ids[1]])                         # ... and the rebuilt index takes removals again
    assert _indexed(st) == want[1:] and _ops(st._index, 2) == [("remove", 1)]


def test_delete_that_leaves_only_empty_documents_raises_at_the_call(store_mod):
    st = store_mod.BM25Store(index_dir=None)
    en = {"language": "en"}
    st.upsert_many(ids=["a", "b", "c", "d"], texts=["", "alpha beta", "the", "gamma"], metadatas=[en] * 4)
    assert _indexed(st) == [[], ["alpha", "beta"], [], ["gamma"]]
    st.delete_many(["d"])
    with pytest.raises(ZeroDivisionError):
        st.delete_many(["b"])
    assert st._id_list == ["a", "c"] and list(st._entries) == ["a", "c"]
    # the same through the pending tail: the token total follows appends
    s2 = store_mod.BM25Store(index_dir=None)
    s2.upsert_many(ids=["a", "b"], texts=["", "alpha"], metadatas=[en] * 2)
    _indexed(s2)
    s2.upsert_many(ids=["c"], texts=["beta beta"], metadatas=[en])
    s2.delete_many(["b"])
    assert _indexed(s2) == [[], ["beta", "beta"]]
    with pytest.raises(ZeroDivisionError):
        s2.delete_many(["c"])


def test_delete_through_a_shared_state_clones_and_rebuilds(store_mod, tmp_path):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    st.save()
    del st
    store_mod.release_all()
    a = store_mod.BM25Store(index_dir=tmp_path)
    a.load()
    b = store_mod.BM25Store(index_dir=tmp_path)
    b.load()
    assert a._st is b._st
    _indexed(a)                                      # the shared state holds an index
    a.delete_many([ids[2], ids[17]])
    assert a._st is not b._st
    keep = [i for i in range(30) if i not in (2, 17)]
    assert _indexed(a) == _fresh(store_mod, ids, texts, metas, keep)
    assert _ops(a._index) == [("build", 28)]
    assert _indexed(b) == _fresh(store_mod, ids, texts, metas, list(range(30)))
    assert _ops(b._index) == [("build", 30)] and len(b._id_list) == 30


def test_sidecar_opened_store_deletes_without_parsing_the_rest(store_mod, tmp_path):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    st.save()
    del st
    store_mod.release_all()
    a = store_mod.BM25Store(index_dir=tmp_path)
    a.load()
    _indexed(a)
    a.delete_many([ids[2], ids[17]])
    keep = [i for i in range(30) if i not in (2, 17)]
    assert _indexed(a) == _fresh(store_mod, ids, texts, metas, keep)
    assert _ops(a._index) == [("build", 30), ("remove", 2)]
    cat = a._entries
    assert cat.pending and all(type(v) is int for v in dict.values(cat))   # no surviving record was parsed
    assert not a._meta_dirty and not any(a._meta.metas.done)
    assert a._meta.metas[3] == dict(metas[4])        # row 3 is document 4 now; parsed on demand
