"""BM25 replace, the parts that need no GPU: the C ABI's argument check that runs before any device
call, and BM25Store's choice between a replacement on the device index and a rebuild (against a
stand-in for the device index that records what it is given)."""
import ctypes

import numpy as np
import pytest


def test_replace_null_handle_is_value_error():
    from classmate_hip import _lib
    rows = np.zeros(1, np.int64)
    off = (ctypes.c_int64 * 2)(0, 0)
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_replace"](None, _lib.ptr(rows), 1, None, off, 1), "cm_bm25_replace")
    assert "handle" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_replace_dev"](None, None, 1, None, None, 0, 1, None), "cm_bm25_replace_dev")
    assert "handle" in _lib.last_error()


# ---- BM25Store's choice between replace and rebuild, against a recording stand-in for the index ----
class _FakeIndex:
    """tests/test_bm25_remove_host.py's stand-in: build, append and remove."""
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

    def remove(self, rows):
        rows = [int(r) for r in rows]
        assert all(0 <= r < len(self.docs) for r in rows) and len(set(rows)) == len(rows)
        gone = set(rows)
        self.docs = [d for r, d in enumerate(self.docs) if r not in gone]
        self.calls.append(("remove", len(rows), sorted(rows)))

    def stats(self):
        return dict(n_live=len(self.docs), sum_len=sum(len(d) for d in self.docs))

    @property
    def num_docs(self):
        return len(self.docs)


class _FakeReplacingIndex(_FakeIndex):
    """... that can also replace rows, as engine.BM25Index can."""

    def replace(self, rows, flat, off, vocab):
        rows = [int(r) for r in rows]
        new = self._split(flat, off)
        assert len(new) == len(rows) == len(set(rows)) and all(0 <= r < len(self.docs) for r in rows)
        assert all(0 <= t < vocab for d in new for t in d)
        for r, d in zip(rows, new):
            self.docs[r] = d
        self.calls.append(("replace", len(rows), rows, vocab))


@pytest.fixture
def store_mod(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _FakeReplacingIndex())
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


def _courses(store):
    store._ensure_meta()
    return [m.get("course") for m in store._meta.metas]


def test_replace_on_a_current_index_replaces(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    st._ensure_meta()
    idx, v0 = st._index, st._version
    texts[4], texts[39] = "brandnewword " + texts[9], texts[2]
    metas[4] = dict(metas[4], course="moved")
    st.upsert_many(ids=[ids[39], ids[4]], texts=[texts[39], texts[4]], metadatas=[metas[39], metas[4]])
    assert st._version > v0 and st._dirty and st._pending_replace == {ids[4], ids[39]} and not st._meta_dirty
    assert st._id_list == ids and st._csr is None and st._prefix_csr is None
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(40))
    assert st._index is idx and _ops(idx) == [("build", 40), ("replace", 2)]
    assert idx.calls[-1][2] == [4, 39] and idx.calls[-1][3] == len(st._vocab) > idx.calls[0][2]
    assert not st._dirty and not st._pending_replace and st._pending_row is None and st._pending_drop is None
    assert _courses(st) == [m["course"] for m in metas] and not st._meta_dirty
    # two replaces of one id between two searches: one row, its last text
    st.upsert_many(ids=[ids[7]], texts=[texts[1]], metadatas=[metas[7]])
    texts[7] = texts[3]
    st.upsert_many(ids=[ids[7]], texts=[texts[7]], metadatas=[metas[7]])
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(40))
    assert _ops(idx, 2) == [("replace", 1)]


def test_one_upsert_mixing_existing_and_new_ids(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    _indexed(st)
    st._ensure_meta()
    texts[3], texts[29] = texts[38], texts[39] + " " + texts[0]
    mix = [30, 3, 31, 32, 31, 29, 33, 34]            # 31 twice: its last text counts
    tx = {i: texts[i] for i in mix}
    first31 = texts[35]
    st.upsert_many(ids=[ids[i] for i in mix], texts=[first31 if k == 2 else tx[i] for k, i in enumerate(mix)],
                   metadatas=[metas[i] for i in mix])
    assert st._id_list == ids[:35] and st._pending_row == 30 and st._pending_replace == {ids[3], ids[29]}
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(35))
    assert _ops(st._index) == [("build", 30), ("replace", 2), ("append", 5)]
    assert st._index.calls[1][2] == [3, 29]
    assert _courses(st) == [m["course"] for m in metas[:35]] and not st._meta_dirty


def test_delete_then_replace_is_remove_then_replace(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    _indexed(st)
    st.delete_many([ids[5], ids[6], ids[20]])
    texts[4], texts[29] = texts[33], texts[34]
    st.upsert_many(ids=[ids[29], ids[4]], texts=[texts[29], texts[4]], metadatas=[metas[29], metas[4]])
    st.upsert_many(ids=ids[30:32], texts=texts[30:32], metadatas=metas[30:32])
    keep = [i for i in range(32) if i not in (5, 6, 20)]
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, keep)
    assert _ops(st._index) == [("build", 30), ("remove", 3), ("replace", 2), ("append", 2)]
    assert st._index.calls[2][2] == [4, 26]          # rows in the numbering after the drop


def test_replace_then_delete_rebuilds(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    texts[4] = texts[9]
    st.upsert_many(ids=[ids[4]], texts=[texts[4]], metadatas=[metas[4]])
    assert st._pending_replace == {ids[4]}
    st.delete_many([ids[0]])
    assert not st._pending_replace
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(1, 40))
    assert _ops(st._index) == [("build", 40), ("build", 39)]


def test_replace_of_an_id_in_the_unappended_tail_calls_no_replace(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    _indexed(st)
    st.upsert_many(ids=ids[30:], texts=texts[30:], metadatas=metas[30:])
    texts[33] = texts[1] + " " + texts[2]
    st.upsert_many(ids=[ids[33]], texts=[texts[33]], metadatas=[metas[33]])
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(40))
    assert _ops(st._index) == [("build", 30), ("append", 10)]


def test_replace_while_no_index_exists_builds(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    texts[4] = texts[9]
    st.upsert_many(ids=[ids[4]], texts=[texts[4]], metadatas=[metas[4]])
    assert not st._pending_replace
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(40))
    assert _ops(st._index) == [("build", 40)]


def test_replace_on_an_index_without_replace_rebuilds(store_mod, monkeypatch):
    monkeypatch.setattr(store_mod.multidev, "new_bm25_index", lambda device=None: _FakeIndex())
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids, texts=texts, metadatas=metas)
    _indexed(st)
    texts[4] = texts[9]
    st.upsert_many(ids=[ids[4]], texts=[texts[4]], metadatas=[metas[4]])
    assert not st._pending_replace and st._meta_dirty
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas, range(40))
    assert _ops(st._index) == [("build", 40), ("build", 40)]


def test_replace_that_leaves_only_empty_documents_raises_at_the_call(store_mod):
    st = store_mod.BM25Store(index_dir=None)
    en = {"language": "en"}
    st.upsert_many(ids=["a", "b", "c"], texts=["", "alpha beta", "the"], metadatas=[en] * 3)
    assert _indexed(st) == [[], ["alpha", "beta"], []]
    with pytest.raises(ZeroDivisionError):
        st.upsert_many(ids=["b"], texts=["the"], metadatas=[en])
    assert st._ntokens == 0 and list(st._entries) == ["a", "b", "c"] and st._entries["b"].tokens == []
    # the same through the count a delete seeded, with a pending tail
    s2 = store_mod.BM25Store(index_dir=None)
    s2.upsert_many(ids=["a", "b", "c"], texts=["", "alpha", "gamma"], metadatas=[en] * 3)
    _indexed(s2)
    s2.upsert_many(ids=["d"], texts=["beta beta"], metadatas=[en])
    s2.delete_many(["c"])
    assert s2._ntokens == 3
    s2.upsert_many(ids=["d"], texts=[""], metadatas=[en])      # a row of the tail: no device work
    assert s2._ntokens == 1
    assert _indexed(s2) == [[], ["alpha"], []]
    assert _ops(s2._index) == [("build", 3), ("remove", 1), ("append", 1)]
    with pytest.raises(ZeroDivisionError):
        s2.upsert_many(ids=["b"], texts=["the"], metadatas=[en])


def test_sidecar_opened_store_rebuilds_once_then_replaces(store_mod, tmp_path):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    st.save()
    del st
    store_mod.release_all()
    a = store_mod.BM25Store(index_dir=tmp_path)
    a.load()
    _indexed(a)
    assert a._entries.pending
    texts[2], texts[17] = texts[31], texts[32]
    a.upsert_many(ids=[ids[17], ids[2]], texts=[texts[17], texts[2]], metadatas=[metas[17], metas[2]])
    assert a._csr is None and not a._entries.pending and not a._pending_replace   # the rebuild, as before
    assert _indexed(a) == _fresh(store_mod, ids, texts, metas, range(30))
    assert _ops(a._index) == [("build", 30), ("build", 30)]
    texts[5] = texts[33]
    metas[5] = dict(metas[5], course="moved")
    a.upsert_many(ids=[ids[5]], texts=[texts[5]], metadatas=[metas[5]])
    assert _indexed(a) == _fresh(store_mod, ids, texts, metas, range(30))
    assert _ops(a._index, 2) == [("replace", 1)]
    assert _courses(a) == [m["course"] for m in metas[:30]]
    a.save()                                         # the save after a replace rewrites the file
    store_mod.release_all()
    b = store_mod.BM25Store(index_dir=tmp_path)
    b.load()
    assert _indexed(b) == _fresh(store_mod, ids, texts, metas, range(30))
