"""BM25 append, the parts that need no GPU: the C ABI's argument check that runs before any device
call, the sharded index's row spans (multidev.shard_spans), and BM25Store's choice between an
append and a rebuild (against a stand-in for the device index that records what it is given)."""
import ctypes

import numpy as np
import pytest


def test_append_null_handle_is_value_error():
    from classmate_hip import _lib
    off = (ctypes.c_int64 * 2)(0, 0)
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_append"](None, None, off, 1, 1), "cm_bm25_append")
    assert "handle" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.fn["cm_bm25_append_dev"](None, None, None, 1, 0, 1, None), "cm_bm25_append_dev")


def _rows(spans):
    return [r for a, e in spans for r in range(a, e)]


@pytest.mark.parametrize("G", [1, 3, 4])
@pytest.mark.parametrize("n_old", [0, 1, 63, 64, 200])
@pytest.mark.parametrize("n_add", [1, 64, 300])
def test_append_spans_extend_build_spans(G, n_old, n_add):
    from classmate_hip.multidev import RowMap, shard_spans
    B, n_new = 64, n_old + n_add
    rm = RowMap(G, B)
    seen = []
    for s in range(G):
        built_old, added = shard_spans(G, B, s, 0, n_old), shard_spans(G, B, s, n_old, n_new)
        built_new = shard_spans(G, B, s, 0, n_new)
        # the shard's rows of the old build followed by the appended ones are its rows of the new build,
        # in its local order: local row l of the sequence is global row to_global(s, l)
        rows = _rows(built_old) + _rows(added)
        assert rows == _rows(built_new)
        assert all(a < e for a, e in added) and all(n_old <= a and e <= n_new for a, e in added)
        assert len(_rows(built_old)) == rm.local_count(s, n_old)
        assert len(rows) == rm.local_count(s, n_new)
        assert rm.to_global(s, np.arange(len(rows), dtype=np.int64)).tolist() == rows
        seen += _rows(added)
    assert sorted(seen) == list(range(n_old, n_new))


# ---- BM25Store's choice between append and rebuild, against a recording stand-in for the index ----
class _FakeIndex:
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


@pytest.fixture
def store_mod(monkeypatch):
    from classmate_hip.retrieval import bm25
    monkeypatch.setattr(bm25.multidev, "new_bm25_index", lambda device=None: _FakeIndex())
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


def _fresh(bm25, ids, texts, metas):
    one = bm25.BM25Store(index_dir=None)
    one.upsert_many(ids=ids, texts=texts, metadatas=metas)
    return _indexed(one)


def test_store_appends_new_ids_and_rebuilds_otherwise(store_mod):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=None)
    st.upsert_many(ids=ids[:20], texts=texts[:20], metadatas=metas[:20])
    v0 = st._version
    assert _indexed(st) == _fresh(store_mod, ids[:20], texts[:20], metas[:20])
    idx = st._index
    st.upsert_many(ids=ids[20:23], texts=texts[20:23], metadatas=metas[20:23])
    assert st._version == v0 + 1 and st._dirty
    assert _indexed(st) == _fresh(store_mod, ids[:23], texts[:23], metas[:23])
    # two upserts before the next search: one append of both
    st.upsert_many(ids=ids[23:30], texts=texts[23:30], metadatas=metas[23:30])
    st.upsert_many(ids=ids[30:], texts=texts[30:], metadatas=metas[30:])
    assert _indexed(st) == _fresh(store_mod, ids, texts, metas)
    assert st._index is idx
    assert [c[:2] for c in idx.calls] == [("build", 20), ("append", 3), ("append", 17)]
    assert idx.calls[-1][2] == len(st._vocab)
    # a replace in place, then a delete: rebuilds
    st.upsert_many(ids=[ids[4], "new"], texts=[texts[9], texts[1]], metadatas=[metas[4], metas[1]])
    assert _indexed(st) == _fresh(store_mod, ids + ["new"], texts[:4] + [texts[9]] + texts[5:] + [texts[1]],
                                  metas + [metas[1]])
    st.delete_many([ids[0]])
    _indexed(st)
    assert [c[:2] for c in idx.calls[3:]] == [("build", 41), ("build", 40)]
    # an append-only upsert while the index is stale for another reason: still a rebuild
    st.delete_many([ids[1]])
    st.upsert_many(ids=["x"], texts=[texts[2]], metadatas=[metas[2]])
    _indexed(st)
    assert idx.calls[-1][:2] == ("build", 40)


def test_store_empty_corpus_error_survives(store_mod):
    st = store_mod.BM25Store(index_dir=None)
    with pytest.raises(ZeroDivisionError):
        st.upsert_many(ids=["a"], texts=[""], metadatas=[{"language": "en"}])
    with pytest.raises(ZeroDivisionError):           # still every token list empty
        st.upsert_many(ids=["b"], texts=["the"], metadatas=[{"language": "en"}])
    st.upsert_many(ids=["c"], texts=["alpha beta"], metadatas=[{"language": "en"}])
    st.upsert_many(ids=["d"], texts=[""], metadatas=[{"language": "en"}])
    assert _indexed(st) == [[], [], ["alpha", "beta"], []]


def test_store_opened_from_sidecar_appends_to_the_persisted_csr(store_mod, tmp_path):
    ids, texts, metas = _corpus()
    st = store_mod.BM25Store(index_dir=tmp_path)
    st.upsert_many(ids=ids[:30], texts=texts[:30], metadatas=metas[:30])
    st.save()
    del st
    store_mod.release_all()
    a = store_mod.BM25Store(index_dir=tmp_path)
    a.load()
    b = store_mod.BM25Store(index_dir=tmp_path)
    b.load()                                         # shares a's state until one of them changes
    assert a._st is b._st and a._entries.pending
    a.upsert_many(ids=ids[30:], texts=texts[30:], metadatas=metas[30:])
    assert a._st is not b._st
    assert _indexed(a) == _fresh(store_mod, ids, texts, metas)
    assert [c[:2] for c in a._index.calls] == [("build", 30), ("append", 10)]
    assert a._entries.pending                        # no persisted record was parsed
    a.upsert_many(ids=["z"], texts=[texts[3]], metadatas=[metas[3]])
    assert _indexed(a) == _fresh(store_mod, ids + ["z"], texts + [texts[3]], metas + [metas[3]])
    assert a._index.calls[-1][:2] == ("append", 1) and a._entries.pending
    assert _indexed(b) == _fresh(store_mod, ids[:30], texts[:30], metas[:30])
    # a copy of a state whose CSR covers only its first rows builds from it, then appends the rest
    a.save()
    c = store_mod.BM25Store(index_dir=tmp_path)
    c.load()
    assert c._st is a._st
    c.upsert_many(ids=["y"], texts=[texts[6]], metadatas=[metas[6]])
    assert _indexed(c) == _fresh(store_mod, ids + ["z", "y"], texts + [texts[3], texts[6]], metas + [metas[3], metas[6]])
    assert [x[:2] for x in c._index.calls] == [("build", 30), ("append", 12)]
