"""MetaIndex.compacted (host side of the stores' compact()): the index of the surviving rows,
renumbered, must evaluate every where clause exactly as a MetaIndex filled by set() with the
surviving metadata in order.  No GPU."""
import numpy as np
import pytest

from classmate_hip.retrieval.filters import MetaIndex

N = 300
COURSES = ["cs101", "math201", "phys150", None]
LANGS = ["en", "it", None]
TAGS = ["exam", "oop", "lab", "proofs"]


def _metas():
    rng = np.random.default_rng(21)
    out = []
    for r in range(N):
        m = {"chunk_id": r}
        c = COURSES[int(rng.integers(len(COURSES)))]
        if c is not None or r % 5 == 0:        # some rows hold course: None, others lack the key
            m["course"] = c
        lang = LANGS[int(rng.integers(len(LANGS)))]
        if lang is not None:
            m["language"] = lang
        k = int(rng.integers(0, 3))
        if k:
            m["tags"] = [TAGS[int(i)] for i in rng.choice(len(TAGS), size=k, replace=False)]
        if r % 4 == 0:
            m["tag_exam"] = True
        out.append(m)
    out[17]["author"] = ["an", "unhashable", "value"]
    out[18]["author"] = "rossi"
    out[200]["author"] = {"also": "unhashable"}
    out[19]["author"] = ["unhashable", "and", "removed"]
    out[42] = None                              # a row upserted without metadata
    return out


CHROMA = [
    {"course": "cs101"},
    {"$and": [{"course": "cs101"}, {"language": "en"}]},
    {"$or": [{"course": "math201"}, {"language": "it"}]},
    {"course": {"$in": ["cs101", "phys150"]}},
    {"course": {"$nin": ["cs101"]}},
    {"language": {"$ne": "en"}},
    {"$and": [{"tag_exam": True}, {"course": {"$ne": "math201"}}]},
    {"chunk_id": {"$gte": 150}},
    {"author": "rossi"},
    None,
]
BM25 = [
    {"course": "cs101"},
    {"course": "cs101", "language": "it"},
    {"tags": {"$contains": "exam"}},
    {"tags": {"$contains": ["exam", "oop"]}},
    {"$and": [{"course": "math201"}, {"tags": {"$contains": "lab"}}]},
    {"course": None, "unit": None},                         # Q4: a None value matches a missing key
    {"course": "phys150", "unit": None, "author": None},
    {"author": ["an", "unhashable", "value"]},
    {"author": "rossi"},
    None,
]


@pytest.fixture(scope="module")
def case():
    metas = _metas()
    full = MetaIndex()
    for r, m in enumerate(metas):
        full.set(r, m)
    dead = [r for r in range(N) if r % 3 == 1]              # a third of the rows
    assert 19 in dead and not {17, 18, 42, 200} & set(dead)
    for r in dead:
        full.remove(r)
    keep = [r for r in range(N) if r % 3 != 1]
    want = MetaIndex()
    for i, r in enumerate(keep):
        want.set(i, metas[r])
    return full, keep, want, metas


def test_compacted_evaluates_like_a_fresh_index(case):
    full, keep, want, metas = case
    got = full.compacted(keep)
    assert len(got) == len(keep) == len(want)
    assert got.uid != full.uid and got.uid != want.uid
    assert got.metas == [metas[r] for r in keep]
    assert got.live[:len(keep)].all()
    for w in CHROMA:
        a, b = got.chroma_mask(w), want.chroma_mask(w)
        assert a.shape == b.shape and (a == b).all(), w
        # and the compaction selected exactly the survivors of the old index's answer
        assert (a == full.chroma_mask(w)[keep]).all(), w
    for w in BM25:
        a, b = got.bm25_mask(w), want.bm25_mask(w)
        assert a.shape == b.shape and (a == b).all(), w
        assert (a == full.bm25_mask(w)[keep]).all(), w
    # the clauses are not vacuous on this data
    assert 0 < got.chroma_mask(CHROMA[1]).sum() < len(keep)
    assert 0 < got.bm25_mask(BM25[3]).sum() < len(keep)
    assert got.bm25_mask(BM25[5]).sum() > 0 and got.bm25_mask(BM25[7]).sum() == (1 if 17 in keep else 0)
    # compiled programs (what the device evaluates) build from the same columns
    for w in CHROMA:
        assert got.chroma_program(w).fits_device == want.chroma_program(w).fits_device


def test_compacted_is_independent_and_mutable(case):
    full, keep, want, metas = case
    got = full.compacted(keep)
    v = full.version
    got.set(len(keep), {"course": "cs101", "tags": ["exam"]})       # a later upsert appends
    got.remove(0)
    assert full.version == v and len(full) == N
    assert got.bm25_mask({"tags": {"$contains": "exam"}})[len(keep)]
    assert not got.live[0]
    assert full.live[keep[0]]
    # tag row sets are on the new numbering only
    for rows in got.tags.values():
        assert all(0 <= r <= len(keep) for r in rows)


def test_compacted_snapshot_round_trips(case):
    full, keep, want, metas = case
    got = full.compacted(keep)
    snap = got.snapshot()
    assert snap is not None
    info, arrays = snap
    assert info["rows"] == len(keep)
    back = MetaIndex.from_snapshot(info, arrays, list(got.metas))
    for w in CHROMA:
        assert (back.chroma_mask(w) == want.chroma_mask(w)).all(), w
    for w in BM25:
        assert (back.bm25_mask(w) == want.bm25_mask(w)).all(), w


def test_compacted_edges():
    m = MetaIndex()
    assert len(m.compacted([])) == 0
    for r in range(5):
        m.set(r, {"course": "a" if r % 2 else "b"})
    e = m.compacted([])
    assert len(e) == 0 and e.chroma_mask({"course": "a"}).shape == (0,)
    same = m.compacted(list(range(5)))
    assert (same.chroma_mask({"course": "a"}) == m.chroma_mask({"course": "a"})).all()
    with pytest.raises(ValueError):
        m.compacted([3, 1])
