"""compact(): reclaiming deleted rows on the device (cm_dense_compact / cm_dense_truncate), through
engine.DenseIndex, multidev.ShardedDenseIndex and the drop-in GpuVectorStore -- the hook the
reference's vacuum_indexes probes for (rag/admin/backup.py:178-202).

Bars: the surviving rows keep their order and their bits (export == rows[map]); a compacted index
answers like a fresh index built from the survivors -- rows equal everywhere, distances bit-equal
on the fp32 path and within 1e-6 on the automatic (coarse + fp64 re-rank) path, where only the
running maxima of the certificate's band (never lowered) may differ.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_dropin import FILTERS, PresetEmbedder, _new_process  # noqa: E402
from test_gpu_growth import _row_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

D = 768
NQS, KS, PATHS = (1, 16, 256), (10, 24), (0, 1)          # path 0 automatic, 1 fp32 (K1)


def _unit(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _pattern(n, step0, tile0, tail):
    """The main case's dead rows: every r % 7 == 3 (every 16-row group and 64-row tile loses rows),
    a whole 128-row step, a whole 64-row tile, row 0 and the last `tail` rows."""
    r = np.arange(n)
    dead = r % 7 == 3
    dead[step0:step0 + 128] = True
    dead[tile0:tile0 + 64] = True
    dead[0] = True
    dead[n - tail:] = True
    return dead


def _searches(idx, Q):
    out = {}
    for path in PATHS:
        idx.set_path(path)
        for nq in NQS:
            for k in KS:
                d, r = idx.search(Q[:nq], k)
                out[path, nq, k] = (d, r, idx.last_fallbacks())
    idx.set_path(0)
    return out


@pytest.fixture(scope="module")
def main_case():
    from classmate_hip import engine
    n = 20480
    rows = _unit(n, D, seed=31)
    Q = _unit(256, D, seed=32)
    Q[:8] = rows[[5, 4100, 6401, 9000, 12345, 20000, 20179, 1]]      # some queries on stored rows
    dead = _pattern(n, 4096, 6400, 300)
    live = ~dead
    assert live.sum() >= 16384                    # search_kind stays on the coarse scans (K1q / K1q-s)
    idx = engine.DenseIndex(D)
    idx.upsert(rows, np.arange(n, dtype=np.int64))
    idx.delete(np.nonzero(dead)[0])
    before = _searches(idx, Q)
    mp = pytest.MonkeyPatch()
    mp.setenv("CM_COMPACT_CHUNK_ROWS", "1000")    # many chunks, joins at no tile or group boundary
    try:
        m = idx.compact()
    finally:
        mp.undo()
    fresh = engine.DenseIndex(D)
    fresh.upsert(rows[m], np.arange(m.shape[0], dtype=np.int64))
    case = dict(idx=idx, fresh=fresh, rows=rows, Q=Q, live=live, map=m, before=before,
                after=_searches(idx, Q), want=_searches(fresh, Q))
    yield case
    idx.close()
    fresh.close()


def test_compact_map_size_and_rows(main_case):
    c = main_case
    idx, m = c["idx"], c["map"]
    assert m.dtype == np.int64 and np.array_equal(m, np.nonzero(c["live"])[0])
    assert idx.size == idx.live_count() == m.shape[0]
    out, live = idx.export(with_live=True)
    assert live.all()
    assert out.tobytes() == c["rows"][m].tobytes()
    assert idx.search_kind(16, 10) == c["fresh"].search_kind(16, 10) != 1
    assert idx.search_kind(256, 10) == c["fresh"].search_kind(256, 10) != 1


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nq", NQS)
def test_compact_searches_like_a_fresh_index(main_case, nq, k, path):
    c = main_case
    d, r, fb = c["after"][path, nq, k]
    dw, rw, fbw = c["want"][path, nq, k]
    assert (r >= 0).all() and np.array_equal(r, rw)
    err = float(np.abs(d.astype(np.float64) - dw).max())
    print(f"\npath {path} nq {nq} k {k}: max |d - d_fresh| = {err:.3g}, fallbacks {fb} (fresh {fbw})")
    if path == 1:
        assert d.tobytes() == dw.tobytes()
    else:
        assert err <= 1e-6
        if fbw == 0:
            assert fb == 0
    # ... and like the same index before the compaction, through the returned map
    db, rb, _ = c["before"][path, nq, k]
    assert np.array_equal(c["map"][r], rb)
    assert float(np.abs(d.astype(np.float64) - db).max()) <= 1e-6


def test_compact_stored_queries_find_their_rows(main_case):
    c = main_case
    new_of_old = {int(o): i for i, o in enumerate(c["map"])}
    d, r, _ = c["after"][0, 16, 10]
    for qi, old in enumerate([5, 4100, 6401, 9000, 12345, 20000, 20179, 1]):
        if c["live"][old]:
            assert r[qi, 0] == new_of_old[old] and abs(d[qi, 0]) < 1e-5
        else:
            assert new_of_old.get(old) is None and d[qi, 0] > 0.5


def test_truncate_on_the_coarse_planes():
    """truncate at n % 64 = 13 on a store large enough for the int8 / f16 scans: the cut tile's
    planes and scales are those of a fresh store of rows[:n]."""
    from classmate_hip import engine
    n0, n = 16640, 16397
    rows = _unit(n0, D, seed=41)
    Q = np.concatenate([rows[[n - 1, n - 13, 16384, 7]], rows[[n, n + 1, n0 - 1]], _unit(9, D, seed=42)])
    idx, fresh = engine.DenseIndex(D), engine.DenseIndex(D)
    idx.upsert(rows, np.arange(n0, dtype=np.int64))
    idx.truncate(n)
    fresh.upsert(rows[:n], np.arange(n, dtype=np.int64))
    assert idx.size == idx.live_count() == n and idx.search_kind(16, 10) != 1
    assert idx.export().tobytes() == rows[:n].tobytes()
    for path in PATHS:
        idx.set_path(path)
        fresh.set_path(path)
        d, r = idx.search(Q, 10)
        dw, rw = fresh.search(Q, 10)
        assert (r >= 0).all() and (r < n).all() and np.array_equal(r, rw)
        assert float(np.abs(d.astype(np.float64) - dw).max()) <= (0.0 if path == 1 else 1e-6)
        assert (r[:4, 0] == [n - 1, n - 13, 16384, 7]).all() and np.abs(d[:4, 0]).max() < 1e-5
    idx.close()
    fresh.close()


# ---- edges (<= 2000 rows: the fp32 scan) ------------------------------------------------------

def _equal_to_fresh(idx, rows_kept, dim, seed=7, k=10):
    from classmate_hip import engine
    fresh = engine.DenseIndex(dim)
    n = rows_kept.shape[0]
    fresh.upsert(rows_kept, np.arange(n, dtype=np.int64))
    Q = np.concatenate([rows_kept[:: max(n // 6, 1)][:6], _unit(10, dim, seed)])
    d, r = idx.search(Q, min(k, n))
    dw, rw = fresh.search(Q, min(k, n))
    assert np.array_equal(r, rw) and d.tobytes() == dw.tobytes()
    fresh.close()


def test_compact_without_dead_rows_is_identity():
    from classmate_hip import engine
    rows = _unit(1000, D, seed=51)
    idx = engine.DenseIndex(D)
    idx.upsert(rows, np.arange(1000, dtype=np.int64))
    m = idx.compact()
    assert np.array_equal(m, np.arange(1000)) and idx.size == 1000
    out, live = idx.export(with_live=True)
    assert live.all() and out.tobytes() == rows.tobytes()
    _equal_to_fresh(idx, rows, D)
    idx.close()


def test_compact_all_dead_then_upsert():
    from classmate_hip import engine
    rows = _unit(1200, D, seed=52)
    idx = engine.DenseIndex(D)
    idx.upsert(rows[:1000], np.arange(1000, dtype=np.int64))
    idx.delete(np.arange(1000))
    m = idx.compact()
    assert m.shape == (0,) and idx.size == 0 and idx.live_count() == 0
    idx.upsert(rows[1000:], np.arange(200, dtype=np.int64))
    assert idx.size == 200 and idx.live_count() == 200
    d, r = idx.search(rows[1000:1200:20], 5)
    assert (r[:, 0] == np.arange(0, 200, 20)).all() and np.abs(d[:, 0]).max() < 1e-5 and (r < 200).all()
    _equal_to_fresh(idx, rows[1000:], D)
    idx.close()


@pytest.mark.parametrize("dim", [384, 100])
def test_compact_other_dims(dim, monkeypatch):
    from classmate_hip import engine
    n = 1500
    rows = _unit(n, dim, seed=53 + dim)
    dead = np.random.default_rng(dim).random(n) < 0.3
    dead[[0, 63, 64, n - 1]] = True
    idx = engine.DenseIndex(dim)
    idx.upsert(rows, np.arange(n, dtype=np.int64))
    idx.delete(np.nonzero(dead)[0])
    monkeypatch.setenv("CM_COMPACT_CHUNK_ROWS", "77")
    m = idx.compact()
    assert np.array_equal(m, np.nonzero(~dead)[0]) and idx.size == idx.live_count() == m.shape[0]
    out, live = idx.export(with_live=True)
    assert live.all() and out.tobytes() == rows[m].tobytes()
    _equal_to_fresh(idx, rows[m], dim)
    idx.close()


def test_compact_then_upsert_delete_and_compact_again(monkeypatch):
    from classmate_hip import engine
    rows = _unit(2000, D, seed=54)
    idx = engine.DenseIndex(D)
    idx.upsert(rows[:1500], np.arange(1500, dtype=np.int64))
    idx.delete(np.arange(1, 1500, 3))
    monkeypatch.setenv("CM_COMPACT_CHUNK_ROWS", "333")
    m1 = idx.compact()
    n1 = m1.shape[0]
    assert n1 == 1000 and idx.size == n1
    idx.upsert(rows[1500:], np.arange(n1, n1 + 500, dtype=np.int64))       # appends at size
    assert idx.size == idx.live_count() == n1 + 500
    cur = np.concatenate([rows[m1], rows[1500:]])
    _equal_to_fresh(idx, cur, D)
    dead2 = np.zeros(n1 + 500, bool)
    dead2[10:700:2] = True
    dead2[n1 + 100:] = True
    idx.delete(np.nonzero(dead2)[0])
    m2 = idx.compact()
    assert np.array_equal(m2, np.nonzero(~dead2)[0]) and idx.size == idx.live_count() == m2.shape[0]
    assert idx.export().tobytes() == cur[m2].tobytes()
    _equal_to_fresh(idx, cur[m2], D)
    idx.close()


def test_compact_expect_live_mismatch_changes_nothing():
    from classmate_hip import engine
    rows = _unit(1000, D, seed=55)
    idx = engine.DenseIndex(D)
    idx.upsert(rows, np.arange(1000, dtype=np.int64))
    idx.delete(np.arange(0, 1000, 4))
    out0, live0 = idx.export(with_live=True)
    for wrong in (749, 751):
        with pytest.raises(ValueError):
            idx.compact(expect_live=wrong)
        out1, live1 = idx.export(with_live=True)
        assert idx.size == 1000 and out1.tobytes() == out0.tobytes() and np.array_equal(live1, live0)
    assert idx.compact(expect_live=750).shape == (750,)
    idx.close()


def test_truncate_inside_a_group():
    from classmate_hip import engine
    n0, n = 1000, 709                                     # 709 % 16 = 5
    rows = _unit(n0, D, seed=56)
    idx = engine.DenseIndex(D)
    idx.upsert(rows, np.arange(n0, dtype=np.int64))
    idx.delete(np.array([3, 700]))
    with pytest.raises(ValueError):
        idx.truncate(n0 + 1)
    idx.truncate(n)
    assert idx.size == n and idx.live_count() == n - 2    # dead rows below n stay dead
    out, live = idx.export(with_live=True)
    assert out.tobytes() == rows[:n].tobytes() and not live[3] and not live[700] and live.sum() == n - 2
    d, r = idx.search(rows[[n, n + 1, 999, 800]], 10)     # queries on dropped rows
    assert (r >= 0).all() and (r < n).all() and d[:, 0].min() > 0.5
    probe = np.array([0, 1, 5, 640, 703, 704, 708])
    d, r = idx.search(rows[probe], 3)
    assert (r[:, 0] == probe).all() and np.abs(d[:, 0]).max() < 1e-5
    idx.upsert(rows[n:n + 50], np.arange(n, n + 50, dtype=np.int64))      # the cleared tail takes rows again
    d, r = idx.search(rows[[n, n + 49]], 3)
    assert (r[:, 0] == [n, n + 49]).all() and np.abs(d[:, 0]).max() < 1e-5
    idx.close()


# ---- shrink -------------------------------------------------------------------------------------

def test_compact_shrink_returns_the_memory():
    import torch
    from classmate_hip import engine
    n0, per = 300_000, 50_000
    idx = engine.DenseIndex(D, capacity=0)
    g = torch.Generator(device="cuda").manual_seed(61)
    probes = {}
    for b in range(n0 // per):
        x = torch.randn(per, D, device="cuda", generator=g)
        x /= x.norm(dim=1, keepdim=True)
        idx.upsert_dev(x, b * per)
        torch.cuda.synchronize()
        if b < 2:
            for j in (0, per // 2, per - 1):
                probes[b * per + j] = x[j].cpu().numpy()
        del x
    n = n0 // 3
    idx.delete(np.arange(n, n0, dtype=np.int64))          # the upper two thirds
    bytes0 = idx.mem_stats()["bytes"]
    m = idx.compact(shrink=True)
    assert m.shape == (n,) and m[0] == 0 and m[-1] == n - 1 and idx.size == idx.live_count() == n
    cap = -(-n // 128) * 128
    assert idx.mem_stats()["bytes"] == _row_bytes(cap) < bytes0
    rows = np.array(sorted(probes), dtype=np.int64)
    d, r = idx.search(np.stack([probes[i] for i in rows]), 3)
    assert (r[:, 0] == rows).all() and np.abs(d[:, 0]).max() < 1e-5
    idx.upsert_dev(torch.ones(10, D, device="cuda"), n)   # a shrunk store grows again
    torch.cuda.synchronize()
    assert idx.size == n + 10
    idx.close()


# ---- sharded ------------------------------------------------------------------------------------

def test_sharded_compact_equals_one_index():
    from classmate_hip import engine, multidev
    n = 5000
    rows = _unit(n, D, seed=71)
    dead = _pattern(n, 1024, 1600, 75)
    sh = multidev.ShardedDenseIndex(D, [0, 0, 0], block=64)
    sh.upsert(rows, np.arange(n, dtype=np.int64))
    sh.delete(np.nonzero(dead)[0])
    with pytest.raises(ValueError):
        sh.compact(expect_live=int((~dead).sum()) + 1)
    out0, live0 = sh.export(with_live=True)
    assert out0.tobytes() == rows.tobytes() and np.array_equal(live0, ~dead)     # nothing was written
    m = sh.compact(expect_live=int((~dead).sum()))
    keep = np.nonzero(~dead)[0]
    assert np.array_equal(m, keep) and sh.size == sh.live_count() == keep.shape[0]
    # rows changed shard: the owner of a new row is not the owner of its old row everywhere
    assert (sh.map.owner_local(m)[0] != sh.map.owner_local(np.arange(m.shape[0]))[0]).any()
    out, live = sh.export(with_live=True)
    assert live.all() and out.tobytes() == rows[keep].tobytes()
    one = engine.DenseIndex(D)
    one.upsert(rows[keep], np.arange(keep.shape[0], dtype=np.int64))
    Q = np.concatenate([rows[keep][::700], _unit(16, D, seed=72)])
    for k in KS:
        d, r = sh.search(Q, k)
        dw, rw = one.search(Q, k)
        assert np.array_equal(r, rw) and d.tobytes() == dw.tobytes()
    sh.compact(shrink=True)                                # no dead rows: shrink only
    assert sh.size == keep.shape[0] and sh.export().tobytes() == rows[keep].tobytes()
    sh.close()
    one.close()


# ---- drop-in ------------------------------------------------------------------------------------

def _full(res):
    return [(r["id"], r["document"], r["metadata"], r["scores"]["vector_distance"], r["scores"]["bm25_score"],
             r["scores"]["fused"]) for r in res]


def _answers(retr, questions, monkeypatch):
    out = {}
    for path in ("device", "host"):
        if path == "host":
            monkeypatch.setenv("CM_RETRIEVE_DEVICE", "0")
        for fname in ("none", "course_only", "tags_exam"):
            out[path, fname] = [_full(retr.retrieve(question=q, filters=FILTERS[fname], top_k=10)) for q in questions]
        monkeypatch.delenv("CM_RETRIEVE_DEVICE", raising=False)
    assert any(len(a) for a in out["device", "tags_exam"])
    return out


@pytest.mark.parametrize("sharded", [False, True])
def test_dropin_store_compact(corpus, tmp_path, monkeypatch, sharded):
    from classmate_hip import multidev
    from classmate_hip.retrieval import BM25Store, ChromaVectorStore, HybridRetriever, vector_store
    if sharded:
        monkeypatch.setenv("CM_DEVICES", "0,0")
        monkeypatch.setenv("CM_SHARD_BLOCK", "64")
    _new_process()
    n, n_del = 600, 200
    ids, texts, emb = corpus["ids"][:n], corpus["texts"][:n], corpus["emb"][:n]
    metas = []
    for m in corpus["metas"][:n]:
        m = dict(m)
        tags = [k[4:] for k, v in m.items() if k.startswith("tag_") and v is True]
        if tags:
            m["tags"] = tags
        metas.append(m)
    vs = ChromaVectorStore(persist_dir=tmp_path / "chroma")
    vs.upsert(ids=ids, documents=texts, metadatas=metas, embeddings=emb)
    bm = BM25Store(index_dir=tmp_path / "bm25")
    bm.upsert_many(ids=ids, texts=texts, metadatas=metas)
    assert isinstance(vs._index, multidev.ShardedDenseIndex) == sharded
    gone = [ids[i] for i in np.random.default_rng(81).choice(n, n_del, replace=False)]
    vs.delete(gone)
    bm.delete_many(gone)
    retr = HybridRetriever(vector_store=vs, bm25_store=bm, embedder=PresetEmbedder(corpus["qtexts"], corpus["qvecs"]),
                           k_vector=10, k_bm25=10)
    questions = corpus["qtexts"][:8]
    before = _answers(retr, questions, monkeypatch)
    assert len(vs._ids) == n and vs._ids != bm._id_list
    version = vs._version

    assert hasattr(vs, "compact")                         # what vacuum_indexes probes for
    st = vs.compact()
    assert st["rows_before"] == n and st["rows_after"] == vs.count() == n - n_del
    assert st["bytes_after"] <= st["bytes_before"]
    assert len(vs._ids) == n - n_del and vs._ids == bm._id_list
    assert vs._version > version and all(vs._row[i] == r for r, i in enumerate(vs._ids))
    kept = [i for i in range(n) if ids[i] in vs._row]
    assert vs._meta.metas == [metas[i] for i in kept]
    assert vs._meta.tags["exam"] == {r for r, i in enumerate(kept) if "exam" in metas[i].get("tags", ())}
    assert _answers(retr, questions, monkeypatch) == before
    d = tmp_path / "chroma" / vs.collection_name
    assert os.path.getsize(d / "vectors.f32") == (n - n_del) * emb.shape[1] * 4
    again = vs.compact()                                  # nothing dead: no version bump, no write
    assert again["rows_before"] == again["rows_after"] == n - n_del and vs._version == version + 1

    vector_store.release_all()                            # a new process opens the directory
    vs2 = ChromaVectorStore(persist_dir=tmp_path / "chroma")
    assert vs2.count() == n - n_del and vs2._st is not vs._st
    retr2 = HybridRetriever(vector_store=vs2, bm25_store=bm, embedder=retr.embedder, k_vector=10, k_bm25=10)
    assert _answers(retr2, questions, monkeypatch) == before
    assert vs2._ids == bm._id_list
