"""The uncomfortable shard shapes of classmate_hip/multidev.py (CM_DEVICES=0,0,0,0: four handles on
one card, as tests/test_gpu_multidev.py): shards smaller than k, shards that hold nothing, a filter
whose candidates all live in one shard, a shard whose documents are all tombstones, and top_k
beyond the fused lists through the drop-in classes.

* BM25: the unsharded C oracle (oracle/corc.py), bit for bit -- rows, scores, valid counts; every
  entry past the candidates is (row -1, score 0.0).  A shard is searched with the GLOBAL candidate
  count (cm_bm25_search_idf), so k and n_cand may both exceed what the shard holds: the full-order
  path (k > cm_max_topk()) must copy no more than its own sorted documents and report, like the
  fused path, only its own valid entries (out_n).
* dense: the exact fp64 scan (test_gpu_scale.exact_topk / check_dense, 1e-4) and equality with one
  engine.DenseIndex over the whole corpus.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_parallel_gloo import _corpus  # noqa: E402
from test_gpu_multidev import _mask, _oracle_bm25, _words  # noqa: E402

from oracle import corc  # noqa: E402

pytestmark = pytest.mark.gpu
DEVS = [0, 0, 0, 0]
BLOCK = 1024


@pytest.fixture(scope="module")
def corpus6k():
    toks, off, vocab, queries = _corpus(nd=6000)
    return toks, off, vocab, queries


def _dev_queries(queries):
    import torch
    q_off = np.zeros(len(queries) + 1, np.int32)
    q_off[1:] = np.cumsum([len(x) for x in queries])
    qt = torch.from_numpy(np.concatenate([np.asarray(x, np.int32) for x in queries])).cuda()
    return qt, torch.from_numpy(q_off).cuda()


def _allow_dev(words):
    import torch
    return torch.from_numpy(words.view(np.int32)).cuda()


def _same(got, want, what):
    """(scores, rows[, nv]) of a sharded search == the oracle's (scores, rows), bit for bit."""
    S, R = got[0], got[1]
    if hasattr(S, "cpu"):
        S, R = S.cpu().numpy(), R.cpu().numpy()
    sc, rw = want[0], want[1]
    assert np.array_equal(R, rw), what
    assert np.array_equal(S, sc), what
    pad = rw < 0
    assert (S[pad] == 0.0).all() and not np.signbit(S[pad]).any(), what
    if len(got) > 2:
        assert np.array_equal(got[2], (rw >= 0).sum(1)), what


def test_bm25_shards_smaller_than_k(corpus6k):
    """6000 documents in blocks of 1024 over 4 shards: 2048 / 1904 / 1024 / 1024.  k = 1500 exceeds
    shards 2 and 3, 2500 every shard, 7000 the corpus; under the filter (2100 candidates) k exceeds
    a shard's own candidates while staying below the global count."""
    from classmate_hip import multidev
    toks, off, vocab, queries = corpus6k
    nd = off.shape[0] - 1
    bm = multidev.ShardedBM25Index(DEVS, block=BLOCK)
    bm.build(toks, off, vocab)
    assert [sh.num_docs for sh in bm.shards] == [2048, 1904, 1024, 1024]
    mask = _mask(nd)
    assert mask.sum() == 2100
    words = _words(mask)
    for k in (300, 1500, 2500, 7000):
        want = _oracle_bm25(toks, off, vocab, queries, k)
        assert ((want[1] >= 0).sum(1) == min(k, nd)).all()
        got = bm.search(queries, k)
        _same(got, want, ("unfiltered", k))
        fwant = _oracle_bm25(toks, off, vocab, queries, k, mask)
        assert ((fwant[1] >= 0).sum(1) == min(k, 2100)).all()
        _same(bm.search(queries, k, words), fwant, ("filtered", k))
        if k == 7000:
            assert (got[1][:, nd:] == -1).all() and (got[0][:, nd:] == 0.0).all()
            assert (got[1][:, :nd] >= 0).all()
    bm.close()


def test_bm25_empty_shards():
    """1500 documents: shards 2 and 3 hold nothing."""
    from classmate_hip import multidev
    toks, off, vocab, queries = _corpus(nd=1500)
    nd = off.shape[0] - 1
    bm = multidev.ShardedBM25Index(DEVS, block=BLOCK)
    bm.build(toks, off, vocab)
    assert [sh.num_docs for sh in bm.shards] == [1024, 476, 0, 0]
    assert bm.num_docs == nd
    mask = _mask(nd)
    words = _words(mask)
    bm.prepare_filtered()
    qt, qo = _dev_queries(queries)
    allow = _allow_dev(words)
    for k in (1, 10, 64, 300, 2000):
        want = _oracle_bm25(toks, off, vocab, queries, k)
        assert ((want[1] >= 0).sum(1) == min(k, nd)).all()
        _same(bm.search(queries, k), want, ("host", k))
        _same(bm.search(queries, k, words), _oracle_bm25(toks, off, vocab, queries, k, mask), ("filtered host", k))
    for k in (1, 10, 64, 256):
        _same(bm.search_dev(qt, qo, k), _oracle_bm25(toks, off, vocab, queries, k), ("dev", k))
        _same(bm.search_filtered(qt, qo, k, allow), _oracle_bm25(toks, off, vocab, queries, k, mask),
              ("filtered dev", k))
    ocsr = corc.build_csr(toks, off, vocab)
    csr = bm.export()
    for key in ("term_off", "post_doc", "post_tf", "dl"):
        assert np.array_equal(csr[key], ocsr[key]), key
    bm.close()


def test_bm25_filter_within_one_shard(corpus6k):
    """The candidates are rows 1024..1099: one block, all of it on shard 1.  Every other shard
    scores with the global candidate statistics and contributes only -1 rows."""
    from classmate_hip import multidev
    toks, off, vocab, queries = corpus6k
    nd = off.shape[0] - 1
    bm = multidev.ShardedBM25Index(DEVS, block=BLOCK)
    bm.build(toks, off, vocab)
    mask = np.zeros(nd, bool)
    mask[1024:1100] = True
    words = _words(mask)
    own, _ = bm.map.owner_local(np.nonzero(mask)[0])
    assert (own == 1).all()
    qt, qo = _dev_queries(queries)
    allow = _allow_dev(words)
    for k in (10, 300):
        want = _oracle_bm25(toks, off, vocab, queries, k, mask)
        assert ((want[1] >= 0).sum(1) == min(k, 76)).all()
        got = bm.search(queries, k, words)
        _same(got, want, ("host", k))
        assert (got[2] == min(k, 76)).all()
    for k in (10, 64):
        _same(bm.search_filtered(qt, qo, k, allow), _oracle_bm25(toks, off, vocab, queries, k, mask), ("dev", k))
    bm.close()


def test_bm25_one_shard_all_tombstones(corpus6k):
    """Rows 2048..3071 (block 2 = everything shard 2 holds) are dead at build."""
    from classmate_hip import multidev
    toks, off, vocab, queries = corpus6k
    nd = off.shape[0] - 1
    live = np.ones(nd, bool)
    live[2048:3072] = False
    bm = multidev.ShardedBM25Index(DEVS, block=BLOCK)
    bm.build(toks, off, vocab, live=live.astype(np.uint8))
    assert bm.shards[2].num_docs == 1024 and bm.shards[2].num_postings == 0   # no live document: no postings
    assert bm.stats()["n_live"] == 4976
    qt, qo = _dev_queries(queries)

    def alive(R):
        R = R.cpu().numpy() if hasattr(R, "cpu") else R
        return not ((R >= 2048) & (R < 3072)).any()

    for k in (10, 300, 1500):
        want = _oracle_bm25(toks, off, vocab, queries, k, live)
        assert ((want[1] >= 0).sum(1) == k).all()
        got = bm.search(queries, k)
        _same(got, want, ("host", k))
        assert alive(got[1])
    for k in (10, 64):
        got = bm.search_dev(qt, qo, k)
        _same(got, _oracle_bm25(toks, off, vocab, queries, k, live), ("dev", k))
        assert alive(got[1])
    bm.close()


@pytest.mark.parametrize("k", [100, 300])
def test_bm25_search_idf_out_n_counts_local_entries(corpus6k, k):
    """cm_bm25_search_idf at the C ABI on an index of the first 64 documents with the 6000-document
    statistics and n_cand = 6000: out_n is 64 (not min(k, n_cand)) on the fused path (k = 100) and
    the full-order path (k = 300), rows past it are -1 and scores 0.0, and the 64 entries equal the
    oracle's scores of those documents under the same statistics."""
    from classmate_hip import _lib as L, engine
    toks, off, vocab, queries = corpus6k
    nd = off.shape[0] - 1
    n = 64
    gcsr = corc.build_csr(toks, off, vocab)
    idf, _ = corc.bm25_idf(gcsr["df"], gcsr["first_key"], nd)
    avgdl = float(off[-1]) / nd
    sub_toks, sub_off = toks[:off[n]], off[:n + 1]
    want = corc.bm25_topk(corc.build_csr(sub_toks, sub_off, vocab), idf, avgdl, queries, k)
    assert ((want[1] >= 0).sum(1) == n).all()
    bm = engine.BM25Index(device=0)
    bm.build(sub_toks, sub_off, vocab)
    nq = len(queries)
    q_off = np.zeros(nq + 1, np.int32)
    q_off[1:] = np.cumsum([len(x) for x in queries])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32) for x in queries]), np.int32)
    q_idf = np.ascontiguousarray([idf[t] if 0 <= t < vocab else 0.0 for t in flat.tolist()], np.float64)
    sc = np.full((nq, k), 7.0, np.float64)
    rw = np.full((nq, k), 7, np.int64)
    nv = np.full(nq, -7, np.int32)
    L.check(L.fn["cm_bm25_search_idf"](bm._h, L.ptr(flat), L.ptr(q_off), nq, int(k), None, L.ptr(q_idf), avgdl,
                                       int(nd), L.ptr(sc), L.ptr(rw), L.ptr(nv)), "cm_bm25_search_idf")
    assert (nv == n).all()
    assert (rw[:, n:] == -1).all() and (sc[:, n:] == 0.0).all()
    assert np.array_equal(rw, want[1]) and np.array_equal(sc, want[0])
    bm.close()


def _dense_case(nd, shard_rows):
    import torch
    from classmate_hip import engine, multidev
    from test_gpu_scale import check_dense, exact_topk
    D, NQ, SLACK = 768, 24, 40
    rng = np.random.default_rng(nd)
    emb = rng.standard_normal((nd, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    emb[70] = emb[11]                                  # a duplicate pair on shards 0 and 1: tie by global row
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    q[0] = emb[11]
    rows = np.arange(nd, dtype=np.int64)
    full = engine.DenseIndex(D, device=0, capacity=nd)
    full.upsert(emb, rows)
    sh = multidev.ShardedDenseIndex(D, DEVS, capacity=nd, block=64)
    sh.upsert(emb, rows)
    assert [s.size for s in sh.shards] == shard_rows and sh.size == nd
    mask = np.ones(nd, bool)
    mask[1::4] = False                                 # the allow bitmap clears every fourth row
    words = _words(mask)
    qd = torch.from_numpy(q).cuda()
    live = np.ones(nd, bool)
    for deleted in (False, True):
        if deleted:
            drop = np.arange(5, nd, 7)                 # every 7th row (not 11, not 70)
            full.delete(drop)
            sh.delete(drop)
            live[drop] = False
            assert sh.live_count() == live.sum()
        for allow in (None, words):
            cand = np.nonzero(live & (mask if allow is not None else True))[0]
            nc = cand.shape[0]
            o_d, o_r = exact_topk(emb[cand], q, nc)
            # no candidate lies past the list's end: an unreachable entry stands for "nothing more"
            o_d = np.concatenate([o_d, np.full((NQ, 1), np.inf)], 1)
            o_r = np.concatenate([cand[o_r], np.full((NQ, 1), -2, np.int64)], 1)
            al = None if allow is None else _allow_dev(allow)
            for k in (10, 100, 256, 300, 400):
                kc = min(k, nc)
                d0, r0, v0 = full.search(q, k, allow, return_vectors=True)
                d1, r1, v1 = sh.search(q, k, allow, return_vectors=True)
                lists = [("one", d0, r0), ("sharded host", d1, r1)]
                if k <= 256:
                    d2, r2 = sh.search_dev(qd, k, allow=al)
                    lists.append(("sharded dev", d2.cpu().numpy(), r2.cpu().numpy()))
                for name, dd, rr in lists:
                    what = (name, nd, deleted, allow is not None, k)
                    assert (rr[:, :kc] >= 0).all() and (rr[:, kc:] == -1).all(), what
                    assert (dd[:, kc:] == 0).all(), what
                    check_dense(dd, rr, o_d[:, :kc + SLACK], o_r[:, :kc + SLACK], kc)
                    assert np.array_equal(rr, r0) and np.array_equal(dd, d0), what
                assert r0[0, 0] == 11 and r0[0, 1] == 70
                for vv, rr in ((v0, r0), (v1, r1)):
                    assert (vv[rr < 0] == 0).all()
                    assert np.array_equal(vv[rr >= 0], emb[rr[rr >= 0]])
    full.close()
    sh.close()


def test_dense_shards_smaller_than_k():
    """300 rows in blocks of 64: 108 / 64 / 64 / 64, every shard below k = 256 / 300 / 400."""
    _dense_case(300, [108, 64, 64, 64])


def test_dense_empty_shards():
    """100 rows in blocks of 64: 64 / 36 / 0 / 0."""
    _dense_case(100, [64, 36, 0, 0])


@pytest.mark.parametrize("top_k", [300, 999, 5000])
def test_dropin_sharded_top_k_beyond_fused_lists(corpus, monkeypatch, top_k):
    """test_gpu_dropin.test_top_k_beyond_fused_lists on four shards of the golden 1000-chunk corpus
    (blocks of 64: 256 / 256 / 256 / 232 per shard, every one below top_k)."""
    from classmate_hip import multidev
    from classmate_hip.retrieval import BM25Store, GpuVectorStore
    from test_gpu_dropin import check_top_k_beyond_fused_lists
    monkeypatch.setenv("CM_DEVICES", ",".join(map(str, DEVS)))
    monkeypatch.setenv("CM_SHARD_BLOCK", "64")
    vs = GpuVectorStore(persist_dir=None)
    vs.upsert(ids=corpus["ids"], documents=corpus["texts"], metadatas=corpus["metas"], embeddings=corpus["emb"])
    bm = BM25Store(index_dir=None)
    bm.upsert_many(ids=corpus["ids"], texts=corpus["texts"], metadatas=corpus["metas"])
    check_top_k_beyond_fused_lists(vs, bm, corpus, top_k)
    assert isinstance(vs._index, multidev.ShardedDenseIndex) and isinstance(bm._index, multidev.ShardedBM25Index)
    assert all(s.size < 300 for s in vs._index.shards) and all(s.num_docs < 300 for s in bm._index.shards)
