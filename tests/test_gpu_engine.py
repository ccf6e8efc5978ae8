"""GPU parity of the HIP kernels (through the C ABI) against the CPU oracle.

Bars: BM25 scores bit-identical (fp64) with identical ids/order; dense top-k
set equality with cosine distance within 1e-4 (north_star tolerance) and the
exact order wherever neighbouring oracle distances differ by more than 1e-5;
MMR orders and RRF scores identical to the reference-semantics oracle.
"""
import numpy as np
import pytest

from oracle import ref_semantics as orc

pytestmark = pytest.mark.gpu

DIST_TOL = 1e-4


@pytest.fixture(scope="module")
def eng():
    from classmate_hip import engine
    return engine


def _bits(mask: np.ndarray) -> np.ndarray:
    n = mask.shape[0]
    words = np.zeros((n + 31) // 32, np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def _check_dense(dist, rows, emb, q, k, allow=None):
    o_rows, o_dist = orc.dense_topk_exact(emb, q, k, allow)
    for i in range(q.shape[0]):
        n = len(o_rows[i])
        got_r = rows[i][rows[i] >= 0]
        assert len(got_r) == n
        np.testing.assert_allclose(dist[i][:n], o_dist[i], atol=DIST_TOL)
        # set equality except for ties within tolerance at the boundary
        if n == k and n < emb.shape[0]:
            all_d = 1.0 - (emb.astype(np.float64) @ q[i].astype(np.float64)) / np.linalg.norm(emb, axis=1) / \
                np.linalg.norm(q[i])
            kth = o_dist[i][-1]
            unsure = set(np.nonzero(np.abs(all_d - kth) < 1e-5)[0].tolist())
            assert set(got_r.tolist()) ^ set(o_rows[i].tolist()) <= unsure
        else:
            assert set(got_r.tolist()) == set(o_rows[i].tolist())
        # order: strict wherever the oracle distances are separated
        sep = np.diff(o_dist[i]) > 1e-5
        for j in np.nonzero(sep)[0]:
            assert got_r[j] == o_rows[i][j] or abs(dist[i][j] - o_dist[i][j]) < 1e-5


def test_dense_golden_corpus(eng, corpus, golden):
    emb, qv = corpus["emb"], corpus["qvecs"]
    idx = eng.DenseIndex(768)
    idx.upsert(emb, np.arange(emb.shape[0]))
    assert idx.live_count() == emb.shape[0]
    dist, rows = idx.search(qv, 24)
    _check_dense(dist, rows, emb, qv, 24)
    # goldens: same ids & fp32 distances as the reference-run exact store
    ids = corpus["ids"]
    for i, want in enumerate(golden["dense"]["none"]):
        assert [ids[r] for r in rows[i]] == [w[0] for w in want]
        np.testing.assert_allclose(dist[i], [w[1] for w in want], atol=DIST_TOL)


# auto, K1 fp32, K1c coarse (256-query passes), K1s coarse (<= 32-query streams), K1q (int8 resident
# passes), K1q-s (int8 <= 32-query streams); forced kinds a shape cannot take run the automatic rule
PATHS = [0, 1, 3, 4, 5, 6]


@pytest.mark.parametrize("path", PATHS[1:])
def test_dense_filtered_and_deleted(eng, corpus, path):
    emb, qv = corpus["emb"], corpus["qvecs"]
    idx = eng.DenseIndex(768)
    idx.set_path(path)
    idx.upsert(emb, np.arange(emb.shape[0]))
    allow = np.array([m.get("course") == "cs101" for m in corpus["metas"]])
    dist, rows = idx.search(qv, 24, _bits(allow))
    _check_dense(dist, rows, emb, qv, 24, allow)
    dele = np.arange(0, emb.shape[0], 3)
    idx.delete(dele)
    live = np.ones(emb.shape[0], bool)
    live[dele] = False
    dist, rows = idx.search(qv, 10)
    _check_dense(dist, rows, emb, qv, 10, live)
    assert idx.live_count() == int(live.sum())
    # fewer allowed rows than k -> padded with -1
    few = np.zeros(emb.shape[0], bool)
    few[[1, 4, 7]] = True
    dist, rows = idx.search(qv[:2], 10, _bits(few))
    assert (rows[:, 3:] == -1).all()
    assert set(rows[0, :3].tolist()) == {1, 4, 7}


@pytest.mark.parametrize("n,nq,k,dim", [(20000, 1, 10, 768), (20000, 48, 24, 768), (9000, 64, 10, 384),
                                        (5000, 7, 100, 768), (3000, 3, 256, 256), (777, 33, 5, 1000)])
@pytest.mark.parametrize("path", PATHS)
def test_dense_shapes(eng, n, nq, k, dim, path):
    rng = np.random.default_rng(n + nq + k)
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[: nq // 2] = emb[rng.integers(0, n, nq // 2)] + 0.05 * q[: nq // 2]
    idx = eng.DenseIndex(dim)
    idx.set_path(path)
    perm = rng.permutation(n)       # scattered upsert order
    idx.upsert(emb[perm], perm)
    dist, rows = idx.search(q, k)
    _check_dense(dist, rows, emb, q, k)


@pytest.mark.parametrize("n,nq,k,dim", [(30000, 64, 24, 768), (12345, 100, 10, 384), (5000, 300, 32, 100),
                                        (40000, 256, 1, 768), (257, 80, 32, 64), (16448, 300, 10, 384)])
@pytest.mark.parametrize("path", [2, 3, 4, 5, 6])
def test_dense_batched_split_paths(eng, n, nq, k, dim, path):
    """K1c (coarse f16 scan, all queries of a pass resident) and K1s (<= 32 queries, per-wave
    streams), both + certified exact re-rank; path 2 (the retired K1b) means automatic:
    distances within 1e-4, sets/order as the oracle, deletes and filters honoured, multiple
    query passes (nq > 256).  (16448, 300, 10, 384): K1c's ld-384 instance over two passes, on
    the smallest corpus (a multiple of 64 rows) the coarse kinds take."""
    rng = np.random.default_rng(n + nq + k)
    emb = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.1, 10, (n, 1)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[: nq // 2] = emb[rng.integers(0, n, nq // 2)] + 0.05 * q[: nq // 2]
    idx = eng.DenseIndex(dim)
    idx.set_path(path)
    idx.upsert(emb, np.arange(n))
    if (n, dim, path) == (16448, 384, 3):
        assert idx.search_kind(nq, k) == 3   # not the fp32 scan
    dist, rows = idx.search(q, k)
    _check_dense(dist, rows, emb, q, k)
    allow = rng.random(n) < 0.3
    dele = np.nonzero(rng.random(n) < 0.1)[0]
    idx.delete(dele)
    live = allow.copy()
    live[dele] = False
    dist, rows = idx.search(q, k, _bits(allow))
    _check_dense(dist, rows, emb, q, k, live)


@pytest.mark.parametrize("path", [3, 4, 5, 6])
def test_dense_coarse_certificate(eng, path):
    """K1c / K1s / K1q / K1q-s: on well-separated data every query is certified (no exact re-run);
    on a cluster of near-duplicates wider than the coarse lists the certificate fails and the
    exact fp32 K1 pass takes over for those queries (K1q / K1q-s: the wide re-rank, from the
    complete candidate buffers) -- results stay within tolerance."""
    rng = np.random.default_rng(77)
    n, dim = 30000, 768
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    nq = 64 if path in (3, 5) else 16
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = eng.DenseIndex(dim)
    idx.set_path(path)
    idx.upsert(emb, np.arange(n))
    assert idx.search_kind(nq, 24) == path
    dist, rows = idx.search(q, 24)
    _check_dense(dist, rows, emb, q, 24)
    assert idx.last_fallbacks() == 0
    # near-duplicates of one vector (cosine gaps ~1e-8, far inside the 2E band): 600 overflow
    # K1c's 64-slot (range, query) buffers; K1s's 1024 small groups hold them, so it gets a
    # cluster wider than the re-rank band cap (1024 rows) instead; the int8 kinds get one wider
    # than their 4096-row band
    nd = {3: 600, 4: 1500, 5: 9000, 6: 9000}[path]
    base = rng.standard_normal(dim).astype(np.float32)
    dup = base + 1e-4 * rng.standard_normal((nd, dim)).astype(np.float32)
    emb2 = np.concatenate([emb, dup])
    idx.upsert(dup, np.arange(n, n + nd))
    q2 = np.concatenate([q[:8], base + 0.01 * rng.standard_normal((8, dim)).astype(np.float32)])
    dist, rows = idx.search(q2, 24)
    _check_dense(dist, rows, emb2, q2, 24)
    # (the duplicates are contiguous rows, so they overflow the int8 kinds' 128-slot (group, query)
    # buffers too: an incomplete candidate set, which the wide re-rank cannot finish -> the exact pass)
    assert idx.last_fallbacks() + max(idx.last_wide_reranks(), 0) >= 8
    assert (rows[8:] >= n).all()


def test_dense_device_path_and_gather(eng):
    import torch
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((4096, 768)).astype(np.float32)
    q = rng.standard_normal((16, 768)).astype(np.float32)
    idx = eng.DenseIndex(768)
    idx.upsert_dev(torch.from_numpy(emb).cuda(), 0)
    d_t, r_t = idx.search_dev(torch.from_numpy(q).cuda(), 24)
    torch.cuda.synchronize()
    d_h, r_h = idx.search(q, 24)
    assert np.array_equal(r_t.cpu().numpy(), r_h)
    _check_dense(d_t.cpu().numpy(), r_t.cpu().numpy(), emb, q, 24)  # the device entry vs the fp64 oracle
    g = idx.gather_dev(r_t.reshape(-1)).cpu().numpy().reshape(16, 24, 768)
    assert np.array_equal(g, emb[r_h])


def _term_ids(token_lists, vocab=None):
    vocab = {} if vocab is None else vocab
    out = []
    for toks in token_lists:
        out.append(np.array([vocab.setdefault(t, len(vocab)) for t in toks], np.int32))
    return out, vocab


def _build_bm25(eng, tok_lists, path=0):
    ids, vocab = _term_ids(tok_lists)
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in ids])
    flat = np.concatenate(ids) if off[-1] else np.zeros(0, np.int32)
    b = eng.BM25Index()
    b.build(flat, off, len(vocab))
    b.set_path(path)
    return b, vocab


# BM25 search strategies: 1 = full K2 scan, 2 = tail pass + bounded re-score (same bits)
BM25_PATHS = [1, 2]


FILTERS = [None, {"course": "cs101", "unit": None, "author": None, "semester": None},
           {"course": "math201"}, {"language": "en", "doc_type": "pptx"}]


@pytest.mark.parametrize("where", FILTERS)
@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_bit_exact(eng, corpus, where, path):
    toks = [orc.tokenize(t, "en") for t in corpus["texts"]]
    b, vocab = _build_bm25(eng, toks, path)
    ora = orc.BM25Oracle()
    ora.upsert_many(corpus["ids"], corpus["texts"], corpus["metas"])
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in corpus["qtexts"]]
    allow = None
    if where:
        allow = _bits(np.array([orc.bm25_matches_filter(m, where) for m in corpus["metas"]]))
    scores, rows, nvalid = b.search(qs, 10, allow)
    for i, q in enumerate(corpus["qtexts"]):
        want = ora.search(q, where, top_k=10)
        got = [[corpus["ids"][r], s] for r, s in zip(rows[i][:nvalid[i]], scores[i][:nvalid[i]])]
        assert got == [[w["id"], w["score"]] for w in want]


@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_padding_negative_eps_and_dupes(eng, path):
    # many docs share 'common' (negative idf), few match the rest; duplicates in the query
    rng = np.random.default_rng(3)
    words = [f"w{chr(97 + i)}{chr(97 + j)}" for i in range(20) for j in range(20)]
    words = ["".join(c for c in w if c.isalpha()) for w in words]
    texts = []
    for d in range(3000):
        n = int(rng.integers(0, 30))
        ws = [words[int(x)] for x in rng.integers(0, len(words), n)]
        if rng.random() < 0.8:
            ws.append("common")
        texts.append(" ".join(ws))
    toks = [orc.tokenize(t, "en") for t in texts]
    b, vocab = _build_bm25(eng, toks, path)
    ora = orc.BM25Oracle()
    ids = [f"d{i}" for i in range(len(texts))]
    ora.upsert_many(ids, texts, [{"language": "en"}] * len(texts))
    queries = ["common", "common common wbc", "wbc wbc wbc", "zzzz", "the of", "wab wcd common wab"]
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in queries]
    for k in (1, 10, 37, 256):
        scores, rows, nvalid = b.search(qs, k)
        for i, q in enumerate(queries):
            want = ora.search(q, None, top_k=k)
            got = [[ids[r], s] for r, s in zip(rows[i][:nvalid[i]], scores[i][:nvalid[i]])]
            assert got == [[w["id"], w["score"]] for w in want], (q, k)
    # filtered subset small enough that 'common' goes negative inside it (filtered eps path)
    mask = np.zeros(len(texts), bool)
    mask[:40] = True
    allow = _bits(mask)
    scores, rows, nvalid = b.search(qs, 12, allow)
    sub = orc.BM25Oracle()
    sub.upsert_many(ids[:40], texts[:40], [{"language": "en"}] * 40)
    for i, q in enumerate(queries):
        want = sub.search(q, None, top_k=12)
        got = [[ids[r], s] for r, s in zip(rows[i][:nvalid[i]], scores[i][:nvalid[i]])]
        assert got == [[w["id"], w["score"]] for w in want], q


def test_bm25_zero_division(eng):
    b = eng.BM25Index()
    with pytest.raises(ZeroDivisionError):
        b.build(np.zeros(0, np.int32), np.zeros(3, np.int64), 5)


def test_bm25_device_build_matches_host_build(eng, corpus):
    import torch
    toks = [orc.tokenize(t, "en") for t in corpus["texts"]]
    ids, vocab = _term_ids(toks)
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in ids])
    flat = np.concatenate(ids)
    bh = eng.BM25Index()
    bh.build(flat, off, len(vocab))
    bd = eng.BM25Index()
    bd.build_dev(torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), len(vocab))
    assert bh.stats() == bd.stats()
    assert bh.num_postings == bd.num_postings
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in corpus["qtexts"]]
    s1, r1, _ = bh.search(qs, 10)
    s2, r2, _ = bd.search(qs, 10)
    assert np.array_equal(r1, r2) and np.array_equal(s1, s2)
    # unfiltered device path == host path
    qoff = np.zeros(len(qs) + 1, np.int32)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    qflat = np.concatenate([np.asarray(q, np.int32) for q in qs])
    s3, r3 = bd.search_dev(torch.from_numpy(qflat).cuda(), torch.from_numpy(qoff).cuda(), 10)
    torch.cuda.synchronize()
    assert np.array_equal(r3.cpu().numpy(), r1) and np.array_equal(s3.cpu().numpy(), s1)
    # the gated form (the bench step's schedule): preparation on a side stream at once, scoring behind
    # an event recorded after a producer on the main stream -- same lists
    qt_d, qo_d = torch.from_numpy(qflat).cuda(), torch.from_numpy(qoff).cuda()
    side, gate = torch.cuda.Stream(), torch.cuda.Event()
    x = torch.randn(2048, 2048, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    y = x @ x                                            # the producer (the encode in the step)
    gate.record()
    with torch.cuda.stream(side):
        s4, r4 = bd.search_dev(qt_d, qo_d, 10, gate=gate)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(r4.cpu().numpy(), r1) and np.array_equal(s4.cpu().numpy(), s1)
    del y


def test_mmr_matches_reference_goldens(eng, corpus, golden):
    idx = {i: n for n, i in enumerate(corpus["ids"])}
    cands = np.stack([corpus["emb"][[idx[i] for i in c["pool"]]] for c in golden["mmr"]])
    order = eng.mmr_order_batch(corpus["qvecs"], cands, 10, 0.5)
    for i, c in enumerate(golden["mmr"]):
        assert order[i].tolist() == c["order"]
    # ragged pools and k > pool
    nv = np.array([24, 5, 1, 0] * 4, np.int32)
    order = eng.mmr_order_batch(corpus["qvecs"], cands, 12, 0.3, n_valid=nv)
    for i in range(16):
        n = int(nv[i])
        want = orc.mmr_order(corpus["qvecs"][i], cands[i][:n], list(range(n)), 12, 0.3)
        assert order[i][: len(want)].tolist() == want
        assert (order[i][len(want):] == -1).all()


def test_rrf(eng, golden):
    for case in golden["rrf"]:
        names = {}
        lists = [[names.setdefault(x, len(names)) for x in l] for l in case["lists"]]
        keys, scores = eng.rrf_fuse_keys(lists, case["weights"], case["rrf_k"])
        inv = {v: k for k, v in names.items()}
        got = {inv[int(k)]: float(s) for k, s in zip(keys, scores)}
        assert got == case["out"] and list(got) == list(case["out"])


def test_meanpool_l2norm(eng):
    import torch
    torch.manual_seed(0)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        h = torch.randn(5, 37, 768, device="cuda").to(dt)
        m = (torch.rand(5, 37, device="cuda") > 0.3).to(torch.int64)
        m[3] = 0                                    # empty mask -> zero vector
        out = eng.meanpool_l2norm(h, m)
        hf, mf = h.float(), m.float().unsqueeze(-1)
        ref = (hf * mf).sum(1) / mf.sum(1).clamp(min=1e-9)
        ref = torch.nn.functional.normalize(ref, p=2, dim=1)
        torch.testing.assert_close(out, ref, atol=2e-6, rtol=1e-5)
        raw = eng.meanpool_l2norm(h, m.to(torch.int32), normalize=False)
        torch.testing.assert_close(raw, (hf * mf).sum(1) / mf.sum(1).clamp(min=1e-9), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("policy", [(1.0 / 64, 8 << 30), (0.0, 8 << 30), (1.0, 0), (0.0, 0)])
@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_head_tile_policies_bit_exact(eng, corpus, policy, path):
    """Dense head-term tiles (any split of head/tail terms) give the same bits as the oracle."""
    toks = [orc.tokenize(t, "en") for t in corpus["texts"]]
    b, vocab = _build_bm25(eng, toks, path)
    b.set_head_policy(*policy)
    if policy[1] == 0:
        assert b.num_head_terms == 0
    elif policy[0] == 0.0:
        assert b.num_head_terms == len(vocab)
    ora = orc.BM25Oracle()
    ora.upsert_many(corpus["ids"], corpus["texts"], corpus["metas"])
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in corpus["qtexts"]]
    for where in (None, {"course": "math201"}):
        allow = None if where is None else _bits(np.array([orc.bm25_matches_filter(m, where)
                                                           for m in corpus["metas"]]))
        scores, rows, nvalid = b.search(qs, 10, allow)
        for i, q in enumerate(corpus["qtexts"]):
            want = ora.search(q, where, top_k=10)
            got = [[corpus["ids"][r], s] for r, s in zip(rows[i][:nvalid[i]], scores[i][:nvalid[i]])]
            assert got == [[w["id"], w["score"]] for w in want]


@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_saturated_tf_slow_path(eng, path):
    texts = ["spam " * 300 + "eggs", "spam eggs eggs", "eggs", "spam " * 256, "ham"] * 3
    ids = [f"d{i}" for i in range(len(texts))]
    toks = [orc.tokenize(t, "en") for t in texts]
    b, vocab = _build_bm25(eng, toks, path)
    b.set_head_policy(0.0, 1 << 30)               # every term in a tile -> tf 300 saturates the byte
    ora = orc.BM25Oracle()
    ora.upsert_many(ids, texts, [{"language": "en"}] * len(texts))
    for q in ["spam", "eggs spam", "ham spam spam"]:
        scores, rows, nvalid = b.search([[vocab.get(t, -1) for t in orc.tokenize(q, "en")]], 8)
        want = ora.search(q, None, top_k=8)
        assert [[ids[r], s] for r, s in zip(rows[0][:nvalid[0]], scores[0][:nvalid[0]])] == \
            [[w["id"], w["score"]] for w in want]


@pytest.mark.parametrize("policy", [(1.0 / 64, 8 << 30), (1.0, 0)])
@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_long_queries_and_tail_overflow(eng, corpus, policy, path):
    """> 96 query terms per workgroup and > 768 tail postings per range exercise
    K2's global-memory fallbacks; results stay bit-identical."""
    texts = corpus["texts"] * 3                      # 3000 docs -> ranges of 1024 docs
    ids = [f"r{i}" for i in range(len(texts))]
    toks = [orc.tokenize(t, "en") for t in texts]
    b, vocab = _build_bm25(eng, toks, path)
    b.set_head_policy(*policy)
    rng = np.random.default_rng(11)
    words = list(vocab)
    queries = [" ".join(words[int(x)] for x in rng.integers(0, 40, 45)) for _ in range(6)]   # frequent terms
    queries += [" ".join(words[int(x)] for x in rng.integers(0, len(words), 30)) for _ in range(3)]
    ora = orc.BM25Oracle()
    ora.upsert_many(ids, texts, [{"language": "en"}] * len(texts))
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in queries]
    scores, rows, nvalid = b.search(qs, 10)
    for i, q in enumerate(queries):
        want = ora.search(q, None, top_k=10)
        assert [[ids[r], s] for r, s in zip(rows[i][:nvalid[i]], scores[i][:nvalid[i]])] == \
            [[w["id"], w["score"]] for w in want]


@pytest.mark.parametrize("policy", [(1.0 / 64, 8 << 30), (1.0, 0)])
@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_many_ranges_vs_c_oracle(eng, policy, path):
    """~150 ranges of 1024 docs: K2's per-query global threshold pruning and the K3
    merge must keep the exact oracle top-k (ties by row, zero-score padding for a
    rare term, k up to the 256 maximum)."""
    from oracle import corc
    rng = np.random.default_rng(5)
    nd, vocab = 150_000, 4000
    lens = np.maximum(rng.poisson(30, nd), 1)
    off = np.zeros(nd + 1, np.int64)
    off[1:] = np.cumsum(lens)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.1
    toks = rng.choice(vocab, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    b = eng.BM25Index()
    b.build(toks, off, vocab)
    b.set_head_policy(*policy)
    b.set_path(path)
    csr = corc.build_csr(toks, off, vocab)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], nd)
    avgdl = float(lens.sum()) / nd
    rare = int(np.nonzero(csr["df"] == csr["df"][csr["df"] > 0].min())[0][0])
    queries = [rng.integers(0, vocab, 6).tolist() for _ in range(20)]
    queries += [[0, 1, 2], [3, 3, 7], [rare], [rare, vocab - 1], [int(x) for x in rng.integers(0, 50, 40)]]
    for k in (1, 8, 9, 10, 12, 13, 256):     # every merge form: 256-thread K = 8 / 10 / 12, 1024-thread
        scores, rows, nvalid = b.search(queries, k)
        o_sc, o_rw = corc.bm25_topk(csr, idf, avgdl, queries, k)
        for i in range(len(queries)):
            assert nvalid[i] == k
            assert rows[i][:k].tolist() == o_rw[i].tolist(), (k, i)
            assert scores[i][:k].tolist() == o_sc[i].tolist(), (k, i)


@pytest.mark.gpu
@pytest.mark.parametrize("df_frac", [0.02, 0.035, 0.06])
def test_bm25_tail_pass_super_range_halving(eng, df_frac):
    """K2a gathers 4 consecutive ranges per iteration and halves the span when their candidate
    postings overflow its LDS lists (320 per query group): query groups whose only candidate
    generators are designated head terms of ~2-6 % df land on 4-, 2- and 1-range spans (and on
    the K2 re-score when one range overflows).  Bit-identical to the full scan and the C oracle."""
    from oracle import corc
    rng = np.random.default_rng(33)
    nd, vocab = 60_000, 3000
    lens = np.maximum(rng.poisson(20, nd), 1)
    off = np.zeros(nd + 1, np.int64)
    off[1:] = np.cumsum(lens)
    toks = rng.integers(10, vocab, int(off[-1])).astype(np.int32)       # rare background terms
    for t in range(4):                                                    # terms 0..3: ~df_frac each
        docs = np.nonzero(rng.random(nd) < df_frac * (1 + 0.3 * t))[0]
        toks[off[docs] + rng.integers(0, lens[docs])] = t
    b = eng.BM25Index()
    b.build(toks, off, vocab)
    b.set_head_policy(0.01, 8 << 30)                                      # terms 0..3 get head tiles
    queries = [[0], [1], [0, 1], [2], [3, 0], [1, 2, 3], [0, 1, 2, 3], [2, 3],
               [int(toks[off[5]]), 0], [1, int(toks[off[9]])], [3], [0, 0, 2]]
    k = 10
    csr = corc.build_csr(toks, off, vocab)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], nd)
    o_sc, o_rw = corc.bm25_topk(csr, idf, float(lens.sum()) / nd, queries, k)
    b.set_path(1)
    s1, r1, _ = b.search(queries, k)
    b.set_path(2)
    s2, r2, _ = b.search(queries, k)
    assert np.array_equal(r1, r2) and np.array_equal(s1, s2)
    for i in range(len(queries)):
        assert r2[i][:k].tolist() == o_rw[i].tolist(), i
        assert s2[i][:k].tolist() == o_sc[i].tolist(), i


@pytest.mark.gpu
def test_bm25_pruned_skips_ranges_and_matches_full_scan(eng):
    """Bench-shaped workload (Zipf corpus, 8-term queries drawn from documents, head tiles on):
    the pruned search re-scores only a fraction of the (query, range) pairs and returns the
    same bits as the full K2 scan and the C oracle, with and without an allow filter."""
    from oracle import corc
    rng = np.random.default_rng(21)
    nd, vocab = 200_000, 50_000
    lens = np.maximum(rng.poisson(60, nd), 1)
    off = np.zeros(nd + 1, np.int64)
    off[1:] = np.cumsum(lens)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.07
    toks = rng.choice(vocab, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    b = eng.BM25Index()
    b.build(toks, off, vocab)
    assert b.num_head_terms > 0
    tgt = rng.integers(0, nd, 48)
    queries = [[int(toks[off[d] + rng.integers(0, lens[d])]) for _ in range(8)] for d in tgt]
    queries += [[0, 1, 2, 3], [5], [vocab - 1, 7]]            # head-only and rare-term queries
    k = 10
    csr = corc.build_csr(toks, off, vocab)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], nd)
    o_sc, o_rw = corc.bm25_topk(csr, idf, float(lens.sum()) / nd, queries, k)
    b.set_path(1)
    s1, r1, _ = b.search(queries, k)
    assert b.last_rescored() == -1
    b.set_path(2)
    s2, r2, _ = b.search(queries, k)
    n_pairs = ((len(queries) + 3) // 4) * 4 * ((nd + 1023) // 1024)
    assert 0 <= b.last_rescored() < n_pairs * 0.9, (b.last_rescored(), n_pairs)
    assert np.array_equal(r1, r2) and np.array_equal(s1, s2)
    for i in range(len(queries)):
        assert r2[i].tolist() == o_rw[i].tolist(), i
        assert s2[i].tolist() == o_sc[i].tolist(), i
    # filtered: every third document allowed (statistics recomputed over the subset)
    mask = np.zeros(nd, bool)
    mask[::3] = True
    allow = _bits(mask)
    b.set_path(1)
    f1 = b.search(queries, k, allow)
    b.set_path(2)
    f2 = b.search(queries, k, allow)
    assert np.array_equal(f1[1], f2[1]) and np.array_equal(f1[0], f2[0])
    assert all(int(r) % 3 == 0 for r in f2[1].ravel() if r >= 0)


@pytest.mark.gpu
def test_bm25_pruned_ties_at_threshold(eng):
    """The pruned search's fp32 pre-bounds (planner, K2a, K2b: a candidate is dropped only when an
    inflated fp32 upper bound of its score is below the query's threshold T) must keep every
    document whose exact score equals T.  300 identical copies of a tail + head template and 300
    of a head-only template, spread over ~120 ranges, put hundreds of exact ties at the k-th
    score (broken by row).  Both paths equal the C oracle bit for bit for k = 1, 10, 64."""
    from oracle import corc
    rng = np.random.default_rng(44)
    nd, vocab = 120_000, 6000
    lens = np.maximum(rng.poisson(25, nd), 1)
    docs_a = rng.choice(nd, 300, replace=False)
    docs_b = rng.choice(np.setdiff1d(np.arange(nd), docs_a), 300, replace=False)
    lens[docs_a] = 8
    lens[docs_b] = 8
    off = np.zeros(nd + 1, np.int64)
    off[1:] = np.cumsum(lens)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.05
    toks = rng.choice(vocab, size=int(off[-1]), p=p / p.sum()).astype(np.int32)
    tmpl_a = np.array([0, 1, 1, 2, 5000, 5001, 3, 0], np.int32)  # heads 0..3 + two rare terms
    tmpl_b = np.array([0, 1, 2, 2, 3, 0, 1, 4], np.int32)        # head terms only
    for d in docs_a:
        toks[off[d]:off[d] + 8] = tmpl_a
    for d in docs_b:
        toks[off[d]:off[d] + 8] = tmpl_b
    b = eng.BM25Index()
    b.build(toks, off, vocab)
    b.set_head_policy(1.0 / 128, 8 << 30)
    assert b.num_head_terms >= 5
    queries = [[0, 1, 2, 3, 5000, 5001], [0, 1, 2, 3, 4], [5000, 0, 1], [2, 2, 0, 4, 1],
               [5001, 3], [0, 1, 2, 3, 4, 5000], [4, 0]]
    csr = corc.build_csr(toks, off, vocab)
    idf, _ = corc.bm25_idf(csr["df"], csr["first_key"], nd)
    avgdl = float(lens.sum()) / nd
    for k in (1, 10, 64):
        o_sc, o_rw = corc.bm25_topk(csr, idf, avgdl, queries, k)
        b.set_path(1)
        s1, r1, _ = b.search(queries, k)
        b.set_path(2)
        s2, r2, _ = b.search(queries, k)
        assert np.array_equal(r1, r2) and np.array_equal(s1, s2), k
        for i in range(len(queries)):
            assert r2[i][:k].tolist() == o_rw[i].tolist(), (k, i)
            assert s2[i][:k].tolist() == o_sc[i].tolist(), (k, i)
    # the tail + head template query really is tie-bound: its top 64 share one score
    o_sc, _ = corc.bm25_topk(csr, idf, avgdl, queries[:1], 64)
    assert len(set(o_sc[0].tolist())) == 1


@pytest.mark.parametrize("D", [768, 1024, 20, 2048])
def test_add_layernorm_matches_torch(eng, D):
    """cm_add_layernorm == F.layer_norm(x + r) (torch fp32 reference of the same op)."""
    import torch
    import torch.nn.functional as F
    torch.manual_seed(D)
    rows = 6144 + 3
    for dt, tol in ((torch.float32, 2e-5), (torch.bfloat16, 1.6e-2)):
        x = torch.randn(rows, D, device="cuda").to(dt)
        r = (3 * torch.randn(rows, D, device="cuda") + 1).to(dt)
        w = torch.randn(D, device="cuda").to(dt)
        b = torch.randn(D, device="cuda").to(dt)
        ref = F.layer_norm((x + r).float(), (D,), w.float(), b.float(), 1e-5)   # sum rounded to dt as torch does
        out = eng.add_layernorm(x, r, w, b, 1e-5)
        assert out.dtype == dt and out.shape == x.shape
        torch.testing.assert_close(out.float(), ref, atol=tol, rtol=tol)
        # broadcast residual (positional table tiled over the batch) and no residual
        pt = torch.randn(24, D, device="cuda").to(dt)
        xb = x[: 24 * 256]
        ref = F.layer_norm((xb.view(256, 24, D) + pt).float(), (D,), w.float(), b.float(), 1e-5).view(-1, D)
        torch.testing.assert_close(eng.add_layernorm(xb, pt, w, b, 1e-5).float(), ref, atol=tol, rtol=tol)
        ref = F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5)
        torch.testing.assert_close(eng.add_layernorm(x, None, w, b, 1e-5).float(), ref, atol=tol, rtol=tol)
    with pytest.raises(ValueError):
        eng.add_layernorm(x, r[:5], w, b, 1e-5)


def test_e5_lean_forward_fp32_matches_hf():
    """The graph-captured lean E5 forward (fused QKV GEMM, flash SDPA, HIP add+LayerNorm) equals the
    Hugging Face XLM-R module in fp32."""
    import torch
    from classmate_hip.embeddings import E5MultilingualEmbedder
    emb = E5MultilingualEmbedder.random_init(seed=3, device="cuda", num_layers=2, dtype="float32")
    B, S = 8, 24
    g = torch.Generator(device="cuda").manual_seed(9)
    ids = torch.randint(5, 250002, (B, S), device="cuda", generator=g)
    mask = torch.ones_like(ids)
    u_ids, u_mask, u_out, graph = emb.capture_graph(B, S, unpadded=True)
    u_ids.copy_(ids)
    graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(u_out, emb._encode_hf(ids, mask), atol=2e-5, rtol=0)
    torch.testing.assert_close(emb.encode_token_ids(ids, mask), emb._encode_hf(ids, mask), atol=2e-5, rtol=0)
    mask[2, 11:] = 0                                   # ragged rows: lean padded path == HF
    mask[5, 3:] = 0
    ids[2, 11:] = 1
    ids[5, 3:] = 1
    torch.testing.assert_close(emb.encode_token_ids(ids, mask), emb._encode_hf(ids, mask), atol=2e-5, rtol=0)


def test_e5_small_batch_graph_matches_hf(monkeypatch):
    """Single queries / small batches (B <= 8, S <= 32) replay a hipGraph of the K10 lean forward
    with the tokens padded into a 16 / 32 bucket and masked: equal to the Hugging Face fp32 module
    and to the eager lean forward within 2e-5, ragged rows included; one graph per (B, bucket)."""
    import torch
    from classmate_hip.embeddings import E5MultilingualEmbedder
    emb = E5MultilingualEmbedder.random_init(seed=4, device="cuda", num_layers=2, dtype="float32")
    g = torch.Generator(device="cuda").manual_seed(11)
    for B, S, cut in ((1, 7, None), (1, 16, None), (3, 20, 9), (8, 32, 5), (2, 17, 1)):
        ids = torch.randint(5, 250002, (B, S), device="cuda", generator=g)
        ids[:, 0] = 0
        mask = torch.ones_like(ids)
        if cut is not None:
            mask[B - 1, cut:] = 0
            ids[B - 1, cut:] = 1
        got = emb.encode_token_ids(ids, mask)
        got2 = emb.encode_token_ids(ids, mask)           # replay of the cached graph
        torch.testing.assert_close(got, emb._encode_hf(ids, mask), atol=2e-5, rtol=0)
        assert torch.equal(got, got2)
        monkeypatch.setenv("CM_E5_SMALL_GRAPH", "0")
        torch.testing.assert_close(got, emb.encode_token_ids(ids, mask), atol=2e-5, rtol=0)
        monkeypatch.delenv("CM_E5_SMALL_GRAPH")
    assert sorted((b, s) for b, s, _ in emb._small_graphs) == [(1, 16), (2, 32), (3, 32), (8, 32)]


@pytest.mark.parametrize("S", [1, 7, 16, 24, 32, 33, 64])
def test_short_attention_matches_torch(eng, S):
    """cm_short_attention == per-head softmax(q k^T / 8) v on the (B, S, 3, H, 64) QKV layout
    (torch fp32 reference)."""
    import torch
    torch.manual_seed(S)
    B, H = 37, 12
    for dt, tol in ((torch.float32, 2e-5), (torch.bfloat16, 1e-2)):
        qkv = (2 * torch.randn(B, S, 3 * H * 64, device="cuda")).to(dt)
        q, k, v = qkv.float().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
        ref = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
        ref = ref.transpose(1, 2).reshape(B, S, H * 64)
        out = eng.short_attention(qkv, H, 1 / 8.0)
        assert out.dtype == dt and out.shape == (B, S, H * 64)
        torch.testing.assert_close(out.float(), ref, atol=tol, rtol=tol)
    with pytest.raises(ValueError):
        eng.short_attention(torch.zeros(2, 65, 3 * H * 64, device="cuda"), H, 0.125)


@pytest.mark.gpu
def test_rrf_pool_prep_matches_torch_glue(eng):
    """cm_rrf_pool_prep_dev == the torch ops it replaces in the batched step: the MMR-ordered pool
    keys / distances (gather by order, -1 padding) and the valid counts of both lists."""
    import torch
    g = torch.Generator().manual_seed(3)
    nq, pool, kv, kb = 37, 24, 10, 10
    keys = torch.randint(0, 1 << 40, (nq, pool), generator=g, dtype=torch.int64)
    dist = torch.rand((nq, pool), generator=g, dtype=torch.float32)
    order = torch.stack([torch.randperm(pool, generator=g)[:kv] for _ in range(nq)]).to(torch.int32)
    nsel = torch.randint(0, kv + 1, (nq,), generator=g)
    order[torch.arange(kv).unsqueeze(0) >= nsel.unsqueeze(1)] = -1
    bkeys = torch.randint(0, 1 << 40, (nq, kb), generator=g, dtype=torch.int64)
    nb = torch.randint(0, kb + 1, (nq,), generator=g)
    bkeys[torch.arange(kb).unsqueeze(0) >= nb.unsqueeze(1)] = -1
    dv = [t.cuda() for t in (keys, dist, order, bkeys)]
    vk, vd, vn, bn = eng.rrf_pool_prep_dev(*dv)
    o = order.long().clamp(min=0)
    want_k = torch.where(order >= 0, torch.gather(keys, 1, o), torch.full_like(o, -1))
    want_d = torch.where(order >= 0, torch.gather(dist, 1, o), torch.zeros_like(dist[:, :kv]))
    assert torch.equal(vk.cpu(), want_k) and torch.equal(vd.cpu(), want_d)
    assert torch.equal(vn.cpu(), (order >= 0).sum(1, dtype=torch.int32))
    assert torch.equal(bn.cpu(), (bkeys >= 0).sum(1, dtype=torch.int32))


@pytest.mark.parametrize("pool", [24, 32, 33, 48])
def test_mmr_small_and_large_pools_match_oracle(eng, pool):
    """Pools <= 32 run the LDS-staged MMR kernel, larger ones the streaming kernel: both give the
    reference's greedy order (oracle: rag/retrieval/fusion.py:39-61 restated)."""
    rng = np.random.default_rng(pool)
    nq, dim = 40, 768
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    base = q[:, None, :] + 0.9 * rng.standard_normal((nq, pool, dim)).astype(np.float32) / np.sqrt(dim)
    cands = (base / np.linalg.norm(base, axis=2, keepdims=True)).astype(np.float32)
    nv = rng.integers(0, pool + 1, nq).astype(np.int32)
    nv[:4] = pool
    for k, lam in ((10, 0.5), (pool + 3, 0.3)):
        order = eng.mmr_order_batch(q, cands, k, lam, n_valid=nv)
        for i in range(nq):
            n = int(nv[i])
            want = orc.mmr_order(q[i], cands[i][:n], list(range(n)), k, lam)
            assert order[i][: len(want)].tolist() == want, (i, n, k)
            assert (order[i][len(want):] == -1).all()
        if pool == 24:   # fp64 LDS rows (pool 24) and fp32 LDS rows (the same items in a 32-slot pool)
            wide = np.zeros((nq, 32, dim), np.float32)
            wide[:, :pool] = cands
            assert np.array_equal(eng.mmr_order_batch(q, wide, k, lam, n_valid=nv), order)


def _merge_ref(vk, vd, bk, bs, w_vec, w_bm25, rrf_k, top_k):
    """HybridRetriever.retrieve's merge (rag/retrieval/fusion.py:130-167) on one query's lists."""
    fused = orc.rrf_fuse(rank_lists=[list(vk), list(bk)], weights=[w_vec, w_bm25], rrf_k=rrf_k)
    by_id = {}
    for i, d in zip(vk, vd):
        by_id.setdefault(i, [i, None, None])[1] = float(d)
    for i, b in zip(bk, bs):
        by_id.setdefault(i, [i, None, None])[2] = float(b)
    items = sorted(by_id.values(), key=lambda it: (fused[it[0]], -(it[1] if it[1] is not None else 0.0)),
                   reverse=True)[:top_k]
    return [(it[0], fused[it[0]], it[1], it[2]) for it in items]


def test_rrf_merge_wave_lds_and_global_paths_agree(eng):
    """kv + kb <= 64 runs the wave-per-query RRF merge, longer lists the lane-per-query kernel on
    global scratch: the same valid items give the same fused lists (bit-identical) on both paths,
    equal to the reference's merge (dict order, stable sort on (fused, -distance)) -- including
    equal distances, BM25 ids that are also vector ids, and empty lists."""
    rng = np.random.default_rng(7)
    nq = 300
    vk = np.stack([rng.choice(90, 40, replace=False) for _ in range(nq)]).astype(np.int64)
    bk = np.stack([rng.choice(90, 40, replace=False) for _ in range(nq)]).astype(np.int64)
    vd = rng.random((nq, 40)).astype(np.float32)
    vd[:, 3] = vd[:, 2]                                     # equal distances: tie order
    bs = rng.standard_normal((nq, 40))
    vn = rng.integers(0, 17, nq).astype(np.int32)
    bn = rng.integers(0, 17, nq).astype(np.int32)
    vn[:3], bn[:3] = 0, (0, 5, 0)
    bn[3] = 0
    bk[5, :8] = vk[5, 7::-1]                                # BM25 = reversed vector ids: every fused value ties pairwise
    vn[5] = bn[5] = 8
    kw = dict(w_vec=1.0, w_bm25=0.7, rrf_k=60, top_k=12)
    runs = [eng.rrf_merge(vk[:, :c].copy(), vd[:, :c].copy(), vn, bk[:, :c].copy(), bs[:, :c].copy(), bn, **kw)
            for c in (16, 32, 40)]                          # wave, wave (kv + kb = 64), global
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    ok, of, ov, ob, ofl, on = runs[0]
    assert int(np.asarray(on).max()) > 0
    for q in range(nq):
        want = _merge_ref(vk[q, :vn[q]].tolist(), vd[q, :vn[q]], bk[q, :bn[q]].tolist(), bs[q, :bn[q]],
                          kw["w_vec"], kw["w_bm25"], kw["rrf_k"], kw["top_k"])
        assert on[q] == len(want), q
        for r, (i, f, d, b) in enumerate(want):
            assert ok[q, r] == i and of[q, r] == f, (q, r)
            assert ofl[q, r] == (1 if d is not None else 0) | (2 if b is not None else 0)
            assert ov[q, r] == (np.float32(d) if d is not None else 0.0)
            assert ob[q, r] == (b if b is not None else 0.0)
        assert (ok[q, len(want):] == -1).all()


def _dev_queries(qs):
    import torch
    off = np.zeros(len(qs) + 1, np.int32)
    off[1:] = np.cumsum([len(q) for q in qs])
    flat = np.concatenate([np.asarray(q, np.int32) for q in qs]) if off[-1] else np.zeros(1, np.int32)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()


@pytest.mark.parametrize("path", BM25_PATHS)
def test_bm25_filtered_device_entry_matches_host(eng, path):
    """cm_bm25_search_filtered_dev (candidate statistics, idf from the glibc log table, epsilon
    recovery) == the host-array filtered search == the oracle over the filtered subset, bit for
    bit; includes filters whose candidates make a query term's idf negative (epsilon floor)."""
    import torch
    rng = np.random.default_rng(3)
    words = [f"w{chr(97 + i)}{chr(97 + j)}" for i in range(20) for j in range(20)]
    texts = []
    for d in range(3000):
        n = int(rng.integers(0, 30))
        ws = [words[int(x)] for x in rng.integers(0, len(words), n)]
        if rng.random() < 0.8:
            ws.append("common")
        texts.append(" ".join(ws))
    toks = [orc.tokenize(t, "en") for t in texts]
    b, vocab = _build_bm25(eng, toks, path)
    b.prepare_filtered()
    ids = [f"d{i}" for i in range(len(texts))]
    queries = ["common", "common common wbc", "wbc wbc wbc", "zzzz", "wab wcd common wab", "wab"]
    qs = [[vocab.get(t, -1) for t in orc.tokenize(q, "en")] for q in queries]
    qt, qo = _dev_queries(qs)
    masks = {"first40": np.arange(len(texts)) < 40, "every3": np.arange(len(texts)) % 3 == 0,
             "all": np.ones(len(texts), bool), "none": np.zeros(len(texts), bool)}
    for name, mask in masks.items():
        words_ = _bits(mask)
        allow = torch.from_numpy(words_.view(np.int32)).cuda()
        for k in (1, 12, 64):
            s_h, r_h, n_h = b.search(qs, k, words_)
            s_d, r_d = b.search_filtered(qt, qo, k, allow)
            s_d, r_d = s_d.cpu().numpy(), r_d.cpu().numpy()
            for i in range(len(qs)):
                n = int(n_h[i])
                assert r_d[i][:n].tolist() == r_h[i][:n].tolist(), (name, k, i)
                assert s_d[i][:n].tolist() == s_h[i][:n].tolist(), (name, k, i)
                assert (r_d[i][n:] == -1).all()
        sub = [i for i in range(len(texts)) if mask[i]]
        if sub:
            ora = orc.BM25Oracle()
            ora.upsert_many([ids[i] for i in sub], [texts[i] for i in sub], [{"language": "en"}] * len(sub))
            s_d, r_d = b.search_filtered(qt, qo, 12, allow)
            for i, q in enumerate(queries):
                want = ora.search(q, None, top_k=12)
                got = [[ids[r], s] for r, s in zip(r_d[i].tolist(), s_d[i].tolist()) if r >= 0]
                assert got == [[w["id"], w["score"]] for w in want], (name, q)
    # the status word reports the missing epsilon instead of guessing it
    mask = np.arange(len(texts)) < 40
    allow = torch.from_numpy(_bits(mask).view(np.int32)).cuda()
    _, _, st = b.search_filtered_dev(qt, qo, 10, allow)
    assert int(st.item()) & b.FILT_EPS_MISSING
