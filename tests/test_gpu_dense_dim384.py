"""The certified int8 coarse search of stores with row stride 384 (dims 257-384; cm_dense.hip
dense_kind / coarse_config, cm_dense_q8.inc dense_q8_stream_kernel<QT, R, 3> and the <384> re-ranks):
prep -> f16 seed sample (K1s MINONLY, one launch per pass) -> K1q-s, one stream pass per 32 queries
-> certified re-rank straight to fp64 -> gated exact fallback, the same results as the exact search.
The kind is automatic up to 32 queries; above that the store stays on K1c and a forced K1q-s runs in
passes, which is how the multi-pass cases here reach it.

Bars: the project's (test_gpu_scale.py DIST_TOL / TIE, the ones test_gpu_q8.py holds dim 768 to):
distances within 1e-4 of the exact fp64 1 - cos, rows equal wherever the oracle's neighbouring
distances differ by more than 1e-5, every list ascending in (distance, row).  The oracle and the
numpy model of a mutated store are test_gpu_dense_mutations.py's.

Shapes.  20 011 rows (16 384 is the smallest store with a coarse path; 20 011 % 64 = 43 and % 32 = 11,
so the last tile and the last live word are partial).  At that size every wave streams one 64-row
tile, so no 128-slot (group, query) buffer can overflow: the overflow cases use 200 011 rows (256
rows per wave at 256 CUs), as test_gpu_q8.py's cluster cases do at dim 768.  The seed sample is rows
[0, 640): ten 64-row groups, so k = 24 and 32 search with an infinite seed (every live row a
candidate, certified from the complete set) and k = 1 and 10 with a finite one.
"""
import contextlib
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_dense_mutations import Model, _bits, both, check_lists, gauss, near, q8_group_of, q8_group_rows
from test_gpu_scale import check_dense, exact_topk, unit_rows

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
from int8_band_center import aniso_rows  # noqa: E402

pytestmark = pytest.mark.gpu

F32, COARSE, STREAM, Q8, Q8S = 1, 3, 4, 5, 6
D = 384
N = 20011
KS = (1, 10, 24, 32)
NQS_AUTO = (1, 16, 17, 32)      # one pass: one q-tile, a full q-tile, a one-query second q-tile, two full ones
NQS_FORCED = (33, 70)           # forced K1q-s: a one-query last pass; three passes, the last one partial
SQ = 32                         # kSQ: queries per stream pass = the automatic cut-off


@contextlib.contextmanager
def path(idx, kind):
    """The index with a forced kind (0: automatic), automatic again afterwards."""
    idx.set_path(kind)
    try:
        yield idx
    finally:
        idx.set_path(0)


def q8s_for(nq):
    """The kind to force so that nq queries run K1q-s: none up to the cut-off."""
    return 0 if nq <= SQ else Q8S


def _store(dim, seed, n=N, capacity=0):
    from classmate_hip import engine
    C = unit_rows(n, dim, seed=seed)
    idx = engine.DenseIndex(dim, capacity=capacity)
    model = Model(dim)
    rows = np.arange(n, dtype=np.int64)
    idx.upsert(C, rows)
    model.upsert(C, rows)
    return C, idx, model


@pytest.fixture(scope="module", params=[384, 300])
def store(request):
    dim = request.param
    C, idx, model = _store(dim, seed=300 + dim)
    nq = max(NQS_FORCED)
    Q = gauss(nq, dim, 310 + dim)
    Q[1::2] = near(C[np.arange(1, nq, 2) * 251 % N], np.random.default_rng(320 + dim), noise=0.3)
    yield dict(dim=dim, C=C, idx=idx, model=model, Q=Q)
    idx.close()


def _search_all_entries(idx, Q, k, words=None):
    """The host entry, search_dev, and search_dev_deferred + exact_fallback_dev on the same queries ->
    (dist, rows) of the host entry after asserting the device entries return the same bits; also the
    counters of the host search and of the device search's workspace."""
    import torch
    d, r = idx.search(Q, k, words)
    ctr = dict(fb=idx.last_fallbacks(), wide=idx.last_wide_reranks(), band=idx.last_band_rows())
    q = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    wdev = None if words is None else torch.from_numpy(words.view(np.int32).copy()).cuda()
    ws = torch.empty(idx.workspace_bytes(Q.shape[0], k), dtype=torch.uint8, device="cuda")
    dd, rd = idx.search_dev(q, k, allow=wdev, workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(rd.cpu().numpy(), r) and np.array_equal(dd.cpu().numpy(), d), "search_dev"
    assert idx.workspace_fallbacks(Q.shape[0], k, ws) == ctr["fb"]
    assert idx.workspace_wide_reranks(Q.shape[0], k, ws) == ctr["wide"]
    assert idx.workspace_band_rows(Q.shape[0], k, ws) == ctr["band"]
    out = idx.search_dev(q, k, allow=wdev, workspace=ws, defer_exact=True)
    idx.exact_fallback_dev(q, k, out, workspace=ws, allow=wdev)
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), r) and np.array_equal(out[0].cpu().numpy(), d), "deferred"
    return d, r, ctr


def test_kind(store):
    """1. ld 384: K1q-s is the automatic kind up to 32 queries (K1s before this path existed), K1c
    above; a forced K1q-s is honoured at every batch size, forced K1c and K1s as before, a forced K1q
    (no 384 instance) falls to the automatic rule; k > 32, a forced fp32 and a small store are exact."""
    from classmate_hip import engine
    idx = store["idx"]
    for nq in (1, 16, 32):
        assert idx.search_kind(nq, 24) == Q8S, nq
    for nq in (33, 256):
        assert idx.search_kind(nq, 24) == COARSE, nq
    with path(idx, Q8S):
        for nq in (1, 33, 70, 300):
            assert idx.search_kind(nq, 24) == Q8S, nq
    with path(idx, COARSE):
        for nq in (1, 16, 70):
            assert idx.search_kind(nq, 24) == COARSE, nq
    with path(idx, STREAM):
        assert idx.search_kind(1, 24) == STREAM and idx.search_kind(32, 24) == STREAM
        assert idx.search_kind(33, 24) == COARSE                  # K1s holds 32 queries: the automatic rule
    with path(idx, Q8):
        assert idx.search_kind(16, 24) == Q8S and idx.search_kind(70, 24) == COARSE
    assert idx.search_kind(16, 33) == F32
    with path(idx, Q8S):
        assert idx.search_kind(16, 33) == F32
    with path(idx, F32):
        assert idx.search_kind(16, 10) == F32
    small = engine.DenseIndex(store["dim"])
    try:
        small.upsert(store["C"][:16000], np.arange(16000, dtype=np.int64))
        assert small.search_kind(16, 24) == F32
        with path(small, Q8S):
            assert small.search_kind(16, 24) == F32
    finally:
        small.close()


@pytest.mark.parametrize("nq", NQS_AUTO + NQS_FORCED)
def test_matches_exact_fp64(store, nq):
    """2. dims 384 and 300 (ld 384, zero tail): one pass by the automatic rule, two and three passes
    forced (a full, a one-query and a partial last pass), through the three entries; the coarse route
    ran (band rows > 0) and no query went to the exact pass."""
    idx, model, Q = store["idx"], store["model"], np.ascontiguousarray(store["Q"][:nq])
    with path(idx, q8s_for(nq)):
        for k in KS:
            assert idx.search_kind(nq, k) == Q8S
            d, r, ctr = _search_all_entries(idx, Q, k)
            print(f"\n[dim {store['dim']} nq {nq} k {k}] band rows {ctr['band']}, wide {ctr['wide']}, "
                  f"fallbacks {ctr['fb']}", end="")
            check_lists(d, r, model, Q, k)
            assert ctr["band"] > 0
            assert ctr["fb"] == 0


@pytest.mark.parametrize("nq", [16, 40])
def test_selective_filters(store, nq):
    """3. allow bitmaps: nothing allowed inside the seed sample (infinite seed), fewer than k rows
    allowed (padded lists), bits set at and past `size` (never returned); one automatic pass and two
    forced ones."""
    idx, model, Q = store["idx"], store["model"], np.ascontiguousarray(store["Q"][:nq])
    allow = np.zeros(N, bool)
    allow[4096::37] = True                                  # nothing in rows [0, 640)
    few = np.zeros(N, bool)
    few[[5, 700, 9000, 15000, N - 1]] = True                # 5 rows < k
    past = np.ones(((N + 31) // 32 + 4) * 32, bool)         # every bit set, 21 + 128 of them past size
    pwords = _bits(past)
    assert pwords.shape[0] == (N + 31) // 32 + 4 and pwords[-5] == 0xFFFFFFFF
    pads = {}
    with path(idx, F32):
        for name, a in (("outside the sample", allow), ("fewer than k", few)):
            for k in (10, 24):
                pads[name, k] = idx.search(Q, k, _bits(a))[0]
    with path(idx, q8s_for(nq)):
        assert idx.search_kind(nq, 24) == Q8S
        dfull = {k: idx.search(Q, k)[0] for k in (10, 24)}
        for name, a in (("outside the sample", allow), ("fewer than k", few)):
            for k in (10, 24):
                d, r, ctr = _search_all_entries(idx, Q, k, _bits(a))
                print(f"\n[{name} k {k}] band rows {ctr['band']}, fallbacks {ctr['fb']}", end="")
                check_lists(d, r, model, Q, k, allow=a, pad_ref=pads[name, k])
        for k in (10, 24):
            d, r, _ = _search_all_entries(idx, Q, k, pwords)
            assert (r < N).all()
            check_lists(d, r, model, Q, k)
            assert np.array_equal(d, dfull[k])


# ---- the certificate under stress: buffers that overflow ---------------------------------------
N_BIG = 200011


@pytest.fixture(scope="module")
def cluster():
    """200 011 x 384 rows with 3 000 contiguous near-duplicates of row 5 (1 - cos in [1e-5, 5e-4]):
    far more than kQCap = 128 of them in one wave's 256 rows."""
    from classmate_hip import engine
    rng = np.random.default_rng(393)
    C = unit_rows(N_BIG, D, seed=390)
    base = C[5].astype(np.float64)
    at = np.arange(100_000, 103_000)
    d_c = rng.permutation(np.linspace(1e-5, 5e-4, at.size))
    u = rng.standard_normal((at.size, D))
    u -= np.outer(u @ base, base)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t = np.sqrt(2.0 * d_c - d_c ** 2)
    C[at] = (np.sqrt(1.0 - t ** 2)[:, None] * base + t[:, None] * u).astype(np.float32)
    Q = gauss(40, D, 394)
    hot = np.r_[0:8, 28:40]                                 # 20 queries on the cluster, 12 + 8 over the two passes
    Q[hot] = (base + 1e-4 * rng.standard_normal((hot.size, D)) / 20.0).astype(np.float32)
    k = 24
    o_d, o_r = exact_topk(C, Q, k + 600)                    # cluster gaps ~2e-7: the tie analysis needs a long tail
    idx = engine.DenseIndex(D, capacity=N_BIG)
    idx.upsert(C, np.arange(N_BIG, dtype=np.int64))
    yield dict(C=C, Q=Q, k=k, o_d=o_d, o_r=o_r, idx=idx, hot=hot, at=at)
    idx.close()


def test_cluster_overflows_into_the_wide_rerank(cluster):
    """4. a 16-query search (automatic), 8 of them on the cluster: their (group, query) buffers
    overflow and the wide re-rank re-scans the overflowed groups on the int8 plane (24 16-byte pieces
    per row at ld 384); every list equals the oracle, on the three entries."""
    idx, Q, k = cluster["idx"], np.ascontiguousarray(cluster["Q"][:16]), cluster["k"]
    assert idx.search_kind(16, k) == Q8S
    d, r, ctr = _search_all_entries(idx, Q, k)
    print(f"\n[cluster nq 16] wide {ctr['wide']}, fallbacks {ctr['fb']}, band rows {ctr['band']}", end="")
    check_dense(d, r, cluster["o_d"][:16], cluster["o_r"][:16], k)
    assert ctr["wide"] > 0
    assert ctr["wide"] + ctr["fb"] >= 8


def test_more_failing_queries_than_wide_slots(cluster):
    """4. 20 of 40 queries (two forced passes) fail the LDS re-rank: the first 16 by query index take
    the wide re-rank's slots, the rest the exact pass, whatever order the workgroups run in -- the
    same bits on every run -- and all 40 lists equal the oracle; then deletes in the cluster and an
    allow filter."""
    idx, Q, k, at = cluster["idx"], cluster["Q"], cluster["k"], cluster["at"]
    with path(idx, Q8S):
        assert idx.search_kind(40, k) == Q8S
        d, r, ctr = _search_all_entries(idx, Q, k)
        print(f"\n[cluster nq 40] wide {ctr['wide']}, fallbacks {ctr['fb']}", end="")
        check_dense(d, r, cluster["o_d"], cluster["o_r"], k)
        assert ctr["wide"] + ctr["fb"] >= 20 and ctr["wide"] <= 16
        for _ in range(2):
            d2, r2 = idx.search(Q, k)
            assert np.array_equal(r2, r) and np.array_equal(d2, d)
    drop = at[::5]
    allow = np.ones(N_BIG, bool)
    allow[at[1::7]] = False
    allow[::11] = False
    keep = allow.copy()
    keep[drop] = False
    rows = np.nonzero(keep)[0]
    o_d2, o_r2 = exact_topk(cluster["C"][rows], Q[:16], k + 600)
    idx.delete(drop)
    try:
        d3, r3, _ = _search_all_entries(idx, np.ascontiguousarray(Q[:16]), k, _bits(allow))
        check_dense(d3, r3, o_d2, rows[o_r2], k)
        assert not np.isin(r3, drop).any() and allow[r3[r3 >= 0]].all()
    finally:
        idx.upsert(cluster["C"][drop], drop.astype(np.int64))


# ---- derived copies follow the fp32 rows ---------------------------------------------------------
def _verify(tag, idx, model, Q, ks=(10, 24), fresh=True):
    """40 queries (two forced passes) and the first 16 of them (automatic) on K1q-s against the oracle
    of the model, and against a fresh index built from the model's final state: rows equal, distances
    within 1e-6 (the never-lowered maxima may differ).  -> the 40-query results by k."""
    from classmate_hip import engine
    assert idx.size == model.size and idx.live_count() == int(model.live.sum())
    out, live = idx.export(with_live=True)
    assert np.array_equal(live, model.live) and out.tobytes() == model.vecs.tobytes(), tag
    new = None
    if fresh:
        rows = model.live_rows()
        new = engine.DenseIndex(model.dim)
        new.upsert(model.vecs[rows], rows)
    res = {}
    try:
        for k in ks:
            for nq in (40, 16):
                q = np.ascontiguousarray(Q[:nq])
                with path(idx, q8s_for(nq)):
                    assert idx.search_kind(nq, k) == (Q8S if idx.size >= 16384 else F32), tag
                    d, r, ctr = _search_all_entries(idx, q, k)
                print(f"\n[{tag} k {k} nq {nq}] band rows {ctr['band']}, wide {ctr['wide']}, fallbacks {ctr['fb']}",
                      end="")
                check_lists(d, r, model, q, k)
                if new is not None:
                    with path(new, q8s_for(nq)):
                        dn, rn = new.search(q, k)
                    assert np.array_equal(r, rn), (tag, k)
                    assert float(np.abs(d.astype(np.float64) - dn).max()) <= 1e-6, (tag, k)
                if nq == 40:
                    res[k] = (d, r)
    finally:
        if new is not None:
            new.close()
    return res


@pytest.fixture(scope="module")
def base():
    C = unit_rows(N, D, seed=401)
    return dict(C=C, Q=gauss(40, D, 402))


def _index_of(C, capacity=0):
    from classmate_hip import engine
    idx = engine.DenseIndex(D, capacity=capacity)
    model = Model(D)
    rows = np.arange(C.shape[0], dtype=np.int64)
    idx.upsert(C, rows)
    model.upsert(C, rows)
    return idx, model


def test_overwrite_scale_jump_delete_and_reuse(base):
    """5. in-place overwrite (row 0, the last row, a whole scale group, one row of a group, rows inside
    and outside the seed sample), a 10x scale jump inside a group (a near one-hot row), delete then
    reuse."""
    C, Q = base["C"], base["Q"].copy()
    rng = np.random.default_rng(410)
    idx, model = _index_of(C)
    try:
        m = both(idx, model)
        planted = np.array([0, N - 1, 100, int(q8_group_rows(q8_group_of(9000))[0]), 12345, 300, 640, 4097])
        rows = np.unique(np.concatenate([planted, q8_group_rows(q8_group_of(9000)), [5, 63, 64, 511],
                                         rng.choice(np.arange(700, N - 1), 450, replace=False)]))
        rows = rows[rows < N]
        vecs = gauss(rows.shape[0], D, 411)
        Q[:8] = near(vecs[np.searchsorted(rows, planted)], rng)
        m.upsert(vecs, rows)
        for k, (d, r) in _verify("overwrite", idx, model, Q).items():
            assert (r[:8, 0] == planted).all() and (d[:8, 0] < 1e-3).all(), k
        # scale jump: one row of three groups becomes near one-hot, its group mates keep their values
        groups = [q8_group_of(x) for x in (40, 9100, N - 50)]
        hot_rows, keep_rows = [], []
        for G in groups:
            g = q8_group_rows(G)
            hot_rows.append(g[1])
            keep_rows += [g[0], g[14]]
        hot = np.zeros((3, D), np.float32)
        hot[np.arange(3), rng.integers(0, D, 3)] = 1.0
        hot = near(hot, rng)
        assert np.abs(hot / np.linalg.norm(hot, axis=1, keepdims=True)).max(axis=1).min() > 0.99
        m.upsert(hot, np.array(hot_rows, np.int64))
        want = np.array(keep_rows + hot_rows)
        Q[8:17] = near(model.vecs[want], rng)
        for k, (d, r) in _verify("scale jump", idx, model, Q).items():
            assert (r[8:17, 0] == want).all() and (d[8:17, 0] < 1e-3).all(), k
        # delete then reuse
        stay, back = np.array([2, 130, 4100, 9002, 16000]), np.array([7, 333, 8000, 12000, N - 2])
        old_stay = model.vecs[stay].copy()
        m.delete(np.concatenate([stay, back, rng.choice(np.arange(1300, N - 64), 300, replace=False)]))
        new_back = gauss(5, D, 412)
        m.upsert(new_back, back)
        Q[17:27] = np.concatenate([near(old_stay, rng), near(new_back, rng)])
        for k, (d, r) in _verify("delete + reuse", idx, model, Q).items():
            for j in range(5):
                assert stay[j] not in r[17 + j] and d[17 + j, 0] > 0.5, (k, j)
                assert r[22 + j, 0] == back[j] and d[22 + j, 0] < 1e-3, (k, j)
    finally:
        idx.close()


@pytest.mark.parametrize("shrink", [False, True])
def test_compact_and_truncate(base, shrink, monkeypatch):
    """5. compact() (with and without shrink, in 1 000-row chunks), then truncate at n % 64 == 13: the
    int8 plane and its scales follow."""
    monkeypatch.setenv("CM_COMPACT_CHUNK_ROWS", "1000")
    C, Q = base["C"], base["Q"].copy()
    rng = np.random.default_rng(430)
    idx, model = _index_of(C)
    try:
        dead = np.arange(N) % 11 == 3
        dead[4096:4224] = True
        dead[0] = True
        dead[N - 200:] = True
        both(idx, model).delete(np.nonzero(dead)[0])
        before = idx.mem_stats()["bytes"]
        old = idx.compact(shrink=shrink)
        assert np.array_equal(old, model.compact()) and idx.size == model.size >= 16384 + 64
        assert (idx.mem_stats()["bytes"] < before) == shrink
        probe = np.array([0, 5, 600, 4000, 12000, model.size - 1])
        Q[:6] = near(model.vecs[probe], rng)
        for k, (d, r) in _verify(f"compact shrink={shrink}", idx, model, Q).items():
            assert (r[:6, 0] == probe).all() and (d[:6, 0] < 1e-3).all(), k
        n = 16397
        assert n % 64 == 13 and n < model.size
        gone = model.vecs[[n, model.size - 1]].copy()
        idx.truncate(n)
        model.truncate(n)
        probe = np.array([0, 600, 12000, n - 1, n - 13])
        Q[:5] = near(model.vecs[probe], rng)
        Q[5:7] = near(gone, rng)
        for k, (d, r) in _verify("truncate", idx, model, Q).items():
            assert (r[:5, 0] == probe).all() and (d[:5, 0] < 1e-3).all() and (d[5:7, 0] > 0.5).all() and (r < n).all(), k
    finally:
        idx.close()


# ---- centre -------------------------------------------------------------------------------------------
def test_store_recenter_keeps_results_and_shrinks_the_band():
    """6. anisotropic rows normalize(sqrt(a) m + sqrt(1 - a) u) at a = 0.5 in a dim-384 GpuVectorStore:
    recenter() (the mean of the normalised rows) returns the same ids and the same distance bits on
    K1q-s -- every distance is the fp64 stage's, no query takes the exact fp32 pass: at 64 rows per
    wave no buffer can overflow -- and its certified band is not larger than the plain plane's."""
    from classmate_hip.retrieval import GpuVectorStore
    k = 10
    C = aniso_rows(N, D, 0.5, seed=441)
    rng = np.random.default_rng(442)
    Q = aniso_rows(16, D, 0.5, seed=443)
    Q[1::2] = near(C[np.arange(1, 16, 2) * 997 % N], rng, noise=0.3)
    model = Model(D)
    model.upsert(C, np.arange(N))
    vs = GpuVectorStore(persist_dir=None)
    vs.upsert(ids=[f"c{i}" for i in range(N)], documents=["x"] * N, metadatas=[{"n": i} for i in range(N)],
              embeddings=C)

    def lists():
        assert vs._index.search_kind(16, k) == Q8S
        got = vs.query_batch(query_embeddings=Q, top_k=k)
        band, fb = vs._index.last_band_rows(), vs._index.last_fallbacks()
        d = np.array([[it["distance"] for it in items] for items in got], np.float32)
        r = np.array([[int(it["id"][1:]) for it in items] for items in got], np.int64)
        check_lists(d, r, model, Q, k)
        one = vs.query(query_embeddings=Q[1], top_k=k)
        assert [it["id"] for it in one] == [it["id"] for it in got[1]]
        return d, r, band, fb

    d0, r0, band0, fb0 = lists()
    assert vs._index.center() is None
    out = vs.recenter()
    assert out["rows"] == N and 0.6 < out["norm"] <= 1.0     # ||mean|| ~ sqrt(a) = 0.71
    assert vs._index.center() is not None
    d1, r1, band1, fb1 = lists()
    print(f"\n[recenter] band rows plain {band0}, centred {band1}; fallbacks {fb0}, {fb1}", end="")
    assert fb0 == 0 and fb1 == 0
    assert np.array_equal(r1, r0) and np.array_equal(d1, d0)
    assert 0 < band1 <= band0
    vs.recenter(clear=True)
    d2, r2, band2, _ = lists()
    assert np.array_equal(r2, r0) and np.array_equal(d2, d0) and band2 == band0


# ---- drop-in level ----------------------------------------------------------------------------------
def test_vector_store_dim384(tmp_path):
    """7. GpuVectorStore at dim 384: query, query_batch and query_batch(where=[...]) equal the
    oracle (check_lists over the rows the ids name), and the store reopens from its directory; a
    single question and a 16-question batch are on K1q-s."""
    from classmate_hip.retrieval import GpuVectorStore
    n, k = 17003, 10
    C = unit_rows(n, D, seed=440)
    ids = [f"c{i}" for i in range(n)]
    metas = [{"g": f"g{i % 3}", "n": i} for i in range(n)]
    vs = GpuVectorStore(persist_dir=tmp_path)
    vs.upsert(ids=ids, documents=[f"doc {i}" for i in range(n)], metadatas=metas, embeddings=C)
    Q = gauss(16, D, 441)
    model = Model(D)
    model.upsert(C, np.arange(n))
    g1 = np.arange(n) % 3 == 1

    def same(lists, q, allow=None):
        assert all(len(items) == k for items in lists)
        d = np.array([[it["distance"] for it in items] for items in lists], np.float32)
        r = np.array([[int(it["id"][1:]) for it in items] for items in lists], np.int64)
        check_lists(d, r, model, np.ascontiguousarray(q), k, allow=allow)

    odd, even = np.arange(1, 16, 2), np.arange(0, 16, 2)
    for v in (vs, None):
        if v is None:
            v = GpuVectorStore(persist_dir=tmp_path)              # reopened from its directory
            assert v.count() == n
        assert v._index.search_kind(1, k) == Q8S and v._index.search_kind(16, k) == Q8S
        same([v.query(query_embeddings=Q[0], top_k=k)], Q[:1])
        assert v._index.last_band_rows() > 0
        same([v.query(query_embeddings=Q[0], where={"g": "g1"}, top_k=k)], Q[:1], g1)
        same(v.query_batch(query_embeddings=Q, top_k=k), Q)
        assert v._index.last_band_rows() > 0
        same(v.query_batch(query_embeddings=Q, where={"g": "g1"}, top_k=k), Q, g1)
        wheres = [{"g": "g1"} if i % 2 else None for i in range(Q.shape[0])]
        got = v.query_batch(query_embeddings=Q, where=wheres, top_k=k)
        same([got[i] for i in odd], Q[odd], g1)
        same([got[i] for i in even], Q[even])


def test_sharded_index_equals_one_index():
    """7. ShardedDenseIndex(dim=384, devices=[0, 0]): two shards of >= 16 384 rows, each on K1q-s for
    16 queries, merged lists equal to one index's and to the oracle; the device entry equals the
    host's."""
    import torch
    from classmate_hip import engine, multidev
    n = 33100                                               # blocks of 64 rows: 16 576 and 16 524 rows
    C = unit_rows(n, D, seed=450)
    Q = gauss(16, D, 451)
    rows = np.arange(n, dtype=np.int64)
    sh = multidev.ShardedDenseIndex(dim=D, devices=[0, 0], block=64)
    one = engine.DenseIndex(D)
    model = Model(D)
    try:
        sh.upsert(C, rows)
        one.upsert(C, rows)
        model.upsert(C, rows)
        for s in sh.shards:
            assert s.size >= 16384 and s.search_kind(16, 24) == Q8S
        for k in (10, 24):
            d, r = sh.search(Q, k)
            check_lists(d, r, model, Q, k)
            d1, r1 = one.search(Q, k)
            assert np.array_equal(r, r1) and float(np.abs(d.astype(np.float64) - d1).max()) <= 1e-6
            dd, rd = sh.search_dev(torch.from_numpy(Q).cuda(), k)
            torch.cuda.synchronize()
            assert np.array_equal(rd.cpu().numpy(), r) and np.array_equal(dd.cpu().numpy(), d)
    finally:
        sh.close()
        one.close()
