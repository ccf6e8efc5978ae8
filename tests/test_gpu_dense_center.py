"""Centred int8 plane (cm_dense_set_center; cm_dense_q8.inc "Centred plane") on anisotropic rows:
rows normalize(sqrt(a) m + sqrt(1 - a) u_i), pairwise cosine ~ a, as E5 output has.  A centre changes
which rows the certified band holds and nothing else: every list stays exact under any centre, the
band shrinks under the mean, mean() is the fp64 mean of the normalised live rows, every mutation
quantises under the handle's centre, and the vector store keeps the centre in center.f32.

N = 40 000 x 768 (test_gpu_rerank_pilot's size: 192-row K1q ranges, 64-row K1q-s ranges).  The CPU
model tools/int8_band_center.py is run on the test's own arrays before the GPU is asked: at a = 0.5 it
puts plain and centred bands inside the re-rank's 4 096 rows, at a = 0.8 the plain band beyond them
(~6 700 rows per near-duplicate query) and the centred one at ~570."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_scale import TIE, check_dense, exact_topk, mixed_queries

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
from int8_band_center import aniso_rows, model, quantise_rows  # noqa: E402

pytestmark = pytest.mark.gpu

Q8, Q8S = 5, 6
N, DIM = 40_000, 768
CASES = ((256, 24), (40, 10), (33, 32), (16, 24), (1, 1))
KQ_BAND = 4096          # kQBand: int8-band rows the re-rank holds per query
KQ_CAP = 128            # kQCap: candidate slots per (range, query)
SLACK = 40

_DATA = {}


def corpus(a):
    """(C, Q, exact distances, exact rows, fp64 mean of the normalised rows), computed once per a."""
    if a not in _DATA:
        C = aniso_rows(N, DIM, a, seed=911)
        Q = mixed_queries(C, 256, seed=912)
        o_d, o_r = exact_topk(C, Q, 32 + SLACK)
        Cn = C.astype(np.float64)
        Cn /= np.linalg.norm(Cn, axis=1, keepdims=True)
        for x in (C, Q, o_d, o_r):
            x.setflags(write=False)
        _DATA[a] = (C, Q, o_d, o_r, Cn.mean(0))
    return _DATA[a]


def _index(monkeypatch, mode, C, rows=None, capacity=None, mu=None, keep_env=False):
    from classmate_hip import engine
    monkeypatch.setenv("CM_DENSE_F16", mode)
    idx = engine.DenseIndex(DIM, capacity=C.shape[0] if capacity is None else capacity)
    if mu is not None:
        idx.set_center(mu)
    idx.upsert(C, np.arange(C.shape[0], dtype=np.int64) if rows is None else rows)
    if not keep_env:     # (the policy is read at every allocation: a store that grows later needs it kept)
        monkeypatch.delenv("CM_DENSE_F16")
    return idx


def _search(idx, Q, k, allow=None):
    d, r = idx.search(Q, k, allow)
    return d, r, idx.last_band_rows(), idx.last_fallbacks(), idx.last_wide_reranks()


def _words(allow):
    return np.packbits(allow, bitorder="little").view(np.uint32)


def same_rows(r, r0, o_d, o_r):
    """Two lists of one search agree: the same row at every place, except where the two rows' exact
    distances are within TIE of each other -- a query the plain store re-ran on its exact fp32 pass
    orders such near-ties by fp32 distances (at a = 0.8 the distances crowd together)."""
    for i, j in zip(*np.nonzero(r != r0)):
        da = o_d[i][o_r[i] == r[i, j]]
        db = o_d[i][o_r[i] == r0[i, j]]
        assert da.size == 1 and db.size == 1 and abs(da[0] - db[0]) < TIE, (i, j, r[i, j], r0[i, j])


def _bad_center():
    v = np.random.default_rng(913).standard_normal(DIM)
    return (0.5 * v / np.linalg.norm(v)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# 1. exactness under any centre
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["prefix", "full"])
@pytest.mark.parametrize("a", [0.5, 0.8])
def test_exact_under_any_centre(a, mode, monkeypatch):
    """No centre, the mean and a bad centre (0.5 x a random unit vector): every list exact, the rows
    equal across the three, and the distances bit-equal wherever no query took the exact fp32 pass.
    At a = 0.5 that is every run but one: with the full f16 plane the re-rank has no pilot bound, its
    int8 band comes from kth_up alone, and under the bad centre (||xn - mu|| ~ 1.12 instead of 1) it
    passes the re-rank's 4 096 rows for 40 of the 256 queries (measured: 16 finished by the wide
    re-rank, 24 by the exact pass; fp32 distances within 1e-6 there)."""
    C, Q, o_d, o_r, _ = corpus(a)
    idx = _index(monkeypatch, mode, C)
    try:
        assert idx.center() is None
        first = {}
        for nq, k in CASES:
            assert idx.search_kind(nq, k) == (Q8 if nq > 32 else Q8S)
            first[nq, k] = _search(idx, Q[:nq], k)
        mean = idx.mean()
        for name, mu in (("mean", mean), ("bad", _bad_center())):
            idx.set_center(mu)
            assert np.array_equal(idx.center(), mu)
            for nq, k in CASES:
                d, r, b, fb, w = _search(idx, Q[:nq], k)
                d0, r0, b0, fb0, w0 = first[nq, k]
                print(f"a={a} {mode} {name} nq={nq} k={k}: band {b} (plain {b0}) fallbacks {fb} ({fb0}) wide {w} ({w0})")
                check_dense(d, r, o_d[:nq, :k + SLACK], o_r[:nq, :k + SLACK], k)
                check_dense(d0, r0, o_d[:nq, :k + SLACK], o_r[:nq, :k + SLACK], k)
                if fb == 0 and fb0 == 0:
                    assert np.array_equal(r, r0), (name, nq, k)
                else:
                    same_rows(r, r0, o_d[:nq, :k + SLACK], o_r[:nq, :k + SLACK])
                if a == 0.5 and (name == "mean" or mode == "prefix"):
                    assert fb == 0 and fb0 == 0, (name, nq, k)
                if fb == 0 and fb0 == 0:   # no exact fp32 pass: every distance is the fp64 re-rank's
                    assert np.array_equal(d, d0), (name, nq, k)
                else:                      # fp32 K1 distances for the re-run queries
                    np.testing.assert_allclose(d, d0, atol=1e-6)
        idx.set_center(None)
        assert idx.center() is None
        for nq, k in CASES:
            got = _search(idx, Q[:nq], k)
            assert np.array_equal(got[0], first[nq, k][0]) and np.array_equal(got[1], first[nq, k][1])
            assert got[2:] == first[nq, k][2:], (nq, k, got[2:], first[nq, k][2:])
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------
# 2. the band shrinks
# ---------------------------------------------------------------------------------------------------
def _model_both(C, Q, mu, range_rows, sample):
    plain = model(C, Q, 24, None, sample=sample, range_rows=range_rows)
    cent = model(C, Q, 24, mu, sample=sample, range_rows=range_rows)
    return plain, cent


def test_band_shrinks_at_cosine_half(monkeypatch):
    C, Q, _, _, mean64 = corpus(0.5)
    mu = mean64.astype(np.float32)
    sel = np.r_[0:8, 248:256]                    # near-duplicate and random-direction queries
    for rr, sample in ((192, 16), (64, 32)):     # K1q / K1q-s ranges and seed samples at this size
        plain, cent = _model_both(C, Q[sel], mu, rr, sample)
        for m in (plain, cent):                  # the model: no overflow, no wide re-rank either way
            assert m["band_pilot"].max() < KQ_BAND and m["band_kth_up"].max() < KQ_BAND
            assert m["cand_range_max"].max() <= KQ_CAP
        assert cent["band_pilot"].sum() < plain["band_pilot"].sum()
    idx = _index(monkeypatch, "prefix", C)
    try:
        for nq, k in ((256, 24), (16, 24)):
            _, r0, b0, fb0, w0 = _search(idx, Q[:nq], k)
            idx.set_center(idx.mean())
            _, r1, b1, fb1, w1 = _search(idx, Q[:nq], k)
            idx.set_center(None)
            print(f"a=0.5 nq={nq}: band rows plain {b0} centred {b1} ({b0 / nq:.0f} / {b1 / nq:.0f} per query)")
            assert fb0 == 0 and w0 == 0 and fb1 == 0 and w1 == 0
            assert 0 < b1 < b0
            assert np.array_equal(r0, r1)
    finally:
        idx.close()


def test_band_shrinks_at_cosine_08(monkeypatch):
    C, Q, o_d, o_r, mean64 = corpus(0.8)
    mu = mean64.astype(np.float32)
    for rr, sample in ((192, 16), (64, 32)):
        plain, cent = _model_both(C, Q[:16], mu, rr, sample)   # near-duplicate queries: the wide ones
        assert plain["band_pilot"].max() > KQ_BAND             # plain: beyond the re-rank's LDS
        assert cent["band_pilot"].max() < KQ_BAND and cent["cand_range_max"].max() <= KQ_CAP
    idx = _index(monkeypatch, "prefix", C)
    try:
        for nq, k in ((256, 24), (16, 24)):
            _, r0, b0, fb0, w0 = _search(idx, Q[:nq], k)
            idx.set_center(idx.mean())
            _, r1, b1, fb1, w1 = _search(idx, Q[:nq], k)
            idx.set_center(None)
            print(f"a=0.8 nq={nq}: plain band {b0} fallbacks {fb0} wide {w0}; centred band {b1} fallbacks {fb1} wide {w1}")
            assert fb1 == 0
            assert fb1 + w1 < fb0 + w0
            same_rows(r1, r0, o_d[:nq, :k + SLACK], o_r[:nq, :k + SLACK])
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------
# 3. mean()
# ---------------------------------------------------------------------------------------------------
def test_mean(monkeypatch):
    from classmate_hip import engine
    C, _, _, _, _ = corpus(0.8)
    idx = _index(monkeypatch, "prefix", C)
    try:
        drop = np.random.default_rng(914).choice(N, N // 10, replace=False)
        idx.delete(drop)
        live = np.ones(N, bool)
        live[drop] = False
        Cn = C[live].astype(np.float64)
        Cn /= np.linalg.norm(Cn, axis=1, keepdims=True)
        want = Cn.mean(0)
        m1, m2 = idx.mean(), idx.mean()
        print(f"mean: max |device - numpy fp64| = {np.abs(m1 - want).max():.3g}, |mean| = {np.linalg.norm(want):.4f}")
        assert m1.dtype == np.float32 and m1.shape == (DIM,)
        assert np.abs(m1.astype(np.float64) - want).max() <= 1e-6
        assert m1.tobytes() == m2.tobytes()
        s1, n1 = idx.column_sums()
        s2, n2 = idx.column_sums()
        assert n1 == n2 == int(live.sum()) and s1.tobytes() == s2.tobytes()
    finally:
        idx.close()
    empty = engine.DenseIndex(DIM)
    try:
        sums, n = empty.column_sums()
        assert n == 0 and not sums.any() and not empty.mean().any()
    finally:
        empty.close()


# ---------------------------------------------------------------------------------------------------
# 4. mutations under a centre
# ---------------------------------------------------------------------------------------------------
class _Model:
    """Host truth of the store: vectors by row and the live mask."""

    def __init__(self, C):
        self.vecs, self.live = C.copy(), np.ones(C.shape[0], bool)

    def put(self, rows, vecs):
        top = int(np.max(rows)) + 1
        if top > self.vecs.shape[0]:
            grow = top - self.vecs.shape[0]
            self.vecs = np.concatenate([self.vecs, np.zeros((grow, DIM), np.float32)])
            self.live = np.concatenate([self.live, np.zeros(grow, bool)])
        self.vecs[rows], self.live[rows] = vecs, True

    def oracle(self, Q, kk):
        rows = np.nonzero(self.live)[0]
        d, r = exact_topk(self.vecs[rows], Q, kk)
        return d, rows[r]


def _like_fresh(monkeypatch, idx, mdl, mu, Q, step):
    """Lists pass check_dense; lists and band rows equal those of a fresh index that is given the same
    centre and then the same final rows: the fp32 data of every row, and the deletes (a deleted row
    keeps its data and its share in its group's scale until a compaction, on both sides)."""
    fresh = _index(monkeypatch, "prefix", mdl.vecs, capacity=mdl.vecs.shape[0], mu=mu, keep_env=True)
    if not mdl.live.all():
        fresh.delete(np.nonzero(~mdl.live)[0])
    try:
        o_d, o_r = mdl.oracle(Q, 24 + SLACK)
        for nq, k in ((64, 24), (16, 24)):
            d, r, b, fb, w = _search(idx, Q[:nq], k)
            df, rf, bf, fbf, wf = _search(fresh, Q[:nq], k)
            print(f"{step} nq={nq}: band {b} (fresh {bf}) fallbacks {fb} wide {w}")
            check_dense(d, r, o_d[:nq], o_r[:nq], k)
            assert fb == 0 and fbf == 0
            assert np.array_equal(r, rf) and np.array_equal(d, df), (step, nq)
            assert (b, w) == (bf, wf), (step, nq, b, bf)
    finally:
        fresh.close()


def test_mutations_under_a_centre(monkeypatch):
    import torch
    C0, Q, _, _, mean64 = corpus(0.5)
    mu = mean64.astype(np.float32)
    rng = np.random.default_rng(915)
    new = aniso_rows(8_000, DIM, 0.5, seed=916)
    C = C0.copy()
    # rnorm[2], the largest ||s_r q8|| of any row ever quantised, is never lowered by a mutation: for the
    # band rows of the mutated and of a fresh store to be equal bit for bit both must see the same
    # maximum.  Row 0 pins it: -mean / |mean| has ||xn - mu|| = 1 + |mu| (the other rows ~0.7), sets the
    # scale of whatever group it lands in, and no step below touches it.
    C[0] = (-mean64 / np.linalg.norm(mean64)).astype(np.float32)
    _, _, _, _, xn = quantise_rows(C, mu)
    ynorm = np.linalg.norm(xn.astype(np.float64) - mu, axis=1)
    assert ynorm[0] > 1.5 and ynorm[1:].max() < 1.0
    Q = Q[:64]
    mdl = _Model(C)
    idx = _index(monkeypatch, "prefix", C, capacity=N, mu=mu, keep_env=True)   # growth allocates again
    try:
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "build")
        # overwrite 500 rows in place; one of them 10x its group mates' scale
        rows = 1 + np.sort(rng.choice(N - 1, 500, replace=False))
        vecs = new[:500].copy()
        vecs[7] *= 10.0
        idx.upsert(vecs, rows)
        mdl.put(rows, vecs)
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "overwrite")
        # delete 1 000 rows, reuse 200 of them
        dead = 1 + np.sort(rng.choice(N - 1, 1000, replace=False))
        idx.delete(dead)
        mdl.live[dead] = False
        reuse = np.sort(rng.choice(dead, 200, replace=False))
        idx.upsert(new[500:700], reuse)
        mdl.put(reuse, new[500:700])
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "delete + reuse")
        # upsert_dev over a range that is no multiple of the 64-row tile
        r0, n = 5_003, 611
        idx.upsert_dev(torch.from_numpy(new[700:700 + n]).cuda(), r0)
        torch.cuda.synchronize()
        mdl.put(np.arange(r0, r0 + n), new[700:700 + n])
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "upsert_dev")
        # grow past the capacity
        grow = np.arange(N, N + 3_001, dtype=np.int64)
        idx.upsert(new[2_000:2_000 + grow.size], grow)
        mdl.put(grow, new[2_000:2_000 + grow.size])
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "growth")
        # one live all-zero row: distance 1, in its place among the few allowed rows
        zr = 9_999
        idx.upsert(np.zeros((1, DIM), np.float32), np.array([zr], np.int64))
        near = [s + int(np.nonzero(mdl.live[s:])[0][0]) for s in (17, 4_001, 12_345, 20_002, 33_333, 41_000)]
        some = np.array(sorted(set(near) - {zr}) + [zr])
        allow = np.zeros(idx.size, bool)
        allow[some] = True
        assert some.size == 7 and mdl.live[some[:-1]].all()
        d, r, _, _, _ = _search(idx, Q[:16], 10, _words(allow))
        others = some[some != zr]
        o_d, o_r = exact_topk(mdl.vecs[others], Q[:16], others.size)
        for i in range(16):
            want_d = np.concatenate([o_d[i], [1.0]])
            want_r = np.concatenate([others[o_r[i]], [zr]])
            o = np.lexsort((want_r, want_d))
            assert (np.diff(want_d[o]) > TIE).all()
            assert np.array_equal(r[i, :7], want_r[o]) and (r[i, 7:] == -1).all()
            assert d[i, list(r[i, :7]).index(zr)] == 1.0
        idx.upsert(new[7_000:7_001], np.array([zr], np.int64))      # back to a real vector
        mdl.put(np.array([zr]), new[7_000:7_001])
        # compact
        old = idx.compact()
        keep = np.nonzero(mdl.live)[0]
        assert np.array_equal(old, keep)
        mdl.vecs, mdl.live = mdl.vecs[keep], np.ones(keep.size, bool)
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "compact")
        # truncate inside a tile
        cut = idx.size - 777
        idx.truncate(cut)
        mdl.vecs, mdl.live = mdl.vecs[:cut], mdl.live[:cut]
        _like_fresh(monkeypatch, idx, mdl, mu, Q, "truncate")
        # invalid centres leave everything as it was
        before = _search(idx, Q, 24)
        nan = mu.copy()
        nan[5] = np.nan
        for bad in (nan, (1.5 * mu / np.linalg.norm(mu)).astype(np.float32)):
            with pytest.raises(ValueError):
                idx.set_center(bad)
            assert np.array_equal(idx.center(), mu)
            after = _search(idx, Q, 24)
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
            assert after[2:] == before[2:]
        # reset clears the centre
        idx.reset()
        assert idx.center() is None and idx.size == 0
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------
# 5. filters
# ---------------------------------------------------------------------------------------------------
def test_filters_under_the_mean_centre(monkeypatch):
    C, Q, _, _, _ = corpus(0.8)
    idx = _index(monkeypatch, "prefix", C)
    try:
        third = np.zeros(N, bool)
        third[np.random.default_rng(917).permutation(N)[:N // 3]] = True
        seven = np.zeros(N, bool)
        seven[np.random.default_rng(918).choice(N, 7, replace=False)] = True
        plain = {}
        for name, allow in (("third", third), ("seven", seven)):
            for nq in (40, 16):
                plain[name, nq] = _search(idx, Q[:nq], 10, _words(allow))
        idx.set_center(idx.mean())
        for name, allow in (("third", third), ("seven", seven)):
            for nq in (40, 16):
                d, r, _, fb, _ = _search(idx, Q[:nq], 10, _words(allow))
                d0, r0 = plain[name, nq][:2]
                assert fb == 0
                assert np.array_equal(r, r0), (name, nq)
                live = r >= 0
                assert allow[r[live]].all()
                np.testing.assert_allclose(d, d0, atol=1e-6)
                if name == "seven":
                    assert (live.sum(1) == 7).all() and (r[:, 7:] == -1).all() and (d[:, 7:] == 0).all()
                    assert np.array_equal(d, d0)
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------
# 6. device entry
# ---------------------------------------------------------------------------------------------------
def test_device_entry_under_a_centre(monkeypatch):
    import torch
    C, Q, _, _, _ = corpus(0.8)
    idx = _index(monkeypatch, "prefix", C)
    try:
        idx.set_center(idx.mean())
        for nq, k in ((256, 24), (16, 24)):
            dh, rh, bh, _, _ = _search(idx, Q[:nq], k)
            ws = torch.empty(idx.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            q = torch.from_numpy(Q[:nq]).cuda()
            for _ in range(2):
                dd, rd = idx.search_dev(q, k, workspace=ws)
                torch.cuda.synchronize()
                assert idx.workspace_band_rows(nq, k, ws) == bh > 0
                assert np.array_equal(rd.cpu().numpy(), rh) and np.array_equal(dd.cpu().numpy(), dh)
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------
# 7. the vector store
# ---------------------------------------------------------------------------------------------------
N_STORE = 20_000    # above the coarse kinds' 16 384-row floor; the store's host tables are per row


def _fill(vs, C):
    ids = [f"d{i}" for i in range(C.shape[0])]
    vs.upsert(ids=ids, documents=["x"] * len(ids), metadatas=[{"s": i % 3} for i in range(len(ids))], embeddings=C)


def _ids(vs, Q, k):
    return [[it["id"] for it in items] for items in vs.query_batch(query_embeddings=Q, top_k=k)]


def test_store_recenter_and_cold_open(tmp_path, monkeypatch):
    from classmate_hip.retrieval import GpuVectorStore, vector_store
    monkeypatch.delenv("CM_DEVICES", raising=False)
    C, Q, _, _, _ = corpus(0.8)
    C, Q = C[:N_STORE], Q[96:160]      # near-duplicate and random-direction queries
    plain = GpuVectorStore(persist_dir=None)
    _fill(plain, C)
    want = _ids(plain, Q, 10)
    plain_band = plain._index.last_band_rows()
    want1 = [it["id"] for it in plain.query(query_embeddings=Q[0], top_k=10)]
    vs = GpuVectorStore(persist_dir=tmp_path, collection_name="c")
    _fill(vs, C)
    d = tmp_path / "c"
    assert not (d / "center.f32").exists()
    v0 = vs._version
    out = vs.recenter()
    assert out["rows"] == N_STORE and 0.8 < out["norm"] <= 1.0 and vs._version == v0 + 1
    mu = vs._index.center()
    assert np.array_equal(np.fromfile(d / "center.f32", np.float32), mu)
    assert _ids(vs, Q, 10) == want
    band = vs._index.last_band_rows()
    assert band > 0 and plain_band > 0
    assert [it["id"] for it in vs.query(query_embeddings=Q[0], top_k=10)] == want1
    del vs
    vector_store.release_all()
    cold = GpuVectorStore(persist_dir=tmp_path, collection_name="c")
    assert cold.count() == N_STORE
    assert np.array_equal(cold._index.center(), mu)
    assert _ids(cold, Q, 10) == want and cold._index.last_band_rows() == band
    cold.delete([f"d{i}" for i in range(0, 300, 3)])
    cold.compact()
    assert (d / "center.f32").exists() and np.array_equal(cold._index.center(), mu)
    cold.recenter(clear=True)
    assert not (d / "center.f32").exists() and cold._index.center() is None
    cold.recenter(mu)
    assert (d / "center.f32").exists()
    cold.reset_collection()
    assert not (d / "center.f32").exists()
    vector_store.release_all()


def test_sharded_store_takes_one_centre(monkeypatch):
    from classmate_hip import multidev
    from classmate_hip.retrieval import GpuVectorStore
    C, Q, _, _, _ = corpus(0.8)
    C, Q = C[:N_STORE], Q[96:160]
    monkeypatch.delenv("CM_DEVICES", raising=False)
    one = GpuVectorStore(persist_dir=None)
    _fill(one, C)
    want = one.query_batch(query_embeddings=Q, top_k=10)
    mean = one._index.mean()
    monkeypatch.setenv("CM_DEVICES", "0,0,0")
    monkeypatch.setenv("CM_SHARD_BLOCK", "1024")
    sh = GpuVectorStore(persist_dir=None)
    _fill(sh, C)
    assert isinstance(sh._index, multidev.ShardedDenseIndex) and sh._index.G == 3
    before = _ids(sh, Q, 10)
    out = sh.recenter()
    assert out["rows"] == N_STORE
    mu = sh._index.center()
    assert np.abs(mu.astype(np.float64) - mean.astype(np.float64)).max() <= 1e-6
    assert all(np.array_equal(s.center(), mu) for s in sh._index.shards)
    got = sh.query_batch(query_embeddings=Q, top_k=10)
    assert [[it["id"] for it in items] for items in got] == before
    # the unsharded lists (shards this small run the exact fp32 kind: a near-tie within 1e-5 may swap)
    for a_items, b_items in zip(got, want):
        assert len(a_items) == len(b_items) == 10
        for x, y in zip(a_items, b_items):
            assert abs(x["distance"] - y["distance"]) <= 1e-5
            assert x["id"] == y["id"] or any(abs(z["distance"] - x["distance"]) < TIE and z["id"] == x["id"]
                                             for z in b_items)
    sh._index.set_center(None)
    assert all(s.center() is None for s in sh._index.shards)
