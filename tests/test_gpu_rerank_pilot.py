"""K1q re-rank's pilot bound (cm_dense_q8.inc, dense_rerank_q8_kernel step 3'): the int8 band is cut at
the k-th exact distance of the k rows with the smallest upper bounds instead of at kth_up.  It changes
which rows the fp64 stage re-scores and nothing else, so every list must equal the one $CM_K1Q_PILOT=0
gives (the band from kth_up alone) bit for bit, on a prefix-plane store (where the pilot runs) and on a
full-plane store, on K1q and K1q-s, with filters, deletes, ties on the bound and the wide re-rank; and
the band-row counter (last_band_rows) must never grow with it."""
import numpy as np
import pytest

from test_gpu_scale import TIE, check_dense, exact_topk, mixed_queries, unit_rows

pytestmark = pytest.mark.gpu

Q8, Q8S = 5, 6
N, DIM = 40_000, 768
CASES = ((256, 24), (40, 10), (33, 32), (16, 24), (1, 1))


def _index(monkeypatch, mode, C):
    from classmate_hip import engine
    monkeypatch.setenv("CM_DENSE_F16", mode)
    idx = engine.DenseIndex(DIM, capacity=C.shape[0])
    idx.upsert(C, np.arange(C.shape[0], dtype=np.int64))
    monkeypatch.delenv("CM_DENSE_F16")
    return idx


def _search(monkeypatch, idx, Q, k, pilot, allow=None):
    """One host search with the pilot on / off -> (dist, rows, band rows, exact re-runs, wide re-ranks)."""
    if not pilot:
        monkeypatch.setenv("CM_K1Q_PILOT", "0")
    try:
        d, r = idx.search(Q, k, allow)
    finally:
        monkeypatch.delenv("CM_K1Q_PILOT", raising=False)
    return d, r, idx.last_band_rows(), idx.last_fallbacks(), idx.last_wide_reranks()


def _words(allow):
    return np.packbits(allow, bitorder="little").view(np.uint32)


@pytest.fixture(scope="module")
def data():
    C = unit_rows(N, DIM, seed=711)
    Q = mixed_queries(C, 256, seed=712)
    o_d, o_r = exact_topk(C, Q, 32 + 40)
    return C, Q, o_d, o_r


def test_pilot_on_equals_pilot_off(data, monkeypatch):
    C, Q, o_d, o_r = data
    pre, full = _index(monkeypatch, "prefix", C), _index(monkeypatch, "full", C)
    try:
        for nq, k in CASES:
            want = Q8 if nq > 32 else Q8S
            assert pre.search_kind(nq, k) == want and full.search_kind(nq, k) == want
            lists = {}
            for name, idx in (("prefix", pre), ("full", full)):
                d1, r1, b1, fb1, _ = _search(monkeypatch, idx, Q[:nq], k, True)
                d0, r0, b0, fb0, _ = _search(monkeypatch, idx, Q[:nq], k, False)
                print(f"{name} nq={nq} k={k}: band rows pilot on {b1} off {b0}")
                assert fb1 == 0 and fb0 == 0
                for d, r in ((d1, r1), (d0, r0)):
                    check_dense(d, r, o_d[:nq, :k + 40], o_r[:nq, :k + 40], k)
                assert np.array_equal(r1, r0) and np.array_equal(d1, d0), (name, nq, k)
                assert 0 < b1 <= b0, (name, nq, k, b1, b0)
                if name == "prefix" and (nq, k) == (256, 24):
                    assert b1 < b0
                lists[name] = (d1, r1)
            assert np.array_equal(lists["prefix"][1], lists["full"][1])
            assert np.array_equal(lists["prefix"][0], lists["full"][0]), (nq, k)
    finally:
        pre.close()
        full.close()


@pytest.mark.parametrize("n_allowed", [7, 10])
def test_fewer_candidates_than_k_and_exactly_k(data, monkeypatch, n_allowed):
    C, Q, _, _ = data
    k = 10
    keep = np.random.default_rng(713).choice(N, n_allowed, replace=False)
    allow = np.zeros(N, bool)
    allow[keep] = True
    o_d, o_r = exact_topk(C[np.sort(keep)], Q[:40], n_allowed)
    o_r = np.sort(keep)[o_r]
    pre = _index(monkeypatch, "prefix", C)
    try:
        for nq in (40, 16):
            d1, r1, b1, fb1, _ = _search(monkeypatch, pre, Q[:nq], k, True, _words(allow))
            d0, r0, b0, fb0, _ = _search(monkeypatch, pre, Q[:nq], k, False, _words(allow))
            assert fb1 == 0 and fb0 == 0 and b1 <= b0
            assert np.array_equal(r1, r0) and np.array_equal(d1, d0)
            assert np.array_equal(r1[:, :n_allowed], o_r[:nq]), nq
            np.testing.assert_allclose(d1[:, :n_allowed], o_d[:nq], atol=1e-4)
            assert (r1[:, n_allowed:] == -1).all() and (d1[:, n_allowed:] == 0).all()
    finally:
        pre.close()


@pytest.mark.parametrize("layout", ["scattered", "groups"])
def test_ties_on_the_bound(data, monkeypatch, layout):
    """300 identical rows (more than the pilot's 256 slots) and 40 identical rows (the pilot holds
    ties): exact ties go lower row first.  Scattered rows share their embedding but not their 16-row
    scale group, so their upper bounds differ in the last bits; "groups" plants 19 whole scale groups
    (304 rows: one scale, one code, one upper bound), the mass tie that leaves the pilot out."""
    C0, Q0, _, _ = data
    k, nq = 10, 40
    rng = np.random.default_rng(714)
    C = C0.copy()
    e = unit_rows(2, DIM, seed=715)
    at = rng.choice(N, 340, replace=False)
    big, small = np.sort(at[:300]), np.sort(at[300:])
    if layout == "groups":      # scale group G = rows 64 (G >> 2) + 16 (i >> 2) + 4 (G & 3) + (i & 3), i < 16
        G = rng.choice(N // 16, 19, replace=False)
        i = np.arange(16)
        big = np.sort((((G >> 2) * 64 + 4 * (G & 3))[:, None] + (16 * (i >> 2) + (i & 3))[None, :]).ravel())
        small = np.sort(rng.choice(np.setdiff1d(np.arange(N), big), 40, replace=False))
    C[big], C[small] = e[0], e[1]
    Q = Q0[:nq].copy()
    Q[:4], Q[4:8] = e[0], e[1]
    o_d, o_r = exact_topk(C, Q, k + 400)
    assert (o_d[:, -1] > o_d[:, k - 1] + TIE).all()     # check_dense's slack, before any GPU work
    for idx_mode in ("prefix", "full"):
        idx = _index(monkeypatch, idx_mode, C)
        try:
            d1, r1, b1, fb1, _ = _search(monkeypatch, idx, Q, k, True)
            d0, r0, b0, fb0, _ = _search(monkeypatch, idx, Q, k, False)
            assert fb1 == 0 and fb0 == 0 and b1 <= b0
            check_dense(d1, r1, o_d, o_r, k)
            assert np.array_equal(r1, r0) and np.array_equal(d1, d0), idx_mode
            assert (r1[:4] == big[:k]).all() and (r1[4:8] == small[:k]).all()
            assert (d1[:8] == d1[:8, :1]).all()
        finally:
            idx.close()


def test_deletes_plus_a_filter(data, monkeypatch):
    C, Q, _, _ = data
    pre, full = _index(monkeypatch, "prefix", C), _index(monkeypatch, "full", C)
    try:
        Q = Q[:64]
        _, r = pre.search(Q, 10)
        drop = np.unique(r[:, :2].ravel())
        allow = np.ones(N, bool)
        allow[1::3] = False
        for idx in (pre, full):
            idx.delete(drop)
        d1, r1, b1, fb1, _ = _search(monkeypatch, pre, Q, 10, True, _words(allow))
        d0, r0, b0, fb0, _ = _search(monkeypatch, pre, Q, 10, False, _words(allow))
        df, rf, _, fbf, _ = _search(monkeypatch, full, Q, 10, True, _words(allow))
        assert fb1 == 0 and fb0 == 0 and fbf == 0 and b1 <= b0
        assert np.array_equal(r1, r0) and np.array_equal(d1, d0)
        assert np.array_equal(r1, rf) and np.array_equal(d1, df)
        assert (r1 >= 0).all() and not np.isin(r1, drop).any() and allow[r1].all()
    finally:
        pre.close()
        full.close()


def test_wide_path(monkeypatch):
    """A scattered 5 000-row cluster within 5e-4 of one row: the band exceeds the re-rank's LDS with or
    without the pilot (the bounds' width is ~30x the cluster's), so the wide re-rank finishes the
    cluster's queries from the pilot's tighter bound."""
    rng = np.random.default_rng(716)
    C = unit_rows(60_000, DIM, seed=717)
    base = C[7].astype(np.float64)
    at = rng.choice(np.arange(8, 60_000), 5_000, replace=False)
    d_c = rng.permutation(np.linspace(1e-5, 5e-4, at.size))
    u = rng.standard_normal((at.size, DIM))
    u -= np.outer(u @ base, base)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t = np.sqrt(2.0 * d_c - d_c ** 2)
    C[at] = (np.sqrt(1.0 - t ** 2)[:, None] * base + t[:, None] * u).astype(np.float32)
    nq, k = 40, 24
    Q = mixed_queries(C, nq, seed=718)
    Q[:4] = (base + 1e-4 * rng.standard_normal((4, DIM)) / np.sqrt(DIM)).astype(np.float32)
    o_d, o_r = exact_topk(C, Q, k + 900)
    idx = _index(monkeypatch, "prefix", C)
    try:
        d1, r1, _, fb1, w1 = _search(monkeypatch, idx, Q, k, True)
        d0, r0, _, fb0, w0 = _search(monkeypatch, idx, Q, k, False)
        print(f"wide re-ranks pilot on {w1} off {w0}, exact re-runs {fb1} / {fb0}")
        check_dense(d1, r1, o_d, o_r, k)
        assert w1 >= 1
        assert np.array_equal(r1, r0) and np.array_equal(d1, d0)
    finally:
        idx.close()


def test_candidates_beyond_the_gather_capacity(monkeypatch):
    """More candidates than the re-rank gathers into LDS (4 096), a band that fits: the pilot rows are
    then told by their upper bounds in the global buffers, not by a mark in LDS.  A 4 500-row cluster at
    distances 0.01 .. 0.5 of one row, none of it among the first eighth of the rows (the seed sample is
    the first sixteenth): every row whose exact distance is at most the k-th smallest exact distance of
    the sample's rows is a candidate (lo <= d, and the seed is at least that distance), and the CPU
    count of those rows is above 4 096 before the GPU is asked."""
    n, n_c, k = 60_000, 4_500, 24
    rng = np.random.default_rng(719)
    C = unit_rows(n, DIM, seed=720)
    base = unit_rows(1, DIM, seed=721)[0].astype(np.float64)
    at = rng.choice(np.arange(n // 8, n), n_c, replace=False)
    d_c = rng.permutation(np.linspace(0.01, 0.5, n_c))
    u = rng.standard_normal((n_c, DIM))
    u -= np.outer(u @ base, base)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t = np.sqrt(2.0 * d_c - d_c ** 2)
    C[at] = (np.sqrt(1.0 - t ** 2)[:, None] * base + t[:, None] * u).astype(np.float32)
    Q = mixed_queries(C, 40, seed=722)
    Q[:4] = (base + 1e-3 * rng.standard_normal((4, DIM)) / np.sqrt(DIM)).astype(np.float32)
    Cn = C.astype(np.float64)
    Cn /= np.linalg.norm(Cn, axis=1, keepdims=True)
    D = 1.0 - Cn @ (Q[:4].astype(np.float64) / np.linalg.norm(Q[:4].astype(np.float64), axis=1, keepdims=True)).T
    seed_lb = np.sort(D[:n // 8], axis=0)[k - 1]
    assert ((D <= seed_lb).sum(axis=0) > 4096).all(), (D <= seed_lb).sum(axis=0)
    o_d, o_r = exact_topk(C, Q, k + 40)
    idx = _index(monkeypatch, "prefix", C)
    try:
        for nq in (40, 16):
            d1, r1, b1, fb1, w1 = _search(monkeypatch, idx, Q[:nq], k, True)
            d0, r0, b0, fb0, w0 = _search(monkeypatch, idx, Q[:nq], k, False)
            print(f"nq={nq}: band rows pilot on {b1} off {b0}")
            assert fb1 == 0 and fb0 == 0 and w1 == 0 and w0 == 0      # every band fitted in LDS
            check_dense(d1, r1, o_d[:nq], o_r[:nq], k)
            assert np.array_equal(r1, r0) and np.array_equal(d1, d0), nq
            assert b1 < b0
    finally:
        idx.close()


def test_device_entry_counter(data, monkeypatch):
    import torch
    C, Q, _, _ = data
    pre = _index(monkeypatch, "prefix", C)
    try:
        for nq, k in ((256, 24), (16, 24)):
            _, rh, bh, _, _ = _search(monkeypatch, pre, Q[:nq], k, True)
            ws = torch.empty(pre.workspace_bytes(nq, k), dtype=torch.uint8, device="cuda")
            q = torch.from_numpy(Q[:nq]).cuda()
            for _ in range(2):                       # the second search re-zeroes the counter
                _, rd = pre.search_dev(q, k, workspace=ws)
                torch.cuda.synchronize()
                assert pre.workspace_band_rows(nq, k, ws) == bh > 0
                assert np.array_equal(rd.cpu().numpy(), rh)
    finally:
        pre.close()
