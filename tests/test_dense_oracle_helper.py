"""The oracle helper of test_gpu_dense_mutations.py / test_gpu_dense_filters.py, without a GPU: its
expected lists are oracle.ref_semantics.dense_topk_exact's over the model's live and allowed rows
(dead rows, fewer allowed rows than k, exact duplicates), and check_lists accepts exactly those."""
import numpy as np
import pytest

from oracle import ref_semantics as orc
from test_gpu_dense_mutations import Model, assert_lex_order, check_lists, expected_lists, tie_slack_share


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(7)
    n, dim = 300, 32
    emb = rng.standard_normal((n + 20, dim)).astype(np.float32)
    model = Model(dim)
    model.upsert(emb[:n], np.arange(n))
    dup = np.array([5, 17, 64, 150, 299])
    model.upsert(np.tile(emb[5], (5, 1)), dup)                  # exact duplicates
    model.upsert(np.zeros((1, dim), np.float32), [40])          # a zero vector: distance 1
    dead = np.concatenate([np.arange(0, n, 7), [17, 298]])
    model.delete(dead)
    model.delete([-1, n, n + 5])                                # out of range: nothing
    model.upsert(emb[n:n + 20], np.arange(n + 50, n + 70))      # a hole of 50 never-written rows
    Q = rng.standard_normal((6, dim)).astype(np.float32)
    Q[0] = emb[5]
    Q[1] = 0.0
    return model, Q


def _ref(model, Q, k, allow):
    ok = model.live if allow is None else model.live & allow
    return orc.dense_topk_exact(model.vecs, Q, k, ok)


@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("filt", ["none", "dense", "few", "nothing"])
def test_expected_lists_are_the_reference_oracle(case, k, filt):
    model, Q = case
    n = model.size
    assert n == 370 and not model.live[300:350].any() and not model.vecs[300:350].any()
    allow = {"none": None, "dense": np.arange(n) % 3 != 1, "few": np.isin(np.arange(n), [5, 17, 64, 0, 320, 360]),
             "nothing": np.zeros(n, bool)}[filt]
    rows, dists = expected_lists(model, Q, k, allow)
    r_rows, r_dists = _ref(model, Q, k, allow)
    for i in range(Q.shape[0]):
        assert np.array_equal(rows[i], r_rows[i]) and np.array_equal(dists[i], r_dists[i]), i
    if filt == "few":                                           # 5, 64 and 360 are live: three entries, then pads
        assert all(len(r) == 3 for r in rows) and rows[0][:2].tolist() == [5, 64]
    if filt == "none":                                          # the duplicates tie: lower row first
        assert rows[0][:4].tolist() == [5, 64, 150, 299]
    # check_lists accepts the oracle's own lists (fp32 distances, -1 / 0.0 pads) ...
    dist = np.zeros((Q.shape[0], k), np.float32)
    out = np.full((Q.shape[0], k), -1, np.int64)
    for i in range(Q.shape[0]):
        out[i, :len(rows[i])] = rows[i]
        dist[i, :len(rows[i])] = dists[i]
    pad = np.zeros_like(dist)
    check_lists(dist, out, model, Q, k, allow, pad_ref=pad)
    # ... and rejects a dead or filtered row, a missing neighbour, a wrong pad and a list out of order
    if len(rows[2]) >= 2:
        bad = out.copy()
        bad[2, 0] = 0                                           # row 0 is dead
        with pytest.raises(AssertionError):
            check_lists(dist, bad, model, Q, k, allow, pad_ref=pad)
        bad_r, bad_d = out.copy(), dist.copy()
        bad_r[2, :2], bad_d[2, :2] = out[2, 1::-1], dist[2, 1::-1]
        with pytest.raises(AssertionError):
            assert_lex_order(bad_d, bad_r)
        bad_r, bad_d = out.copy(), dist.copy()
        m = len(rows[2])
        bad_r[2, :m - 1], bad_d[2, :m - 1] = out[2, 1:m], dist[2, 1:m]
        bad_r[2, m - 1], bad_d[2, m - 1] = -1, 0.0              # the nearest neighbour dropped
        with pytest.raises(AssertionError):
            check_lists(bad_d, bad_r, model, Q, k, allow, pad_ref=pad)
    if len(rows[2]) < k:
        bad = dist.copy()
        bad[2, -1] = 1.0
        with pytest.raises(AssertionError):
            check_lists(bad, out, model, Q, k, allow, pad_ref=pad)


def test_tie_slack_share_counts_the_tied_positions(case):
    model, Q = case
    assert tie_slack_share(model, Q[2:], 10) == 0.0             # random directions: no gap under 1e-5
    assert tie_slack_share(model, Q[:1], 10) == pytest.approx(0.4)   # the four live duplicates of query 0
    assert tie_slack_share(model, Q[1:2], 10) == 1.0            # the zero query ties every row at 1
