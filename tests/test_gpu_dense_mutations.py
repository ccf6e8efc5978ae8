"""Rows that change after they were written, on every scan kind of the dense index.

The dense index keeps five derived copies of a row (the fp32 row, invc, the f16 plane Xh, the int8
plane Xq with its per-16-row-group scale in rmeta, the running maxima in rnorm).  The coarse kinds
(K1c 3, K1s 4, K1q 5, K1q-s 6) scan only the derived copies: a stale plane, a stale scale or a bound
that is too small drops a true neighbour before the exact re-rank sees it.  Every case here mutates
an index and a numpy model of it in step, then checks every kind against the exact fp64 oracle of
the model (check_lists), against a fresh index built from the model's final state (like_fresh), and
the assertions that carry the case on planted vectors whose rank is known by construction.

Bars (the project's): distances within 1e-4 of the exact fp64 1 - cos, sets equal except rows within
1e-5 of the k-th exact distance, order strict where exact neighbours differ by more than 1e-5; against
a fresh index rows equal, distances bit-equal on the fp32 kind and within 1e-6 on the coarse kinds
(only the never-lowered rnorm maxima may differ); export equal to the model byte for byte.

Seed samples at 20 480 rows of dim 768 (coarse_config in cm_dense.hip: rows_end_sample =
round_up(rows_end / frac, 64), frac = 32 for K1q-s and 16 for K1q, K1c and K1s below 1M rows): rows
[0, 640) are inside every kind's sample, rows >= 1 280 outside every sample; 1 280 rows is also the
f16 prefix of a CM_DENSE_F16=prefix store of this size.  The cases use rows < 512 as "inside every
sample" and rows >= 4 096 as "outside every sample" (the holes / growth cases change rows_end by
under 2 000 rows, which moves neither).  The sample is 64-row groups: 20 of them (10 for K1q-s), so
at k = 24 dense_seed_kernel's seed is +inf at this size and every live row is a candidate: K1c and
K1s overflow their 64-slot buffers and finish every query in the exact fp32 pass, K1q and K1q-s hold
a whole range in their 128 slots and certify from the complete set; k = 10 runs the seeded route.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_scale import DIST_TOL, TIE, unit_rows

pytestmark = pytest.mark.gpu

D, N = 768, 20480
F32, COARSE, STREAM, Q8, Q8S = 1, 3, 4, 5, 6
KINDS = [F32, COARSE, STREAM, Q8, Q8S]
AUTO, AUTO16 = 0, 2               # automatic; 2 (the retired K1b) also means automatic: used for the 16-query searches
STREAM_KINDS = (STREAM, Q8S, AUTO16)
KS = (10, 24)
SLACK_CAP = 0.02
NOISE = 0.01            # planted vectors: 1 - cos ~ 5e-5 to their query, the next neighbour ~ 0.85


# ---------------------------------------------------------------------------
# the numpy model of the store and the oracle over it (no GPU, no package import)
# ---------------------------------------------------------------------------
class Model:
    """row -> fp32 vector plus a live mask; `size` is the high-water row count, as in the index.
    A deleted row keeps its vector (the index only clears its live bit); never-written, reset and
    truncated rows are zero and not live."""

    def __init__(self, dim):
        self.dim = dim
        self.vecs = np.zeros((0, dim), np.float32)
        self.live = np.zeros(0, bool)
        self._cache = {}

    @property
    def size(self):
        return self.vecs.shape[0]

    def upsert(self, vecs, rows):
        rows = np.asarray(rows, np.int64)
        assert np.unique(rows).shape[0] == rows.shape[0]
        need = int(rows.max()) + 1
        if need > self.size:
            grow = need - self.size
            self.vecs = np.concatenate([self.vecs, np.zeros((grow, self.dim), np.float32)])
            self.live = np.concatenate([self.live, np.zeros(grow, bool)])
        self.vecs[rows] = np.asarray(vecs, np.float32)
        self.live[rows] = True
        self._cache = {}

    def delete(self, rows):
        rows = np.asarray(rows, np.int64)
        self.live[rows[(rows >= 0) & (rows < self.size)]] = False
        self._cache = {}

    def reset(self):
        self.truncate(0)

    def truncate(self, n):
        self.vecs, self.live = self.vecs[:n].copy(), self.live[:n].copy()
        self._cache = {}

    def compact(self):
        keep = np.nonzero(self.live)[0]
        self.vecs, self.live = self.vecs[keep].copy(), np.ones(keep.shape[0], bool)
        self._cache = {}
        return keep

    def live_rows(self):
        return np.nonzero(self.live)[0]


def exact_dist(model, Q, allow=None):
    """(nq, size) exact fp64 1 - q.c / (|q| |c|); +inf at rows that are dead or not allowed.  A zero
    vector is at distance 1 of everything (oracle.ref_semantics.dense_topk_exact's convention)."""
    c = model.vecs.astype(np.float64)
    q = np.atleast_2d(Q).astype(np.float64)
    cn = np.linalg.norm(c, axis=1)
    cn[cn == 0] = np.inf
    qn = np.linalg.norm(q, axis=1, keepdims=True)
    qn[qn == 0] = np.inf
    d = 1.0 - (q @ c.T) / qn / cn[None, :]
    ok = model.live.copy()
    if allow is not None:
        ok &= np.asarray(allow, bool)[:model.size]
    d[:, ~ok] = np.inf
    return d


ORACLE_DEPTH = 40                 # rows per query the oracle orders (> max k + 1)


def _oracle(model, Q, allow=None):
    """(dist matrix, per query its first ORACLE_DEPTH rows by (distance, row)), computed once per
    model state.  Every row tied with the last one kept is ordered too, so ties go to the lower row."""
    key = (hash(np.ascontiguousarray(Q).tobytes()), None if allow is None else hash(np.asarray(allow, bool).tobytes()))
    if key not in model._cache:
        d = exact_dist(model, Q, allow)
        order = []
        for i in range(d.shape[0]):
            if d.shape[1] > ORACLE_DEPTH:
                cand = np.nonzero(d[i] <= np.partition(d[i], ORACLE_DEPTH)[ORACLE_DEPTH])[0]
            else:
                cand = np.arange(d.shape[1])
            order.append(cand[np.argsort(d[i, cand], kind="stable")][:ORACLE_DEPTH])
        model._cache[key] = (d, order)
    return model._cache[key]


def expected_lists(model, Q, k, allow=None):
    """Per query the exact list: rows of the model that are live and allowed, ascending exact fp64
    distance, ties -> lower row, at most k of them.  Returns (rows, dists), lists of arrays."""
    d, order = _oracle(model, Q, allow)
    rows, dists = [], []
    for i in range(d.shape[0]):
        o = order[i][:k]
        o = o[np.isfinite(d[i, o])]
        rows.append(o)
        dists.append(d[i, o])
    return rows, dists


def tie_slack_share(model, Q, k, allow=None):
    """Share of the (query, rank) positions of the expected lists that check_lists' tie slack could
    cover: positions with another live and allowed row within TIE of their exact distance (the row
    after the k-th included).  From the oracle alone."""
    d, order = _oracle(model, Q, allow)
    n_pos = n_slack = 0
    for i in range(d.shape[0]):
        o = order[i][:k + 1]
        v = d[i, o]
        v = v[np.isfinite(v)]
        m = min(k, v.shape[0])
        if m == 0:
            continue
        gap = np.diff(v) <= TIE
        near = np.zeros(v.shape[0], bool)
        near[:-1] |= gap
        near[1:] |= gap
        n_pos += m
        n_slack += int(near[:m].sum())
    return n_slack / max(n_pos, 1)


def assert_lex_order(dist, rows):
    """cm_dense_search's contract: every list ascends in (distance, row) over its non-pad entries."""
    for i in range(rows.shape[0]):
        m = int((rows[i] >= 0).sum())
        assert (rows[i, :m] >= 0).all() and (rows[i, m:] == -1).all(), i
        dd, rr = dist[i, :m], rows[i, :m]
        bad = (dd[1:] < dd[:-1]) | ((dd[1:] == dd[:-1]) & (rr[1:] <= rr[:-1]))
        assert not bad.any(), (i, np.nonzero(bad)[0], dd, rr)


def check_lists(dist, rows, model, Q, k, allow=None, pad_ref=None):
    """GPU lists (possibly shorter than k) against the exact fp64 lists over the model's live and
    allowed rows: distances within DIST_TOL, sets equal except rows within TIE of the k-th exact
    distance, order strict where exact neighbours differ by more than TIE; entries past m = min(k,
    live allowed rows) are row -1 with the pad distance of the fp32 kind's output for the same search
    (pad_ref); every list ascends in (distance, row)."""
    assert k < ORACLE_DEPTH
    d_all, _ = _oracle(model, Q, allow)
    o_rows, o_dist = expected_lists(model, Q, k, allow)
    assert dist.shape == rows.shape == (d_all.shape[0], k)
    assert_lex_order(dist, rows)
    for i in range(rows.shape[0]):
        m = len(o_rows[i])
        got = rows[i, :m]
        assert (got >= 0).all() and (rows[i, m:] == -1).all(), (i, m, rows[i])
        if m < k:
            assert pad_ref is not None, "a padded list needs the fp32 kind's output"
            assert dist[i, m:].tobytes() == np.asarray(pad_ref, np.float32)[i, m:].tobytes(), (i, dist[i, m:])
        if m == 0:
            continue
        assert np.unique(got).shape[0] == m and got.max() < model.size, (i, got)
        own = d_all[i, got]
        assert np.isfinite(own).all(), (i, got[~np.isfinite(own)])          # live and allowed rows only
        np.testing.assert_allclose(dist[i, :m], own, rtol=0, atol=DIST_TOL)
        np.testing.assert_allclose(dist[i, :m], o_dist[i], rtol=0, atol=DIST_TOL)
        if m == k:
            kth = o_dist[i][-1]
            unsure = set(np.nonzero(np.abs(d_all[i] - kth) < TIE)[0].tolist())
            assert set(got.tolist()) ^ set(o_rows[i].tolist()) <= unsure, i
        else:
            assert set(got.tolist()) == set(o_rows[i].tolist()), i
        for j in np.nonzero(np.diff(o_dist[i]) > TIE)[0]:
            assert got[j] == o_rows[i][j] or abs(dist[i, j] - o_dist[i][j]) < TIE, (i, j)


# ---------------------------------------------------------------------------
# searches: one forced kind, host entry and the two device entries
# ---------------------------------------------------------------------------
def q8_group_of(row):
    return (row >> 6) * 4 + ((row >> 2) & 3)


def q8_group_rows(G):
    """The 16 rows of scale group G (cm_dense_q8.inc q8_group_row)."""
    return np.array([(G >> 2) * 64 + 16 * (i >> 2) + 4 * (G & 3) + (i & 3) for i in range(16)], np.int64)


def _bits(mask):
    n = mask.shape[0]
    words = np.zeros((n + 31) // 32, np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def queries_of(kind, Q):
    """The stream kinds take nq = 16 per search (the first 32 queries, two searches), the batched
    kinds and the fp32 kind the whole batch (64, or 300 = two passes of 256)."""
    return Q[:32] if kind in STREAM_KINDS else Q


def host_lists(idx, kind, Q, k, words=None, expect=None):
    """idx.search on the forced kind -> (dist, rows, fallbacks, wide re-ranks); asserts the kind that
    runs (expect: what a store that cannot take the kind runs instead)."""
    step = 16 if kind in STREAM_KINDS else Q.shape[0]
    ds, rs, fb, wide = [], [], 0, 0
    idx.set_path(kind)
    try:
        for s in range(0, Q.shape[0], step):
            q = np.ascontiguousarray(Q[s:s + step])
            assert idx.search_kind(q.shape[0], k) == (kind if expect is None else expect), (kind, q.shape[0], k)
            d, r = idx.search(q, k, words)
            assert idx.last_fallbacks() >= 0
            fb += idx.last_fallbacks()
            wide += max(idx.last_wide_reranks(), 0)
            ds.append(d)
            rs.append(r)
    finally:
        idx.set_path(0)
    return np.concatenate(ds), np.concatenate(rs), fb, wide


def device_lists(idx, kind, Q, k, words_dev=None, expect=None):
    """search_dev, and search_dev(defer_exact=True) + exact_fallback_dev (what device_batch.py
    enqueues), on the forced kind -> two (dist, rows) pairs of host arrays."""
    import torch
    step = 16 if kind in STREAM_KINDS else Q.shape[0]
    one, two = ([], []), ([], [])
    idx.set_path(kind)
    try:
        for s in range(0, Q.shape[0], step):
            q = torch.from_numpy(np.ascontiguousarray(Q[s:s + step])).cuda()
            assert idx.search_kind(q.shape[0], k) == (kind if expect is None else expect)
            d, r = idx.search_dev(q, k, allow=words_dev)
            torch.cuda.synchronize()
            one[0].append(d.cpu().numpy())
            one[1].append(r.cpu().numpy())
            out = idx.search_dev(q, k, allow=words_dev, defer_exact=True)
            idx.exact_fallback_dev(q, k, out, allow=words_dev)
            torch.cuda.synchronize()
            two[0].append(out[0].cpu().numpy())
            two[1].append(out[1].cpu().numpy())
    finally:
        idx.set_path(0)
    return (np.concatenate(one[0]), np.concatenate(one[1])), (np.concatenate(two[0]), np.concatenate(two[1]))


def words_dev_of(words):
    import torch
    return None if words is None else torch.from_numpy(words.view(np.int32).copy()).cuda()


def verify(tag, idx, model, Q, ks=KS, kinds=KINDS, allow=None, device=True, expect=None, slack_from=0):
    """Every kind (the fp32 kind first: its output is the pad reference) and both entries against
    the oracle; the tie-slack share of the expected lists (queries slack_from..) stays under 2 %.
    Prints the route counters.  Returns {(kind, k): (dist, rows, fallbacks, wide)}."""
    words = None if allow is None else _bits(np.asarray(allow, bool))
    wdev = words_dev_of(words) if device else None
    out = {}
    for k in ks:
        share = tie_slack_share(model, Q[slack_from:], k, allow)
        assert share <= SLACK_CAP, (tag, k, share)
        d1, r1, _, _ = host_lists(idx, F32, Q, k, words)
        for kind in [F32] + [x for x in kinds if x != F32]:
            ex = None if expect is None else expect.get(kind)
            Qk = queries_of(kind, Q)
            d, r, fb, wide = (d1, r1, 0, 0) if kind == F32 else host_lists(idx, kind, Qk, k, words, ex)
            print(f"\n[{tag}] kind {kind} k {k} nq {Qk.shape[0]}: fallbacks {fb}, wide re-ranks {wide}, "
                  f"tie-slack share {share:.4f}", end="")
            check_lists(d, r, model, Qk, k, allow, pad_ref=d1[:Qk.shape[0]])
            if allow is not None:          # the same filter as a device tensor through the host entry
                idx.set_path(kind)
                try:
                    q = np.ascontiguousarray(Qk[:16] if kind in STREAM_KINDS else Qk)
                    dt, rt = idx.search(q, k, wdev if wdev is not None else words)
                finally:
                    idx.set_path(0)
                assert np.array_equal(rt, r[:q.shape[0]]) and np.array_equal(dt, d[:q.shape[0]]), (tag, kind, k)
            if device:
                for name, (dd, rd) in zip(("search_dev", "deferred"), device_lists(idx, kind, Qk, k, wdev, ex)):
                    assert np.array_equal(rd, r) and np.array_equal(dd, d), (tag, kind, k, name)
            out[kind, k] = (d, r, fb, wide)
    return out


def assert_export(idx, model):
    assert idx.size == model.size and idx.live_count() == int(model.live.sum())
    if model.size == 0:
        return
    out, live = idx.export(with_live=True)
    assert np.array_equal(live, model.live)
    assert out.tobytes() == model.vecs.tobytes()


def like_fresh(idx, model, Q, k, kinds, expect=None):
    """The mutated index against a fresh index built from the model's final state with one upsert:
    rows equal, distances bit-equal on the fp32 kind and within 1e-6 on the coarse kinds; export, size
    and live_count equal to the model."""
    from classmate_hip import engine
    assert_export(idx, model)
    rows = model.live_rows()
    fresh = engine.DenseIndex(model.dim)
    try:
        fresh.upsert(model.vecs[rows], rows)
        for kind in kinds:
            ex = None if expect is None else expect.get(kind)
            Qk = queries_of(kind, Q)
            d, r, fb, _ = host_lists(idx, kind, Qk, k, None, ex)
            dw, rw, fbw, _ = host_lists(fresh, kind, Qk, k, None, ex)
            assert np.array_equal(r, rw), (kind, k)
            if kind == F32:
                assert d.tobytes() == dw.tobytes(), (kind, k)
            else:
                err = float(np.abs(d.astype(np.float64) - dw).max())
                print(f"\n[like_fresh] kind {kind} k {k}: max |d - d_fresh| = {err:.3g}, fallbacks {fb} (fresh {fbw})",
                      end="")
                assert err <= 1e-6, (kind, k, err)
    finally:
        fresh.close()


def near(v, rng, noise=NOISE):
    """v + small noise: 1 - cos ~ noise^2 / 2, far above TIE below the next neighbour's ~0.85."""
    v = np.asarray(v, np.float32)
    g = rng.standard_normal(v.shape).astype(np.float32)
    scale = np.linalg.norm(v, axis=-1, keepdims=True) / np.sqrt(v.shape[-1])
    return (v + noise * scale * g).astype(np.float32)


def gauss(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# ---------------------------------------------------------------------------
# the base store and case 1's overwrites (shared with the prefix and the sharded case)
# ---------------------------------------------------------------------------
OLD_ROWS = np.array([3, 200, 511, 700, 1279, 1280, 4096, 5000, 7777, 9001, 11111, 13000, 15000, 17000, 19000, 20400])
G_ALL = q8_group_of(9000)         # every row of this scale group is overwritten (9001 among them)
ROW_ALONE = 12345                 # the only overwritten row of its scale group


def pick_queries(C, nq, seed, k=max(KS)):
    """nq random directions, taken in order from a seeded Gaussian pool, whose exact top-(k + 1) over
    the rows C holds no two rows within TIE of each other.  At 20 480 x 768 about 2 % of the
    (query, rank) positions of unselected Gaussian queries sit in such a tie at k = 24 -- the whole
    tie-slack budget -- so the choice of queries, made from the oracle alone, keeps the slack for the
    few ties that the mutations and the planted queries bring."""
    pool = gauss(3 * nq + 32, C.shape[1], seed)
    m = Model(C.shape[1])
    m.upsert(C, np.arange(C.shape[0]))
    d = exact_dist(m, pool)
    top = np.sort(np.partition(d, k + 1, axis=1)[:, :k + 2], axis=1)[:, :k + 1]
    clean = (np.diff(top, axis=1) > TIE).all(axis=1)
    assert clean.sum() >= nq, (clean.sum(), nq)
    return np.ascontiguousarray(pool[clean][:nq])


def near_tie_free(C, rows, seed, k=max(KS)):
    """One query near each row of `rows` (rank 0 by construction) whose exact top-(k + 1) over C holds
    no two rows within TIE, like pick_queries' random directions."""
    rng = np.random.default_rng(seed)
    m = Model(C.shape[1])
    m.upsert(C, np.arange(C.shape[0]))
    out = []
    for r in rows:
        for _ in range(50):
            q = near(C[r], rng)
            top = np.sort(np.partition(exact_dist(m, q)[0], k + 1)[:k + 2])[:k + 1]
            if (np.diff(top) > TIE).all():
                break
        else:
            raise AssertionError(f"no tie-free query near row {r}")
        out.append(q)
    return np.stack(out)


def base_store(n, seed, nq=64):
    """(C, Q): n unit Gaussian rows and nq queries (pick_queries); row OLD_ROWS[j] is then planted as
    rank 0 of query 16 + j."""
    C = unit_rows(n, D, seed=seed)
    Q = pick_queries(C, nq, seed + 1)
    C[OLD_ROWS] = near(Q[16:32], np.random.default_rng(seed + 2))
    return C, Q


def case1_overwrites(n, Q, seed):
    """~500 scattered rows with new vectors: row 0, row n - 1, all 16 rows of group G_ALL, exactly one
    row of ROW_ALONE's group, rows inside (< 512) and outside (>= 4096) every seed sample, OLD_ROWS
    (the planted rank 0 of queries 16..31, gone afterwards); the first 16 are planted as rank 0 of
    queries 0..15.  Returns (rows, vecs, planted rows)."""
    rng = np.random.default_rng(seed)
    planted = np.array([0, n - 1, 100, int(q8_group_rows(G_ALL)[0]), ROW_ALONE, 300, 640, 1000, 4095, 4097, 6000,
                        10000, 14000, 16383, 16384, 18000])
    alone = q8_group_rows(q8_group_of(ROW_ALONE))
    fixed = np.unique(np.concatenate([planted, OLD_ROWS, q8_group_rows(G_ALL), [5, 63, 64, 450, 511]]))
    pool = np.setdiff1d(np.arange(n), np.concatenate([fixed, alone]))
    extra = rng.choice(pool, 500 - fixed.shape[0], replace=False)
    rest = np.setdiff1d(np.concatenate([fixed, extra]), planted)
    rows = np.concatenate([planted, rng.permutation(rest)])
    assert np.isin(alone, rows).sum() == 1 and np.isin(q8_group_rows(G_ALL), rows).all()
    assert (rows < 512).sum() >= 8 and (rows >= 4096).sum() >= 300
    vecs = gauss(rows.shape[0], D, seed + 1)
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    vecs[:16] = near(Q[:16], rng)
    return rows.astype(np.int64), vecs, planted


def assert_case1_planted(res, planted):
    """Every kind: the new planted rows are rank 0 of queries 0..15, the overwritten old ones are gone
    from the lists of queries 16..31 (whose nearest row is now a random one)."""
    for (kind, k), (d, r, _, _) in res.items():
        assert (r[:16, 0] == planted).all() and (d[:16, 0] < 1e-3).all(), (kind, k)
        for j in range(16):
            assert OLD_ROWS[j] not in r[16 + j] and d[16 + j, 0] > 0.5, (kind, k, j)


@pytest.fixture(scope="module")
def base():
    C, Q = base_store(N, 501)
    Q300 = pick_queries(C, 300, 504)
    Q300[:32] = Q[:32]
    return dict(C=C, Q=Q, Q300=Q300)


def new_index(C, capacity=0):
    from classmate_hip import engine
    idx = engine.DenseIndex(C.shape[1], capacity=capacity)
    model = Model(C.shape[1])
    rows = np.arange(C.shape[0], dtype=np.int64)
    idx.upsert(C, rows)
    model.upsert(C, rows)
    return idx, model


def both(idx, model):
    """Apply one mutation to the index and to the model."""
    class _Both:
        def upsert(self, vecs, rows):
            idx.upsert(vecs, rows)
            model.upsert(vecs, rows)

        def delete(self, rows):
            idx.delete(rows)
            model.delete(rows)
    return _Both()


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def test_overwrite_in_place(base):
    """Case 1: one host upsert over ~500 live rows; every kind and entry equals the oracle, the new
    planted vectors are rank 0, the overwritten planted vectors are gone, and the index answers like a
    fresh one.  One search of 300 queries (two passes of 256) on the batched kinds."""
    C, Q = base["C"], base["Q"]
    idx, model = new_index(C)
    try:
        d, r, _, _ = host_lists(idx, Q8, Q, 10)
        assert (r[16:32, 0] == OLD_ROWS).all() and (d[16:32, 0] < 1e-3).all()        # the premise
        rows, vecs, planted = case1_overwrites(N, Q, seed=510)
        both(idx, model).upsert(vecs, rows)
        res = verify("overwrite", idx, model, Q)
        assert_case1_planted(res, planted)
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
        res = verify("overwrite nq=300", idx, model, base["Q300"], ks=(10,), kinds=[COARSE, Q8], device=False)
        assert_case1_planted(res, planted)
    finally:
        idx.close()


def test_scale_change_inside_a_group(base):
    """Case 2: in six scale groups one row becomes near one-hot (the group's scale jumps ~10x), one is
    scaled by 1e-3, one by 1e3, one becomes the zero vector.  Queries 0..11 sit near two *unchanged*
    rows of each group, 12..23 near the rescaled rows: rank 0 by construction on every kind."""
    C, Q0 = base["C"], base["Q"]
    rng = np.random.default_rng(520)
    idx, model = new_index(C)
    try:
        for kind in KINDS[1:]:                 # the base store: the certified route, no exact re-run
            _, _, fb, _ = host_lists(idx, kind, queries_of(kind, Q0), 10)
            assert fb == 0, kind
        groups = [q8_group_of(r) for r in (40, 900, 5000, 9000, 15000, 20470)]
        rows, vecs, keep, scaled = [], [], [], []
        for G in groups:
            g = q8_group_rows(G)
            hot = np.zeros(D, np.float32)
            hot[int(rng.integers(D))] = 1.0
            u = unit_rows(2, D, seed=521 + G)
            rows += [g[1], g[5], g[9], g[13]]
            vecs += [near(hot, rng), 1e-3 * u[0], 1e3 * u[1], np.zeros(D, np.float32)]
            keep += [g[0], g[14]]
            scaled += [g[5], g[9]]
        rows, vecs = np.array(rows, np.int64), np.stack(vecs).astype(np.float32)
        assert 0.99 < np.abs(vecs[0] / np.linalg.norm(vecs[0])).max() <= 1.0
        both(idx, model).upsert(vecs, rows)
        Q = Q0.copy()
        want = np.array(keep + scaled)
        Q[:24] = near(model.vecs[want], rng)
        res = verify("scale change", idx, model, Q)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:24, 0] == want).all() and (d[:24, 0] < 1e-3).all(), (kind, k)
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
    finally:
        idx.close()


def _group_mate(r):
    """Another row of r's scale group."""
    g = q8_group_rows(q8_group_of(int(r)))
    return int(g[(int(np.nonzero(g == r)[0][0]) + 5) % 16])


def delete_and_reuse(target, model, n, seed, protect=()):
    """Case 3's mutations on `target` (an index or a sharded index) and the model; rows in `protect`
    are left alone.  Returns (the case's 24 queries, the rows that stay dead, the rows that are live
    again)."""
    rng = np.random.default_rng(seed)
    m = both(target, model)
    stay = np.array([2, 130, 510, 4100, 4101, 9002, 12346, 16000])               # deleted, stay dead
    back = np.array([7, 333, 4200, 8000, 9003, 12000, 17001, n - 2])             # deleted, then re-upserted
    more = np.setdiff1d(rng.choice(np.arange(1300, n - 64), 300, replace=False),
                        np.concatenate([stay, back, np.asarray(protect, np.int64)]))
    dead = np.concatenate([stay, back, more])
    old_stay, old_back = model.vecs[stay].copy(), model.vecs[back].copy()
    m.delete(dead)
    # other rows of the same scale groups get new vectors: the groups are re-quantised, dead rows included
    other = np.unique([_group_mate(r) for r in np.concatenate([stay, back, more[:40]])])
    other = np.setdiff1d(other, np.concatenate([dead, np.asarray(protect, np.int64)]))
    m.upsert(gauss(other.shape[0], D, seed + 1), other)
    assert not model.live[dead].any()
    new_back = gauss(back.shape[0], D, seed + 2)
    m.upsert(new_back, back)
    m.delete(np.concatenate([stay[:3], more[:5]]))                                # already dead: no change
    Qc = np.concatenate([near(old_stay, rng), near(new_back, rng), near(old_back, rng)])
    return Qc, stay, back


def assert_case3(res, stay, back):
    for (kind, k), (d, r, _, _) in res.items():
        for j in range(8):
            assert stay[j] not in r[j] and d[j, 0] > 0.5, (kind, k, j)            # deleted: not found
            assert r[8 + j, 0] == back[j] and d[8 + j, 0] < 1e-3, (kind, k, j)     # live again, new vector
            assert d[16 + j, 0] > 0.5, (kind, k, j)                                # its old vector is gone


def test_delete_then_reuse(base):
    """Case 3: deleted rows stay dead on every kind although their scale group is re-quantised by an
    upsert of its other rows; re-upserted rows are live again with their new vectors only; deleting
    out-of-range and already-dead rows changes nothing."""
    C, Q0 = base["C"], base["Q"]
    idx, model = new_index(C)
    try:
        Qc, stay, back = delete_and_reuse(idx, model, N, seed=530)
        before = idx.export(with_live=True)
        idx.delete(np.array([-1, N, N + 1000, 1 << 40, stay[0]], np.int64))
        after = idx.export(with_live=True)
        assert before[0].tobytes() == after[0].tobytes() and np.array_equal(before[1], after[1])
        Q = Q0.copy()
        Q[:24] = Qc
        res = verify("delete + reuse", idx, model, Q)
        assert_case3(res, stay, back)
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
    finally:
        idx.close()


def test_upsert_dev_over_existing_rows(base):
    """Case 4: device batches at row0 % 64 == 13 over live rows, dead rows (live again) and past
    `size`; a second one past the allocation (dense_grow re-planes).  The rows of the cut tiles that
    the calls did not write keep their values (cm_dense_upsert_dev's group range g_lo..g_hi)."""
    import torch
    C, Q0 = base["C"], base["Q"]
    rng = np.random.default_rng(540)
    idx, model = new_index(C, capacity=21000)
    try:
        cap = idx.mem_stats()["bytes"]
        dead = np.arange(20000, 20100)
        both(idx, model).delete(dead)
        row0, n1 = 19981, 600                                  # [19981, 20581): live, dead, past size
        assert row0 % 64 == 13 and row0 + n1 > N
        v1 = gauss(n1, D, 541)
        idx.upsert_dev(torch.from_numpy(v1).cuda(), row0)
        torch.cuda.synchronize()
        model.upsert(v1, np.arange(row0, row0 + n1))
        assert idx.mem_stats()["bytes"] == cap                 # inside the allocation
        Q = Q0.copy()
        probe = np.array([19968, 19980, 19981, 20000, 20099, 20479, 20480, 20580, 19900, 5])
        Q[:10] = near(model.vecs[probe], rng)
        res = verify("upsert_dev 1", idx, model, Q, ks=(10,))
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:10, 0] == probe).all() and (d[:10, 0] < 1e-3).all(), (kind, k)
        like_fresh(idx, model, Q, 10, KINDS)
        row1, n2 = 20557, 1000                                 # overlaps call 1, runs past the allocation
        assert row1 % 64 == 13
        v2 = gauss(n2, D, 542)
        idx.upsert_dev(torch.from_numpy(v2).cuda(), row1)
        torch.cuda.synchronize()
        model.upsert(v2, np.arange(row1, row1 + n2))
        assert idx.mem_stats()["bytes"] > cap                  # grown
        probe = np.array([19968, 19981, 20544, 20556, 20557, 20580, 20581, 21556, 100, 12345])
        Q[:10] = near(model.vecs[probe], rng)
        res = verify("upsert_dev 2", idx, model, Q)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:10, 0] == probe).all() and (d[:10, 0] < 1e-3).all(), (kind, k)
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
    finally:
        idx.close()


def test_holes_are_never_returned(base):
    """Case 5: rows [size + 200, size + 300) are written; the 200 rows between were never written.
    No kind returns one, not for a zero query (every row at distance 1: the lists are the lowest
    live rows) nor for queries on the rows beside the hole; they export as zero and not live."""
    C, Q0 = base["C"], base["Q"]
    rng = np.random.default_rng(550)
    idx, model = new_index(C)
    try:
        rows = np.arange(N + 200, N + 300)
        both(idx, model).upsert(gauss(100, D, 551), rows)
        assert idx.size == N + 300 and idx.live_count() == N + 100
        out, live = idx.export(N, 200, with_live=True)
        assert not out.any() and not live.any()
        Q = Q0.copy()
        probe = np.array([N - 1, N + 200, N + 299, N - 64, 0])
        Q[:5] = near(model.vecs[probe], rng)
        res = verify("holes", idx, model, Q)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:5, 0] == probe).all() and (d[:5, 0] < 1e-3).all(), (kind, k)
            assert not ((r >= N) & (r < N + 200)).any(), (kind, k)
        # the zero query ties every row at distance 1: outside the tie-slack budget by construction,
        # so its own assertions are explicit (live rows only, never a hole, distance 1, (distance, row) order)
        Qz = Q0[:32].copy()
        Qz[0] = 0.0
        for k in KS:
            d1 = None
            for kind in KINDS:
                d, r, fb, wide = host_lists(idx, kind, Qz, k)
                d1 = d if kind == F32 else d1
                print(f"\n[holes, zero query] kind {kind} k {k}: fallbacks {fb}, wide re-ranks {wide}", end="")
                check_lists(d, r, model, Qz, k, pad_ref=d1)
                assert (r[0] >= 0).all() and not ((r[0] >= N) & (r[0] < N + 200)).any()
                assert np.abs(d[0] - 1.0).max() <= DIST_TOL
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
    finally:
        idx.close()


def test_reset_leaves_nothing_behind(base):
    """Case 6: reset() empties the store (every search is all pads), and a refill -- 1 000 rows on the
    fp32 kind, then 17 000 rows with a never-written hole on the coarse kinds -- answers like a fresh
    index: nothing of the old planes, scales or maxima is left."""
    import torch
    C, Q0 = base["C"], base["Q"]
    rng = np.random.default_rng(560)
    idx, model = new_index(C)
    try:
        idx.reset()
        model.reset()
        assert idx.size == 0 and idx.live_count() == 0
        for kind in KINDS:
            idx.set_path(kind)
            assert idx.search_kind(16, 10) == F32
            d, r = idx.search(Q0[:16], 10)
            assert (r == -1).all()
            check_lists(d, r, model, Q0[:16], 10, pad_ref=d)
            dd, rd = idx.search_dev(torch.from_numpy(Q0[:16]).cuda(), 10)
            torch.cuda.synchronize()
            assert (rd.cpu().numpy() == -1).all() and np.array_equal(dd.cpu().numpy(), d)
        idx.set_path(0)
        C2 = unit_rows(17000, D, seed=561)
        both(idx, model).upsert(C2[:1000], np.arange(1000))
        Q = pick_queries(C2, 64, 562)
        Q[:4] = near(C2[[0, 999, 500, 63]], rng)
        res = verify("reset, 1000 rows", idx, model, Q, kinds=[F32])
        assert (res[F32, 10][1][:4, 0] == [0, 999, 500, 63]).all()
        for kind in KINDS:
            idx.set_path(kind)
            assert idx.search_kind(16, 10) == F32 and idx.search_kind(64, 24) == F32
        idx.set_path(0)
        like_fresh(idx, model, Q, 10, [F32])
        rows = np.setdiff1d(np.arange(1000, 17000), np.arange(5000, 5100))        # [5000, 5100) stays a hole
        both(idx, model).upsert(C2[rows], rows)
        probe = np.array([0, 999, 1000, 4999, 5100, 16999, 640, 12345])
        Q[:8] = near(C2[probe], rng)
        Q[8:12] = near(C[[5000, 5050, 17000, 20479]], rng)                      # rows of the store before the reset
        res = verify("reset, 17000 rows", idx, model, Q)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:8, 0] == probe).all() and (d[:8, 0] < 1e-3).all(), (kind, k)
            assert (d[8:12, 0] > 0.5).all() and not ((r >= 5000) & (r < 5100)).any(), (kind, k)
        for k in KS:
            like_fresh(idx, model, Q, k, KINDS)
    finally:
        idx.close()


def _pattern(n, step0, tile0, tail):
    """test_gpu_compact.py's dead rows: every r % 7 == 3, a whole 128-row step, a whole 64-row tile,
    row 0 and the last `tail` rows."""
    r = np.arange(n)
    dead = r % 7 == 3
    dead[step0:step0 + 128] = True
    dead[tile0:tile0 + 64] = True
    dead[0] = True
    dead[n - tail:] = True
    return dead


def compact_and_truncate(dim, kinds, seed, expect=None, ks=KS):
    """Case 7's body: delete test_gpu_compact.py's pattern, compact in 1 000-row chunks
    (CM_COMPACT_CHUNK_ROWS, set by the caller), truncate at n % 64 == 13 above 16 384 rows; after each
    of the two the kinds equal the oracle and a fresh index."""
    from classmate_hip import engine
    rng = np.random.default_rng(seed)
    assert os.environ.get("CM_COMPACT_CHUNK_ROWS") == "1000"
    C = unit_rows(N, dim, seed=seed + 1)
    idx, model = engine.DenseIndex(dim), Model(dim)
    try:
        m = both(idx, model)
        m.upsert(C, np.arange(N))
        dead = _pattern(N, 4096, 6400, 300)
        m.delete(np.nonzero(dead)[0])
        old = idx.compact()
        assert np.array_equal(old, model.compact()) and idx.size == model.size >= 16384 + 64
        Q = pick_queries(model.vecs, 64, seed + 2)
        probe = np.array([0, 5, 600, 4000, 6000, 12000, model.size - 1, 16396])
        Q[:8] = near(model.vecs[probe], rng)
        res = verify(f"compact dim {dim}", idx, model, Q, ks=ks, kinds=kinds, expect=expect)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:8, 0] == probe).all() and (d[:8, 0] < 1e-3).all(), (kind, k)
        for k in ks:
            like_fresh(idx, model, Q, k, kinds, expect)
        n = 16397
        assert n % 64 == 13 and n < model.size
        gone = model.vecs[[n, n + 1, model.size - 1]].copy()
        idx.truncate(n)
        model.truncate(n)
        probe = np.array([0, 5, 600, 4000, 6000, 12000, n - 1, n - 13])
        Q[:8] = near(model.vecs[probe], rng)
        Q[8:11] = near(gone, rng)                                              # queries on dropped rows
        res = verify(f"truncate dim {dim}", idx, model, Q, ks=ks, kinds=kinds, expect=expect)
        for (kind, k), (d, r, _, _) in res.items():
            assert (r[:8, 0] == probe).all() and (d[:8, 0] < 1e-3).all(), (kind, k)
            assert (d[8:11, 0] > 0.5).all() and (r < n).all(), (kind, k)
        for k in ks:
            like_fresh(idx, model, Q, k, kinds, expect)
    finally:
        idx.close()


@pytest.mark.parametrize("dim,kinds", [(768, [COARSE, STREAM, Q8, Q8S]), (384, [F32, COARSE, STREAM])])
def test_compact_and_truncate_on_the_coarse_kinds(dim, kinds, monkeypatch):
    """Case 7: K1c and K1s on the f16 plane that a compaction and a truncate rebuilt, K1q and K1q-s on
    the re-quantised groups; dim 384 (ld 384: K1c and K1s only) at a size that takes the coarse scans."""
    monkeypatch.setenv("CM_COMPACT_CHUNK_ROWS", "1000")
    compact_and_truncate(dim, kinds, seed=570 + dim)


def q8_off_child():
    """The body of test_compact_and_truncate_with_q8_off, in a process started with CM_DENSE_Q8=0
    (dense_kind reads it once per process): the automatic kinds are K1c (64 queries) and K1s (16 queries)."""
    assert os.environ.get("CM_DENSE_Q8") == "0"
    compact_and_truncate(768, [AUTO, AUTO16], seed=580, expect={AUTO: COARSE, AUTO16: STREAM})


def test_compact_and_truncate_with_q8_off():
    """Case 7 with CM_DENSE_Q8=0 on the automatic kinds (K1c for 64 queries, K1s for 16; its own
    process, since the knob is read once)."""
    tests = Path(__file__).resolve().parent
    env = dict(os.environ, CM_DENSE_Q8="0", CM_COMPACT_CHUNK_ROWS="1000",
               PYTHONPATH=os.pathsep.join([str(tests), str(tests.parent), str(tests.parent / "classmate-rag_amd")]
                                          + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_dense_mutations as t; t.q8_off_child(); print('\\nchild ok')"],
                       env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-4000:]


def test_prefix_plane_overwrites(base, monkeypatch):
    """Case 8: case 1's overwrites on a CM_DENSE_F16=prefix store (rows < 1 280 are in the f16 plane,
    dense_scatter_kernel's in_plane branch; the rest are not): lists equal to the full-plane store's
    -- rows equal, distances bit-equal (test_gpu_f16_prefix.py's bar) -- and to the oracle.  A prefix
    store runs K1q / K1q-s whatever kind is forced."""
    from classmate_hip import engine
    C, Q = base["C"], base["Q"]
    monkeypatch.setenv("CM_DENSE_F16", "prefix")
    pre = engine.DenseIndex(D, capacity=N)
    pre.upsert(C, np.arange(N, dtype=np.int64))
    monkeypatch.setenv("CM_DENSE_F16", "full")
    full = engine.DenseIndex(D, capacity=N)
    full.upsert(C, np.arange(N, dtype=np.int64))
    monkeypatch.delenv("CM_DENSE_F16")
    model = Model(D)
    model.upsert(C, np.arange(N))
    try:
        assert full.mem_stats()["bytes"] - pre.mem_stats()["bytes"] >= 0.9 * N * D * 2
        rows, vecs, planted = case1_overwrites(N, Q, seed=510)
        assert (rows < 1280).sum() >= 10 and (rows >= 1280).sum() >= 400
        pre.upsert(vecs, rows)
        full.upsert(vecs, rows)
        model.upsert(vecs, rows)
        expect = {COARSE: Q8, STREAM: Q8S}
        res = verify("prefix overwrite", pre, model, Q, expect=expect)
        assert_case1_planted(res, planted)
        for k in KS:
            for kind in (F32, Q8, Q8S):
                d0, r0, _, _ = host_lists(full, kind, queries_of(kind, Q), k)
                d1, r1, _, _ = res[kind, k]
                assert np.array_equal(r0, r1) and np.array_equal(d0, d1), (kind, k)
        assert_export(pre, model)
    finally:
        pre.close()
        full.close()


def test_exact_duplicates(base):
    """Case 9: 40 byte-identical copies of one vector in different tiles and scale groups, inside and
    outside the samples.  Searched with that vector: on the coarse kinds (fp64 re-rank of the stored
    rows), when no query went to the exact fp32 pass, the copies' distances are bit-equal, their rows
    ascend and they are the *lowest* copies; on every kind the (distance, row) order holds
    (check_lists).  The copies tie by construction, so the duplicate query is held to these explicit
    assertions and the tie-slack budget covers the other queries."""
    C, Q0 = base["C"], base["Q"]
    rng = np.random.default_rng(590)
    idx, model = new_index(C)
    try:
        dup = np.sort(np.concatenate([[1, 17, 70, 300, 511, 639, 641, 1279, 1281, 4095, 4096, N - 1],
                                      rng.choice(np.arange(4100, N - 1), 28, replace=False)]))
        assert np.unique(dup).shape[0] == 40 and np.unique(dup >> 6).shape[0] >= 30
        v = unit_rows(1, D, seed=591)[0]
        both(idx, model).upsert(np.tile(v, (40, 1)), dup)
        Q = Q0.copy()
        Q[0] = v
        res = verify("duplicates", idx, model, Q, slack_from=1)
        for (kind, k), (d, r, fb, _) in res.items():
            assert np.isin(r[0], dup).all() and (np.abs(d[0]) < 1e-5).all(), (kind, k)
            if kind != F32 and fb == 0:
                assert np.array_equal(r[0], dup[:k]), (kind, k, r[0])
                assert (d[0].view(np.uint32) == d[0].view(np.uint32)[0]).all(), (kind, k, d[0])
    finally:
        idx.close()


# ---- sharded -------------------------------------------------------------------------------------
N_SH = 50112                      # 783 blocks of 64 rows: 261 per shard, 16 704 rows each


def sharded_case():
    """Case 10's state: a 3-shard index (block 64) and one index after case 1's overwrites and case
    3's delete-and-reuse, with the model of both.  Returns (sharded, one, model, Q of the case, the
    planted rows, stay, back)."""
    from classmate_hip import engine, multidev
    C, Q = base_store(N_SH, 601)
    sh = multidev.ShardedDenseIndex(D, [0, 0, 0], block=64)
    one = engine.DenseIndex(D)
    model = Model(D)
    rows = np.arange(N_SH, dtype=np.int64)
    sh.upsert(C, rows)
    model.upsert(C, rows)
    for s in sh.shards:
        assert s.size >= 16384 and s.search_kind(64, 10) == Q8 and s.search_kind(16, 24) == Q8S
    ow_rows, ow_vecs, planted = case1_overwrites(N_SH, Q, seed=610)
    both(sh, model).upsert(ow_vecs, ow_rows)
    Qc, stay, back = delete_and_reuse(sh, model, N_SH, seed=620, protect=planted)
    live = model.live_rows()
    one.upsert(model.vecs[live], live)
    Qs = Q.copy()
    Qs[32:56] = Qc
    return sh, one, model, Qs, planted, stay, back


def sharded_lists(sh, kind, Q, k, words=None):
    """ShardedDenseIndex.search with `kind` forced on every shard (16 queries per search on the
    stream kinds)."""
    step = 16 if kind in STREAM_KINDS else Q.shape[0]
    ds, rs = [], []
    for s in sh.shards:
        s.set_path(kind)
    try:
        for s0 in range(0, Q.shape[0], step):
            q = np.ascontiguousarray(Q[s0:s0 + step])
            for s in sh.shards:
                assert s.search_kind(q.shape[0], k) == kind
            d, r = sh.search(q, k, words)
            ds.append(d)
            rs.append(r)
    finally:
        for s in sh.shards:
            s.set_path(0)
    return np.concatenate(ds), np.concatenate(rs)


def test_sharded_overwrite_delete_and_reuse():
    """Case 10: three shards of >= 16 384 rows (every one on a coarse kind), case 1's overwrites and
    case 3's delete-and-reuse through the sharded interface: rows equal to one index of the same
    final state, distances within 1e-6, and equal to the oracle; the device entry equals the host's."""
    import torch
    sh, one, model, Q, planted, stay, back = sharded_case()
    try:
        assert sh.size == model.size and sh.live_count() == int(model.live.sum())
        out, live = sh.export(with_live=True)
        assert np.array_equal(live, model.live) and out.tobytes() == model.vecs.tobytes()
        for k in KS:
            assert tie_slack_share(model, Q, k) <= SLACK_CAP
            d1 = sharded_lists(sh, F32, Q, k)[0]
            for kind in KINDS:
                d, r = sharded_lists(sh, kind, Q, k)
                check_lists(d, r, model, Q, k, pad_ref=d1)
                dw, rw, _, _ = host_lists(one, kind, Q, k)
                assert np.array_equal(r, rw), (kind, k)
                assert float(np.abs(d.astype(np.float64) - dw).max()) <= 1e-6, (kind, k)
                assert_case1_planted({(kind, k): (d, r, 0, 0)}, planted)
                assert_case3({(kind, k): (d[32:], r[32:], 0, 0)}, stay, back)
            q = torch.from_numpy(Q).cuda()
            dd, rd = sh.search_dev(q, k)
            torch.cuda.synchronize()
            d, r = sh.search(Q, k)
            assert np.array_equal(rd.cpu().numpy(), r) and np.array_equal(dd.cpu().numpy(), d), k
    finally:
        sh.close()
        one.close()
