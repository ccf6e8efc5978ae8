"""engine.BM25Index.search_lists (cm_bm25_search_lists): one batch whose queries carry different
where clauses, against BM25Index.search asked one query and one clause at a time -- scores with ==,
rows and nvalid -- under both head policies (terms that own tiles read the tile byte, all others
binary-search their postings), plus the epsilon floor, the ZeroDivisionError, the argument errors
and rank_bm25's own arithmetic (oracle.ref_semantics.BM25Okapi) on two clauses."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, V, V_PLAIN = 3001, 2000, 1990          # N is no multiple of 32; terms from V_PLAIN up are planted
T_BIG, T_EPS, T_MISS = 1999, 1998, 1997
CHUNK = 256                               # cm_bm25_lists.inc: kBmListChunk
DEAD = [5, 100, 1234, 2500]
EMPTY_DOCS = [2000, 2001, 2002, 2003]     # live documents without tokens
ROW_BIG, RUN = 700, (1200, 1260)
KS = (1, 10, 300)                         # 300: beyond several lists and cm_max_topk


def _bits(rows, extra_word_bits=0):
    w = np.zeros((N + 31) // 32, np.uint32)
    for r in rows:
        w[r >> 5] |= np.uint32(1 << (r & 31))
    w[-1] |= np.uint32(extra_word_bits)
    return w


def _make():
    rng = np.random.default_rng(20240611)
    p = 1.0 / np.arange(1, V_PLAIN + 1)
    p /= p.sum()
    docs = [rng.choice(V_PLAIN, size=int(rng.integers(8, 40)), p=p).astype(np.int32) for _ in range(N)]
    for r in EMPTY_DOCS:
        docs[r] = np.zeros(0, np.int32)
    docs[ROW_BIG] = np.concatenate([docs[ROW_BIG], np.full(300, T_BIG, np.int32)])          # a tf >= 255
    for r in (10, 701, 2999):
        docs[r] = np.append(docs[r], np.int32(T_BIG))
    for r in range(*RUN):                                                                      # df = Nc in the run
        docs[r] = np.append(docs[r], np.int32(T_EPS))
    docs[0] = np.append(docs[0], np.int32(T_MISS))
    live = np.ones(N, np.uint8)
    live[DEAD] = 0
    ok = [r for r in range(1, N) if live[r] and r not in EMPTY_DOCS and r != ROW_BIG]
    pick = lambda n: sorted(rng.choice(ok, size=n, replace=False).tolist())
    clauses = [
        sorted(pick(CHUNK - 1) + [ROW_BIG]),                     # 0: exactly one chunk
        pick(CHUNK + 1),                                         # 1: one row more
        [ROW_BIG],                                               # 2: one row
        [5, 100],                                                # 3: only dead rows
        pick(100),                                               # 4: used by no query
        sorted(set(pick(50)) | {N - 1}),                         # 5: ends at the last row
        list(range(2990, N)),                                    # 6: with bits at and above N set (below)
        list(range(*RUN)),                                       # 7: a contiguous run (one dead row inside)
        sorted(set(r for r in ok if rng.random() < 0.233) | {2500}),   # 8: scattered, ~700 rows, one dead
    ]
    words = np.stack([_bits(c, 0xFE000000 if f == 6 else 0) for f, c in enumerate(clauses)])
    used = [0, 1, 2, 3, 5, 6, 7, 8]
    nq = 64
    filter_of = np.asarray([used[i % len(used)] for i in range(nq)], np.int32)
    queries = [rng.choice(V_PLAIN, size=int(rng.integers(2, 7)), p=p).tolist() for _ in range(nq)]
    queries[0].append(-1)                                        # an unknown term
    queries[1] = [queries[1][0], queries[1][0], queries[1][1]]   # a duplicated term
    queries[8] = [T_BIG, 3]                                      # clause 0 holds ROW_BIG
    queries[9] = []                                              # no terms
    queries[10] = [T_BIG, 0]                                     # clause 2: the one row, df = Nc
    queries[15] = [T_MISS]                                       # clause 8: no candidate holds it
    queries[14] = [T_EPS, 1, 2]                                  # clause 7: the planted term
    queries[22] = [1, T_EPS, T_EPS]
    queries[20] = rng.choice(V_PLAIN, size=70, p=p).tolist()     # more slots than one LDS stage
    assert filter_of[8] == 0 and filter_of[10] == 2 and filter_of[15] == 8 and filter_of[14] == 7 and filter_of[22] == 7
    return types.SimpleNamespace(docs=docs, live=live, clauses=clauses, words=words, filter_of=filter_of, queries=queries)


def _build(data, tiles: bool):
    from classmate_hip import engine
    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum([d.shape[0] for d in data.docs])
    idx = engine.BM25Index()
    idx.build(np.concatenate(data.docs), off, V, live=data.live)
    if not tiles:
        idx.set_head_policy(max_bytes=0)
    return idx


@pytest.fixture(scope="module")
def data():
    return _make()


@pytest.fixture(scope="module", params=["tiles", "postings"])
def world(request, data):
    """The index under one head policy, and the per-query reference (BM25Index.search, one query and
    one clause per call), computed once per k."""
    idx = _build(data, request.param == "tiles")
    refs = {}

    def ref(k):
        if k not in refs:
            out = [idx.search([q], k, data.words[f]) for q, f in zip(data.queries, data.filter_of)]
            refs[k] = tuple(np.concatenate([o[j] for o in out]) for j in range(3))
        return refs[k]
    return types.SimpleNamespace(idx=idx, ref=ref, tiles=request.param == "tiles")


def _candidates(data, f):
    return [r for r in data.clauses[f] if data.live[r]]


def _pair_signs(data):
    """{(filter, term): candidate idf < 0} over the batch's pairs with a candidate df > 0, in numpy:
    rank_bm25's idf log(Nc - df + 0.5) - log(df + 0.5) is negative iff df > Nc - df."""
    if not hasattr(data, "signs"):
        data.signs = {}
        for q, f in zip(data.queries, data.filter_of.tolist()):
            cand = _candidates(data, f)
            for t in set(q) - {x for g, x in data.signs if g == f}:
                df = sum(1 for r in cand if t in data.docs[r])
                if df:
                    data.signs[(f, t)] = df > len(cand) - df
    return data.signs


def test_the_inputs_are_the_cases_to_cover(data, world):
    lens = [len(_candidates(data, f)) for f in range(len(data.clauses))]
    assert lens[0] == CHUNK and lens[1] == CHUNK + 1 and lens[2] == 1 and lens[3] == 0
    assert 4 not in data.filter_of and data.clauses[5][-1] == N - 1 and 600 < lens[8] < 800
    assert data.words[6, -1] >> (N & 31) and lens[6] == N - 2990 and N % 32
    assert (data.docs[ROW_BIG] == T_BIG).sum() >= 255 and ROW_BIG in data.clauses[0]
    assert not any(T_MISS in data.docs[r] for r in data.clauses[8])
    # head tiles: df > N / 128, no tf >= 255 (cm_bm25.hip: build_head_tiles)
    df = np.zeros(V, np.int64)
    for r, d in enumerate(data.docs):
        df[np.unique(d)] += 1
    margin = len(DEAD)                                   # whether or not dead rows count towards a term's df
    heads = {t for t in range(V) if df[t] > N / 128 + margin and t != T_BIG}
    tails = {t for t in range(V) if 0 < df[t] < N / 128 - margin}
    if world.tiles:
        assert world.idx.num_head_terms >= len(heads)
        assert len({t for q in data.queries for t in q} & heads) >= 8      # and tail terms too
        assert len({t for q in data.queries for t in q} & tails) >= 8
    else:
        assert world.idx.num_head_terms == 0


@pytest.mark.parametrize("k", KS)
def test_batch_equals_one_search_per_query(data, world, k):
    want_s, want_r, want_n = world.ref(k)
    # a condition on the inputs: some, not all, of the batch's (filter, term) pairs have a negative idf
    signs = _pair_signs(data)
    assert 0 < sum(signs.values()) < len(signs)
    got_s, got_r, got_n = world.idx.search_lists(data.queries, k, data.words, data.filter_of)
    assert np.array_equal(got_n, want_n)
    assert np.array_equal(got_r, want_r)
    assert (got_s == want_s).all()
    assert world.idx.last_eps_filters() == len({f for (f, _), neg in signs.items() if neg})
    # out_n = min(k, Nc), pads (0.0, -1), descending scores
    for i, f in enumerate(data.filter_of.tolist()):
        nc = len(_candidates(data, f))
        assert got_n[i] == min(k, nc)
        assert (got_r[i, got_n[i]:] == -1).all() and (got_s[i, got_n[i]:] == 0.0).all()
        assert (np.diff(got_s[i, :got_n[i]]) <= 0).all()
    # every term misses the clause: zero scores in row order (quirk Q1)
    n = got_n[15]
    assert (got_s[15, :n] == 0.0).all() and got_r[15, :n].tolist() == _candidates(data, 8)[:n]
    assert got_r[9, :got_n[9]].tolist() == _candidates(data, data.filter_of[9])[:got_n[9]]      # no terms


def test_allow_word_forms_and_a_clause_per_call(data, world):
    """Device words, a sequence of bitmaps, and a call that holds one query: the same answers."""
    import torch
    k = 10
    want_s, want_r, want_n = world.ref(k)
    dev = torch.from_numpy(data.words.view(np.int32)).to(f"cuda:{world.idx.device}")
    for words in (dev, [w for w in data.words], [dev[f] if f % 2 else data.words[f] for f in range(len(data.words))]):
        got = world.idx.search_lists(data.queries, k, words, data.filter_of)
        assert (got[0] == want_s).all() and np.array_equal(got[1], want_r) and np.array_equal(got[2], want_n)
    for i in (8, 10, 14):
        s, r, n = world.idx.search_lists([data.queries[i]], k, data.words[data.filter_of[i]][None, :], [0])
        assert (s[0] == want_s[i]).all() and np.array_equal(r[0], want_r[i]) and n[0] == want_n[i]


def test_both_head_policies_agree(data):
    idx = _build(data, True)
    a = idx.search_lists(data.queries, 40, data.words, data.filter_of)
    assert idx.num_head_terms > 0
    idx.set_head_policy(max_bytes=0)
    assert idx.num_head_terms == 0
    b = idx.search_lists(data.queries, 40, data.words, data.filter_of)
    assert (a[0] == b[0]).all() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_zero_division_like_search_and_the_handle_survives(data, world):
    idx = world.idx
    empty = _bits(EMPTY_DOCS)
    q = data.queries[3]
    with pytest.raises(ZeroDivisionError):
        idx.search([q], 5, empty)
    words = np.stack([data.words[0], empty])
    with pytest.raises(ZeroDivisionError) as e:
        idx.search_lists([q, q], 5, words, [0, 1])
    assert "float division by zero (candidate documents have no tokens)" in str(e.value)
    # the clause is there but no query uses it: no error; and the next call answers correctly
    got = idx.search_lists([q, q], 5, words, [0, 0])
    want = idx.search([q], 5, data.words[0])
    for j in range(2):
        assert (got[0][j] == want[0][0]).all() and np.array_equal(got[1][j], want[1][0]) and got[2][j] == want[2][0]


def test_argument_errors_leave_the_handle_usable(data, world):
    from classmate_hip import _lib
    from test_bm25_lists_host import _call
    idx = world.idx
    cases = [dict(nq=0), dict(k=0), dict(n_filters=0), dict(filter_of=(1,)), dict(filter_of=(-1,)),
             dict(nq=2, filter_of=(0, 3), n_filters=3), dict(nq=2, filter_of=(0, 0), q_off=[0, 2, 1])]
    cases += [dict(null=name) for name in ("q_terms", "q_off", "allow", "filter_of", "score", "row", "n")]
    want = world.ref(10)
    for kw in cases:
        assert _call(idx._h, **kw) == _lib.CM_EINVAL, kw
    with pytest.raises(ValueError):
        idx.search_lists(data.queries, 10, data.words, data.filter_of[:-1])
    with pytest.raises(ValueError):
        idx.search_lists(data.queries[:1], 10, data.words, [len(data.words)])
    got = idx.search_lists(data.queries, 10, data.words, data.filter_of)
    assert (got[0] == want[0]).all() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("f", [0, 7])
def test_scores_are_rank_bm25s(data, world, f):
    """Independent of the per-clause route: BM25Okapi over the clause's candidate token lists."""
    from oracle.ref_semantics import BM25Okapi
    cand = _candidates(data, f)
    okapi = BM25Okapi([data.docs[r].tolist() for r in cand])
    sel = [i for i in range(len(data.queries)) if data.filter_of[i] == f]
    assert any(T_BIG in data.queries[i] or T_EPS in data.queries[i] for i in sel)
    k = 300
    got_s, got_r, got_n = world.idx.search_lists([data.queries[i] for i in sel], k, data.words[f][None, :],
                                                 np.zeros(len(sel), np.int32))
    for j, i in enumerate(sel):
        scores = okapi.get_scores(data.queries[i])
        order = sorted(range(len(cand)), key=lambda c: -scores[c])[:k]       # stable: ties keep the lower row
        assert got_n[j] == len(order)
        assert got_r[j, :got_n[j]].tolist() == [cand[c] for c in order]
        assert (got_s[j, :got_n[j]] == scores[order]).all()
