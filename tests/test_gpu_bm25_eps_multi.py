"""engine.BM25Index.filter_eps_multi (cm_bm25_filter_eps_multi): the epsilon floors of many filters
from shared postings passes, against BM25Index.filter_eps asked one filter at a time, with == --
under both head policies, with host and device words, over one, two and three rounds -- against
rank_bm25's own arithmetic (oracle.ref_semantics.BM25Okapi), on a corpus whose terms cross the
pass's slices, through search_lists, and its ZeroDivisionError."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, V, V_PLAIN = 3001, 2000, 1990          # N is no multiple of 32; vocabulary ids from V_PLAIN up have no posting
DEAD = [5, 100, 1234, 2500]
EMPTY_DOCS = [2000, 2001, 2002, 2003]     # live documents without tokens
TWINS = (40, 41)                          # two documents that share most of their terms
BLOCK = (1216, 1280)                      # 64 consecutive rows
SLICE = 4096                              # cm_bm25_eps.inc: kBmEpsSlice
SIZES = (1, 31, 32, 33, 70)
PASSES = (1, 1, 1, 2, 3)


def _bits(rows, n=N, extra_word_bits=0):
    w = np.zeros((n + 31) // 32, np.uint32)
    rows = np.asarray(rows, np.int64)
    np.bitwise_or.at(w, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
    w[-1] |= np.uint32(extra_word_bits)
    return w


def _make():
    rng = np.random.default_rng(20240611)
    p = 1.0 / np.arange(1, V_PLAIN + 1)
    p /= p.sum()
    docs = [rng.choice(V_PLAIN, size=int(rng.integers(8, 40)), p=p).astype(np.int32) for _ in range(N)]
    for r in EMPTY_DOCS:
        docs[r] = np.zeros(0, np.int32)
    docs[TWINS[1]] = np.append(docs[TWINS[0]], np.int32(1234))
    live = np.ones(N, np.uint8)
    live[DEAD] = 0
    ok = [r for r in range(N) if live[r] and r not in EMPTY_DOCS and r not in TWINS and not 2900 <= r]
    perm = rng.permutation(ok).tolist()
    take = lambda n: sorted(perm.pop() for _ in range(n))
    named = {}
    # 0 .. 31: every one holds the same 64 consecutive rows: one wave step sets every membership bit
    filters = [sorted(set(range(*BLOCK)) | set(rng.choice(ok, size=20, replace=False).tolist())) for _ in range(32)]
    # 32 .. 37
    named["n700"] = len(filters)
    filters.append(sorted(r for r in ok if rng.random() < 0.233) + [2500])           # ~700 rows, one dead
    named["all"] = len(filters)
    filters.append(list(range(N)))
    same = sorted(rng.choice(ok, size=100, replace=False).tolist())
    named["same"] = (len(filters), len(filters) + 1)
    filters += [same, list(same)]
    filters.append(sorted(rng.choice(ok, size=64, replace=False).tolist()))
    filters.append(sorted(rng.choice(ok, size=1000, replace=False).tolist()))
    # 38 .. 69: pairwise disjoint
    first_disjoint = len(filters)
    for n in (1, 2, 3, 5, 33, 255, 256, 257):
        named[f"n{n}"] = len(filters)
        filters.append(take(n))
    named["twins"] = len(filters)
    filters.append(list(TWINS))
    named["dead"] = len(filters)
    filters.append(list(DEAD))
    named["late"] = len(filters)
    filters.append(list(range(2900, 2990)))                                           # only rows >= 2900
    named["last_word"] = len(filters)
    filters.append(list(range(2990, N)))                                              # bits at and above N set below
    while len(filters) < first_disjoint + 32:
        filters.append(take(40))
    assert len(filters) == 70 and named["dead"] >= 33
    words = np.stack([_bits(c, N, 0xFE000000 if f == named["last_word"] else 0) for f, c in enumerate(filters)])
    return types.SimpleNamespace(docs=docs, live=live, filters=filters, words=words, named=named,
                                 first_disjoint=first_disjoint, p=p)


def _build(docs, vocab, live, tiles: bool):
    from classmate_hip import engine
    off = np.zeros(len(docs) + 1, np.int64)
    off[1:] = np.cumsum([d.shape[0] for d in docs])
    idx = engine.BM25Index()
    idx.build(np.concatenate(docs), off, vocab, live=live)
    if not tiles:
        idx.set_head_policy(max_bytes=0)
    return idx


@pytest.fixture(scope="module")
def data():
    return _make()


@pytest.fixture(scope="module", params=["tiles", "postings"])
def world(request, data):
    """The index under one head policy and the reference: filter_eps, one filter per call."""
    idx = _build(data.docs, V, data.live, request.param == "tiles")
    want = np.asarray([idx.filter_eps(w) for w in data.words])
    return types.SimpleNamespace(idx=idx, want=want)


def _candidates(data, f):
    return [r for r in data.filters[f] if data.live[r]]


def _numpy_sums(data, f):
    """The idf sum of filter f's candidate vocabulary in first-occurrence order and in ascending
    term-id order (numpy's logs are glibc's on this platform; only their difference is used)."""
    cand = _candidates(data, f)
    df, order = {}, []
    for r in cand:
        for t in data.docs[r].tolist():
            if t not in df:
                df[t] = 0
                order.append(t)
        for t in set(data.docs[r].tolist()):
            df[t] += 1
    idf = {t: np.log(len(cand) - df[t] + 0.5) - np.log(df[t] + 0.5) for t in order}
    a = b = 0.0
    for t in order:
        a = a + idf[t]
    for t in sorted(order):
        b = b + idf[t]
    return a, b


def test_the_inputs_are_the_cases_to_cover(data, world):
    nm, lens = data.named, [len(_candidates(data, f)) for f in range(70)]
    assert N % 32 and world.idx.num_docs == N
    for n in (1, 2, 3, 5, 33, 255, 256, 257):
        assert lens[nm[f"n{n}"]] == n
    assert 600 < lens[nm["n700"]] < 800 and lens[nm["all"]] == N - len(DEAD) and lens[nm["dead"]] == 0
    assert (data.words[nm["same"][0]] == data.words[nm["same"][1]]).all()
    assert data.words[nm["last_word"], -1] >> (N & 31)
    assert min(data.filters[nm["late"]]) >= 2900
    assert all(set(range(*BLOCK)) <= set(data.filters[f]) for f in range(32))
    seen = set()
    for f in range(data.first_disjoint, data.first_disjoint + 32):
        assert not seen & set(data.filters[f])
        seen |= set(data.filters[f])
    a, b = (set(data.docs[r].tolist()) for r in TWINS)
    assert len(a & b) > len(a ^ b)
    used = set(np.concatenate(data.docs).tolist())
    assert max(used) < V_PLAIN < V and all(len(data.docs[r]) == 0 and data.live[r] for r in EMPTY_DOCS)


@pytest.mark.parametrize("device_words", [False, True], ids=["host", "device"])
def test_bit_equal_to_filter_eps_over_one_two_and_three_rounds(data, world, device_words):
    import torch
    idx = world.idx
    for n, passes in zip(SIZES, PASSES):
        words = data.words[:n]
        if device_words:
            words = torch.from_numpy(words.view(np.int32)).to(f"cuda:{idx.device}")
        got = idx.filter_eps_multi(words)
        assert got.shape == (n,) and got.dtype == np.float64
        assert (got == world.want[:n]).all(), (n, np.nonzero(got != world.want[:n])[0])
        assert idx.last_eps_passes() == passes
    assert world.want[data.named["dead"]] == 0.0
    assert world.want[data.named["same"][0]] == world.want[data.named["same"][1]]
    # a sequence of bitmaps, and another order: each answer belongs to its own bitmap
    order = np.random.default_rng(3).permutation(70)
    got = idx.filter_eps_multi([data.words[f] for f in order])
    assert (got == world.want[order]).all()


def test_epsilons_are_rank_bm25s(data, world):
    """Independent of filter_eps: BM25Okapi over the candidates' token lists."""
    from oracle.ref_semantics import BM25Okapi
    pick = [data.named[name] for name in ("twins", "n33", "n256", "n700")]
    got = world.idx.filter_eps_multi(data.words[pick])
    for g, f in zip(got, pick):
        okapi = BM25Okapi([data.docs[r].tolist() for r in _candidates(data, f)])
        assert g == okapi.epsilon * okapi.average_idf, f


def test_the_comparison_is_not_blind(data, world):
    """The order of the sum shows in its bits, and both signs occur."""
    big = [f for f in range(70) if len(_candidates(data, f)) >= 33]
    differ = 0
    for f in big:
        a, b = _numpy_sums(data, f)
        differ += a != b
    print(f"first-occurrence and term-id sums differ for {differ} of {len(big)} filters with >= 33 rows")
    assert 3 * differ >= len(big)
    assert (world.want < 0).any() and (world.want > 0).any()
    assert world.want[data.named["twins"]] < 0


@pytest.mark.parametrize("tiles", [True, False], ids=["tiles", "postings"])
def test_terms_that_cross_slices(tiles):
    """Corpus B: term 0 (in every document) and term 1 (from row SLICE + 5 on) each span more than
    two slices of the pass; term 1 neither begins nor ends on a slice border."""
    rng = np.random.default_rng(7)
    n = 3 * SLICE + 37
    docs = []
    for r in range(n):
        d = [0] + ([1] if r >= SLICE + 5 else []) + rng.integers(2, 400, size=int(rng.integers(1, 5))).tolist()
        docs.append(np.asarray(d[:6], np.int32))
    assert all(2 <= len(d) <= 6 for d in docs)
    idx = _build(docs, 400, np.ones(n, np.uint8), tiles)
    assert (idx.num_head_terms > 0) == tiles
    words = np.stack([_bits(range(n), n), _bits(range(n - 100, n), n), _bits(range(0, n, 97), n)])
    want = np.asarray([idx.filter_eps(w) for w in words])
    got = idx.filter_eps_multi(words)
    assert (got == want).all(), (got, want)
    assert idx.last_eps_passes() == 1


def test_search_lists_takes_its_epsilons_in_rounds(data, world):
    """40 clauses that all have a negative-idf query term: two rounds, and one search per query's answers."""
    idx = world.idx
    rng = np.random.default_rng(11)
    ok = [r for r in range(N) if data.live[r] and len(data.docs[r])]
    clauses, queries = [], []
    for _ in range(40):
        rows = sorted(rng.choice(ok, size=int(rng.integers(3, 60)), replace=False).tolist())
        df = np.bincount(np.concatenate([np.unique(data.docs[r]) for r in rows]), minlength=V)
        t_neg = int(np.argmax(df))
        assert df[t_neg] > len(rows) - df[t_neg]                 # idf < 0 iff df > Nc - df
        clauses.append(rows)
        queries.append([t_neg] + rng.choice(V_PLAIN, size=3, p=data.p).tolist())
    words = np.stack([_bits(c) for c in clauses])
    k = 10
    got_s, got_r, got_n = idx.search_lists(queries, k, words, np.arange(40, dtype=np.int32))
    assert idx.last_eps_filters() == 40 and idx.last_eps_passes() == 2
    for i in range(40):
        s, r, n = idx.search([queries[i]], k, words[i])
        assert (got_s[i] == s[0]).all() and np.array_equal(got_r[i], r[0]) and got_n[i] == n[0]


def test_zero_division_and_argument_errors_leave_the_handle_usable(data, world):
    from classmate_hip import _lib
    idx = world.idx
    words = np.concatenate([data.words[:20], _bits(EMPTY_DOCS)[None, :], data.words[20:34]])
    assert words.shape[0] == 35
    with pytest.raises(ZeroDivisionError) as e:
        idx.filter_eps_multi(words)
    assert "float division by zero (candidate documents have no tokens)" in str(e.value)
    with pytest.raises(ZeroDivisionError):
        idx.filter_eps(_bits(EMPTY_DOCS))
    got = idx.filter_eps_multi(data.words[:34])
    assert (got == world.want[:34]).all() and idx.last_eps_passes() == 2
    # too many words for one call: refused from the arguments alone
    eps = np.zeros(1)
    n_big = (2 ** 31 - 1) // words.shape[1] + 1
    assert _lib.fn["cm_bm25_filter_eps_multi"](idx._h, _lib.ptr(words), n_big, _lib.ptr(eps)) == _lib.CM_EUNSUPPORTED
    with pytest.raises(ValueError):
        idx.filter_eps_multi(data.words[:3, :-1])
    got = idx.filter_eps_multi(data.words[34:])
    assert (got == world.want[34:]).all()
