"""The row-list searches with device inputs and outputs (cm_dense_search_lists_dev,
cm_bm25_search_lists_dev; engine.DenseIndex.search_lists(dev=True), engine.BM25Index.search_lists(
dev=True, eps_io=...)).  The reference throughout is the existing host function on the same handle:
the device forms share its body, so distances, scores, rows and nvalid compare equal as bits -- which
pins the one new kernel (the padded queries and their sequential fp64 norms) -- and eps_io's known
floors replace the postings pass without changing an answer."""
import numpy as np
import pytest

import test_gpu_bm25_lists as bl
from test_gpu_dense_lists import D, N, mask_of, mixed_batch
from test_gpu_dense_mutations import KS, _bits, base_store
from test_gpu_scale import unit_rows

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    import torch
    from classmate_hip import engine
    C, _ = base_store(N, 901, nq=32)
    idx = engine.DenseIndex(D)
    idx.upsert(C, np.arange(N, dtype=np.int64))
    clauses, Q, filter_of, _ = mixed_batch(C)
    words = [_bits(mask_of(N, r)) for r in clauses]
    yield dict(idx=idx, Q=Q, filter_of=filter_of, words=words, dev=torch.device("cuda", idx.device))
    idx.close()


def assert_same_bits(got, want):
    dist, rows = (t.cpu().numpy() for t in got)
    assert dist.dtype == want[0].dtype and rows.dtype == want[1].dtype and dist.shape == want[0].shape
    assert np.array_equal(rows, want[1])
    assert dist.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("k", KS)
def test_dense_mixed_batch_equals_the_host_function(dense, k):
    import torch
    idx, Q, filter_of, words = dense["idx"], dense["Q"], dense["filter_of"], dense["words"]
    want = idx.search_lists(Q, k, words, filter_of)
    assert (want[1] >= 0).any() and (want[1] == -1).any()         # lists longer and shorter than k, an empty one
    q = torch.from_numpy(Q).to(dense["dev"])
    got = idx.search_lists(q, k, words, filter_of, dev=True)
    assert got[0].device == q.device and got[1].device == q.device
    assert_same_bits(got, want)
    # the bitmaps as device words too
    dev_words = torch.from_numpy(np.stack(words).view(np.int32)).to(dense["dev"])
    assert_same_bits(idx.search_lists(q, k, dev_words, filter_of, dev=True), want)


def test_dense_queries_produced_on_another_stream_just_before(dense):
    """The stream contract: q's producer is enqueued on torch's current (non-default) stream right
    before the call and nothing waits for it on the host."""
    import torch
    idx, Q, filter_of, words = dense["idx"], dense["Q"], dense["filter_of"], dense["words"]
    want = idx.search_lists(Q, 10, words, filter_of)
    dev = dense["dev"]
    half = torch.from_numpy(Q * np.float32(0.5)).to(dev)          # x 2 is exact: the producer rebuilds Q's bits
    big = torch.ones((4096, 4096), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        for _ in range(4):                                        # work queued ahead of the producer
            big = big @ big * 1e-4
        q = half * 2.0
        got = idx.search_lists(q, 10, words, filter_of, dev=True)
    assert_same_bits(got, want)                                    # complete on return: no synchronise here
    st.synchronize()
    assert np.array_equal(q.cpu().numpy(), Q)


def test_dense_padded_rows():
    """dim 100 pads to ld 128: the padding is all the new kernel adds beyond the sum."""
    import torch
    from classmate_hip import engine
    dim, n = 100, 2048
    C = unit_rows(n, dim, seed=77)
    idx = engine.DenseIndex(dim)
    try:
        idx.upsert(C, np.arange(n, dtype=np.int64))
        rng = np.random.default_rng(5)
        clauses = [np.arange(n - 100, n), np.sort(rng.choice(n, 300, replace=False)), np.array([0, 31, 32, n - 1])]
        words = np.stack([_bits(mask_of(n, r)) for r in clauses])
        nq = 21
        filter_of = np.arange(nq, dtype=np.int32) % 3
        Q = rng.standard_normal((nq, dim)).astype(np.float32) * np.float32(3.7)     # not unit: the norms matter
        q = torch.from_numpy(Q).to(torch.device("cuda", idx.device))
        for k in KS:
            want = idx.search_lists(Q, k, words, filter_of)
            assert_same_bits(idx.search_lists(q, k, words, filter_of, dev=True), want)
        with pytest.raises(ValueError):
            idx.search_lists(q, 10, words, filter_of, return_vectors=True, dev=True)
        with pytest.raises(RuntimeError):
            idx.search_lists(q, 257, words, filter_of, dev=True)                     # above cm_max_topk
        assert_same_bits(idx.search_lists(q, 10, words, filter_of, dev=True), idx.search_lists(Q, 10, words, filter_of))
    finally:
        idx.close()


# ---------------------------------------------------------------------------
# BM25
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    return bl._make()


@pytest.fixture(scope="module", params=["tiles", "postings"])
def idx(request, data):
    index = bl._build(data, request.param == "tiles")
    yield index
    index.close()


def assert_same_lists(got, want):
    s, r = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert s.dtype == want[0].dtype and np.array_equal(got[2], want[2])
    assert np.array_equal(r, want[1])
    assert (s == want[0]).all()


@pytest.mark.parametrize("k", bl.KS)
def test_bm25_equals_the_host_function(data, idx, k):
    want = idx.search_lists(data.queries, k, data.words, data.filter_of)
    n_eps = idx.last_eps_filters()
    got = idx.search_lists(data.queries, k, data.words, data.filter_of, dev=True)
    assert got[0].is_cuda and got[1].is_cuda and isinstance(got[2], np.ndarray)
    assert_same_lists(got, want)
    assert idx.last_eps_filters() == n_eps > 0


def test_bm25_eps_io(data, idx):
    k = 10
    nf = len(data.words)
    want = idx.search_lists(data.queries, k, data.words, data.filter_of)
    neg = sorted({f for (f, _), is_neg in bl._pair_signs(data).items() if is_neg})
    rest = [f for f in range(nf) if f not in neg]
    assert neg and rest                                            # a condition on the inputs: both kinds
    # all unknown: the same answers, the floors of the negative-idf clauses written back
    eps = np.full(nf, np.nan)
    assert_same_lists(idx.search_lists(data.queries, k, data.words, data.filter_of, dev=True, eps_io=eps), want)
    assert idx.last_eps_filters() == len(neg) and idx.last_eps_passes() >= 1
    for f in neg:
        assert eps[f] == idx.filter_eps(data.words[f]), f
    assert np.isnan(eps[rest]).all()
    # all known: the same answers, nothing computed
    again = eps.copy()
    assert_same_lists(idx.search_lists(data.queries, k, data.words, data.filter_of, dev=True, eps_io=again), want)
    assert idx.last_eps_filters() == 0 and idx.last_eps_passes() == 0
    assert np.array_equal(again, eps, equal_nan=True)
    # another floor for one clause: its scores change, no other clause's do
    f = neg[0]
    other = eps.copy()
    other[f] = 123.0
    s, r, n = idx.search_lists(data.queries, k, data.words, data.filter_of, dev=True, eps_io=other)
    s = s.cpu().numpy()
    mine = data.filter_of == f
    assert (s[mine] != want[0][mine]).any()
    assert (s[~mine] == want[0][~mine]).all() and np.array_equal(r.cpu().numpy()[~mine], want[1][~mine])
    assert other[f] == 123.0 and idx.last_eps_filters() == 0
    # a partly known array: only the unknown floors are computed
    part = eps.copy()
    part[neg[-1]] = np.nan
    assert_same_lists(idx.search_lists(data.queries, k, data.words, data.filter_of, dev=True, eps_io=part), want)
    assert idx.last_eps_filters() == 1 and np.array_equal(part, eps, equal_nan=True)


def test_bm25_device_words_and_errors(data, idx):
    import torch
    want = idx.search_lists(data.queries, 10, data.words, data.filter_of)
    dev_words = torch.from_numpy(data.words.view(np.int32)).to(f"cuda:{idx.device}")
    st = torch.cuda.Stream(device=dev_words.device)
    st.wait_stream(torch.cuda.current_stream(dev_words.device))
    with torch.cuda.stream(st):
        words = dev_words.clone()                                  # produced on this stream, just before
        got = idx.search_lists(data.queries, 10, words, data.filter_of, dev=True)
    assert_same_lists(got, want)
    st.synchronize()
    with pytest.raises(ValueError):
        idx.search_lists(data.queries, 10, data.words, data.filter_of, eps_io=np.full(len(data.words), np.nan))
    with pytest.raises(ValueError):
        idx.search_lists(data.queries, 10, data.words, data.filter_of, dev=True, eps_io=np.full(2, np.nan))
    empty = bl._bits(bl.EMPTY_DOCS)
    with pytest.raises(ZeroDivisionError):
        idx.search_lists([data.queries[3]] * 2, 5, np.stack([data.words[0], empty]), [0, 1], dev=True)
    assert_same_lists(idx.search_lists(data.queries, 10, data.words, data.filter_of, dev=True), want)
