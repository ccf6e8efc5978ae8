"""``HybridRetriever.retrieve`` / ``retrieve_batch`` with the whole batch resident on the device.

The drop-in path (fusion.py) follows the reference's control flow per stage: the vector store
returns result dicts with their embeddings, MMR runs over host copies of the pools, the BM25 store
returns result dicts, and the merge matches items by id on the host (rag/retrieval/fusion.py:
108-167).  For a hybrid query with MMR -- the configuration the reference's callers use
(rag/pipeline/rag.py:531-554: ``ask_question`` sends ONE question with ``filters.to_dict()``) --
every one of those steps has a device form: where-filters as allow bitmaps (cm_filter_eval: Chroma
semantics for the dense side, ``_matches_filter`` semantics with quirk Q4 for BM25), cosine pool
search (K1c/K1s), pool gather + MMR (K4), BM25 top-k (K2a/K2b/K2 + K3; with a filter, K2f's
statistics over the allowed candidates, quirk Q2), pool preparation + RRF merge (K5).  This module
chains them without a host round trip and builds result dicts only for the final top_k items of
each query.  Single questions are a batch of one (their E5 encode replays a small-batch graph).
A batch with one filter per question takes the same chain (``retrieve_batch_clauses``): the stores
plan the searches as their host routes do, the selective clauses share the row-list searches in
their device form, and pools shorter than the MMR pool are served.

Id matching: the merge compares integer keys.  A document's key is its vector-store row; a BM25
document that the vector store does not hold gets ``n_vector_rows + bm25_row``.  The BM25-row ->
key map is a device array rebuilt when either store changes (their ``_version`` counters).

The result dicts equal the host path's (tests/test_gpu_dropin.py checks both on the same
stores): same ids, documents, metadata objects, distances (fp32 -> float), BM25 scores and fused
scores, in the same order.
"""
from __future__ import annotations

from typing import Any, Dict, List, Mapping, Optional, Sequence

import os

import numpy as np

from .. import _lib as L
from .. import engine


class _KeyMap:
    """BM25 rows <-> merge keys for one (vector store version, BM25 store version)."""

    def __init__(self, vs, bm, device: int):
        import torch
        ids_bm = bm._id_list
        nvr = len(vs._ids)
        if len(ids_bm) == nvr and ids_bm == vs._ids:          # the common case: one corpus, same order
            bm2key = np.arange(nvr, dtype=np.int64)
            vs2bm = np.arange(nvr, dtype=np.int64)
        else:
            rowmap = vs._row
            bm2key = np.fromiter((rowmap.get(i, -1) for i in ids_bm), dtype=np.int64, count=len(ids_bm))
            only = bm2key < 0
            bm2key[only] = nvr + np.nonzero(only)[0]
            vs2bm = np.full(nvr, -1, np.int64)
            both = ~only
            vs2bm[bm2key[both]] = np.nonzero(both)[0]
        self.nvr = nvr
        self.vs2bm = vs2bm
        self.bm2key_dev = torch.from_numpy(bm2key).to(torch.device("cuda", device))


def applicable(retr, filters, hybrid: bool) -> bool:
    """The device path covers hybrid retrieval with MMR over this package's stores, filtered or not
    (anything else takes the host path).  With a filter, ``retrieve_batch`` may still decline
    (None) when fewer vectors than the MMR pool pass it: the host path's k clamp covers that."""
    if not hybrid or not retr.use_mmr:
        return False
    if isinstance(filters, (list, tuple)):   # one filter per question: applicable_clauses
        return False
    return _stores_applicable(retr)


def _stores_applicable(retr) -> bool:
    """``applicable``'s conditions on the stores and the retriever's sizes."""
    from .bm25 import BM25Store
    from .vector_store import GpuVectorStore
    vs, bm = retr.vector_store, retr.bm25_store
    if not isinstance(vs, GpuVectorStore) or not isinstance(bm, BM25Store):
        return False
    vs._ensure_loaded()
    if vs._index is None or not bm._entries:
        return False
    pool = max(retr.k_vector, retr.mmr_max_pool)
    limit = L.max_topk()
    if not (0 < retr.k_vector <= pool <= limit and 0 < retr.k_bm25 <= limit):
        return False
    # the host path clamps k to the candidates; the device path needs full lists
    # live rows = the store's id -> row map (a device popcount + sync per call before)
    return len(vs._row) >= pool and len(bm._id_list) >= retr.k_bm25


def applicable_clauses(retr, filters, hybrid: bool) -> bool:
    """``applicable`` for one filter per question (a list or tuple): the same conditions, and both
    indexes must offer ``search_lists`` -- the sharded ones do not and keep the host path.  A clause
    that allows fewer vectors than the MMR pool is served (short pools), never declined.  Every cell
    of the measurement (DESIGN §3 "Hybrid batches with per-question clauses") is at least as fast as
    the host path, so there is no further routing rule here."""
    if not hybrid or not retr.use_mmr or not isinstance(filters, (list, tuple)):
        return False
    if not _stores_applicable(retr):
        return False
    bm = retr.bm25_store
    bm._ensure_index()
    return hasattr(retr.vector_store._index, "search_lists") and hasattr(bm._index, "search_lists")


def _query_vectors(embedder, questions: Sequence[str], dev):
    import torch
    enc = getattr(embedder, "encode_queries_dev", None)
    if enc is not None:
        q = enc(questions)
        if q is not None and q.device == dev and q.dtype == torch.float32:
            return q.contiguous()
    q = np.ascontiguousarray(np.asarray(embedder.encode_queries(list(questions)), np.float32))
    return torch.from_numpy(q).to(dev)


_ALLOW_CACHE_MAX = 64
# Process-level device caches, keyed by the stores' never-reused uids and version counters rather
# than held by one HybridRetriever: the reference builds a new retriever (and new stores) for every
# ask_question call (rag/pipeline/rag.py:531-545), so caches on the retriever object would be rebuilt
# per question -- the key map alone is O(corpus).
_ALLOW_CACHE: dict = {}
_KEYMAPS: dict = {}
_KEYMAPS_MAX = 4
_SIDE_STREAMS: dict = {}


def _canon(v):
    """Hashable, type-exact form of a where clause (True, 1 and "1" stay distinct; None when a
    value has no stable form)."""
    if isinstance(v, Mapping):
        return ("d", tuple(sorted(((str(type(k).__name__), k), _canon(x)) for k, x in v.items())))
    if isinstance(v, (list, tuple)):
        return (type(v).__name__, tuple(_canon(x) for x in v))
    if v is None or isinstance(v, (bool, int, float, str)):
        return (type(v).__name__, v)
    raise TypeError(type(v).__name__)


def _filter_key(meta, where, semantics: str):
    """Cache key of a filter over one metadata object and version: the object's uid (never reused,
    unlike id()), its version and the typed canonical clause (None when ``where`` has no stable
    form)."""
    try:
        return (meta.uid, meta.version, semantics, _canon(where))
    except (TypeError, ValueError):
        return None


def _allow(meta, where, semantics: str, device: int, n_words: int, cache: dict):
    """Device allow words + candidate count of ``where`` (engine.where_bits), cached per (metadata
    version, filter): a caller repeating one filter -- ask_question's to_dict() -- pays the filter
    program once per store change."""
    import torch
    key = _filter_key(meta, where, semantics)
    hit = cache.get(key) if key is not None else None
    if hit is not None and hit[0].numel() >= n_words:
        return hit
    from .. import engine as E
    words, n = E.where_bits(meta, where, semantics, device)
    if not hasattr(words, "data_ptr"):
        words = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(torch.device("cuda", device))
    if words.numel() < n_words:             # rows past the metadata (never written): not allowed
        words = torch.cat([words, torch.zeros(n_words - words.numel(), dtype=words.dtype, device=words.device)])
    if key is not None:
        if len(cache) >= _ALLOW_CACHE_MAX:
            cache.clear()
        cache[key] = (words, n)
    return words, n


def _bm25_filtered(bm, q_terms, q_off, k: int, allow, where, cache: dict):
    """Filtered BM25 top-k on the device (K2f: rank_bm25's statistics over the allowed candidates,
    quirk Q2).  rank_bm25's epsilon floor (0.25 x the mean idf over the candidates' vocabulary,
    needed when some query term's idf is negative) depends on the candidate set only, not on the
    query, so it is computed once per (BM25 version, filter) -- a pass over every posting -- and
    handed to later searches with the same filter."""
    import torch
    index = bm._index
    if getattr(index, "sharded", False):        # multidev: the candidates' statistics over every shard
        return index.search_filtered(q_terms, q_off, k, allow)
    index.prepare_filtered()                    # the device log table (once per index)
    fk = _filter_key(bm._meta, where, "bm25")
    ekey = None if fk is None else ("eps", bm._uid, bm._version) + fk
    eps_t = cache.get(ekey) if ekey is not None else None
    s, r, st = index.search_filtered_dev(q_terms, q_off, k, allow, eps=eps_t)
    code = int(st.item())
    if code & index.FILT_EPS_MISSING:
        eps_t = torch.tensor([index.filter_eps(allow)], dtype=torch.float64, device=q_terms.device)
        if ekey is not None:
            cache[ekey] = eps_t
        s, r, st = index.search_filtered_dev(q_terms, q_off, k, allow, eps=eps_t)
        code = int(st.item())
    if code & index.FILT_ZERO_DIV:
        raise ZeroDivisionError("float division by zero (candidate documents have no tokens)")
    if code:
        raise RuntimeError(f"filtered BM25 search status {code}")
    return s, r


def _keymap(vs, bm, device: int) -> _KeyMap:
    key = (vs._uid, vs._version, bm._uid, bm._version)   # the stores themselves (never-reused uids)
    km = _KEYMAPS.get(key)
    if km is None:
        km = _KeyMap(vs, bm, device)
        if len(_KEYMAPS) >= _KEYMAPS_MAX:
            _KEYMAPS.clear()
        _KEYMAPS[key] = km
    return km


def _side_stream(dev, main):
    import torch
    if os.environ.get("CLASSMATE_BM25_SAME_STREAM") == "1":     # A/B: the serial schedule
        return main
    side = _SIDE_STREAMS.get(dev)
    if side is None:
        side = _SIDE_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return side


def retrieve_batch(retr, questions: Sequence[str], top_k: int,
                   filters: Optional[Dict[str, Any]] = None) -> Optional[List[List[Dict[str, Any]]]]:
    """retr.retrieve_batch(questions, filters, top_k, hybrid=True) on the device (see module
    docstring); the caller checked ``applicable``.  Returns None when a filter leaves fewer vectors
    than the MMR pool (the host path then clamps k as the reference does)."""
    import torch
    from .filters import build_where_filter
    vs, bm = retr.vector_store, retr.bm25_store
    index = vs._index
    dev = torch.device("cuda", index.device)
    nq = len(questions)
    kv, kb = retr.k_vector, retr.k_bm25
    pool = max(kv, retr.mmr_max_pool)
    bm._ensure_index()
    allow_v = allow_b = None
    cache = _ALLOW_CACHE
    if filters:
        chroma_where = build_where_filter(filters)
        if chroma_where:
            allow_v, n_ok = _allow(vs._meta, chroma_where, "chroma", index.device, (index.size + 31) // 32, cache)
            if n_ok < pool:
                return None
        bm._ensure_meta()
        allow_b, n_cand = _allow(bm._meta, filters, "bm25", index.device, (len(bm._id_list) + 31) // 32, cache)
        kb = min(kb, n_cand)
    km = _keymap(vs, bm, index.device)
    # BM25 runs on a side stream that waits only for the allow bitmaps / key map above, so it
    # overlaps the encode and the dense search (a filtered search's status read then waits for the
    # BM25 kernels alone, not for the dense scan queued ahead of it)
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev, main)
    ready = torch.cuda.Event()
    ready.record(main)
    # E5 encode first (its launches return at once), so the host tokenizes the BM25 queries while
    # the device encodes; then dense pool + MMR
    q = _query_vectors(retr.embedder, questions, dev)
    # the certificate's exact pass (device-gated; normally nothing runs) waits for the BM25 join
    # below: its large-LDS grid would otherwise queue behind the BM25 kernels on the CUs
    d, r = index.search_dev(q, pool, allow=allow_v, defer_exact=True)
    blank = np.array([not q_.strip() for q_ in questions], bool)
    qids = [[] if blank[i] else bm._query_ids(q_) for i, q_ in enumerate(questions)]
    off = np.zeros(nq + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in qids])
    flat = np.asarray([t for x in qids for t in x] or [0], np.int32)
    with torch.cuda.stream(side):
        side.wait_event(ready)
        # pinned, stream-ordered copies: a pageable copy would wait here for the encode and search
        q_terms = torch.from_numpy(flat).pin_memory().to(dev, non_blocking=True)
        q_off = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
        # BM25 top-k (whitespace-only queries: no BM25 list, bm25.py:178); with a filter, rank_bm25's
        # statistics over the allowed candidates (K2f; no candidate: empty lists, bm25.py:187)
        if allow_b is None:
            bs, br = bm._index.search_dev(q_terms, q_off, kb)
        elif kb > 0:
            bs, br = _bm25_filtered(bm, q_terms, q_off, kb, allow_b, filters, cache)
        else:
            bs = torch.zeros((nq, 1), dtype=torch.float64, device=dev)
            br = torch.full((nq, 1), -1, dtype=torch.int64, device=dev)
        bkeys = torch.where(br >= 0, km.bm2key_dev[br.clamp(min=0)], torch.full_like(br, -1))
        if blank.any():
            blank_dev = torch.from_numpy(blank).pin_memory().to(dev, non_blocking=True)
            bkeys = torch.where(blank_dev[:, None], torch.full_like(bkeys, -1), bkeys)   # no boolean-index sync
    main.wait_stream(side)
    index.exact_fallback_dev(q, pool, (d, r), allow=allow_v)
    vecs = index.gather_dev(r.reshape(-1)).view(nq, pool, index.dim)
    order = engine.mmr_dev(q, vecs, kv, float(retr.mmr_lambda))
    # side-stream tensors read on main: tell the caching allocator, so an exception
    # between here and the host copies below cannot recycle their blocks under main's kernels
    for t in (bs, br, bkeys, q_terms, q_off):
        t.record_stream(main)
    return _merge_and_build(retr, km, r, d, order, bkeys, bs, top_k, kv + kb)


def _merge_and_build(retr, km, r, d, order, bkeys, bs, top_k: int, n_items: int) -> List[List[Dict[str, Any]]]:
    """The tail both chains share: pool preparation + RRF merge (K5) on torch's current stream, one
    device-to-host copy, result dicts of the final items.  r, d: the (nq, pool) rows and distances
    (row -1 = no entry); order: K4's MMR order; bkeys, bs: the BM25 lists as merge keys and scores
    (key -1 = no entry); n_items: an upper bound of the items of one question (k for top_k <= 0)."""
    import torch
    vs, bm = retr.vector_store, retr.bm25_store
    nq = r.shape[0]
    vk, vd, vn, bn = engine.rrf_pool_prep_dev(r.contiguous(), d.contiguous(), order, bkeys.contiguous())
    k_dev = top_k if top_k > 0 else n_items
    ok, of, ov, ob, ofl, on = engine.rrf_merge_dev(vk, vd, vn, bkeys.contiguous(), bs.contiguous(), bn,
                                                   w_vec=retr.weight_vector, w_bm25=retr.weight_bm25,
                                                   rrf_k=retr.rrf_k, top_k=k_dev)
    # one device-to-host copy of all six outputs (byte views concatenated; six .cpu() calls were six
    # synchronising copies), then Python lists once (per-element numpy indexing + float() costs ~40 %
    # of the dict loop)
    outs = (ok, of, ov, ob, ofl, on)
    blob = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in outs]).cpu().numpy()
    parts, o = [], 0
    for t in outs:
        nb = t.numel() * t.element_size()
        arr = blob[o:o + nb].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape))
        parts.append(arr.tolist())
        o += nb
    ok, of, ov, ob, ofl, on = parts
    flush = getattr(retr.embedder, "flush_pending", None)     # CachingEmbedder: the misses' .npy files
    if flush is not None:
        flush()
    # result dicts of the final top_k items only (fusion.py:132-167 field rules)
    out: List[List[Dict[str, Any]]] = []
    nvr, vs2bm = km.nvr, km.vs2bm
    vids, vdocs, vmetas = vs._ids, vs._docs, vs._meta.metas
    bids, entries = bm._id_list, bm._entries
    dget = dict.__getitem__            # the catalog's stored value without its Python __getitem__ frame;
                                       # a pending (int: not yet parsed) record goes through entries[...]
    for i in range(nq):
        m = len(range(on[i])[:top_k])                    # Python slice of the full order
        res = []
        oki, fli, ofi, ovi, obi = ok[i], ofl[i], of[i], ov[i], ob[i]
        for j in range(m):
            kk, fl = oki[j], fli[j]
            if fl & 1:                                   # a vector item (the vector store's fields first)
                _id = vids[kk]
                doc, meta = vdocs[kk], vmetas[kk] or {}
                if fl & 2 and (not doc or not meta):
                    key = bids[int(vs2bm[kk])]
                    e = dget(entries, key)
                    if type(e) is int:
                        e = entries[key]
                    if not doc and e.text:
                        doc = e.text
                    if not meta and e.metadata:
                        meta = e.metadata
            else:                                        # BM25-only: the BM25 entry's fields (fusion.py:146-151)
                key = bids[int(vs2bm[kk])] if kk < nvr else bids[kk - nvr]
                e = dget(entries, key)
                if type(e) is int:
                    e = entries[key]
                _id, doc, meta = e.id, e.text or None, e.metadata or {}
            res.append({"id": _id, "document": doc, "metadata": meta,
                        "scores": {"vector_distance": ovi[j] if fl & 1 else None,
                                   "bm25_score": obi[j] if fl & 2 else None,
                                   "fused": ofi[j]}})
        out.append(res)
    return out


# Epsilon floors of a batch with per-question clauses, one float per (BM25 version, clause), keyed
# like _bm25_filtered's: the largest single cost of either BM25 route depends on the clause and the
# index only.  The row-list calls take and return them through eps_io, the per-clause filtered
# searches through _bm25_filtered's cache argument.  _ALLOW_CACHE's rule (cleared when full) with a
# bound of its own: an entry here is one float, not a bitmap of the corpus, and a batch may carry
# hundreds of distinct clauses.
_EPS_CACHE: dict = {}
_EPS_CACHE_MAX = 4096


def _eps_key(bm, clause):
    """_bm25_filtered's key of a clause's floor (None: the clause has no stable form, not cached)."""
    fk = _filter_key(bm._meta, clause, "bm25")
    return None if fk is None else ("eps", bm._uid, bm._version) + fk


def _eps_store(key, eps: float) -> None:
    if len(_EPS_CACHE) >= _EPS_CACHE_MAX:
        _EPS_CACHE.clear()
    _EPS_CACHE[key] = eps


def _dev_words(words, n_words: int, dev):
    """A where_bits bitmap (host words or a device tensor) as a device tensor of >= n_words words."""
    import torch
    if not hasattr(words, "data_ptr"):
        words = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)
    if words.numel() < n_words:             # rows past the metadata (never written): not allowed
        words = torch.cat([words, torch.zeros(n_words - words.numel(), dtype=words.dtype, device=words.device)])
    return words


def _rows_index(sel, dev):
    import torch
    return torch.from_numpy(np.asarray(sel, np.int64)).pin_memory().to(dev, non_blocking=True)


def retrieve_batch_clauses(retr, questions: Sequence[str], top_k: int, filters) -> List[List[Dict[str, Any]]]:
    """retr.retrieve_batch(questions, filters=[one per question], top_k, hybrid=True) on the device;
    the caller checked ``applicable_clauses`` and the length of ``filters``.  Both stores plan the
    batch exactly as their host routes do (GpuVectorStore._plan_clauses, BM25Store._plan_clauses:
    one evaluation per distinct clause, scans for the unselective ones, row-list searches for the
    others), every search lands in one (nq, pool) / (nq, k_bm25) pair of device tensors padded with
    row -1, and the rest is ``retrieve_batch``'s: gather + K4 with the pools' own lengths, BM25 on
    the side stream, K5, result dicts for the final items only."""
    import torch
    from .filters import build_where_filter
    vs, bm = retr.vector_store, retr.bm25_store
    index, bindex = vs._index, bm._index
    dev = torch.device("cuda", index.device)
    nq = len(questions)
    kv, kb = retr.k_vector, retr.k_bm25
    pool = max(kv, retr.mmr_max_pool)
    chroma_where = [build_where_filter(f) if f else None for f in filters]
    vplan = vs._plan_clauses(chroma_where, pool)
    bplan = bm._plan_clauses(questions, [f or None for f in filters], kb)   # (blank questions count, as on the host)
    bindex = bm._index
    km = _keymap(vs, bm, index.device)
    nwv, nwb = (index.size + 31) // 32, (len(bm._id_list) + 31) // 32
    main = torch.cuda.current_stream(dev)
    side = _side_stream(dev, main)
    ready = torch.cuda.Event()
    ready.record(main)              # the bitmaps and the key map
    # ---- dense, asynchronous part: encode, the unfiltered search, one scan per unselective clause ----
    q = _query_vectors(retr.embedder, questions, dev)
    d = torch.zeros((nq, pool), dtype=torch.float32, device=dev)
    r = torch.full((nq, pool), -1, dtype=torch.int64, device=dev)

    def put(dst, sel, parts):
        at = _rows_index(sel, dst[0].device)
        for t, p in zip(dst, parts):
            t[at, :p.shape[1]] = p

    if vplan["plain"]:
        # (applicable: at least `pool` live rows, so the host path's k clamp leaves pool)
        sel = vplan["plain"]
        put((d, r), sel, index.search_dev(q.index_select(0, _rows_index(sel, dev)), pool))
    for sel, k, allow in vplan["scan"]:
        # defer_exact=False: the deferred form parks its state in the index's one workspace
        put((d, r), sel, index.search_dev(q.index_select(0, _rows_index(sel, dev)), k,
                                          allow=_dev_words(allow, nwv, dev)))
    # ---- BM25 on the side stream; its list calls block the host while the dense work above runs ----
    blank = [not q_.strip() for q_ in questions]
    with torch.cuda.stream(side):
        side.wait_event(ready)
        bs = torch.zeros((nq, kb), dtype=torch.float64, device=dev)
        br = torch.full((nq, kb), -1, dtype=torch.int64, device=dev)
        keep = [bs, br]

        def terms(sel):
            qids = [bm._query_ids(questions[i]) for i in sel]
            off = np.zeros(len(sel) + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in qids])
            flat = np.asarray([t for x in qids for t in x] or [0], np.int32)
            qt = torch.from_numpy(flat).pin_memory().to(dev, non_blocking=True)
            qo = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
            keep.extend((qt, qo))
            return qids, qt, qo

        sel = [i for i in bplan["plain"] if not blank[i]]
        if sel:
            _, qt, qo = terms(sel)
            put((bs, br), sel, bindex.search_dev(qt, qo, kb))
        for sel, clause, bits, k in bplan["scan"]:
            sel = [i for i in sel if not blank[i]]
            if not sel or k <= 0:
                continue
            _, qt, qo = terms(sel)
            # _bm25_filtered keeps a floor as a device tensor under the key it forms itself: hand it
            # this clause's entry of _EPS_CACHE alone, and take a floor it had to compute back
            key = _eps_key(bm, clause)
            known = _EPS_CACHE.get(key) if key is not None else None
            one = {} if known is None else {key: torch.tensor([known], dtype=torch.float64, device=dev)}
            put((bs, br), sel, _bm25_filtered(bm, qt, qo, k, _dev_words(bits[0], nwb, dev), clause, one))
            if known is None and key in one:
                _eps_store(key, float(one[key].item()))
        for sel, k, words, filter_of, clauses in bplan["lists"]:
            qids = [bm._query_ids(questions[i]) for i in sel]
            keys = [_eps_key(bm, c) for c in clauses]
            eps = np.array([_EPS_CACHE.get(key, np.nan) if key is not None else np.nan for key in keys], np.float64)
            known = ~np.isnan(eps)
            s_, r_, _ = bindex.search_lists(qids, k, words, filter_of, dev=True, eps_io=eps)
            for key, e, was in zip(keys, eps.tolist(), known.tolist()):
                if key is not None and not was and e == e:      # computed by this call
                    _eps_store(key, e)
            keep.extend((s_, r_))
            put((bs, br), sel, (s_, r_))
        bkeys = torch.where(br >= 0, km.bm2key_dev[br.clamp(min=0)], torch.full_like(br, -1))
        keep.append(bkeys)
    # ---- dense, blocking part: the row-list searches (consume q in main's order) ----
    for sel, k, words, filter_of in vplan["lists"]:
        put((d, r), sel, index.search_lists(q.index_select(0, _rows_index(sel, dev)), k, words, filter_of, dev=True))
    # ---- finish: join, K4 over the pools' own lengths, K5 ----
    main.wait_stream(side)
    for t in keep:
        t.record_stream(main)
    n_valid = (r >= 0).sum(dim=1).to(torch.int32)
    vecs = index.gather_dev(r.reshape(-1)).view(nq, pool, index.dim)     # row -1: zeros
    order = engine.mmr_dev(q, vecs, kv, float(retr.mmr_lambda), n_valid=n_valid)
    return _merge_and_build(retr, km, r, d, order, bkeys, bs, top_k, kv + kb)
