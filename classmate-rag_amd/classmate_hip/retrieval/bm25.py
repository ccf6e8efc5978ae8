"""BM25 lexical store, drop-in for ``rag.retrieval.bm25.BM25Store``.

Same dataclass fields, methods, JSONL persistence format and return dicts as
rag/retrieval/bm25.py:114-256.  Tokenization stays on the host (same regex,
stopwords and language handling); the index lives in HBM as CSR postings
(``engine.BM25Index``) and ``search`` is the HIP kernels K2/K3 with
rank_bm25 0.2.x semantics — statistics over the filtered candidates (Q2),
duplicate query tokens counted twice (Q3), zero-score padding in insertion
order (Q1), ZeroDivisionError on an all-empty vocabulary (Q7).

The reference rebuilds BM25Okapi on every mutation and again per search; here
mutations mark the device index dirty and the next search brings it up to date
once.  What happened since the last search decides how:

* left in place (no token list, term id or record of a document that stays is read):
  - upserts of ids new to the store: their rows are appended (``engine.BM25Index.append``);
  - deletes: their rows are dropped (``engine.BM25Index.remove``, a device-side compaction
    of the postings);
  - upserts of ids the store holds: the documents keep their rows
    (``engine.BM25Index.replace``).  One 4096-chunk file replaced in a 10M-chunk index
    costs 0.17 s against the 25.6 s rebuild, a uniform 1 % of the chunks 0.20 s
    (profiles/bm25_replace.txt).
* still a rebuild:
  - a delete that follows a replace before the next search;
  - the first replace on a store opened from its sidecar (it parses the catalog, as before);
  - every replace on the sharded index (``multidev.ShardedBM25Index`` has no ``replace``).
* order: any sequence of such calls between two searches is recorded
  (``_BState.pending_drop`` / ``pending_replace`` / ``pending_row``) and applied as at
  most one ``remove``, then at most one ``replace``, then at most one ``append``.

Persistence: ``save`` writes the reference's JSONL catalog
unchanged (bm25.py:220-231) plus a binary sidecar ``<index_file>.cm/`` -- the
CSR term ids, document offsets, vocabulary and each record's byte offset in the
JSONL.  ``load`` checks the sidecar against the JSONL's size and mtime and, when
it matches, builds the device index straight from the memory-mapped CSR: no JSON
parsing, re-tokenisation or vocabulary mapping at open.  Records are parsed one
by one when a search returns them; metadata is parsed in full only when a
``where`` filter first needs it, and a mutation or ``save`` materializes every
record.  A missing or stale sidecar falls back to the reference's full parse.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import json
import os
import shutil
import threading
import weakref
from collections import OrderedDict
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np

from .. import engine, multidev
from .filters import MetaIndex, next_uid, settle_loaded
from .tokenize import _tokenize, detect_lang_tag


@dataclass
class _Entry:
    id: str
    text: str
    tokens: List[str]
    metadata: Dict[str, Any]
    term_ids: Optional[np.ndarray] = None


_SIDECAR_VERSION = 1

# search_batch(where=[...]): vector_store.route_clauses under BM25's own constants.  A clause that
# allows more than num_docs / BM25_LIST_CUTOFF_DIV rows, or whose questions x allowed rows pass
# num_docs / BM25_LIST_PAIR_DIV, runs the ordinary filtered search once per clause; more selective
# ones share row-list searches (engine.BM25Index.search_lists).  Measured (profiles/bm25_lists.txt,
# 1M documents, medians of 30; DESIGN §3 "BM25 row-list search"), by the dense constants' rule -- half
# of the largest measured share at which the list route still wins: with one question per clause it
# wins at N/1024 (1.38 x) and N/64 (1.14 x), the largest share timed at 30 repetitions, so 128; with
# 16 per clause it still wins at N/8 (1.05 x) = 2 pairs per document, so 1.  $CM_BM25_LIST_CUTOFF_DIV
# (read at every call) overrides the first and switches the pair rule off: 1 sends every clause to
# the list route, a value above the store's size none.
BM25_LIST_CUTOFF_DIV = 128
BM25_LIST_PAIR_DIV = 1
# (query, allowed row) pairs per search_lists call: 24 bytes of keys and rows each, 32M pairs = 768 MiB
BM25_LIST_PAIR_BUDGET = 32 << 20


def _entry_of(rec: Mapping[str, Any]) -> _Entry:
    """bm25.py:240-245: one JSONL record -> _Entry."""
    return _Entry(id=rec["id"], text=rec.get("text", ""), tokens=list(rec.get("tokens", [])),
                  metadata=dict(rec.get("metadata", {})))


class _Catalog(dict):
    """id -> _Entry, in insertion order.  Opened from a sidecar, values start as JSONL line numbers
    and a record is parsed on first read (search results); ``values``/``items``/``materialize``
    parse every pending record in one sequential pass."""

    def __init__(self):
        super().__init__()
        self._src = None  # (jsonl path, line byte offsets, CSR term ids, doc offsets)
        self._fh = None
        self._lock = threading.Lock()   # the shared file object: seek + read as a unit

    def attach(self, path: Path, ids: Sequence[str], line_off, term_ids, doc_off) -> None:
        self._src = (path, line_off, term_ids, doc_off)
        for r, i in enumerate(ids):
            dict.__setitem__(self, i, r)

    @property
    def pending(self) -> bool:
        return self._src is not None

    def _finish(self, row: int, rec: Mapping[str, Any]) -> _Entry:
        _, _, terms, doc_off = self._src
        e = _entry_of(rec)
        e.term_ids = np.array(terms[int(doc_off[row]): int(doc_off[row + 1])], np.int32)
        return e

    def _parse(self, row: int) -> _Entry:
        path, line_off = self._src[0], self._src[1]
        with self._lock:
            if self._fh is None:
                self._fh = open(path, "rb")
            self._fh.seek(int(line_off[row]))
            blob = self._fh.read(int(line_off[row + 1] - line_off[row]))
        return self._finish(row, json.loads(blob))

    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        if type(v) is int:
            v = self._parse(v)
            dict.__setitem__(self, key, v)
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def pop(self, key, *default):
        v = dict.pop(self, key, *default)
        return self._parse(v) if type(v) is int and self._src is not None else v

    def materialize(self) -> None:
        if self._src is None:
            return
        pending = {v: k for k, v in dict.items(self) if type(v) is int}
        if pending:
            with open(self._src[0], "rb") as f:
                for row, line in enumerate(f):
                    key = pending.get(row)
                    if key is not None:
                        dict.__setitem__(self, key, self._finish(row, json.loads(line)))
        self.detach()

    def detach(self) -> None:
        with self._lock:
            if self._fh is not None:
                self._fh.close()
            self._src = self._fh = None

    def values(self):
        self.materialize()
        return dict.values(self)

    def items(self):
        self.materialize()
        return dict.items(self)

    def clear(self):
        self.detach()
        dict.clear(self)


class _BState:
    """One BM25 index's in-memory state (catalog, vocabulary, device index, metadata).  Instances
    loaded from one JSONL file share it while it matches the file (see BM25Store.load)."""

    def __init__(self):
        self.entries: Dict[str, _Entry] = _Catalog()
        self.id_list: List[str] = []
        self.vocab: Dict[str, int] = {}
        self.index: Optional[engine.BM25Index] = None
        self.meta = MetaIndex()
        self.dirty = True
        self.meta_dirty = True
        self.csr: Optional[tuple] = None   # persisted (term_ids, doc_off) to build from
        # the same once rows were appended behind it: the CSR of the first len(doc_off) - 1 rows, to
        # build from before the others are appended (their records are never read for it)
        self.prefix_csr: Optional[tuple] = None
        # set while the device index lacks nothing but the rows from this one on (append-only upserts
        # since it was current): the next search appends them instead of rebuilding
        self.pending_row: Optional[int] = None
        # device rows (ascending, unique) of documents deleted since the index was current: the next
        # search drops them first (engine.BM25Index.remove); pending_row counts in the numbering
        # after that drop.  Together: "drop these device rows, then append the rows from pending_row on"
        self.pending_drop: Optional[np.ndarray] = None
        # ids replaced in place since the index was current: the next search replaces their rows
        # (engine.BM25Index.replace) after the drop and before the append; an id whose row lies in
        # the tail yet to be appended needs nothing, the append reads its current entry
        self.pending_replace: set = set()
        # tokens of all documents in the store, kept in step by deletes and appends once a delete on
        # the device index has seeded it (None: not known); decides bm25.py:145 without the catalog
        self.ntokens: Optional[int] = None
        self.version = 0                   # bumped by every change of the document set
        self.uid = next_uid()              # identity in device caches (never reused)
        self.sig = None                    # the JSONL (+ sidecar) signature it was loaded from / saved to
        self.unsaved = False               # mutated since: private to its holder
        self.holders = weakref.WeakValueDictionary()   # id(store) -> store (dataclasses are unhashable)
        # the JSONL + sidecar this state last wrote or read (path, JSONL size / mtime, record count, line
        # and document offsets, term ids); while only new documents were appended since (append_only),
        # the next save appends their records instead of rewriting the file (same bytes either way)
        self.saved: Optional[dict] = None
        self.append_only = False
        # serialises the state's users (stores attached to it, threads): the device handle's search
        # staging and workspace are per handle (SURVEY §8(b) Threading)
        self.lock = threading.RLock()

    def clone(self) -> "_BState":
        """A private copy for a holder that mutates a shared state (the reference's instances are
        independent copies of the file): host tables copied, the device index and metadata rebuilt
        on demand."""
        st = _BState()
        cat = _Catalog()
        # the clone's own _Entry objects: term ids are filled in lazily against the holder's vocab
        # (_ensure_index / save), so shared entries would carry the other state's ids;
        # pending records (ints: not parsed yet) are parsed by each catalog on its own
        dict.update(cat, ((k, v if type(v) is int else dataclasses.replace(v))
                          for k, v in dict.items(self.entries)))
        cat._src = self.entries._src if isinstance(self.entries, _Catalog) else None
        st.entries = cat
        st.id_list = list(self.id_list)
        st.vocab = dict(self.vocab)
        st.csr = self.csr
        st.prefix_csr = self.prefix_csr   # (pending_row stays None: the clone builds from it, then appends)
        st.version = self.version
        return st


def _jsonl_sig(path) -> Optional[tuple]:
    try:
        s = os.stat(path)
        return (s.st_size, s.st_mtime_ns)
    except OSError:
        return None


def _file_sig(store) -> Optional[tuple]:
    out = []
    for p in (store.index_path, store.sidecar_dir / "meta.json"):
        try:
            s = os.stat(p)
            out.append((s.st_size, s.st_mtime_ns))
        except OSError:
            out.append(None)
    return tuple(out)


class _CatalogMetas(list):
    """MetaIndex.metas of a sidecar-opened store: row r's metadata dict, parsed from its JSONL
    record on first access (the same parse the catalog does for a search result)."""

    def __init__(self, n: int, cat: "_Catalog", ids: List[str]):
        super().__init__([None] * n)
        self.cat, self.ids, self.done = cat, ids, bytearray(n)

    def __getitem__(self, r):
        if isinstance(r, int) and r < len(self.done) and not self.done[r]:
            list.__setitem__(self, r, self.cat[self.ids[r]].metadata)
            self.done[r] = 1
        return list.__getitem__(self, r)

    def __setitem__(self, r, v):
        if isinstance(r, int) and r < len(self.done):
            self.done[r] = 1
        list.__setitem__(self, r, v)


def _load_meta_snapshot(side: Path, n: int, cat: "_Catalog", ids: List[str]) -> Optional[MetaIndex]:
    try:
        info = json.loads((side / "meta_info.json").read_text(encoding="utf-8"))
        arrays = {p.stem[len("meta_"):]: np.load(p) for p in side.glob("meta_*.npy")}
    except (OSError, ValueError):
        return None
    if int(info.get("rows", -1)) > n:
        return None
    m0 = int(info["rows"])
    if m0 < n:   # trailing documents without metadata columns: pad the arrays
        for k in [k for k in arrays if k.endswith("_py") or k.endswith("_ty")]:
            arrays[k] = np.concatenate([arrays[k], np.full(n - m0, -1, np.int32)])
        arrays["live"] = np.concatenate([arrays["live"], np.ones(n - m0, bool)])
        info["rows"] = n
    try:
        return MetaIndex.from_snapshot(info, arrays, _CatalogMetas(n, cat, ids))
    except (KeyError, ValueError):
        return None


def _compacted_meta(meta: MetaIndex, keep: np.ndarray, cat, ids: List[str]) -> MetaIndex:
    """MetaIndex.compacted(keep) that leaves a sidecar-opened store's unparsed metadata unparsed:
    the rows' raw slots move (None where a record is not parsed yet) and the result's ``metas``
    parse on demand against the new id list."""
    lazy = meta.metas if isinstance(meta.metas, _CatalogMetas) else None
    if lazy is None:
        return meta.compacted(keep)
    meta.metas = list(lazy)                    # (list's own iterator: raw slots, nothing parsed)
    try:
        m = meta.compacted(keep)
    finally:
        meta.metas = lazy
    done = np.ones(len(m.metas), np.uint8)
    old = keep < len(lazy.done)                # (rows behind the opened ones were set, not parsed)
    done[old] = np.frombuffer(lazy.done, np.uint8)[keep[old]]
    out = _CatalogMetas(len(m.metas), cat, ids)
    list.__setitem__(out, slice(None), m.metas)
    out.done = bytearray(done.tobytes())
    m.metas = out
    return m


_REGISTRY: "OrderedDict[tuple, _BState]" = OrderedDict()
_REGISTRY_MAX = 8
_REG_LOCK = threading.Lock()


def release_all() -> None:
    """Forget every registered BM25 state (freed once no store holds it)."""
    with _REG_LOCK:
        _REGISTRY.clear()


def _proxy(name: str):
    return property(lambda self: getattr(self._st, name), lambda self, v: setattr(self._st, name, v))


@contextlib.contextmanager
def _store_lock(store):
    """This store's lock, then its current state's: the first serialises the threads that use one
    BM25Store object (a copy on write swaps its state), the second the stores sharing a state."""
    with store._obj_lock:
        with store._st.lock:
            yield


def _locked(fn):
    @functools.wraps(fn)
    def run(self, *a, **kw):
        with _store_lock(self):
            return fn(self, *a, **kw)
    return run


@dataclass
class BM25Store:
    index_dir: Optional[Path] = Path("./indexes/bm25")
    index_file: str = "bm25_index.jsonl"
    device: Optional[int] = None

    _entries = _proxy("entries")
    _id_list = _proxy("id_list")
    _vocab = _proxy("vocab")
    _index = _proxy("index")
    _meta = _proxy("meta")
    _dirty = _proxy("dirty")
    _meta_dirty = _proxy("meta_dirty")
    _csr = _proxy("csr")
    _prefix_csr = _proxy("prefix_csr")
    _pending_row = _proxy("pending_row")
    _pending_drop = _proxy("pending_drop")
    _pending_replace = _proxy("pending_replace")
    _ntokens = _proxy("ntokens")
    _version = _proxy("version")
    _uid = _proxy("uid")

    def __post_init__(self):
        self._obj_lock = threading.RLock()
        self._st = _BState()
        self._st.holders[id(self)] = self

    def lock(self):
        """This store's locks as one context (HybridRetriever holds it across a whole retrieve)."""
        return _store_lock(self)

    def _set_state(self, st: "_BState") -> None:
        self._st.holders.pop(id(self), None)
        self._st = st
        st.holders[id(self)] = self

    def _registry_key(self):
        dev = engine.default_device() if self.device is None else int(self.device)
        return (str(Path(self.index_path).resolve()), dev, os.environ.get("CM_DEVICES", "") if self.device is None else "")

    def _mutating(self) -> None:
        """Before a change of the document set: a state other stores also hold is copied first."""
        if len(self._st.holders) > 1:
            self._set_state(self._st.clone())
        self._st.unsaved = True

    # ---------- core ops ----------
    def _term_ids(self, tokens: Sequence[str]) -> np.ndarray:
        v = self._vocab
        return np.fromiter((v.setdefault(t, len(v)) for t in tokens), dtype=np.int32, count=len(tokens))

    def _rebuild(self) -> None:
        """bm25.py:140-145: the reference rebuilds BM25Okapi here; it raises ZeroDivisionError when
        entries exist but every token list is empty.  We check that and defer the device build."""
        self._id_list = list(self._entries.keys())
        self._version += 1
        self._csr = self._prefix_csr = self._ntokens = None
        self._clear_pending()
        if self._entries and all(len(e.tokens) == 0 for e in self._entries.values()):
            raise ZeroDivisionError("float division by zero")
        self._dirty = self._meta_dirty = True

    def _clear_pending(self) -> None:
        self._pending_row = self._pending_drop = None
        self._pending_replace = set()

    def _tracked(self) -> bool:
        """The device index exists and is current, or lacks only what is recorded as pending (rows to
        drop, rows to replace, rows to append)."""
        return self._index is not None and (not self._dirty or self._pending_row is not None
                                            or self._pending_drop is not None or bool(self._pending_replace))

    def _appended(self, new_ids: Sequence[str]) -> None:
        """_rebuild after an upsert of ids new to the store only: they are the rows after the existing
        ones, so the device index (or the persisted CSR it is yet to be built from) stays a valid
        prefix and _ensure_index appends to it.  No earlier record is read."""
        n0 = len(self._id_list)
        self._id_list.extend(new_ids)
        self._version += 1
        if self._csr is not None:   # no longer the whole index
            self._prefix_csr, self._csr = self._csr, None
        if all(len(self._entries[i].tokens) == 0 for i in new_ids):   # bm25.py:145 over all entries
            c, tokens = 0, 0
            if self._ntokens is not None:      # the count kept since a delete or replace seeded it
                c, tokens = n0, self._ntokens
            elif self._prefix_csr is not None:   # the persisted rows' token count stands for their records
                c, tokens = len(self._prefix_csr[1]) - 1, int(self._prefix_csr[1][-1])
            if tokens == 0 and all(len(self._entries[i].tokens) == 0 for i in self._id_list[c:n0]):
                raise ZeroDivisionError("float division by zero")
        if self._ntokens is not None:
            self._ntokens += sum(len(self._entries[i].tokens) for i in new_ids)
        if self._tracked() and self._pending_row is None:   # from now on the index also lacks the rows from n0 on
            self._pending_row = n0
        self._dirty = True

    def _removable(self) -> bool:
        """delete_many may leave the device index in place: it is _tracked() and can drop rows.  Pending
        replaces are applied to rows in the numbering before the delete: a delete after them rebuilds."""
        return self._tracked() and not self._pending_replace and hasattr(self._index, "remove")

    def _removed(self, popped: Sequence[tuple]) -> None:
        """_rebuild after a delete, on an index that _removable(): the popped documents' rows are
        found in one pass over the id list and recorded for _ensure_index -- device rows to drop, or
        rows taken out of the tail yet to be appended.  No record, token list or term id of a
        document that stays is read.  ``popped``: (id, its _Entry) of the popped documents."""
        gone = dict(popped)
        old_ids = self._id_list
        n0 = len(old_ids)
        self._seed_ntokens(gone)
        self._ntokens -= sum(len(e.tokens) for e in gone.values())
        rows = np.fromiter((r for r, i in enumerate(old_ids) if i in gone), np.int64)
        self._id_list = [i for i in old_ids if i not in gone]
        self._version += 1
        self._csr = self._prefix_csr = None
        have = n0 if self._pending_row is None else self._pending_row
        held = rows[rows < have]               # rows the device holds, in the numbering after the pending drop
        if held.shape[0]:
            drop = self._pending_drop if self._pending_drop is not None else np.zeros(0, np.int64)
            # device row of store row i: i + k, k = the pending drops at or below it (drop[j] - j <= i)
            k = np.searchsorted(drop - np.arange(drop.shape[0]), held, side="right")
            self._pending_drop = np.union1d(drop, held + k)
            if self._pending_row is not None:
                self._pending_row -= int(held.shape[0])
            self._dirty = True
        if not self._meta_dirty and rows.shape[0]:   # the filter columns follow (as GpuVectorStore.compact)
            keep = np.setdiff1d(np.arange(n0, dtype=np.int64), rows, assume_unique=True)
            self._meta = _compacted_meta(self._meta, keep, self._entries, self._id_list)
        if self._ntokens == 0:                 # bm25.py:145: documents remain, every token list is empty
            raise ZeroDivisionError("float division by zero")

    def _replaceable(self) -> bool:
        """upsert_many may leave the device index in place when it replaces documents: it is
        _tracked() and can replace rows.  A catalog opened from a sidecar and not parsed yet keeps
        the rebuild, which parses it (tests/test_gpu_dropin.py holds a replace to that)."""
        return (self._tracked() and hasattr(self._index, "replace")
                and not getattr(self._entries, "pending", False))

    def _seed_ntokens(self, gone: Optional[Mapping[str, _Entry]] = None) -> None:
        """The token count of all documents, from the index's own count plus the tail it does not hold
        yet (before any entry is overwritten and while the id list still names the documents in
        ``gone``, popped from the catalog; nothing is pending but that tail while it is None)."""
        if self._ntokens is None:
            have = len(self._id_list) if self._pending_row is None else self._pending_row
            self._ntokens = int(self._index.stats()["sum_len"]) + sum(
                len(((gone and gone.get(i)) or self._entries[i]).tokens) for i in self._id_list[have:])

    def _rows_csr(self, r0: int, ids: Optional[Sequence[str]] = None):
        """(term ids, offsets from 0) of rows [r0, n) -- or of the documents ``ids`` -- from their entries."""
        entries = [self._entries[i] for i in (self._id_list[r0:] if ids is None else ids)]
        for e in entries:
            if e.term_ids is None:
                e.term_ids = self._term_ids(e.tokens)
        off = np.zeros(len(entries) + 1, np.int64)
        if entries:
            off[1:] = np.cumsum([e.term_ids.shape[0] for e in entries])
        flat = np.concatenate([e.term_ids for e in entries]) if off[-1] else np.zeros(0, np.int32)
        return flat, off

    def _ensure_index(self) -> None:
        if not self._dirty and self._index is not None:
            return
        if self._index is None:
            self._index = multidev.new_bm25_index(device=self.device)
        n = len(self._id_list)
        drop = self._pending_drop  # device rows to drop first, when deletes are pending
        have = self._pending_row   # rows the device index holds (after that drop), when it is a prefix of the store
        repl = self._pending_replace  # ids whose rows the device index holds with an earlier text
        if drop is not None:
            if have is None:
                have = n
            if hasattr(self._index, "remove") and self._index.num_docs == have + drop.shape[0]:
                self._index.remove(drop)
            else:
                have = None
        elif have is None and repl:
            have = n
        if repl and have is not None and self._index.num_docs == have and hasattr(self._index, "replace"):
            # after the drop the device rows [0, have) are id_list[:have]; a rebuild below reads the
            # current entries and needs none of this
            rows = [r for r, i in enumerate(self._id_list[:have]) if i in repl]
            if rows:
                flat, off = self._rows_csr(0, [self._id_list[r] for r in rows])   # (assigns new terms' ids)
                self._index.replace(np.asarray(rows, np.int64), flat, off, max(len(self._vocab), 1))
        if have is None or self._index.num_docs != have:
            csr = self._csr if self._csr is not None else self._prefix_csr
            if csr is not None:  # opened from a sidecar: the persisted CSR is the index (of its rows)
                term_ids, doc_off = csr
                have = len(doc_off) - 1
                # (the vocabulary may have grown with rows appended since; the CSR's ids are below it)
                self._index.build(np.ascontiguousarray(term_ids), np.ascontiguousarray(doc_off),
                                  max(len(self._vocab), 1))
            else:
                have = n
                flat, off = self._rows_csr(0)     # (assigns the vocabulary's ids: before its size is read)
                self._index.build(flat, off, max(len(self._vocab), 1))
        if have < n:
            flat, off = self._rows_csr(have)
            self._index.append(flat, off, max(len(self._vocab), 1))
        self._clear_pending()
        self._dirty = False

    def _ensure_meta(self) -> None:
        """Row-aligned metadata for where-filters (parses every record of a sidecar-opened store)."""
        if not self._meta_dirty:
            return
        self._meta = MetaIndex()
        for r, i in enumerate(self._id_list):
            self._meta.set(r, self._entries[i].metadata)
        self._meta_dirty = False

    @_locked
    def upsert_many(self, *, ids: Sequence[str], texts: Sequence[str], metadatas: Sequence[Mapping[str, Any]]) -> None:
        """bm25.py:147-166: language from metadata (or detected), tokenize, replace in place.

        Each id is new to the store (its row is appended: once, with the last text given for it),
        or the store holds it (it keeps its row).  On an index that _replaceable() the replaced ids
        are recorded for _ensure_index and no other document's tokens or term ids are read; on any
        other, an id the store holds or one given twice rebuilds."""
        if not (len(ids) == len(texts) == len(metadatas)):
            raise ValueError("ids, texts, metadatas must have the same length")
        self._mutating()
        st = self._st
        in_place = self._replaceable() and any(i in self._entries for i in ids)
        meta_ok = not self._meta_dirty
        n0 = len(self._id_list)
        if in_place:
            held = {i for i in ids if i in self._entries}
            row_of = {i: r for r, i in enumerate(self._id_list) if i in held} if meta_ok else {}
            self._seed_ntokens()
        new_ids, new_meta, only_new = [], {}, True
        for i, doc_id in enumerate(ids):
            meta, toks = self._tokenized(texts[i], metadatas[i])
            if doc_id not in self._entries:
                new_ids.append(doc_id)
                new_meta[doc_id] = meta
            else:
                only_new = st.append_only = False   # the saved records are no longer a prefix
                if doc_id in new_meta:     # given twice: its row is yet to be appended, with its last text
                    new_meta[doc_id] = meta
                elif in_place:
                    self._ntokens += len(toks) - len(self._entries[doc_id].tokens)
                    if meta_ok:            # MetaIndex.set clears the row's old values: while the old entry stands
                        self._meta.set(row_of[doc_id], meta)
                    self._pending_replace.add(doc_id)
            self._entries[doc_id] = _Entry(id=doc_id, text=texts[i] or "", tokens=toks, metadata=meta)
        # What is left to do, by case:
        #   in place (with or without new ids): mark the index stale here, append the new ids below,
        #     and check bm25.py:145 last, against the token count kept since _seed_ntokens;
        #   not in place, an id held or given twice: the rebuild, which does all of it;
        #   not in place, new ids only (or no id at all): _appended alone, which marks and checks.
        if in_place:
            self._version += 1
            self._csr = self._prefix_csr = None        # the persisted CSR no longer describes those rows
            self._dirty = True
        elif not only_new:
            return self._rebuild()
        if new_ids or not in_place:
            self._appended(new_ids)
            if meta_ok:                                # the filter columns follow the appended rows
                for r, doc_id in enumerate(new_ids, n0):
                    self._meta.set(r, new_meta[doc_id])
        if in_place and self._ntokens == 0:            # bm25.py:145: every token list is empty
            raise ZeroDivisionError("float division by zero")

    @staticmethod
    def _tokenized(text, metadata):
        """bm25.py:152-160: (metadata with the language filled in, tokens) of one document."""
        text = text or ""
        meta = dict(metadata or {})
        lang = meta.get("language")
        if not lang or lang == "auto":
            lang = detect_lang_tag(text)
            meta["language"] = lang
        return meta, _tokenize(text, lang_hint=lang)

    @_locked
    def delete_many(self, ids: Sequence[str]) -> None:
        self._mutating()
        self._st.append_only = False
        removable = self._removable()
        popped = []
        for doc_id in ids:
            e = self._entries.pop(doc_id, None)
            if e is not None:
                popped.append((doc_id, e))
        if removable and self._entries:
            self._removed(popped)
        else:
            self._rebuild()

    # ---------- query ----------
    def _query_ids(self, query: str) -> List[int]:
        q_lang = detect_lang_tag(query)
        get = self._vocab.get          # (one proxy-property read, not one per token)
        return [get(t, -1) for t in _tokenize(query, lang_hint=q_lang)]

    def search(self, *, query: str, where: Optional[Mapping[str, Any]] = None, top_k: int = 8) -> List[Dict[str, Any]]:
        """bm25.py:175-212 on the GPU."""
        return self.search_batch(queries=[query], where=where, top_k=top_k)[0]

    @_locked
    def search_batch(self, *, queries: Sequence[str], where=None, top_k: int = 8) -> List[List[Dict[str, Any]]]:
        """Many queries: one device launch per filter (build-side addition).  ``where``: one clause (a
        mapping or None) for the whole batch, or a list / tuple with one clause (or None / {}) per
        query.  BM25 statistics are those of the filtered candidate set (quirk Q2): selective clauses
        share row-list searches that score each under its own statistics, the queries of any other
        distinct clause run the filtered search together (_search_clauses); results in query order."""
        if isinstance(where, (list, tuple)):
            if len(where) != len(queries):
                raise ValueError(f"where holds {len(where)} clauses for {len(queries)} queries")
            return self._search_clauses(queries, where, top_k)
        return self._search_one_clause(queries, where, top_k)

    def _search_clauses(self, queries: Sequence[str], where, top_k: int) -> List[List[Dict[str, Any]]]:
        """search_batch with one where clause (or None / {}) per query: result i equals
        search(query=queries[i], where=where[i]).  Every distinct clause is evaluated once; the
        selective ones (vector_store.route_clauses under BM25's constants) share row-list searches
        (engine.BM25Index.search_lists, each clause with its own statistics: quirk Q2), the others --
        and every clause of a negative top_k or of a sharded index -- run _search_one_clause."""
        out: List[List[Dict[str, Any]]] = [[] for _ in queries]
        plan = self._plan_clauses(queries, where, top_k)

        def per_clause(sel, clause, bits):
            res = self._search_one_clause([queries[i] for i in sel], clause, top_k, bits)
            for i, r in zip(sel, res):
                out[i] = r

        if plan["plain"]:
            per_clause(plan["plain"], None, None)
        for sel, clause, bits, _ in plan["scan"]:
            per_clause(sel, clause, bits)
        for sel, k, words, filter_of, _ in plan["lists"]:
            qids = [self._query_ids(queries[i]) for i in sel]
            scores, rows, nvalid = self._index.search_lists(qids, k, words, filter_of)
            for j, i in enumerate(sel):
                out[i] = [self._hit(s, r) for s, r in zip(scores[j][: nvalid[j]], rows[j][: nvalid[j]])]
        return out

    def _plan_clauses(self, queries: Sequence[str], where, top_k: int):
        """The searches that answer a batch with one where clause per query -- what _search_clauses
        runs with host arrays and device_batch.retrieve_batch_clauses with device tensors, so both
        route alike.  Every distinct clause is evaluated once (group_clauses, where_bits) and routed
        by vector_store.route_clauses under this module's constants and $CM_BM25_LIST_CUTOFF_DIV.
        Returns {"plain": queries without a clause (one unfiltered search), "scan": [(queries,
        clause, where_bits output or None, k)] one filtered search each -- k = min(top_k, Nc), None
        when the clause was not evaluated here (no list route: a negative top_k, a sharded index) --
        and "lists": [(non-blank queries, k, [allow words per bitmap], filter_of, [clause per
        bitmap])], one search_lists call each with k = min(top_k, the largest clause of the call), calls without a non-blank query
        or with k <= 0 left out}.  A query whose clause allows no row is in none of them; plain and
        scan keep their blank queries (_search_one_clause drops them).  Builds the index."""
        from .vector_store import group_clauses, route_clauses
        group_of, clauses = group_clauses(where)
        plan = {"plain": [i for i, g in enumerate(group_of) if g < 0], "scan": [], "lists": []}
        if not clauses or not self._entries:
            return plan
        self._ensure_index()
        idx = self._index
        has_lists = hasattr(idx, "search_lists") and top_k >= 0
        bits = None
        if has_lists:
            self._ensure_meta()
            bits = [engine.where_bits(self._meta, w, "bm25", idx.device) for w in clauses]   # once per distinct clause
        # (without the list route the plan only groups: _search_one_clause evaluates its own clause)
        counts = [n for _, n in bits] if bits else [1] * len(clauses)
        forced = os.environ.get("CM_BM25_LIST_CUTOFF_DIV")
        routed = route_clauses(group_of, counts, len(self._id_list), max(top_k, 0), 1 << 62, has_lists,
                               float(forced or BM25_LIST_CUTOFF_DIV), BM25_LIST_PAIR_BUDGET,
                               0.0 if forced else BM25_LIST_PAIR_DIV)   # forced: rows alone
        for g, sel in routed["scan"]:
            plan["scan"].append((sel, clauses[g], bits[g] if bits else None, min(top_k, counts[g]) if bits else None))
        for call in routed["lists"]:
            sel = [i for _, qs in call for i in qs if queries[i].strip()]   # blank queries give []
            if not sel:
                continue
            filter_of = np.concatenate([np.full(sum(1 for i in qs if queries[i].strip()), f, np.int32)
                                        for f, (_, qs) in enumerate(call)])
            k = min(top_k, max(counts[g] for g, _ in call))   # per clause min(top_k, Nc): nvalid
            if k <= 0:
                continue
            plan["lists"].append((sel, k, [bits[g][0] for g, _ in call], filter_of, [clauses[g] for g, _ in call]))
        return plan

    def _hit(self, score, row) -> Dict[str, Any]:
        e = self._entries[self._id_list[int(row)]]
        return {"id": e.id, "document": e.text, "metadata": e.metadata, "score": float(score)}

    def _search_one_clause(self, queries: Sequence[str], where: Optional[Mapping[str, Any]],
                           top_k: int, bits=None) -> List[List[Dict[str, Any]]]:
        """``bits``: the clause's where_bits output, when the caller has evaluated it already."""
        out: List[List[Dict[str, Any]]] = [[] for _ in queries]
        live = [i for i, q in enumerate(queries) if q.strip()]
        if not live or not self._entries:
            return out
        self._ensure_index()
        allow = None
        if where:  # device-evaluated filter; statistics follow it (Q2)
            self._ensure_meta()
            allow, n_cand = bits or engine.where_bits(self._meta, where, "bm25", self._index.device)
        else:
            n_cand = len(self._id_list)
        if n_cand == 0:
            return out
        k = top_k if top_k >= 0 else n_cand + top_k      # python slice semantics of [:top_k]
        k = min(k, n_cand)
        if k <= 0:
            return out
        # k beyond the fused kernels' lists (cm_max_topk) runs the full-order device path
        qids = [self._query_ids(queries[i]) for i in live]
        scores, rows, nvalid = self._index.search(qids, k, allow)
        for j, i in enumerate(live):
            res = []
            for s, r in zip(scores[j][: nvalid[j]], rows[j][: nvalid[j]]):
                e = self._entries[self._id_list[int(r)]]
                res.append({"id": e.id, "document": e.text, "metadata": e.metadata, "score": float(s)})
            out[i] = res
        return out

    def row_of(self, row: int) -> str:
        return self._id_list[row]

    # ---------- persistence (bm25.py:216-248) ----------
    @property
    def index_path(self) -> Path:
        return Path(self.index_dir) / self.index_file

    @property
    def sidecar_dir(self) -> Path:
        return Path(self.index_dir) / (self.index_file + ".cm")

    @_locked
    def save(self) -> None:
        """bm25.py:220-231 (same JSONL records) + the binary sidecar of the device index."""
        if self.index_dir is None:
            return
        Path(self.index_dir).mkdir(parents=True, exist_ok=True)
        side = self.sidecar_dir
        if (side / "meta.json").exists():
            os.remove(side / "meta.json")  # the sidecar is invalid until rewritten below
        bs = self._st
        sv = bs.saved
        n_all = len(self._entries)
        append = (bs.append_only and sv is not None and sv["path"] == str(self.index_path)
                  and sv["n"] <= n_all and _jsonl_sig(self.index_path) == sv["sig"])
        r0 = sv["n"] if append else 0
        ids_new = self._id_list[r0:] if append else list(self._entries.keys())
        entries = [self._entries[i] for i in ids_new] if append else list(self._entries.values())
        line_off = np.zeros(len(entries) + 1, np.int64)
        doc_off = np.zeros(len(entries) + 1, np.int64)
        parts = []
        # the reference rewrites the whole JSONL (bm25.py:220-231); while only documents were appended
        # since this state's last save or load, the file is that file plus their records: append them
        with self.index_path.open("ab" if append else "wb") as f:
            base = f.tell() if append else 0
            for r, e in enumerate(entries):
                rec = {"id": e.id, "text": e.text, "tokens": e.tokens, "metadata": e.metadata}
                line = (json.dumps(rec, ensure_ascii=False) + "\n").encode("utf-8")
                f.write(line)
                line_off[r + 1] = line_off[r] + len(line)
                if e.term_ids is None:
                    e.term_ids = self._term_ids(e.tokens)
                parts.append(e.term_ids)
                doc_off[r + 1] = doc_off[r] + e.term_ids.shape[0]
        new_terms = np.concatenate(parts) if doc_off[-1] else np.zeros(0, np.int32)
        if append:
            line_off = np.concatenate([sv["line_off"], line_off[1:] + base])
            doc_off = np.concatenate([sv["doc_off"], doc_off[1:] + sv["doc_off"][-1]])
            terms = np.concatenate([np.asarray(sv["term_ids"], np.int32), new_terms])
            ids_all = self._id_list
        else:
            terms = new_terms
            ids_all = [e.id for e in entries]
        st = self.index_path.stat()
        tmp = Path(str(side) + ".tmp")
        shutil.rmtree(tmp, ignore_errors=True)
        tmp.mkdir(parents=True)
        np.save(tmp / "term_ids.npy", terms)
        np.save(tmp / "doc_off.npy", doc_off)
        np.save(tmp / "line_off.npy", line_off)
        vocab = [None] * len(self._vocab)
        for t, i in self._vocab.items():
            vocab[i] = t
        (tmp / "vocab.json").write_text(json.dumps(vocab, ensure_ascii=False), encoding="utf-8")
        (tmp / "ids.json").write_text(json.dumps(list(ids_all), ensure_ascii=False), encoding="utf-8")
        # the where-filter columns (filters.MetaIndex), so a sidecar open can filter without parsing
        # every record's metadata (10M records: ~100 s of JSON before the first filtered search)
        self._ensure_meta()
        ms = self._meta.snapshot()
        if ms is not None and ms[0]["rows"] <= len(ids_all):
            info, arrays = ms
            for k, a in arrays.items():
                np.save(tmp / f"meta_{k}.npy", a)
            (tmp / "meta_info.json").write_text(json.dumps(info, ensure_ascii=False), encoding="utf-8")
        (tmp / "meta.json").write_text(json.dumps({
            "version": _SIDECAR_VERSION, "docs": len(ids_all), "postings": int(doc_off[-1]),
            "jsonl_size": st.st_size, "jsonl_mtime_ns": st.st_mtime_ns}), encoding="utf-8")
        shutil.rmtree(side, ignore_errors=True)
        os.replace(tmp, side)
        del terms    # (the saved arrays are kept memory-mapped from the new sidecar, not in RAM)
        bs.saved = dict(path=str(self.index_path), sig=(st.st_size, st.st_mtime_ns), n=len(ids_all),
                        line_off=np.load(side / "line_off.npy", mmap_mode="r"),
                        doc_off=np.load(side / "doc_off.npy", mmap_mode="r"),
                        term_ids=np.load(side / "term_ids.npy", mmap_mode="r"))
        bs.append_only = True
        # the state matches the files again: later load()s of this index attach to it
        st = self._st
        st.sig, st.unsaved = _file_sig(self), False
        with _REG_LOCK:
            key = self._registry_key()
            _REGISTRY[key] = st
            _REGISTRY.move_to_end(key)
            while len(_REGISTRY) > _REGISTRY_MAX:
                _REGISTRY.popitem(last=False)

    def _sidecar_valid(self) -> Optional[dict]:
        try:
            meta = json.loads((self.sidecar_dir / "meta.json").read_text(encoding="utf-8"))
            st = self.index_path.stat()
        except (OSError, ValueError):
            return None
        if (meta.get("version") != _SIDECAR_VERSION or meta.get("jsonl_size") != st.st_size
                or meta.get("jsonl_mtime_ns") != st.st_mtime_ns):
            return None
        return meta

    def _load_sidecar(self, meta: dict) -> bool:
        side = self.sidecar_dir
        try:
            ids = json.loads((side / "ids.json").read_text(encoding="utf-8"))
            vocab = json.loads((side / "vocab.json").read_text(encoding="utf-8"))
            term_ids = np.load(side / "term_ids.npy", mmap_mode="r")
            doc_off = np.load(side / "doc_off.npy", mmap_mode="r")
            line_off = np.load(side / "line_off.npy", mmap_mode="r")
        except (OSError, ValueError):
            return False
        n = len(ids)
        if (n != meta["docs"] or doc_off.shape[0] != n + 1 or line_off.shape[0] != n + 1
                or term_ids.shape[0] != int(doc_off[-1]) or len(set(ids)) != n):
            return False
        if n and int(doc_off[-1]) == 0:
            raise ZeroDivisionError("float division by zero")  # bm25.py:145 on an all-empty corpus
        cat = _Catalog()
        cat.attach(self.index_path, ids, line_off, term_ids, doc_off)
        self._entries = cat
        self._vocab = {t: i for i, t in enumerate(vocab)}
        self._id_list = list(ids)
        self._version += 1
        self._csr = (term_ids, doc_off)
        self._dirty = self._meta_dirty = True
        self._st.saved = dict(path=str(self.index_path), sig=(meta["jsonl_size"], meta["jsonl_mtime_ns"]), n=n,
                              line_off=line_off, doc_off=doc_off, term_ids=term_ids)
        self._st.append_only = True
        meta = _load_meta_snapshot(side, n, cat, self._id_list)
        if meta is not None:   # filter columns restored; a row's metadata dict is parsed on demand
            self._meta, self._meta_dirty = meta, False
        return True

    @_locked
    def load(self) -> None:
        """bm25.py:233-248; through the sidecar when it matches the JSONL.  A state this process
        already holds for the same file -- loaded or saved by another BM25Store, unchanged since on
        disk and in memory -- is attached instead of re-read: the reference's per-call
        ``BM25Store.load_or_create`` (rag/pipeline/rag.py:532) then costs two stat() calls, not a
        corpus parse and index build."""
        if self.index_dir is None or not self.index_path.exists():
            self._set_state(_BState())
            self._rebuild()
            return
        key, sig = self._registry_key(), _file_sig(self)
        with _REG_LOCK:
            st = _REGISTRY.get(key)
            if st is not None and not st.unsaved and st.sig == sig:
                _REGISTRY.move_to_end(key)
                self._set_state(st)
                return
        self._set_state(_BState())
        meta = self._sidecar_valid()
        if not (meta is not None and self._load_sidecar(meta)):
            with self.index_path.open("r", encoding="utf-8") as f:
                for line in f:
                    if not line.strip():
                        continue
                    rec = json.loads(line)
                    self._entries[rec["id"]] = _entry_of(rec)
            self._rebuild()
        settle_loaded()
        st = self._st
        st.sig, st.unsaved = sig, False
        with _REG_LOCK:
            _REGISTRY[key] = st
            _REGISTRY.move_to_end(key)
            while len(_REGISTRY) > _REGISTRY_MAX:
                _REGISTRY.popitem(last=False)

    @classmethod
    def load_or_create(cls, index_dir: str | Path = "./indexes/bm25") -> "BM25Store":
        store = cls(index_dir=Path(index_dir))
        store.load()
        return store
