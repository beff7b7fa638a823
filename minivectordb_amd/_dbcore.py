"""Host-side state shared by VectorDatabase and ShardedVectorDatabase.

The reference keeps ids, metadata and filters in plain Python containers that it walks or rebuilds on every call
(minivectordb/vector_database.py:139-152 renumbering per delete, :157-386 a Python pass over every id per filtered
query, :356 an O(N) set per unfiltered query, :42-47 a full index rebuild after any write; the sharded class duplicates
all of it, sharded_vector_database.py:289-596).  This module keeps the same SEMANTICS — which rows a filter selects,
what errors it raises, what the public attributes show — on structures that are maintained incrementally:

  _RowStore     rows live on the device; rows stored since the last query wait in host blocks (one upload per build)
  _IdIndex      id <-> row through stable handles (no renumbering loop on delete)
  _ValueIndex   per metadata key, value -> handles, appended to on store, filtered through the deleted handles on use
  _Selection    what a filter leaves: everything / everything but a few rows / a sorted row list
  resident row sets (`mvdb_rowset`) cached per filter expression and write generation

Nothing here is on the GPU path; the arithmetic is libmvdb's.  One deliberate difference: a filtered search enumerates its
rows in ASCENDING row order (exact score ties resolve to the lower row, as in the unfiltered search), where the
reference's ``list(set_of_rows)`` (vector_database.py:510) follows CPython's hash-table order.
"""
import bisect
import numbers
import os
import pickle
from array import array
from collections import OrderedDict, defaultdict
from operator import ge, gt, le, lt, ne

import numpy as np

_OPERATORS = {
    "$gt": gt,
    "$gte": ge,
    "$lt": lt,
    "$lte": le,
    "$ne": ne,
    "$in": lambda field, operand: operand in field,  # "operand in metadata value", as the reference
}

_NO_ROWS = np.empty(0, dtype=np.int64)


def _sorted_rows(rows):
    """Any iterable of row numbers -> sorted unique int64 array."""
    if isinstance(rows, np.ndarray):
        return np.unique(rows.astype(np.int64, copy=False))
    return np.array(sorted(set(rows)), dtype=np.int64)


class _Selection:
    """The rows a filter leaves of the n stored ones — never an O(n) Python object:

    rows is None, gone is None   every row        (the reference builds set(range(n)) per query, vector_database.py:356)
    gone = sorted int64 array    every row but these (an exclude-filter over everything; searched as a resident bitmap)
    rows = sorted int64 array    exactly these
    """
    __slots__ = ("n", "rows", "gone")

    def __init__(self, n, rows=None, gone=None):
        self.n = int(n)
        self.rows = rows
        self.gone = gone if gone is not None and len(gone) else None

    def __len__(self):
        if self.rows is not None:
            return int(self.rows.shape[0])
        return self.n - (int(self.gone.shape[0]) if self.gone is not None else 0)

    def __bool__(self):
        return len(self) > 0

    @property
    def everything(self):
        return self.rows is None and self.gone is None

    def materialize(self):
        """The selected rows as a sorted int64 array (O(n) for the symbolic forms: diagnostics and tests only)."""
        if self.rows is not None:
            return self.rows
        every = np.arange(self.n, dtype=np.int64)
        return every if self.gone is None else np.setdiff1d(every, self.gone, assume_unique=True)

    def local(self, lo, hi):
        """The part of the selection inside rows [lo, hi), renumbered from lo (a rank's share in the row-partitioned
        search)."""
        if self.rows is not None:
            a, b = np.searchsorted(self.rows, (lo, hi))
            return _Selection(hi - lo, rows=self.rows[a:b] - lo)
        if self.gone is not None:
            a, b = np.searchsorted(self.gone, (lo, hi))
            return _Selection(hi - lo, gone=self.gone[a:b] - lo)
        return _Selection(hi - lo)


class _RowStore:
    """The stacked embedding matrix of a database, WITHOUT a host mirror of what the device already holds.

    Rows [0, synced) live — normalised — in the device index only; rows stored since the last index build wait,
    un-normalised, in `pending` host blocks and are uploaded by the next build (`flush`, ONE add however many blocks).
    `materialize` reads the device rows back when somebody asks for the whole matrix (the reference exposes it as
    ``self.embeddings`` and pickles it), `row` fetches one row (``get_vector``), `delete` compacts the device matrix
    and/or drops pending rows.  The reference keeps one numpy matrix that it re-stacks on every insert (``np.vstack``,
    vector_database.py:72) and copies on every delete (``np.delete``, :126).
    """

    def __init__(self, d):
        self.d = d
        self.synced = 0      # leading rows resident on the device
        self.pending = []    # float32 [m_i, d] blocks stored since the last build, in row order
        self.npending = 0
        self._cache = None   # materialised matrix, valid until the next mutation

    @classmethod
    def adopt(cls, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        m = cls(arr.shape[1])
        if arr.shape[0]:
            m.pending.append(arr)
            m.npending = arr.shape[0]
        return m

    @property
    def n(self):
        return self.synced + self.npending

    def append(self, rows):
        rows = np.asarray(rows, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.shape[1] != self.d:
            # same failure mode as np.vstack in the reference
            raise ValueError(
                f"all the input array dimensions except for the concatenation axis must match exactly, "
                f"but along dimension 1, the array at index 0 has size {self.d} and the array at index 1 "
                f"has size {rows.shape[1]}")
        self.pending.append(rows)
        self.npending += rows.shape[0]
        self._cache = None

    DIRECT_UPLOAD_BYTES = 8 << 20

    def flush(self, index):
        """Upload the pending rows (normalised on the device, vector_database.py:45-46) and forget the host copies:
        one `mvdb_index_add` per run of small blocks — 1,000 single-row stores followed by a query cost one upload and one
        wait on the index's own stream, not 1,000."""
        if not self.pending:
            return
        # runs of SMALL blocks are stacked into one upload; a block of >= 8 MiB goes up as it stands (stacking ten 200 MB
        # batches cost 155 ms of host memcpy before a 37 ms upload)
        groups, small = [], []
        for block in self.pending:
            if block.nbytes >= self.DIRECT_UPLOAD_BYTES:
                if small:
                    groups.append(small)
                    small = []
                groups.append([block])
            else:
                small.append(block)
        if small:
            groups.append(small)
        done = 0
        try:
            for group in groups:
                block = group[0] if len(group) == 1 else np.concatenate(group, axis=0)
                index.add(block, normalize=True)    # a failed add leaves ITS rows (and the later ones) pending
                self.synced += block.shape[0]
                done += len(group)
        finally:
            self.pending = self.pending[done:]
            self.npending = sum(b.shape[0] for b in self.pending)
            self._cache = None

    def delete(self, rows, index):
        """Remove the given stacked row numbers (np.delete semantics: later rows move up)."""
        rows = sorted(int(r) for r in rows)
        dev = [r for r in rows if r < self.synced]
        host = [r - self.synced for r in rows if r >= self.synced]
        if host:
            stacked = self.pending[0] if len(self.pending) == 1 else np.vstack(self.pending)
            kept = np.delete(stacked, host, axis=0)
            self.pending = [kept] if kept.shape[0] else []
            self.npending = kept.shape[0]
        if dev:
            index.remove_rows(dev)
            self.synced -= len(dev)
        self._cache = None

    def replace(self, rows, vectors, index):
        """Overwrite the stacked rows `rows` (distinct) with vectors[len(rows), d]: the rows the device holds through ONE
        `index.set_rows` (normalised there, as `flush` has them normalised), the rows still waiting for a build in their host
        block.  Nothing moves and no host copy of a synced row is kept.  The device goes first: if it refuses, nothing changed."""
        rows = np.asarray(rows, dtype=np.int64)
        vectors = np.asarray(vectors, dtype=np.float32)
        on_device = rows < self.synced
        if on_device.any():
            index.set_rows(rows[on_device], vectors[on_device], normalize=True)
        if not on_device.all():
            starts = np.cumsum([0] + [b.shape[0] for b in self.pending])
            for r, v in zip(rows[~on_device] - self.synced, vectors[~on_device]):
                b = int(np.searchsorted(starts, r, side="right")) - 1
                if not self.pending[b].flags.writeable:
                    self.pending[b] = self.pending[b].copy()
                self.pending[b][r - starts[b]] = v
        self._cache = None

    def row(self, r, index):
        """A fresh copy of stacked row r (the reference hands out a view of an array that every write REPLACES, so
        an earlier result never changes under the caller, vector_database.py:72,104,126)."""
        if r < self.synced:
            return index.get_rows(r, 1)[0]
        r -= self.synced
        for block in self.pending:
            if r < block.shape[0]:
                return block[r].copy()
            r -= block.shape[0]
        raise IndexError("row out of range")

    def materialize(self, index):
        if self._cache is None:
            out = np.empty((self.n, self.d), dtype=np.float32)
            if self.synced:
                index.get_rows(0, self.synced, out=out[:self.synced])
            at = self.synced
            for block in self.pending:
                out[at:at + block.shape[0]] = block
                at += block.shape[0]
            self._cache = out
        return self._cache


class _IdIndex:
    """row <-> unique id bookkeeping with O(tail memmove) deletes, shared by both database classes.

    The reference keeps dicts (``id_map`` row -> id, ``inverse_id_map`` id -> row; the sharded class a ``unique_ids``
    list) and rebuilds them over every row at every delete (vector_database.py:139-152,
    sharded_vector_database.py:229-241): a Python loop over the whole database.  Here the order lives in ONE list
    (``uids``, row -> id: ``list.pop`` is a C memmove) and ids map to stable HANDLES (insertion counters); the current
    row of a handle is the handle minus the number of deleted handles below it (bisect over a short sorted list).
    Handles are renumbered only by `compact` (every 4096 deletes), which bumps `epoch` — whoever stores handles
    (`_ValueIndex`) starts over then.  The plain dicts the reference exposes are produced on demand (`inverse_dict`,
    `row_dict`) and cached until the next write; producing them does NOT touch the handles.
    """

    def __init__(self, uids=()):
        self.uids = list(uids)
        self.handle = {u: i for i, u in enumerate(self.uids)}
        self.next = len(self.uids)
        self.deleted = []       # sorted handles removed since the last compaction
        self.epoch = 0
        self._deleted_arr = None
        self._row_dict = None
        self._inverse = None

    def __len__(self):
        return len(self.uids)

    def __contains__(self, uid):
        return uid in self.handle

    def _touched(self):
        self._row_dict = None
        self._inverse = None

    def append(self, uid):
        self.handle[uid] = self.next
        self.next += 1
        self.uids.append(uid)
        self._touched()

    def extend(self, uids):
        """append() for a whole batch (a later duplicate id takes the handle over, as one append after the other would)."""
        uids = list(uids)
        self.handle.update(zip(uids, range(self.next, self.next + len(uids))))
        self.next += len(uids)
        self.uids.extend(uids)
        self._touched()

    def row(self, uid):
        h = self.handle[uid]
        return h - bisect.bisect_left(self.deleted, h) if self.deleted else h

    def pop(self, uid):
        r = self.row(uid)
        bisect.insort(self.deleted, self.handle.pop(uid))
        self._deleted_arr = None
        self.uids.pop(r)
        self._touched()
        if len(self.deleted) > 4096:
            self.compact()
        return r

    def remove_many(self, uids):
        """Drop several ids; returns their rows (as they were BEFORE the call), ascending.  A handful go one by one; a
        large batch is one pass over the id list."""
        uids = list(dict.fromkeys(uids))
        if len(uids) <= 32:
            rows = sorted(self.row(u) for u in uids)
            for r, u in sorted(((self.row(u), u) for u in uids), reverse=True):
                bisect.insort(self.deleted, self.handle.pop(u))
                self.uids.pop(r)
            self._deleted_arr = None
            self._touched()
            if len(self.deleted) > 4096:
                self.compact()
            return rows
        rows = sorted(self.row(u) for u in uids)
        doomed = set(rows)
        self.uids = [u for r, u in enumerate(self.uids) if r not in doomed]
        self.compact()
        return rows

    def compact(self):
        self.handle = {u: i for i, u in enumerate(self.uids)}
        self.next = len(self.uids)
        self.deleted = []
        self._deleted_arr = None
        self.epoch += 1
        self._touched()

    def rows_of(self, handles):
        """Sorted int64 handles -> the rows of those still alive (sorted, since rows are monotone in handles)."""
        if not self.deleted or not handles.shape[0]:
            return handles
        if self._deleted_arr is None:
            self._deleted_arr = np.array(self.deleted, dtype=np.int64)
        dead = self._deleted_arr
        below = np.searchsorted(dead, handles)
        alive = dead[np.minimum(below, dead.shape[0] - 1)] != handles
        return (handles - below)[alive]

    def inverse_dict(self):
        """id -> row as a plain dict (what the reference calls inverse_id_map), in row order."""
        if self._inverse is None:
            self._inverse = self.handle if not self.deleted else {u: r for r, u in enumerate(self.uids)}
        return self._inverse

    def row_dict(self):
        """row -> id as a plain dict (the reference's id_map)."""
        if self._row_dict is None:
            self._row_dict = dict(enumerate(self.uids))
        return self._row_dict


_NO_FIELD = object()


class _ValueIndex:
    """Equality filters without the reference's pass over every id per query (vector_database.py:283-302, :332-345).

    Per metadata key (built on the first filter that names it, then maintained by `note_store` / `note_delete`):
    value -> the HANDLES of the rows whose metadata[key] == value, ascending (handles only grow, so appending keeps the
    order), plus the rows whose value is unhashable (compared with == at query time).  A delete does not edit the handle
    arrays: dead handles are filtered out through `_IdIndex.rows_of` when the entry is used and disappear for good when
    the id index compacts (its `epoch` moves: the whole value index is rebuilt on demand).

    CONTRACT: metadata dicts are treated as immutable once stored — the reference re-reads ``self.metadata[row]`` at
    every query, so an in-place edit of a stored dict is honoured there and not seen here.
    """

    def __init__(self, ids):
        self.epoch = ids.epoch
        self.keys = {}   # key -> (by_value: {value: array('q') of handles}, odd: {handle: unhashable field})

    def _build(self, key, uids, ids, metadata):
        by_value, odd = {}, {}
        if 2 * len(uids) >= len(metadata) == len(ids.uids):
            # most rows carry the key: walk the rows in order — handles ascend with the rows, so nothing is sorted and no id is
            # looked up (a million rows: ~0.15 s instead of ~0.3 s)
            missing = _NO_FIELD
            handle_of = ids.handle
            handles = range(len(metadata)) if not ids.deleted and ids.next == len(metadata) else [handle_of[u] for u in ids.uids]
            for h, meta in zip(handles, metadata):
                field = meta.get(key, missing)
                if field is missing:
                    continue
                try:
                    slot = by_value.get(field)
                    if slot is None:
                        slot = by_value[field] = array('q')
                    slot.append(h)
                except TypeError:   # list / dict metadata value
                    odd[h] = field
            self.keys[key] = (by_value, odd)
            return by_value, odd
        pairs = []
        for uid in uids:
            if uid in ids.handle:
                pairs.append((ids.handle[uid], metadata[ids.row(uid)].get(key, None)))
        pairs.sort(key=lambda p: p[0])
        for h, field in pairs:
            try:
                slot = by_value.get(field)
                if slot is None:
                    slot = by_value[field] = array('q')
                slot.append(h)
            except TypeError:   # list / dict metadata value
                odd[h] = field
        self.keys[key] = (by_value, odd)
        return by_value, odd

    def rows_equal(self, key, value, owner):
        """Sorted rows whose metadata[key] == value, or None when `value` is unhashable (the caller walks instead)."""
        try:
            hash(value)
        except TypeError:
            return None
        entry = self.keys.get(key)
        if entry is None:
            entry = self._build(key, list(owner.inverted_index.get(key, ())), owner._ids, owner.metadata)
        by_value, odd = entry
        if value != value:  # NaN never equals anything under the reference's `==`; a dict lookup would match it by identity
            return _NO_ROWS
        slot = by_value.get(value)
        rows = owner._ids.rows_of(np.frombuffer(slot, dtype=np.int64).copy()) if slot else _NO_ROWS
        if odd:
            extra = [h for h, field in odd.items() if field == value]
            if extra:
                rows = np.union1d(rows, owner._ids.rows_of(np.array(sorted(extra), dtype=np.int64)))
        return rows

    def note_store(self, handle, meta):
        for key, field in meta.items():
            entry = self.keys.get(key)
            if entry is None:
                continue   # built when a filter first names the key
            try:
                slot = entry[0].get(field)
                if slot is None:
                    slot = entry[0][field] = array('q')
                slot.append(handle)
            except TypeError:
                entry[1][handle] = field

    def note_delete(self, handle, meta):
        for key in meta:
            entry = self.keys.get(key)
            if entry is not None:
                entry[1].pop(handle, None)   # (hashable values: the dead handle is filtered out at query time)


    def note_update(self, handle, old, new):
        """The metadata of a LIVE handle is replaced (update_embedding).  `note_delete` alone would not do: it leaves a
        hashable value's handle in place and relies on the handle being dead.  The handle leaves the slots of the old dict and
        enters those of the new one at its sorted position (handle arrays stay ascending: `_IdIndex.rows_of`)."""
        for key, field in old.items():
            entry = self.keys.get(key)
            if entry is None:
                continue
            entry[1].pop(handle, None)
            try:
                slot = entry[0].get(field)
            except TypeError:
                continue
            if slot is not None:
                at = bisect.bisect_left(slot, handle)
                if at < len(slot) and slot[at] == handle:
                    del slot[at]
                if not len(slot):
                    del entry[0][field]
        for key, field in new.items():
            entry = self.keys.get(key)
            if entry is None:
                continue   # built when a filter first names the key
            try:
                slot = entry[0].get(field)
                if slot is None:
                    slot = entry[0][field] = array('q')
                bisect.insort(slot, handle)
            except TypeError:
                entry[1][handle] = field


class _MmrShape(Exception):
    """k > fetch_k after clamping: not a ValueError on its way out of the search, which would read as a stale row set."""


class _DistinctShape(Exception):
    """k > 64 after clamping: not a ValueError on its way out of the search, which would read as a stale object."""


class FilterAndRerankMixin:
    """Needs: self.inverted_index, self._ids (_IdIndex), self.metadata, self.hash_vectorizer, self._mat (_RowStore),
    self.index, self.embedding_size, self._device, self.lock."""

    _row_store = _RowStore   # the class that holds the stacked rows (ShardedVectorDatabaseUsearch keeps them on the host)

    # ---- device mirror -----------------------------------------------------------------------------
    def _build_index(self):
        """Bring the device matrix up to date (caller holds the lock).

        Reference: IndexFlatIP(d); normalize_L2(self.embeddings) in place; index.add (vector_database.py:42-47).
        Only rows stored since the last build are uploaded; they are normalised on the device, which from then on
        is their only home (`_RowStore`): ``get_vector`` / ``embeddings`` / ``persist_to_disk`` read them back, so the
        in-place normalisation the reference performs on its host matrix stays visible.
        """
        from . import _native
        if self.index is None:
            self.index = _native.FlatIndex(self.embedding_size, metric=_native.METRIC_IP, device=self._device)
            if self.__dict__.get("_fast_single_query"):
                self.index.set_option("shadow_single_query", 1)
        if self._mat.n > 0:
            self._mat.flush(self.index)
            self._embeddings_changed = False

    # ---- shared ingest / delete bookkeeping ------------------------------------------------------------
    def _admit(self, unique_ids, vectors, metadata_dicts):
        """Append rows + bookkeeping common to both database classes (caller holds the lock, has
        validated ids).  `vectors` is a sequence of float32 1-D arrays.  Returns the first new row."""
        if self.embedding_size is None:
            self.embedding_size = vectors[0].shape[0]
        if self._mat is None:
            self._mat = self._row_store(self.embedding_size)
        first = self._mat.n
        if len(vectors):
            if isinstance(vectors, np.ndarray) and vectors.ndim == 2:   # a batch that arrived as ONE float32 matrix: no per-row work
                self._mat.append(vectors[0] if vectors.shape[0] == 1 else vectors)
            else:
                self._mat.append(vectors[0] if len(vectors) == 1 else np.vstack(vectors))
        self.metadata.extend(metadata_dicts)
        values = self._live_value_index()
        handle = self._ids.next
        self._ids.extend(unique_ids)
        inverted = self.inverted_index
        for uid, meta in zip(unique_ids, metadata_dicts):
            if meta:
                for key in meta:
                    inverted[key].add(uid)
                if values is not None:
                    values.note_store(handle, meta)
            handle += 1
        self._note_write()
        self._embeddings_changed = True
        return first

    def _expel(self, unique_ids):
        """Bookkeeping of a delete (caller holds the lock, ids exist): id maps, metadata list, inverted index — touching
        only what belongs to the doomed ids (the reference walks every inverted-index key per deleted id and rebuilds its
        lists and dicts over all rows, vector_database.py:128-152, sharded_vector_database.py:229-241) — and the device /
        pending rows.  Returns the removed rows, ascending."""
        unique_ids = list(dict.fromkeys(unique_ids))
        values = self._live_value_index()
        sparse = self.__dict__.get("_sparse")
        for uid in unique_ids:
            if sparse:
                sparse.pop(uid, None)   # a later store of the same id starts without a sparse vector
            meta = self.metadata[self._ids.row(uid)]
            if values is not None and meta:
                values.note_delete(self._ids.handle[uid], meta)
            for key in meta:
                holders = self.inverted_index.get(key)
                if holders is not None:
                    holders.discard(uid)
                    if not holders:
                        del self.inverted_index[key]
        rows = self._ids.remove_many(unique_ids)
        if len(rows) <= 32:
            for r in reversed(rows):
                del self.metadata[r]
        else:
            doomed = set(rows)
            self.metadata[:] = [m for r, m in enumerate(self.metadata) if r not in doomed]
        self._partition_rows_removed(rows)
        self._mat.delete(rows, self.index)
        self._note_write()
        self._embeddings_changed = True
        return rows

    def _row_count(self):
        return len(self._ids)

    def _note_write(self):
        """Every store / delete: cached row sets and the exposed dicts belong to the previous state.  (The value index is
        NOT dropped: it is maintained incrementally, `_admit` / `_expel`.)"""
        self.__dict__["_write_gen"] = self.__dict__.get("_write_gen", 0) + 1
        # built against the previous rows: dropped, not closed — a search running outside the lock may still hold one
        # (its device memory goes when the last reference does)
        self.__dict__["_rowsets"] = {}
        self.__dict__["_rowsets_each"] = OrderedDict()   # find_most_similar_each's own cache (bounded by bytes, not entries)
        self.__dict__["_rowsets_each_bytes"] = 0

    _invalidate_filter_cache = _note_write

    def _live_value_index(self):
        """The value index if it exists and its handles are current, else None (it is rebuilt by the next filter)."""
        vi = self.__dict__.get("_values")
        if vi is not None and vi.epoch != self._ids.epoch:
            vi = self.__dict__["_values"] = None
        return vi

    # ---- search plumbing ---------------------------------------------------------------------------------
    def _nearest_rows(self, embedding, metadata_filter, exclude_filter, or_filters, k):
        """Device half of find_most_similar: [(row, score)] best first, rows of the stacked matrix.
        Query prep, lazy device sync, filter evaluation, k clamp and the full / filtered branch follow
        vector_database.py:470-523; the arithmetic is libmvdb's."""
        if self._mat is None:
            return []
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self._nearest_rows_many(query, metadata_filter, exclude_filter, or_filters, k)[0]

    def find_most_similar_batch(self, embeddings, metadata_filter=None, exclude_filter=None, or_filters=None, k=5,
                                autocut=False):
        """Several queries under ONE filter in one call (no reference counterpart: the reference's API is one query per call):
        element i of the returned list is what ``find_most_similar(embeddings[i], ...)`` returns.  The queries share corpus
        passes on the device (2+ queries: the certified batch passes, also under a filter's resident row set) — 10M x 512:
        128 queries in 1.8 ms against 2.84 ms for one."""
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        if queries.shape[0] == 0 or self._mat is None:
            return [([], [], []) for _ in range(queries.shape[0])]
        uids = self._ids.uids
        out = []
        for found in self._nearest_rows_many(queries, metadata_filter, exclude_filter, or_filters, k):
            hits = []
            for row, score in found:
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[row], score, self.metadata[row]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, autocut))
        return out

    def _search_selected(self, metadata_filter, exclude_filter, or_filters, nothing, search, with_selection=False):
        """What every search under one filter shares: lazy device sync, filter evaluation (or the filter's resident row set,
        found in the cache), and the retry after a concurrent delete.  Returns `nothing` when the filter selects no row (or
        there is no index yet), else ``search(index, count, rowset)`` — `count` rows selected, `rowset()` their resident
        row set, None when they are all the rows.  A ValueError out of `search` (another thread deleted rows between the
        filter and the search; the reference would still be searching its old index object) evaluates the filter again on
        the current rows, twice at the most.  with_selection: ``search(index, count, rowset, selection)`` — the `_Selection`
        itself too (the duplicate-pair search takes its query rows from it)."""
        filtered = bool(metadata_filter or exclude_filter or or_filters)
        key = None
        if filtered:
            try:
                key = repr((metadata_filter, exclude_filter, or_filters))
            except Exception:
                key = None
        for attempt in range(3):
            with self.lock:
                if self._embeddings_changed:
                    self._build_index()
                index, n_rows = self.index, self._mat.n
                gen = self.__dict__.get("_write_gen", 0)
                hit = self.__dict__.get("_rowsets", {}).get(key) if key is not None else None
                if hit is not None and hit[0] == gen and hit[1] is index:
                    count, held, wanted = hit[2], hit[3], None
                    selection = hit[4]
                else:
                    wanted = self._get_filtered_indices(metadata_filter, exclude_filter, or_filters)
                    count, held = len(wanted), None
                    selection = wanted
            if not count or index is None:
                return nothing

            def rowset():
                if count == n_rows:
                    return None
                return held if held is not None else self._resident_rowset(index, wanted, key, gen)

            try:
                return search(index, count, rowset, selection) if with_selection else search(index, count, rowset)
            except ValueError:
                # rows were deleted between the filter and the search: evaluate the filter again on the current rows
                if attempt == 2:
                    raise

    def _nearest_rows_many(self, query, metadata_filter, exclude_filter, or_filters, k):
        """_nearest_rows for a [nq, d] float32 matrix of queries: one list of (row, score) per query."""
        nq = query.shape[0]

        def search(index, count, rowset):
            take = min(k, count)
            rs = rowset()
            if rs is None:
                return index.search(query, take, normalize_q=True)
            return index.search_rowset(query, take, rs, normalize_q=True)

        found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        if found is None:
            return [[] for _ in range(nq)]
        scores, rows = found
        return [[(int(r), s) for r, s in zip(rows[i], scores[i]) if r != -1] for i in range(nq)]

    def _resident_rowset(self, index, wanted, key, gen):
        """The filtered rows as a device-resident row set (`mvdb_rowset`), kept until the next write: the reference
        gathers the filtered rows into a throw-away index for EVERY query (vector_database.py:508-523); here consecutive
        queries under one filter upload nothing and do not even evaluate the filter again.  An exclude-filter over
        everything travels as the few excluded rows and lives as a bitmap.  The entry is stamped with the write
        generation captured — under the lock — together with the filter's rows: a set built from rows that a concurrent
        write has since outdated is used for THIS query only and never enters the cache."""
        if wanted.gone is not None:
            rowset = index.rowset(wanted.gone, excluded=True)
        else:
            rowset = index.rowset(wanted.rows)
        if key is not None:
            with self.lock:
                if self.__dict__.get("_write_gen", 0) == gen and self.index is index:
                    cache = self.__dict__.setdefault("_rowsets", {})
                    if len(cache) >= 16:  # a handful of filters in rotation; each holds device memory until its last user drops it
                        cache.clear()
                    cache[key] = (gen, index, len(wanted), rowset, wanted)
        return rowset

    # ---- range search: everything at or above a score, instead of the k best --------------------------------
    def find_all_similar(self, embedding, min_score, metadata_filter=None, exclude_filter=None, or_filters=None, limit=None):
        """EVERY stored embedding whose score against `embedding` is at least `min_score` (cosine: rows and query are
        normalised), best first, under the filters of ``find_most_similar`` — near-duplicate checks, retrieval with a relevance
        floor instead of a fixed k, neighbourhoods of unknown size.  No reference counterpart (its ``autocut`` guesses such a
        floor from a fixed k).  Returns ``(ids, distances, metadatas)`` packaged as ``find_most_similar`` does without
        autocut; ids, scores and order are those of ``find_most_similar`` with k = the number of matches.  `limit`: only the
        best `limit` of them."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self.find_all_similar_batch(query, min_score, metadata_filter, exclude_filter, or_filters, limit)[0]

    def find_all_similar_batch(self, embeddings, min_score, metadata_filter=None, exclude_filter=None, or_filters=None,
                               limit=None):
        """Several queries under ONE filter: element i is what ``find_all_similar(embeddings[i], min_score, ...)`` returns —
        `min_score` one number, or a sequence with one per query (``min_score[i]`` for query i; another length or a NaN entry
        is a ValueError).  A range result is bit for bit the single query's, whichever corpus passes the index shares between
        the queries of the batch."""
        queries = self._range_queries(embeddings)
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        if queries.shape[0] == 0 or self._mat is None:
            self._range_min_scores(min_score, queries.shape[0])   # a bad min_score is an error whatever the database holds
            return [([], [], []) for _ in range(queries.shape[0])]
        uids = self._ids.uids
        out = []
        for found in self._range_rows_many(queries, min_score, metadata_filter, exclude_filter, or_filters):
            hits = []
            for row, score in (found if limit is None else found[:limit]):
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[row], score, self.metadata[row]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, False))
        return out

    def count_similar(self, embedding, min_score, metadata_filter=None, exclude_filter=None, or_filters=None):
        """``len(find_all_similar(...)[0])`` without fetching a single result: one pass on the device, one integer back."""
        query = self._range_queries(np.array([np.array(embedding, dtype=np.float32)]))
        if self._mat is None:
            return 0
        return int(self._range_rows_many(query, min_score, metadata_filter, exclude_filter, or_filters, count_only=True)[0])

    def count_similar_batch(self, embeddings, min_score, metadata_filter=None, exclude_filter=None, or_filters=None):
        """``[count_similar(e, min_score, ...) for e in embeddings]`` in one call on the device, nothing but the integers
        back; `min_score` as in ``find_all_similar_batch``."""
        queries = self._range_queries(embeddings)
        if queries.shape[0] == 0 or self._mat is None:
            self._range_min_scores(min_score, queries.shape[0])
            return [0] * queries.shape[0]
        return [int(c) for c in self._range_rows_many(queries, min_score, metadata_filter, exclude_filter, or_filters, count_only=True)]

    @staticmethod
    def _range_min_scores(min_score, nq):
        """A scalar min_score as a Python float (what a single-threshold index call takes); a sequence as float32[nq]."""
        if np.ndim(min_score) == 0:
            min_score = float(min_score)
            if min_score != min_score:
                raise ValueError("min_score is NaN")
            return min_score
        scores = np.ascontiguousarray(min_score, dtype=np.float32)
        if scores.ndim != 1 or scores.shape[0] != nq:
            raise ValueError(f"min_score has {scores.size} entries for {nq} queries: pass one number or one per query")
        if np.isnan(scores).any():
            raise ValueError("min_score holds a NaN")
        return scores

    def _range_queries(self, embeddings):
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        if self._mat is not None and queries.shape[0] and queries.shape[1] != self._mat.d:
            # before any filter is evaluated (the retry loop would evaluate it three times over before the index's own ValueError)
            raise ValueError(f"query dimension {queries.shape[1]} != index dimension {self._mat.d}")
        return queries

    def _range_rows_many(self, query, min_score, metadata_filter, exclude_filter, or_filters, count_only=False):
        """Device half of find_all_similar: per query [(row, score)] best first — or, count_only, the number of matches.  Lazy
        device sync, filter evaluation, the resident row-set cache and the retry after a concurrent delete are
        `_nearest_rows_many`'s."""
        nq = query.shape[0]
        min_score = self._range_min_scores(min_score, nq)

        def search(index, count, rowset):
            if not hasattr(index, "range_search"):
                raise NotImplementedError(f"{type(index).__name__} has no range search")
            rs = rowset()
            if count_only:
                return [int(c) for c in index.range_count(query, min_score, rowset=rs, normalize_q=True)]
            return index.range_search(query, min_score, rowset=rs, normalize_q=True)

        found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        if found is None:
            return [0] * nq if count_only else [[] for _ in range(nq)]
        if count_only:
            return found
        lims, scores, rows = found
        return [[(int(r), s) for r, s in zip(rows[lims[i]:lims[i + 1]], scores[lims[i]:lims[i + 1]])] for i in range(nq)]

    # ---- duplicate-pair search: which stored embeddings are near each other -------------------------------------------
    def find_duplicate_pairs(self, min_score, metadata_filter=None, exclude_filter=None, or_filters=None, first_row=0, limit=None):
        """Every PAIR of stored embeddings, both inside the filter, whose score is at least `min_score` (cosine: the rows are
        normalised): ``(ids_earlier, ids_later, scores)``, three parallel lists, best pair first, ties by (storage position of
        the later member, of the earlier).  Each pair is listed once.  `first_row`: only pairs whose later-stored member sits
        at storage position >= first_row — pass the store's size from before a bulk add to check only what was added.
        `limit`: only the best `limit` pairs.  The rows never leave the device: only row numbers go up and pairs come back
        (a range join, include/mvdb.h "RANGE JOIN").  No reference counterpart."""
        later, earlier, scores = self._join_pairs(min_score, metadata_filter, exclude_filter, or_filters, first_row, limit)
        uids = self._ids.uids if len(later) else None
        a, b, s = [], [], []
        for r_late, r_early, score in zip(later.tolist(), earlier.tolist(), scores.tolist()):
            try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                pair = (uids[r_early], uids[r_late])
            except (KeyError, IndexError):
                continue
            a.append(pair[0])
            b.append(pair[1])
            s.append(score)
        return a, b, s

    def count_duplicate_pairs(self, min_score, metadata_filter=None, exclude_filter=None, or_filters=None, first_row=0, limit=None):
        """``len(find_duplicate_pairs(...)[0])`` without fetching a single pair: counts only come back from the device."""
        total = self._join_pairs(min_score, metadata_filter, exclude_filter, or_filters, first_row, limit, count_only=True)
        return total if limit is None else min(total, limit)

    def find_duplicate_groups(self, min_score, metadata_filter=None, exclude_filter=None, or_filters=None, first_row=0, limit=None):
        """The connected components of the graph ``find_duplicate_pairs`` lists, as lists of ids: each list in storage order,
        the groups ordered by their first member, singletons left out — keep the first id of each list and drop the rest to
        deduplicate a store.  A host union-find over the pairs."""
        later, earlier, _ = self._join_pairs(min_score, metadata_filter, exclude_filter, or_filters, first_row, limit)
        parent = {}

        def find(r):
            root = r
            while parent.setdefault(root, root) != root:
                root = parent[root]
            while parent[r] != root:
                parent[r], r = root, parent[r]
            return root

        for r_late, r_early in zip(later.tolist(), earlier.tolist()):
            a, b = find(r_early), find(r_late)
            if a != b:
                parent[max(a, b)] = min(a, b)   # the root of a group is its first member
        members = defaultdict(list)
        for r in sorted(parent):
            members[find(r)].append(r)
        uids = self._ids.uids if members else None
        groups = []
        for root in sorted(members):
            try:
                groups.append([uids[r] for r in members[root]])
            except (KeyError, IndexError):
                pass
        return groups

    def _join_pairs(self, min_score, metadata_filter, exclude_filter, or_filters, first_row, limit, count_only=False):
        """Device half of the duplicate-pair search: (later rows, earlier rows, scores) as arrays in the order
        find_duplicate_pairs documents, cut to `limit` — or, count_only, the number of pairs.  The filter becomes the row set
        through `_search_selected`; the query rows are the selected rows at or above first_row."""
        min_score = float(min_score)
        if min_score != min_score:
            raise ValueError("min_score is NaN")
        first_row = int(first_row)
        if first_row < 0:
            raise ValueError("first_row must not be negative")
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        empty = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.float32))
        nothing = 0 if count_only else empty
        if self._mat is None:
            return nothing

        def search(index, count, rowset, selection):
            if not hasattr(index, "range_join"):
                raise NotImplementedError(f"{type(index).__name__} has no range join")
            if selection.everything:
                rows = np.arange(min(first_row, selection.n), selection.n, dtype=np.int64)
            else:
                rows = selection.materialize()
                rows = rows[np.searchsorted(rows, first_row):]
            if rows.shape[0] == 0:
                return nothing
            rs = rowset()
            if count_only:
                return index.range_join_count(min_score, rows=rows, rowset=rs)
            qrows, lims, scores, earlier = index.range_join(min_score, rows=rows, rowset=rs)
            later = np.repeat(qrows, np.diff(lims))
            order = np.lexsort((earlier, later, -scores.astype(np.float64)))   # best first, then (later, earlier) position
            if limit is not None:
                order = order[:limit]
            return later[order], earlier[order], scores[order]

        return self._search_selected(metadata_filter, exclude_filter, or_filters, nothing, search, with_selection=True)

    # ---- MMR search: k results that are relevant and unlike each other ------------------------------------------
    MMR_MAX_FETCH = 1024   # most candidates the device selection takes (include/mvdb.h "MMR SEARCH")

    def find_most_similar_mmr(self, embedding, k=5, fetch_k=None, lambda_mult=0.5, metadata_filter=None, exclude_filter=None,
                              or_filters=None):
        """`k` results picked for relevance AND diversity (maximal marginal relevance) instead of the k best, which on a
        corpus with near-duplicates are k copies of one passage: of the `fetch_k` best rows under the filters of
        ``find_most_similar`` (default ``max(4 * k, 20)``), the best one, then repeatedly the row that maximises
        ``lambda_mult * score - (1 - lambda_mult) * (largest cosine to a row already picked)``.  ``lambda_mult=1`` is
        ``find_most_similar(k=k)``, 0 looks at diversity alone.  No reference counterpart (its ``autocut`` and
        ``hybrid_rerank_results`` work on a fixed top-k after the fact).  The rows never leave the device: the selection
        is one launch behind the search.  Returns ``(ids, distances, metadatas)`` in SELECTION order, packaged as
        ``find_most_similar`` does without autocut; the distances are the rows' search scores.  `k` and `fetch_k` are
        clamped to the number of rows the filters select, `fetch_k` also to 1024; ``k > fetch_k`` after that is a ValueError."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self.find_most_similar_mmr_batch(query, k, fetch_k, lambda_mult, metadata_filter, exclude_filter, or_filters)[0]

    def find_most_similar_mmr_batch(self, embeddings, k=5, fetch_k=None, lambda_mult=0.5, metadata_filter=None,
                                    exclude_filter=None, or_filters=None):
        """Several queries under ONE filter: element i is what ``find_most_similar_mmr(embeddings[i], ...)`` returns."""
        queries = self._range_queries(embeddings)
        nq = queries.shape[0]
        k = int(k)
        fetch_k = max(4 * k, 20) if fetch_k is None else int(fetch_k)
        lambda_mult = float(lambda_mult)
        if k < 1 or fetch_k < 1:
            raise ValueError("k and fetch_k must be positive")
        if not 0.0 <= lambda_mult <= 1.0:
            raise ValueError(f"lambda_mult must lie in [0, 1] (got {lambda_mult})")
        if nq == 0 or self._mat is None:
            return [([], [], []) for _ in range(nq)]

        def search(index, count, rowset):
            if not hasattr(index, "search_mmr"):
                raise NotImplementedError(f"{type(index).__name__} has no MMR search")
            take, fetch = min(k, count), min(fetch_k, count, self.MMR_MAX_FETCH)
            if take > fetch:
                raise _MmrShape(f"k = {take} exceeds fetch_k = {fetch} (fetch_k is clamped to {self.MMR_MAX_FETCH})")
            return index.search_mmr(queries, take, fetch, lambda_mult, rowset=rowset(), normalize_q=True)

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _MmrShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            return [([], [], []) for _ in range(nq)]
        scores, rows = found
        uids = self._ids.uids
        out = []
        for i in range(nq):
            hits = []
            for row, score in zip(rows[i], scores[i]):
                if row == -1:
                    continue
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[int(row)], score, self.metadata[int(row)]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, False))
        return out

    # ---- distinct search: the best row of each metadata group, the k best groups ----------------------------
    DISTINCT_MAX_K = 64        # most groups one call returns (include/mvdb.h "DISTINCT SEARCH")
    DISTINCT_MAX_FETCH = 1024  # most candidates its first tier collapses
    _GROUPINGS_KEPT = 4        # metadata keys whose codes stay resident

    def find_most_similar_distinct(self, embedding, group_by, k=5, fetch_k=None, metadata_filter=None, exclude_filter=None,
                                   or_filters=None):
        """The `k` best GROUPS under the filters of ``find_most_similar``, each represented by its best row — "the k best
        documents" of a store whose documents are chunked into several rows, where ``find_most_similar(k=5)`` often returns
        five chunks of one document.  `group_by` is a metadata key: rows whose value under it compares equal as a dict key
        form one group; a row without the key is a group of its own (no row is silently dropped); an unhashable value is a
        TypeError naming the id.  The answer is EXACT whatever `fetch_k` is (default ``max(4 * k, 32)``): it only sizes the
        cheap first tier — a query whose `fetch_k` best rows hold fewer than `k` groups (one document fills the fetch) is
        answered by one pass over the selected rows on the device.  No reference counterpart.  Returns ``(ids, distances,
        metadatas)``, best group first, packaged as ``find_most_similar`` does without autocut.  `fetch_k` is clamped to 1024
        and to the number of rows the filters select, `k` to that number; ``k > 64`` after that is a ValueError."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self.find_most_similar_distinct_batch(query, group_by, k, fetch_k, metadata_filter, exclude_filter, or_filters)[0]

    def find_most_similar_distinct_batch(self, embeddings, group_by, k=5, fetch_k=None, metadata_filter=None,
                                         exclude_filter=None, or_filters=None):
        """Several queries under ONE filter: element i is what ``find_most_similar_distinct(embeddings[i], ...)`` returns."""
        queries = self._range_queries(embeddings)
        nq = queries.shape[0]
        k = int(k)
        fetch_k = max(4 * k, 32) if fetch_k is None else int(fetch_k)
        if k < 1 or fetch_k < 1:
            raise ValueError("k and fetch_k must be positive")
        if fetch_k < k:
            raise ValueError(f"k = {k} exceeds fetch_k = {fetch_k}")
        hash(group_by)  # (a metadata key: an unhashable one is the caller's TypeError, before anything is searched)
        if nq == 0 or self._mat is None:
            return [([], [], []) for _ in range(nq)]

        def search(index, count, rowset):
            if not hasattr(index, "search_distinct"):
                raise NotImplementedError(f"{type(index).__name__} has no distinct search")
            take = min(k, count)
            if take > self.DISTINCT_MAX_K:
                raise _DistinctShape(f"k = {take} exceeds {self.DISTINCT_MAX_K}, the most groups a distinct search returns")
            fetch = max(take, min(fetch_k, count, self.DISTINCT_MAX_FETCH))
            grouping = self._resident_grouping(index, group_by)   # (an unhashable value: its TypeError is not retried)
            return index.search_distinct(queries, take, fetch, grouping, rowset=rowset(), normalize_q=True)

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            return [([], [], []) for _ in range(nq)]
        scores, rows = found[0], found[1]
        uids = self._ids.uids
        out = []
        for i in range(nq):
            hits = []
            for row, score in zip(rows[i], scores[i]):
                if row == -1:
                    continue
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[int(row)], score, self.metadata[int(row)]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, False))
        return out

    # ---- group hits search: the k best metadata groups, each with its best rows -----------------------------
    GROUPS_MAX_SIZE = 16       # most rows of one group a call returns (include/mvdb.h "GROUP HITS SEARCH")

    def find_most_similar_groups(self, embedding, group_by, k=5, group_size=3, fetch_k=None, metadata_filter=None,
                                 exclude_filter=None, or_filters=None):
        """The `k` best GROUPS under the filters of ``find_most_similar`` — exactly those of ``find_most_similar_distinct``,
        in its order — each with its `group_size` best rows: "the 5 best documents, and the 3 best chunks of each" of a
        chunked store, in one call and exact (over-fetching and bucketing on the host is wrong when one document fills the
        fetch).  `group_by`, `k` and `fetch_k` are as in ``find_most_similar_distinct``.  No reference counterpart.  Returns
        a list of groups, best group first; each is ``(ids, distances, metadatas)``, best row first, packaged as
        ``find_most_similar`` does without autocut; a group with fewer rows is shorter.  ``group_size`` outside [1, 16] is a
        ValueError."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self.find_most_similar_groups_batch(query, group_by, k, group_size, fetch_k, metadata_filter, exclude_filter,
                                                   or_filters)[0]

    def find_most_similar_groups_batch(self, embeddings, group_by, k=5, group_size=3, fetch_k=None, metadata_filter=None,
                                       exclude_filter=None, or_filters=None):
        """Several queries under ONE filter: element i is what ``find_most_similar_groups(embeddings[i], ...)`` returns."""
        queries = self._range_queries(embeddings)
        nq = queries.shape[0]
        k, group_size = int(k), int(group_size)
        fetch_k = max(4 * k, 32) if fetch_k is None else int(fetch_k)
        if k < 1 or fetch_k < 1:
            raise ValueError("k and fetch_k must be positive")
        if fetch_k < k:
            raise ValueError(f"k = {k} exceeds fetch_k = {fetch_k}")
        if not 1 <= group_size <= self.GROUPS_MAX_SIZE:
            raise ValueError(f"group_size must lie in [1, {self.GROUPS_MAX_SIZE}] (got {group_size})")
        hash(group_by)  # (a metadata key: an unhashable one is the caller's TypeError, before anything is searched)
        if nq == 0 or self._mat is None:
            return [[] for _ in range(nq)]

        def search(index, count, rowset):
            if not hasattr(index, "search_groups"):
                raise NotImplementedError(f"{type(index).__name__} has no group hits search")
            take = min(k, count)
            if take > self.DISTINCT_MAX_K:
                raise _DistinctShape(f"k = {take} exceeds {self.DISTINCT_MAX_K}, the most groups a group hits search returns")
            fetch = max(take, min(fetch_k, count, self.DISTINCT_MAX_FETCH))
            grouping = self._resident_grouping(index, group_by)   # (an unhashable value: its TypeError is not retried)
            return index.search_groups(queries, take, group_size, fetch, grouping, rowset=rowset(), normalize_q=True)

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            return [[] for _ in range(nq)]
        scores, rows = found[0], found[1]
        uids = self._ids.uids
        out = []
        for i in range(nq):
            groups = []
            for grows, gscores in zip(rows[i], scores[i]):
                hits = []
                for row, score in zip(grows, gscores):
                    if row == -1:
                        continue
                    try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                        hits.append((uids[int(row)], score, self.metadata[int(row)]))
                    except (KeyError, IndexError):
                        pass
                if hits:
                    groups.append(self._package(hits, False))
            out.append(groups)
        return out

    # ---- MaxSim search: a question of several vectors, scored per metadata group ----------------------------
    MAXSIM_MAX_K = 64          # most groups one call returns (include/mvdb.h "MAXSIM SEARCH")
    MAXSIM_MAX_VECTORS = 256   # most query vectors of one question

    def find_most_similar_maxsim(self, embeddings, group_by, k=5, metadata_filter=None, exclude_filter=None, or_filters=None):
        """The `k` best GROUPS for ONE question that is several vectors — sub-questions, paraphrases, the token states of a
        late-interaction encoder: `embeddings` is a 2-D ``[T, d]`` array-like, ``1 <= T <= 256``.  A group (the rows that
        share a value under the metadata key `group_by`, as in ``find_most_similar_distinct``: a row without the key is a
        group of its own, an unhashable value is a TypeError naming the id) scores the SUM over the T vectors of its best
        row for each vector (MaxSim), under the filters of ``find_most_similar``; every vector is normalised on the device.
        One pass over the selected rows scores each row against up to 32 of the vectors.  No reference counterpart.  Returns
        ``(ids, scores, metadatas)``, best group first: ``ids[j]`` is a tuple of T unique ids — the row of group j that
        answered vector t —, ``scores[j]`` the group's sum (np.float32), ``metadatas[j]`` the list of those T metadata
        dicts.  `k` is clamped to the number of rows the filters select; ``k > 64`` after that is a ValueError."""
        return self.find_most_similar_maxsim_batch([embeddings], group_by, k, metadata_filter, exclude_filter, or_filters)[0]

    def find_most_similar_maxsim_batch(self, list_of_embeddings, group_by, k=5, metadata_filter=None, exclude_filter=None,
                                       or_filters=None):
        """Several questions — a list of ``[T_i, d]`` arrays — under ONE filter: element i is what
        ``find_most_similar_maxsim(list_of_embeddings[i], ...)`` returns.  One device call per question."""
        questions = []
        for e in list_of_embeddings:
            q = np.ascontiguousarray(np.asarray(e, dtype=np.float32))
            if q.ndim != 2:
                raise ValueError("a MaxSim question must be a 2-D array-like [T, d], one query vector per row")
            if not 1 <= q.shape[0] <= self.MAXSIM_MAX_VECTORS:
                raise ValueError(f"a MaxSim question holds 1 to {self.MAXSIM_MAX_VECTORS} query vectors (got {q.shape[0]})")
            if self._mat is not None and q.shape[1] != self._mat.d:
                raise ValueError(f"query dimension {q.shape[1]} != index dimension {self._mat.d}")
            questions.append(q)
        k = int(k)
        if k < 1:
            raise ValueError("k must be positive")
        hash(group_by)  # (a metadata key: an unhashable one is the caller's TypeError, before anything is searched)
        if not questions or self._mat is None:
            return [([], [], []) for _ in questions]

        def search(index, count, rowset):
            if not hasattr(index, "search_maxsim"):
                raise NotImplementedError(f"{type(index).__name__} has no MaxSim search")
            take = min(k, count)
            if take > self.MAXSIM_MAX_K:
                raise _DistinctShape(f"k = {take} exceeds {self.MAXSIM_MAX_K}, the most groups a MaxSim search returns")
            grouping = self._resident_grouping(index, group_by)   # (an unhashable value: its TypeError is not retried)
            rs = rowset()
            return [index.search_maxsim(q, take, grouping, rowset=rs, normalize_q=True) for q in questions]

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            return [([], [], []) for _ in questions]
        uids = self._ids.uids
        out = []
        for scores, codes, rows, _ in found:
            hits = []
            for j in range(len(codes)):
                if codes[j] < 0:
                    continue
                try:  # a row a concurrent delete has just renumbered away drops its document, as the other searches skip such rows
                    picked = [int(r) for r in rows[j]]
                    hits.append((tuple(uids[r] for r in picked), scores[j], [self.metadata[r] for r in picked]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, False))
        return out

    # ---- search by examples: rows like the positives, unlike the negatives ------------------------------------------
    EXAMPLES_MAX_VECTORS = 256   # most examples of one call, positives and negatives together (include/mvdb.h "SEARCH BY EXAMPLES")
    EXAMPLES_MAX_K = 64

    def _example_matrix(self, ids, embeddings, what):
        """The examples of one side as a [m, d] float32 matrix: the stored vectors of `ids` (what ``get_vector`` returns, an
        unknown id raises what it raises), then `embeddings`."""
        rows = [np.asarray(self.get_vector(u), dtype=np.float32).reshape(-1) for u in ids]
        if embeddings is not None and len(embeddings):
            e = np.asarray(embeddings, dtype=np.float32)
            if e.ndim != 2:
                raise ValueError(f"{what} embeddings must be a 2-D array-like [m, d], one example per row")
            rows.extend(e)
        if not rows:
            return None
        if len({r.shape[0] for r in rows}) != 1:
            raise ValueError(f"{what} examples differ in dimension")
        m = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
        if self._mat is not None and m.shape[1] != self._mat.d:
            raise ValueError(f"example dimension {m.shape[1]} != index dimension {self._mat.d}")
        return m

    def find_most_similar_by_examples(self, positive_ids=(), negative_ids=(), positive_embeddings=None, negative_embeddings=None,
                                      k=5, strategy="best_score", metadata_filter=None, exclude_filter=None, or_filters=None,
                                      autocut=False):
        """The `k` stored embeddings most like the positive examples and unlike the negative ones — "more like these three",
        "like this one, but not like those two" — under the filters of ``find_most_similar``.  An example is a stored id
        (looked up as ``get_vector`` does; the id itself never comes back, even when the filters would not select it) or an
        embedding (which excludes nothing); at least one positive, at most 256 examples in all.  No reference counterpart.

        ``strategy="best_score"``: a row scores ``bp``, its cosine to the NEAREST positive, when that beats ``bn``, its
        cosine to the nearest negative; otherwise ``-(bn * bn)`` — so three positives from three topics return rows of all
        three, and rows near a negative sink by how near they are.  One pass over the selected rows per 32 examples, on the
        device; nothing but the k results comes back.  ``strategy="average_vector"``: the classic single query ``mean(pos)``,
        or ``2 * mean(pos) - mean(neg)`` with negatives (float32 means of the vectors as given), through the same device call
        — ``find_most_similar`` of that vector minus the examples.  Returns ``(ids, scores, metadatas)`` packaged as
        ``find_most_similar`` does.  `k` is clamped to the number of rows the filters select, ``k > 64`` after that is a
        ValueError; fewer than `k` results come back when the examples eat into a small selection."""
        if strategy not in ("best_score", "average_vector"):
            raise ValueError(f"strategy must be 'best_score' or 'average_vector' (got {strategy!r})")
        k = int(k)
        if k < 1:
            raise ValueError("k must be positive")
        positive_ids, negative_ids = list(positive_ids or ()), list(negative_ids or ())
        pos = self._example_matrix(positive_ids, positive_embeddings, "positive")
        neg = self._example_matrix(negative_ids, negative_embeddings, "negative")
        if pos is None:
            raise ValueError("search by examples needs at least one positive example")
        total = pos.shape[0] + (0 if neg is None else neg.shape[0])
        if total > self.EXAMPLES_MAX_VECTORS:
            raise ValueError(f"search by examples takes at most {self.EXAMPLES_MAX_VECTORS} examples (got {total})")
        if neg is not None and neg.shape[1] != pos.shape[1]:
            raise ValueError("positive and negative examples differ in dimension")
        if self._mat is None:
            return [], [], []
        if strategy == "average_vector":
            q = pos.mean(axis=0, dtype=np.float32)
            if neg is not None:
                q = np.float32(2) * q - neg.mean(axis=0, dtype=np.float32)
            pos, neg = np.ascontiguousarray(q[None, :], dtype=np.float32), None
        skip_ids = list(dict.fromkeys(positive_ids + negative_ids))

        def search(index, count, rowset):
            if not hasattr(index, "search_examples"):
                raise NotImplementedError(f"{type(index).__name__} has no search by examples")
            take = min(k, count)
            if take > self.EXAMPLES_MAX_K:
                raise _DistinctShape(f"k = {take} exceeds {self.EXAMPLES_MAX_K}, the most rows a search by examples returns")
            with self.lock:   # the examples' rows as they are NOW: a concurrent delete renumbers them (and outdates the row set)
                try:
                    skip = [self._ids.row(u) for u in skip_ids]
                except KeyError:
                    raise ValueError("Unique ID does not exist.") from None
            return index.search_examples(pos, neg, take, rowset=rowset(), skip_rows=skip, normalize=True)

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            return [], [], []
        scores, rows = found
        uids = self._ids.uids
        hits = []
        for r, s in zip(rows, scores):
            if r == -1:
                continue
            try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                hits.append((uids[int(r)], s, self.metadata[int(r)]))
            except (KeyError, IndexError):
                pass
        return self._package(hits, autocut)

    # ---- boosted search: the cosine plus weighted per-row terms, ranked in one exact pass -------------------------------
    BOOST_MAX_K = 64       # most rows a boosted search returns (include/mvdb.h "BOOSTED SEARCH")
    BOOST_MAX_TERMS = 4    # most metadata keys of one call
    _BOOST_COLUMNS_KEPT = 8   # (key, missing) columns that stay resident

    def _boost_values(self, key, missing):
        """The float32 column of metadata key `key` over the stored rows (caller holds the lock): ``np.float32(v)`` where
        the row's value is a real number — bool is not one —, `missing` where it is anything else or the key is absent."""
        out = np.full(len(self.metadata), missing, dtype=np.float32)
        for row, meta in enumerate(self.metadata):
            v = meta.get(key) if meta else None
            if isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_)):
                out[row] = np.float32(v)
        return out

    def _resident_boost_column(self, index, key, missing):
        """The device-resident column of `key` (`mvdb_rowterm`), cached per (key, missing) — at most eight — and stamped with
        the write generation and the index object, as `_resident_grouping` stamps groupings: any store, delete or metadata
        update since makes the next use build the column again with one pass over the metadata and upload it once (4 bytes
        per row); an embedding-only update keeps it.  A ValueError where the device index is no longer the state the
        metadata describes: `_search_selected` starts over."""
        with self.lock:
            if self._embeddings_changed or self.index is not index:
                raise ValueError("the index changed between the filter and the search")
            gen = self.__dict__.get("_write_gen", 0)
            cache = self.__dict__.get("_boost_columns")
            if cache is None:
                cache = self.__dict__["_boost_columns"] = OrderedDict()
            slot = (key, float(missing))
            hit = cache.get(slot)
            if hit is not None and hit[0] == gen and hit[1] is index:
                cache.move_to_end(slot)
                return hit[2]
            term = index.rowterm(self._boost_values(key, missing))
            # an outdated entry is dropped, not freed: a search running outside the lock may still hold it (its device
            # memory goes when the last reference does)
            cache[slot] = (gen, index, term)
            cache.move_to_end(slot)
            while len(cache) > self._BOOST_COLUMNS_KEPT:
                cache.popitem(last=False)
            return term

    def _boosted(self, queries, boosts, id_boosts, k, score_weight, missing, metadata_filter, exclude_filter, or_filters, autocut):
        k = int(k)
        if k < 1:
            raise ValueError("k must be positive")
        if k > self.BOOST_MAX_K:
            raise ValueError(f"k = {k} exceeds {self.BOOST_MAX_K}, the most rows a boosted search returns")
        boosts = dict(boosts) if boosts else {}
        id_boosts = dict(id_boosts) if id_boosts else {}
        if not boosts and not id_boosts:
            raise ValueError("a boosted search needs something to boost by: boosts or id_boosts")
        if len(boosts) > self.BOOST_MAX_TERMS:
            raise ValueError(f"a boosted search takes at most {self.BOOST_MAX_TERMS} metadata keys (got {len(boosts)})")
        keys = list(boosts)
        for key in keys:
            hash(key)
        weights = np.array([boosts[key] for key in keys], dtype=np.float32)
        missing = np.float32(missing)
        if missing != missing:
            raise ValueError("missing must not be NaN")
        score_weight = float(np.float32(score_weight))
        nq = queries.shape[0]
        if nq == 0 or self._mat is None:
            return [([], [], []) for _ in range(nq)]
        if queries.shape[1] != self._mat.d:
            raise ValueError(f"query dimension {queries.shape[1]} != index dimension {self._mat.d}")

        def search(index, count, rowset):
            if not hasattr(index, "search_boosted"):
                raise NotImplementedError(f"{type(index).__name__} has no boosted search")
            take = min(k, count)
            terms = [self._resident_boost_column(index, key, missing) for key in keys]
            rows, values = [], []
            if id_boosts:
                with self.lock:   # the ids' rows as they are NOW: a concurrent delete renumbers them (and outdates the terms)
                    if self._embeddings_changed or self.index is not index:
                        raise ValueError("the index changed between the filter and the search")
                    for uid, value in id_boosts.items():
                        try:
                            rows.append(self._ids.row(uid))
                        except (KeyError, TypeError):
                            continue   # an id that is not stored boosts nothing
                        values.append(value)
            if not terms and not rows:   # every boosted id is unknown: the plain ranking, through the same call
                rows, values = [0], [0.0]
            return index.search_boosted(queries, take, terms, weights, score_weight=score_weight, sparse_rows=rows or None,
                                        sparse_values=np.asarray(values, dtype=np.float32) if rows else None, rowset=rowset(),
                                        normalize_q=True)

        found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        if found is None:
            return [([], [], []) for _ in range(nq)]
        scores, rows = found
        uids = self._ids.uids
        out = []
        for i in range(nq):
            hits = []
            for row, score in zip(rows[i], scores[i]):
                if row == -1:
                    continue
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[int(row)], score, self.metadata[int(row)]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, autocut))
        return out

    def find_most_similar_boosted(self, embedding, boosts=None, id_boosts=None, k=5, score_weight=1.0, missing=0.0,
                                  metadata_filter=None, exclude_filter=None, or_filters=None, autocut=False):
        """The `k` stored embeddings with the largest ``S = score_weight * cosine + sum(weight * metadata[key]) + id_boost``
        under the filters of ``find_most_similar`` — "rank by relevance, but prefer newer or better-rated passages", or the
        convex combination of hybrid search with the scores of a lexical engine.  The ranking is exact over every selected
        row, in one pass on the device: a row that wins on S from far down the plain ranking is found, which fetching a
        larger top-k and re-ranking on the host cannot promise.  No reference counterpart (its ``hybrid_rerank_results``
        re-weights only the k rows the dense search returned).

        `boosts`: ``{metadata_key: weight}``, one to four keys; the terms are added in the dict's order (float32: ``w1 * v1``,
        then ``+ w2 * v2`` ...).  A row's value under a key is ``np.float32(v)`` when ``v`` is a real number
        (``numbers.Real``; a bool is not one), else — or when the key is absent — `missing`.  The per-key columns stay on the
        device until the next store, delete or metadata update.  `id_boosts`: ``{unique_id: value}``, added as is; ids that
        are not stored are ignored, and an id the filters exclude is still never a result.  At least one of the two.
        Returns ``(ids, scores, metadatas)`` packaged as ``find_most_similar`` does; ``scores`` holds S (np.float32), best
        first, equal S in storage order.  A row whose S is NaN is never a result.  `k` is clamped to the number of rows the
        filters select; ``k > 64`` is a ValueError."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        if query.ndim != 2:
            raise ValueError("embedding must be one vector")
        return self._boosted(query, boosts, id_boosts, k, score_weight, missing, metadata_filter, exclude_filter, or_filters, autocut)[0]

    def find_most_similar_boosted_batch(self, embeddings, boosts, k=5, score_weight=1.0, missing=0.0, metadata_filter=None,
                                        exclude_filter=None, or_filters=None, autocut=False):
        """Several queries under ONE filter and ONE set of `boosts`: element i is what
        ``find_most_similar_boosted(embeddings[i], boosts, ...)`` returns.  The queries share the combined column and one
        launch; each still reads the selected rows once.  No reference counterpart."""
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        if not boosts:
            raise ValueError("a boosted search needs something to boost by: boosts")
        return self._boosted(queries, boosts, None, k, score_weight, missing, metadata_filter, exclude_filter, or_filters, autocut)

    # ---- sparse vectors: exact sparse search, and hybrid search ranked in one exact pass -------------------------------
    SPARSE_MAX_K = 64             # most rows a sparse or hybrid search returns (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH")
    SPARSE_MAX_DIM = 2**31 - 1    # indices live in [0, SPARSE_MAX_DIM)

    @staticmethod
    def _sparse_pair(sparse):
        """``{index: weight}`` or ``(indices, values)`` as (int64 indices ascending, float32 values); None for None or an
        empty one.  A ValueError for an index that is no integer, negative or too large, for a duplicate index and for
        arrays of different lengths."""
        if sparse is None:
            return None
        if isinstance(sparse, dict):
            indices, values = list(sparse.keys()), list(sparse.values())
        else:
            try:
                indices, values = sparse
            except (TypeError, ValueError):
                raise ValueError("a sparse vector is {index: weight} or (indices, values)") from None
        raw = np.asarray(indices).reshape(-1)
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        if len(raw) != len(values):
            raise ValueError(f"a sparse vector needs one value per index ({len(raw)} indices, {len(values)} values)")
        if len(raw) == 0:
            return None
        if raw.dtype.kind not in "iu":
            as_int = raw.astype(np.int64) if raw.dtype.kind == "f" else None
            if as_int is None or not np.array_equal(as_int, raw):
                raise ValueError("the indices of a sparse vector must be integers")
            raw = as_int
        if raw.dtype.kind == "u":
            if raw.max() >= FilterAndRerankMixin.SPARSE_MAX_DIM:
                raise ValueError(f"sparse index {int(raw.max())} is outside [0, 2^31 - 1)")
        idx = raw.astype(np.int64)
        if idx.min() < 0 or idx.max() >= FilterAndRerankMixin.SPARSE_MAX_DIM:
            bad = idx.min() if idx.min() < 0 else idx.max()
            raise ValueError(f"sparse index {int(bad)} is outside [0, 2^31 - 1)")
        order = np.argsort(idx, kind="stable")
        idx, values = idx[order], values[order]
        dup = np.flatnonzero(idx[1:] == idx[:-1])
        if len(dup):
            raise ValueError(f"sparse index {int(idx[dup[0]])} is listed twice")
        return idx, np.ascontiguousarray(values)

    @staticmethod
    def _sparse_dim_for(largest):
        """The smallest power of two above the index `largest` (at most 2^31 - 1)."""
        dim = 1
        while dim <= largest:
            dim *= 2
        return min(dim, FilterAndRerankMixin.SPARSE_MAX_DIM)

    @staticmethod
    def _sparse_csr(uids, vectors):
        """The CSR arrays of the rows `uids` (row order): (indptr int64[n + 1], indices int32, values float32); an id without a
        sparse vector is an empty row."""
        indptr = np.zeros(len(uids) + 1, dtype=np.int64)
        idx, val = [], []
        for row, uid in enumerate(uids):
            pair = vectors.get(uid)
            if pair is not None:
                idx.append(pair[0])
                val.append(pair[1])
                indptr[row + 1] = len(pair[0])
        np.cumsum(indptr, out=indptr)
        indices = np.concatenate(idx).astype(np.int32) if idx else np.empty(0, np.int32)
        values = np.concatenate(val).astype(np.float32) if val else np.empty(0, np.float32)
        return indptr, indices, values

    def _sparse_vectors(self):
        vectors = self.__dict__.get("_sparse")
        if vectors is None:
            vectors = self.__dict__["_sparse"] = {}
        return vectors

    @property
    def sparse_dim(self):
        """The dimension of the sparse vectors: what ``set_sparse_dim`` fixed, else the smallest power of two above the
        largest index stored so far (None before the first one)."""
        return self.__dict__.get("_sparse_dim")

    def set_sparse_dim(self, dim):
        """Fix the dimension of the sparse vectors: indices live in [0, dim), and a later vector with a larger index is a
        ValueError instead of growing the dimension.  `dim` must cover what is stored."""
        dim = int(dim)
        if not 1 <= dim <= self.SPARSE_MAX_DIM:
            raise ValueError("sparse_dim must be in [1, 2^31 - 1]")
        with self.lock:
            largest = max((int(pair[0][-1]) for pair in self._sparse_vectors().values()), default=-1)
            if largest >= dim:
                raise ValueError(f"sparse_dim = {dim} does not cover the stored index {largest}")
            self.__dict__["_sparse_dim"] = dim
            self.__dict__["_sparse_dim_fixed"] = True
            self.__dict__["_sparse_gen"] = self.__dict__.get("_sparse_gen", 0) + 1

    def set_sparse_vector(self, unique_id, sparse):
        """Give the stored id `unique_id` the sparse vector `sparse` — ``{index: weight}`` or ``(indices, values)``, indices
        distinct integers in [0, sparse_dim) — beside its embedding; it replaces an earlier one, None or an empty one removes
        it.  An unknown id is a ValueError.  The vectors live on the host keyed by id (a deleted id loses its vector); the
        next sparse or hybrid search uploads them once.  No reference counterpart."""
        self.set_sparse_vectors_batch([unique_id], [sparse])

    def set_sparse_vectors_batch(self, unique_ids, sparses):
        """``set_sparse_vector`` for several ids; nothing is stored when one of them is refused."""
        unique_ids = list(unique_ids)
        sparses = list(sparses)
        if len(unique_ids) != len(sparses):
            raise ValueError("Sparse vectors must be provided for all unique IDs.")
        pairs = [self._sparse_pair(s) for s in sparses]
        with self.lock:
            for uid in unique_ids:
                if uid not in self._ids:
                    raise ValueError("Unique ID does not exist.")
            largest = max((int(p[0][-1]) for p in pairs if p is not None), default=-1)
            dim = self.__dict__.get("_sparse_dim")
            if largest >= 0 and (dim is None or largest >= dim):
                if self.__dict__.get("_sparse_dim_fixed"):
                    raise ValueError(f"sparse index {largest} is outside [0, {dim}), the dimension set_sparse_dim fixed")
                self.__dict__["_sparse_dim"] = self._sparse_dim_for(largest)
            vectors = self._sparse_vectors()
            for uid, pair in zip(unique_ids, pairs):
                if pair is None:
                    vectors.pop(uid, None)
                else:
                    vectors[uid] = pair
            self.__dict__["_sparse_gen"] = self.__dict__.get("_sparse_gen", 0) + 1

    def get_sparse_vector(self, unique_id):
        """``(indices, values)`` of the id's sparse vector, sorted by index (int64, float32), or None when it has none."""
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            pair = self._sparse_vectors().get(unique_id)
            return None if pair is None else (pair[0].copy(), pair[1].copy())

    def _resident_sparse_store(self, index):
        """The device-resident sparse store (`mvdb_sparse`), stamped with the write generation, the sparse generation and the
        index object as `_resident_boost_column` stamps its columns: a store, a delete, a metadata update or a change of a
        sparse vector since makes the next search assemble the CSR arrays in row order once and upload them once; an
        embedding-only update keeps the store.  A ValueError where the device index is no longer the state the ids describe:
        `_search_selected` starts over."""
        with self.lock:
            if self._embeddings_changed or self.index is not index:
                raise ValueError("the index changed between the filter and the search")
            stamp = (self.__dict__.get("_write_gen", 0), self.__dict__.get("_sparse_gen", 0))
            hit = self.__dict__.get("_sparse_store")
            if hit is not None and hit[0] == stamp and hit[1] is index:
                return hit[2]
            indptr, indices, values = self._sparse_csr(self._ids.uids, self._sparse_vectors())
            store = index.sparse(indptr, indices, values, self.__dict__.get("_sparse_dim") or 1)
            if self.__dict__.get("_sparse_postings"):
                self._sparse_postings_dim_check(store.dim)
                store.build_postings()
            # an outdated store is dropped, not freed: a search running outside the lock may still hold it
            self.__dict__["_sparse_store"] = (stamp, index, store)
            self.__dict__["_sparse_builds"] = self.__dict__.get("_sparse_builds", 0) + 1
            return store

    # ---- the inverted form of the resident sparse store: same results, read from the query's posting lists only ----
    @staticmethod
    def _sparse_postings_dim_check(dim):
        from . import _native
        cap = _native.sparse_postings_geometry()[2]
        if dim is not None and dim > cap:
            raise ValueError(f"sparse postings need sparse_dim <= {cap} (it is {dim}): fix a smaller one with set_sparse_dim, "
                             "or stay without postings (drop_sparse_postings)")

    def build_sparse_postings(self):
        """From now on every resident sparse store this database assembles also builds its posting lists (include/mvdb.h
        "SPARSE POSTINGS"), and sparse and hybrid searches score through them: the same ids and scores, element for element,
        at the cost of the query's lists instead of every stored non-zero.  The first store is assembled at once when
        sparse vectors exist; after a store, a delete, an update or a ``set_sparse_vector`` the next sparse or hybrid search
        rebuilds both, once.  Device memory: + 8 bytes per non-zero + 8 (sparse_dim + 1).  Derived state: not persisted.  A
        ``sparse_dim`` above the cap is a ValueError that names ``set_sparse_dim``.  No reference counterpart."""
        with self.lock:
            self._sparse_postings_dim_check(self.__dict__.get("_sparse_dim"))
            self.__dict__["_sparse_postings"] = True
            # a store assembled without them is dropped, not rebuilt in place: a search outside the lock may still hold it
            self.__dict__.pop("_sparse_store", None)
            if not self._sparse_vectors() or self._mat is None:
                return
            if self._embeddings_changed:
                self._build_index()
            index = self.index
        # outside the lock: it is not re-entrant, and _resident_sparse_store takes it itself
        if index is not None and hasattr(index, "sparse"):
            try:
                self._resident_sparse_store(index)
            except ValueError:
                pass    # a write from another thread came between: the next sparse or hybrid search assembles the store

    def drop_sparse_postings(self):
        """Back to the CSR pass: stores assembled from now on build no posting lists, and the resident one is let go."""
        with self.lock:
            self.__dict__["_sparse_postings"] = False
            self.__dict__.pop("_sparse_store", None)

    def sparse_postings_info(self):
        """``{'enabled', 'built', 'nnz', 'dim', 'bytes'}``: whether ``build_sparse_postings`` is in force, whether the resident
        sparse store is current and holds its posting lists, and then its non-zeros, its dimension and the lists' device
        bytes (0 while not built)."""
        with self.lock:
            stamp = (self.__dict__.get("_write_gen", 0), self.__dict__.get("_sparse_gen", 0))
            hit = self.__dict__.get("_sparse_store")
            built = bool(hit is not None and hit[0] == stamp and hit[1] is self.index and not self._embeddings_changed
                         and hit[2].has_postings)
            nnz = hit[2].nnz if built else 0
            dim = hit[2].dim if built else (self.__dict__.get("_sparse_dim") or 0)
            return {'enabled': bool(self.__dict__.get("_sparse_postings")), 'built': built, 'nnz': nnz, 'dim': dim,
                    'bytes': 8 * nnz + 8 * (dim + 1) if built else 0}

    def _sparse_save(self, path):
        """The sparse vectors beside the main file (caller holds the lock): written when there are any, a leftover file
        removed when there are none."""
        vectors = self._sparse_vectors()
        if vectors:
            with open(path, 'wb') as f:
                pickle.dump({'dim': self.__dict__.get("_sparse_dim"), 'dim_fixed': bool(self.__dict__.get("_sparse_dim_fixed")),
                             'vectors': {uid: (pair[0], pair[1]) for uid, pair in vectors.items()}}, f)
        elif os.path.exists(path):
            os.remove(path)

    def _sparse_load(self, path):
        """Read what `_sparse_save` wrote (caller holds the lock); entries of ids that are not stored are dropped."""
        self.__dict__["_sparse"] = {}
        self.__dict__.pop("_sparse_store", None)
        self.__dict__["_sparse_postings"] = False   # derived state: a loaded database starts without posting lists
        self.__dict__["_sparse_gen"] = self.__dict__.get("_sparse_gen", 0) + 1
        if not os.path.exists(path):
            return
        with open(path, 'rb') as f:
            data = pickle.load(f)
        self.__dict__["_sparse_dim"] = data.get('dim')
        self.__dict__["_sparse_dim_fixed"] = bool(data.get('dim_fixed'))
        self.__dict__["_sparse"] = {uid: (np.asarray(pair[0], dtype=np.int64), np.asarray(pair[1], dtype=np.float32))
                                    for uid, pair in data['vectors'].items() if uid in self._ids}

    def _sparse_search(self, dense, sparse_queries, k, dense_weight, sparse_weight, metadata_filter, exclude_filter, or_filters, autocut):
        """Sparse search (dense None) or hybrid search of the queries: one result triple per query."""
        k = int(k)
        if k < 1:
            raise ValueError("k must be positive")
        if k > self.SPARSE_MAX_K:
            raise ValueError(f"k = {k} exceeds {self.SPARSE_MAX_K}, the most rows a sparse or hybrid search returns")
        pairs = [self._sparse_pair(q) for q in sparse_queries]
        nq = len(pairs)
        if nq == 0 or self._mat is None:
            return [([], [], []) for _ in range(nq)]
        if dense is not None:
            if dense.shape[0] != nq:
                raise ValueError(f"{dense.shape[0]} embeddings, {nq} sparse queries")
            if dense.shape[1] != self._mat.d:
                raise ValueError(f"query dimension {dense.shape[1]} != index dimension {self._mat.d}")
            dense_weight = float(np.float32(dense_weight))
        sparse_weight = float(np.float32(sparse_weight))
        answered = []   # the queries the device sees (sparse search: those that are not empty)

        def search(index, count, rowset):
            if not hasattr(index, "search_sparse"):
                raise NotImplementedError(f"{type(index).__name__} has no sparse search")
            take = min(k, count)
            store = self._resident_sparse_store(index)
            # indices the store's dimension does not cover are dropped: no row can hold them
            queries = []
            for pair in pairs:
                if pair is None:
                    queries.append((np.empty(0, np.int64), np.empty(0, np.float32)))
                else:
                    keep = pair[0] < store.dim
                    queries.append((pair[0][keep], pair[1][keep]))
            del answered[:]
            if dense is None:
                answered.extend(i for i, q in enumerate(queries) if len(q[0]))
                if not answered:
                    return None
                return index.search_sparse(store, [queries[i] for i in answered], take, rowset=rowset())
            answered.extend(range(nq))
            if any(len(q[0]) == 0 for q in queries):
                # a query left empty ranks by the dense score alone, through the same call: the smallest stored index at weight 0
                with self.lock:
                    first = min((int(p[0][0]) for p in self._sparse_vectors().values()), default=0)
                filler = (np.array([min(first, store.dim - 1)], np.int64), np.zeros(1, np.float32))
                queries = [q if len(q[0]) else filler for q in queries]
            return index.search_hybrid(store, dense, queries, take, dense_weight=dense_weight, sparse_weight=sparse_weight, rowset=rowset(),
                                       normalize_q=True)

        found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        out = [([], [], []) for _ in range(nq)]
        if found is None:
            return out
        scores, rows = found
        uids = self._ids.uids
        for slot, i in enumerate(answered):
            hits = []
            for row, score in zip(rows[slot], scores[slot]):
                if row == -1:
                    continue
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[int(row)], score, self.metadata[int(row)]))
                except (KeyError, IndexError):
                    pass
            out[i] = self._package(hits, autocut)
        return out

    def find_most_similar_sparse(self, sparse_query, k=5, metadata_filter=None, exclude_filter=None, or_filters=None, autocut=False):
        """The `k` stored ids whose SPARSE vector scores highest against `sparse_query` (``{index: weight}`` or ``(indices,
        values)``, at most 1,024 terms): the float32 dot product over the indices both hold, under the filters of
        ``find_most_similar``.  Only ids that share an index with the query are results; the ranking is exact over every
        selected row, in one pass over the stored non-zeros on the device.  Query indices beyond ``sparse_dim`` are dropped
        (no row can hold them); a query left empty gives ``([], [], [])``.  Returns ``(ids, scores, metadatas)`` packaged as
        ``find_most_similar`` does, best first, equal scores in storage order; ``k > 64`` is a ValueError.  No reference
        counterpart."""
        return self._sparse_search(None, [sparse_query], k, 1.0, 1.0, metadata_filter, exclude_filter, or_filters, autocut)[0]

    def find_most_similar_sparse_batch(self, sparse_queries, k=5, metadata_filter=None, exclude_filter=None, or_filters=None, autocut=False):
        """Several sparse queries under ONE filter in one launch: element i is what ``find_most_similar_sparse(sparse_queries[i],
        ...)`` returns."""
        return self._sparse_search(None, list(sparse_queries), k, 1.0, 1.0, metadata_filter, exclude_filter, or_filters, autocut)

    def find_most_similar_hybrid(self, embedding, sparse_query, k=5, dense_weight=1.0, sparse_weight=1.0, metadata_filter=None,
                                 exclude_filter=None, or_filters=None, autocut=False):
        """The `k` stored ids with the largest ``S = dense_weight * cosine + sparse_weight * sparse`` — `sparse` the score of
        ``find_most_similar_sparse``, 0 for an id that shares no index with the query — under the filters of
        ``find_most_similar``.  Every selected row is ranked on S in one exact pass on the device: the sparse scores of all rows
        are written as one column, then the boosted search's scan runs over it — a row that wins on S from far down the dense
        ranking is found, which re-ranking a dense top-k (the reference's ``hybrid_rerank_results``) cannot promise.  A sparse
        query left empty (None, or only indices beyond ``sparse_dim``) ranks by ``dense_weight * cosine``.  Returns ``(ids,
        scores, metadatas)``; ``scores`` holds S (np.float32).  ``k > 64`` is a ValueError.  No reference counterpart."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        if query.ndim != 2:
            raise ValueError("embedding must be one vector")
        return self._sparse_search(query, [sparse_query], k, dense_weight, sparse_weight, metadata_filter, exclude_filter, or_filters,
                                   autocut)[0]

    def find_most_similar_hybrid_batch(self, embeddings, sparse_queries, k=5, dense_weight=1.0, sparse_weight=1.0, metadata_filter=None,
                                       exclude_filter=None, or_filters=None, autocut=False):
        """Several (embedding, sparse query) pairs under ONE filter: element i is what ``find_most_similar_hybrid(embeddings[i],
        sparse_queries[i], ...)`` returns.  The queries follow each other on the device; each writes its column and reads the
        selected rows once."""
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        return self._sparse_search(queries, list(sparse_queries), k, dense_weight, sparse_weight, metadata_filter, exclude_filter,
                                   or_filters, autocut)

    # ---- clustering: every selected row labelled by the nearest of a few vectors; spherical k-means -----------------
    ASSIGN_MAX_VECTORS = 4096   # most vectors / clusters of one call (include/mvdb.h "ASSIGN AND K-MEANS")

    def _centre_matrix(self, vectors, what):
        c = np.ascontiguousarray(np.asarray(vectors, dtype=np.float32))
        if c.ndim != 2:
            raise ValueError(f"{what} must be a 2-D array-like [C, d], one vector per row")
        if not 1 <= c.shape[0] <= self.ASSIGN_MAX_VECTORS:
            raise ValueError(f"{what} hold 1 to {self.ASSIGN_MAX_VECTORS} vectors (got {c.shape[0]})")
        if self._mat is not None and c.shape[1] != self._mat.d:
            raise ValueError(f"vector dimension {c.shape[1]} != index dimension {self._mat.d}")
        return c

    def _labelled(self, rows, labels, scores):
        """(ids, labels, scores) of the selected rows, in storage order."""
        uids = self._ids.uids
        return [uids[int(r)] for r in rows], np.ascontiguousarray(labels[rows], dtype=np.int32), np.ascontiguousarray(scores[rows], dtype=np.float32)

    def assign_to_nearest(self, vectors, metadata_filter=None, exclude_filter=None, or_filters=None):
        """Label EVERY stored embedding the filters select with the nearest of `vectors` (a 2-D ``[C, d]`` array-like,
        ``1 <= C <= 4096``; cosine: rows and vectors are normalised) — tag passages with the closest of a set of label
        embeddings, route rows to topics, bucket a corpus.  One pass over the selected rows per 32 vectors, on the device;
        nothing but the labels comes back.  No reference counterpart.  Returns ``(ids, labels, scores)``: `ids` the
        selected unique ids in storage order, ``labels[i]`` (int32) the index into `vectors` of the nearest one — equal
        scores go to the lower index, -1 for a row that scores NaN against all of them —, ``scores[i]`` (float32) that
        score."""
        c = self._centre_matrix(vectors, "the vectors to assign to")
        empty = ([], np.empty(0, np.int32), np.empty(0, np.float32))
        if self._mat is None:
            return empty

        def search(index, count, rowset, selection):
            if not hasattr(index, "assign"):
                raise NotImplementedError(f"{type(index).__name__} has no clustering")
            labels, scores = index.assign(c, rowset=rowset(), normalize_c=True)
            return selection.materialize(), labels, scores

        found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search, with_selection=True)
        return empty if found is None else self._labelled(*found)

    def cluster_embeddings(self, n_clusters, max_iter=25, seed=0, init=None, metadata_filter=None, exclude_filter=None,
                           or_filters=None):
        """Cluster the stored embeddings the filters select into `n_clusters` clusters: spherical k-means (Lloyd's algorithm
        under the cosine), every iteration on the device, bit-identical run to run.  Initial centres: `init`, an
        ``[n_clusters, d]`` array-like, or — ``init=None`` — the stored rows
        ``numpy.random.default_rng(seed).choice(selected_rows, n_clusters, replace=False)``.  At most `max_iter` updates of
        the centres; the run ends earlier once no label changes.  No reference counterpart.  Returns ``(ids, labels, scores,
        centroids)``: `ids`, `labels` (int32) and `scores` (float32) as ``assign_to_nearest(centroids, ...)`` returns them,
        `centroids` the float32 ``[n_clusters, d]`` unit-length centres (a cluster that lost every member keeps its centre).
        Fewer selected rows than `n_clusters` is a ValueError."""
        n_clusters, max_iter = int(n_clusters), int(max_iter)
        if not 1 <= n_clusters <= self.ASSIGN_MAX_VECTORS:
            raise ValueError(f"n_clusters must lie in [1, {self.ASSIGN_MAX_VECTORS}] (got {n_clusters})")
        if max_iter < 1:
            raise ValueError("max_iter must be positive")
        start = None
        if init is not None:
            start = self._centre_matrix(init, "the initial centres")
            if start.shape[0] != n_clusters:
                raise ValueError(f"init holds {start.shape[0]} centres, n_clusters is {n_clusters}")
        too_few = "fewer rows selected ({}) than n_clusters ({})"
        if self._mat is None:
            raise ValueError(too_few.format(0, n_clusters))

        def search(index, count, rowset, selection):
            if not hasattr(index, "kmeans"):
                raise NotImplementedError(f"{type(index).__name__} has no clustering")
            if count < n_clusters:
                raise _DistinctShape(too_few.format(count, n_clusters))
            rows = selection.materialize()
            centres = start
            if centres is None:
                picked = np.random.default_rng(seed).choice(rows, n_clusters, replace=False)
                centres = np.concatenate([index.get_rows(int(r), 1) for r in picked])
            centres, labels, scores, _, _ = index.kmeans(centres, max_iter, rowset=rowset())
            return rows, labels, scores, centres

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search, with_selection=True)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        if found is None:
            raise ValueError(too_few.format(0, n_clusters))
        return self._labelled(*found[:3]) + (found[3],)

    # ---- probed search: a k-means partition of the rows, a query scans the lists of its nprobe nearest centres ----------------
    PROBE_MAX_K = 64

    def build_partition(self, n_clusters=None, max_iter=10, seed=0, train_rows=None, centroids=None):
        """Partition the stored embeddings into `n_clusters` lists by their nearest centre, for ``find_most_similar_approx``.
        `n_clusters` defaults to ``min(4096, max(1, round(sqrt(n))))``.  The centres come from spherical k-means (at most
        `max_iter` updates) over ``min(n, train_rows or 256 * n_clusters)`` stored rows drawn by
        ``numpy.random.default_rng(seed)``, which also draws the initial centres among them; then EVERY row is labelled by its
        nearest centre on the device.  ``centroids=`` (an ``[n_clusters, d]`` array-like, e.g. a saved
        ``partition_centroids()``) skips the training.  The partition lives on the device (8 bytes per row plus the
        centres), follows later stores, updates and deletes by itself and is not persisted.  Returns the list sizes
        (int64 ``[n_clusters]``).  No reference counterpart."""
        with self.lock:
            if self._mat is None or self._mat.n == 0:
                raise ValueError("a partition needs stored embeddings")
            if self._embeddings_changed:
                self._build_index()
            index, n = self.index, self._mat.n
            if not hasattr(index, "partition"):
                raise NotImplementedError(f"{type(index).__name__} has no probed search")
            if centroids is not None:
                centres = self._centre_matrix(centroids, "the centroids")
                if n_clusters is not None and int(n_clusters) != centres.shape[0]:
                    raise ValueError(f"centroids hold {centres.shape[0]} centres, n_clusters is {n_clusters}")
                part = index.partition(centres, labels=None, normalize_c=True)
            else:
                C = min(self.ASSIGN_MAX_VECTORS, max(1, int(round(np.sqrt(n))))) if n_clusters is None else int(n_clusters)
                if not 1 <= C <= min(n, self.ASSIGN_MAX_VECTORS):
                    raise ValueError(f"n_clusters must lie in [1, {min(n, self.ASSIGN_MAX_VECTORS)}] (got {C})")
                if int(max_iter) < 1:
                    raise ValueError("max_iter must be positive")
                rng = np.random.default_rng(seed)
                m = min(n, int(train_rows) if train_rows else 256 * C)
                if m < C:
                    raise ValueError(f"train_rows ({m}) is below n_clusters ({C})")
                sample = np.sort(rng.choice(n, m, replace=False)) if m < n else None
                picked = rng.choice(sample if sample is not None else n, C, replace=False)
                start = np.concatenate([index.get_rows(int(r), 1) for r in picked])
                centres = index.kmeans(start, int(max_iter), rowset=index.rowset(sample) if sample is not None else None)[0]
                part = index.partition(centres, labels=None, normalize_c=False)
            self.__dict__["_partition"] = {"index": index, "part": part, "labels": None, "centres": part.centres(), "changed": set()}
            return part.sizes()

    def drop_partition(self):
        """Forget the partition (its device memory goes with the last search that holds it)."""
        with self.lock:
            self.__dict__["_partition"] = None

    def partition_centroids(self):
        """float32 ``[n_clusters, d]``: the partition's centres as stored (unit length); ``build_partition(centroids=...)``
        rebuilds the same partition from them without k-means."""
        with self.lock:
            state = self.__dict__.get("_partition")
            if state is None:
                raise ValueError("there is no partition: call build_partition first")
            return state["centres"].copy()

    def _partition_rows_changed(self, rows):
        """update_embeddings_batch wrote new vectors into these rows (caller holds the lock): the next approximate search
        assigns them again."""
        state = self.__dict__.get("_partition")
        if state is not None:
            state["changed"].update(int(r) for r in rows)

    def _partition_rows_removed(self, rows):
        """A delete removed these stacked rows, ascending (caller holds the lock): the labels come back to the host once, the
        removed rows' labels are dropped, and the next approximate search re-creates the partition from what is left — no
        k-means, no re-assign."""
        state = self.__dict__.get("_partition")
        if state is None or not len(rows):
            return
        if state["part"] is not None:
            state["labels"] = state["part"].labels()
            state["part"] = None   # dropped, not freed: a search running outside the lock may still hold it
        rows = np.asarray(rows, dtype=np.int64)
        labels = state["labels"]
        state["labels"] = np.delete(labels, rows[rows < labels.shape[0]])
        doomed = set(int(r) for r in rows)
        state["changed"] = {r - int(np.searchsorted(rows, r)) for r in state["changed"] if r not in doomed}

    def _resident_partition(self, index):
        """The partition, brought to the index's current rows (takes the lock).  After stores: ``update``, which labels the new
        rows; after ``update_embedding``: the same call with the changed rows; after a delete: re-created from the labels
        that are left.  A ValueError where the device index is no longer the state the rows describe: `_search_selected`
        starts over."""
        with self.lock:
            if self._embeddings_changed or self.index is not index:
                raise ValueError("the index changed between the filter and the search")
            state = self.__dict__.get("_partition")
            if state is None or state["index"] is not index:
                raise _DistinctShape("there is no partition: call build_partition first")
            n = index.ntotal
            part, changed = state["part"], state["changed"]
            if part is None:
                kept = state["labels"]
                labels = np.full(n, -1, dtype=np.int32)
                labels[:kept.shape[0]] = kept
                changed.update(range(kept.shape[0], n))
                part = state["part"] = index.partition(state["centres"], labels=labels, normalize_c=False)
                state["labels"] = None
            if len(part) < n or changed:
                part.update(sorted(changed))
                changed.clear()
            return part

    def find_most_similar_approx(self, embedding, k=5, nprobe=8, metadata_filter=None, exclude_filter=None, or_filters=None,
                                 autocut=False):
        """``find_most_similar`` over the lists of the `nprobe` centres nearest to the query only (``build_partition``
        first): the ONE search here whose answer can differ from ``find_most_similar`` — a true neighbour that lives in a
        list the query does not probe is missed.  Given the lists the answer is exact (the same scores, ties to the earlier
        row); ``nprobe`` is clipped to the number of lists, where the two calls agree.  A filter that selects few rows
        (its resident row set is a list, not a bitmap) is answered by the exact search under that filter: a superset in
        quality.  ``k > 64`` and a database without a partition are a ValueError.  No reference counterpart."""
        query = np.array([np.array(embedding, dtype=np.float32)])  # [1, d]; normalised on the device
        return self.find_most_similar_approx_batch(query, k, nprobe, metadata_filter, exclude_filter, or_filters, autocut)[0]

    def find_most_similar_approx_batch(self, embeddings, k=5, nprobe=8, metadata_filter=None, exclude_filter=None, or_filters=None,
                                       autocut=False):
        """Several queries under ONE filter: element i is what ``find_most_similar_approx(embeddings[i], ...)`` returns."""
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        k, nprobe = int(k), int(nprobe)
        if k > self.PROBE_MAX_K:
            raise ValueError(f"find_most_similar_approx returns at most {self.PROBE_MAX_K} results per query (k = {k})")
        if nprobe < 1:
            raise ValueError("nprobe must be positive")
        if self.__dict__.get("_partition") is None:
            raise ValueError("there is no partition: call build_partition first")
        nq = queries.shape[0]
        if nq == 0:
            return []

        def search(index, count, rowset):
            if not hasattr(index, "search_probe"):
                raise NotImplementedError(f"{type(index).__name__} has no probed search")
            take = min(k, count)
            rs = rowset()
            if rs is not None and not rs.is_bitmap:   # few rows: the exact gathered scan under the filter, query by query
                each = [index.search_rowset(queries[i:i + 1], take, rs, normalize_q=True) for i in range(nq)]
                return np.concatenate([e[0] for e in each]), np.concatenate([e[1] for e in each])
            part = self._resident_partition(index)
            return index.search_probe(queries, take, min(nprobe, part.n_lists), part, rowset=rs, normalize_q=True)

        try:
            found = self._search_selected(metadata_filter, exclude_filter, or_filters, None, search)
        except _DistinctShape as e:
            raise ValueError(str(e)) from None
        uids = self._ids.uids
        out = []
        for i in range(nq):
            hits = []
            if found is not None:
                for row, score in zip(found[1][i], found[0][i]):
                    if row == -1:
                        continue
                    try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                        hits.append((uids[int(row)], score, self.metadata[int(row)]))
                    except (KeyError, IndexError):
                        pass
            out.append(self._package(hits, autocut))
        return out

    def _group_codes(self, group_by):
        """One pass over the metadata (under the lock): an int32 code per row and the value -> code dict.  Rows that share a
        value share a code; a row without the key gets a code of its own."""
        n = len(self.metadata)
        codes = np.empty(n, dtype=np.int32)
        table = {}
        nxt = 0
        for row, meta in enumerate(self.metadata):
            if group_by in meta:
                value = meta[group_by]
                try:
                    code = table.get(value)
                except TypeError:
                    raise TypeError(f"the value of {group_by!r} of id {self._ids.uids[row]!r} is unhashable "
                                    f"({type(value).__name__}): it cannot name a group") from None
                if code is None:
                    code = table[value] = nxt
                    nxt += 1
            else:
                code = nxt
                nxt += 1
            codes[row] = code
        return codes, table, nxt

    def _resident_grouping(self, index, group_by):
        """The device-resident group codes of `group_by` (`mvdb_grouping`), cached per key — at most four keys — and stamped
        with the write generation and the index object: any store, delete or metadata update since makes the next use build
        the codes again with one pass over the metadata and upload them once (4 bytes per row).  A ValueError where the
        device index is no longer the state the metadata describes: `_search_selected` starts over."""
        with self.lock:
            if self._embeddings_changed or self.index is not index:
                raise ValueError("the index changed between the filter and the search")
            gen = self.__dict__.get("_write_gen", 0)
            cache = self.__dict__.get("_groupings")
            if cache is None:
                cache = self.__dict__["_groupings"] = OrderedDict()
            hit = cache.get(group_by)
            if hit is not None and hit[0] == gen and hit[1] is index:
                cache.move_to_end(group_by)
                return hit[2]
            codes, table, n_groups = self._group_codes(group_by)
            grouping = index.grouping(codes, n_groups)
            # an outdated entry is dropped, not freed: a search running outside the lock may still hold it (its device
            # memory goes when the last reference does)
            cache[group_by] = (gen, index, grouping, codes, table)
            cache.move_to_end(group_by)
            while len(cache) > self._GROUPINGS_KEPT:
                cache.popitem(last=False)
            return grouping

    # ---- a batch in which every query brings its own filter -------------------------------------------------
    _EACH_FILTER_KEYS = ("metadata_filter", "exclude_filter", "or_filters")

    def find_most_similar_each(self, embeddings, filters, k=5, autocut=False):
        """Several queries, EACH UNDER ITS OWN FILTER, in one call (no reference counterpart; a serving layer that collects
        the queries of many callers): ``filters[i]`` is None or a dict with any of ``metadata_filter``, ``exclude_filter``,
        ``or_filters``, and element i of the returned list is what
        ``find_most_similar(embeddings[i], k=k, autocut=autocut, **filters[i])`` returns.  Each distinct filter is evaluated
        once; all queries whose rows live on the device as a row LIST share one gathered launch (`search_grouped`: bit for bit
        the single call's arithmetic), unfiltered queries and queries under one dense (bitmap) set go through the batch
        passes of `find_most_similar_batch`."""
        queries = np.ascontiguousarray(np.asarray(embeddings, dtype=np.float32))
        if queries.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like, one query per row")
        filters = list(filters)
        if len(filters) != queries.shape[0]:
            raise ValueError(f"{len(filters)} filters for {queries.shape[0]} queries")
        specs = []
        for f in filters:
            if f is None:
                specs.append((None, None, None))
                continue
            if not isinstance(f, dict) or any(name not in self._EACH_FILTER_KEYS for name in f):
                raise ValueError("a filter is None or a dict with any of metadata_filter, exclude_filter, or_filters")
            specs.append(tuple(f.get(name) for name in self._EACH_FILTER_KEYS))
        if queries.shape[0] == 0 or self._mat is None:
            return [([], [], []) for _ in range(queries.shape[0])]
        if queries.shape[1] != self._mat.d:
            # before any filter is evaluated: the retry loop below would re-evaluate every distinct filter three times over
            # before handing the index's own ValueError on
            raise ValueError(f"query dimension {queries.shape[1]} != index dimension {self._mat.d}")
        uids = self._ids.uids
        out = []
        for found in self._nearest_rows_each(queries, specs, k):
            hits = []
            for row, score in found:
                try:  # a row a concurrent delete has just renumbered away is skipped, as in find_most_similar
                    hits.append((uids[row], score, self.metadata[row]))
                except (KeyError, IndexError):
                    pass
            out.append(self._package(hits, autocut))
        return out

    def _nearest_rows_each(self, query, specs, k):
        """_nearest_rows_many with one (metadata_filter, exclude_filter, or_filters) triple per query."""
        nq = query.shape[0]
        keys = []
        for i, spec in enumerate(specs):
            if not (spec[0] or spec[1] or spec[2]):
                keys.append(None)            # unfiltered
                continue
            try:
                keys.append(repr(spec))
            except Exception:
                keys.append(("unprintable", i))  # evaluated for this query alone, never cached
        for attempt in range(3):
            # one pass under the lock: device up to date, every DISTINCT filter evaluated (or found resident), generation captured
            groups = OrderedDict()   # key -> [count, rowset, wanted, [queries]]
            with self.lock:
                if self._embeddings_changed:
                    self._build_index()
                index, n_rows = self.index, self._mat.n
                gen = self.__dict__.get("_write_gen", 0)
                cache = self.__dict__.get("_rowsets_each")
                for i, key in enumerate(keys):
                    group = groups.get(key)
                    if group is None:
                        hit = cache.get(key) if (cache and isinstance(key, str)) else None
                        if hit is not None and hit[0] == gen and hit[1] is index:
                            cache.move_to_end(key)
                            group = [hit[2], hit[3], None, []]
                        elif key is None:
                            group = [self._row_count(), None, None, []]
                        else:
                            wanted = self._get_filtered_indices(*specs[i])
                            group = [len(wanted), None, wanted, []]
                        groups[key] = group
                    group[3].append(i)
            found = [[] for _ in range(nq)]
            if index is None:
                return found
            try:
                everything, listed = [], []   # queries over every row; (queries, rowset, count) of the list-form sets
                for key, (count, rowset, wanted, members) in groups.items():
                    if not count:
                        continue
                    if count == n_rows:
                        everything.extend(members)
                        continue
                    if rowset is None:
                        rowset = self._resident_rowset_each(index, wanted, key, gen, n_rows)
                    if getattr(rowset, "is_bitmap", False):
                        # a dense set: its queries share corpus passes under the bitmap (the existing batch route)
                        scores, rows = index.search_rowset(query[members], min(k, count), rowset, normalize_q=True)
                        self._scatter_hits(found, members, scores, rows)
                    else:
                        listed.append((members, rowset, count))
                if everything:
                    everything.sort()
                    scores, rows = index.search(query[everything], min(k, n_rows), normalize_q=True)
                    self._scatter_hits(found, everything, scores, rows)
                if listed and hasattr(index, "search_grouped"):
                    # ONE launch for every query under a row list; a query with fewer rows than the call's k gets -1 padding
                    members = [i for group in listed for i in group[0]]
                    sets = [group[1] for group in listed for _ in group[0]]
                    take = min(k, max(group[2] for group in listed))
                    scores, rows = index.search_grouped(query[members], take, sets, normalize_q=True)
                    self._scatter_hits(found, members, scores, rows)
                else:
                    # an index without a grouped search (the int8 cosine index): one search per distinct filter
                    for members, rowset, count in listed:
                        scores, rows = index.search_rowset(query[members], min(k, count), rowset, normalize_q=True)
                        self._scatter_hits(found, members, scores, rows)
                return found
            except ValueError:
                # another thread deleted rows between the filters and the search: evaluate them again on the current rows
                if attempt == 2:
                    raise
        return found

    @staticmethod
    def _scatter_hits(found, members, scores, rows):
        for j, i in enumerate(members):
            found[i] = [(int(r), s) for r, s in zip(rows[j], scores[j]) if r != -1]

    def _resident_rowset_each(self, index, wanted, key, gen, n_rows):
        """`_resident_rowset` for find_most_similar_each.  A batch with 50 tenants would empty the 16-entry cache of the
        single-filter methods on every call, so this method keeps its own, bounded by DEVICE BYTES: least-recently-used sets go
        once the sets held exceed 2 x 8 B x the current row count (a partition of the corpus into disjoint tenants costs
        exactly 8 B x n as row lists; the factor 2 allows overlapping filters).  Dropped by the same `_note_write`; an evicted
        set stays alive while a running call holds it."""
        if wanted.gone is not None:
            rowset = index.rowset(wanted.gone, excluded=True)
        else:
            rowset = index.rowset(wanted.rows)
        if isinstance(key, str):
            nbytes = (n_rows + 7) // 8 if getattr(rowset, "is_bitmap", False) else 8 * len(wanted)
            bound = 2 * 8 * n_rows
            with self.lock:
                if self.__dict__.get("_write_gen", 0) == gen and self.index is index and nbytes <= bound:
                    cache = self.__dict__.get("_rowsets_each")
                    if cache is None:
                        cache = self.__dict__["_rowsets_each"] = OrderedDict()
                        self.__dict__["_rowsets_each_bytes"] = 0
                    held = self.__dict__.get("_rowsets_each_bytes", 0)
                    old = cache.pop(key, None)
                    if old is not None:
                        held -= old[4]
                    while cache and held + nbytes > bound:
                        held -= cache.popitem(last=False)[1][4]
                    cache[key] = (gen, index, len(wanted), rowset, nbytes)
                    self.__dict__["_rowsets_each_bytes"] = held + nbytes
        return rowset

    def _package(self, hits, autocut):
        """[(id, score, metadata)] -> (ids, distances, metadatas): tuples, three empty lists when there
        is nothing, lists after an autocut (the reference's conventions, vector_database.py:526-536)."""
        if not hits:
            return [], [], []
        ids, distances, metadatas = zip(*hits)
        if autocut and len(distances) > 1:
            dropped = set(self.autocut_scores(distances))
            if dropped:
                keep = [i for i in range(len(ids)) if i not in dropped]
                return [ids[i] for i in keep], [distances[i] for i in keep], [metadatas[i] for i in keep]
        return ids, distances, metadatas

    # ---- metadata filters (semantics of vector_database.py:157-386) ------------------------------------
    def _rows_matching(self, key, value, operators_allowed=True):
        """Sorted rows whose metadata[key] satisfies `value`: plain equality, or {"$op": operand} where operators are
        allowed — only the FIRST operator of the dict is honoured and an unknown one is a ValueError, as in the
        reference (:163-176); exclude-filters compare a dict value by equality (:330-345)."""
        predicate = None
        if operators_allowed and isinstance(value, dict):
            name = next(iter(value))
            test = _OPERATORS.get(name)
            if test is None:
                raise ValueError(f"Invalid operator: {name}")
            operand = value[name]
            predicate = lambda field: test(field, operand)  # noqa: E731
        else:
            values = self._live_value_index()
            if values is None:
                values = self.__dict__["_values"] = _ValueIndex(self._ids)
            rows = values.rows_equal(key, value, self)
            if rows is not None:
                return rows
            predicate = lambda field: field == value  # noqa: E731  (unhashable operand: walk)
        # operators (and unhashable operands) look at every row that has the key, like the reference; an exception of
        # the comparison itself ($gt against None, $in on a number) propagates, as there
        ids, found = self._ids, []
        holders = self.inverted_index.get(key, ())
        if 2 * len(holders) >= len(self.metadata) == len(ids.uids):
            # most rows carry the key: one pass over the rows in order (no id lookups, nothing to sort)
            return np.fromiter((row for row, meta in enumerate(self.metadata) if key in meta and predicate(meta[key])),
                               dtype=np.int64)
        for uid in list(holders):
            if uid in ids.handle:
                row = ids.row(uid)
                if predicate(self.metadata[row].get(key, None)):
                    found.append(row)
        return _sorted_rows(found)

    def _get_filtered_indices(self, metadata_filters, exclude_filter, or_filters):
        """The reference's filter pipeline (vector_database.py:354-386) on sorted row arrays: AND clauses, then OR
        clauses intersected with them, then exclusions.  Returns a `_Selection`.  Control flow that decides which errors
        surface is kept: an AND pass stops reading the keys of one clause once nothing is left (:291-292), an exclusion
        likewise (:347-348), a filter list holding only empty dicts leaves "no selection" behind, which an exclusion then
        trips over with the reference's TypeError."""
        n = self._row_count()
        as_list = lambda f: [f] if isinstance(f, dict) else f  # noqa: E731
        chosen = None        # None: no AND/OR clause has selected anything yet
        if metadata_filters:
            for clause in as_list(metadata_filters):
                for key, value in clause.items():
                    rows = self._rows_matching(key, value)
                    chosen = rows if chosen is None else np.intersect1d(chosen, rows, assume_unique=True)
                    if not len(chosen):
                        break
        selects_all = not metadata_filters   # the reference starts from every row only when no AND filter was given
        if or_filters:
            clauses = [c for c in as_list(or_filters) if c]
            if clauses:
                either = _NO_ROWS
                for clause in clauses:
                    for key, value in clause.items():
                        either = np.union1d(either, self._rows_matching(key, value))
                chosen = either if (chosen is None or selects_all) else np.intersect1d(chosen, either, assume_unique=True)
                selects_all = False
        if exclude_filter:
            if chosen is None and not selects_all:
                # `None -= set` in the reference (metadata_filter=[{}] with an exclusion)
                for clause in as_list(exclude_filter):
                    for key, value in clause.items():
                        self._rows_matching(key, value, operators_allowed=False)
                        raise TypeError("unsupported operand type(s) for -=: 'NoneType' and 'set'")
                return _Selection(n, rows=_NO_ROWS)   # (exclusions without a single key: nothing was ever selected)
            gone = _NO_ROWS
            left = n if chosen is None else len(chosen)
            for clause in as_list(exclude_filter):
                for key, value in clause.items():
                    rows = self._rows_matching(key, value, operators_allowed=False)
                    if chosen is None:
                        gone = np.union1d(gone, rows)
                        left = n - len(gone)
                    else:
                        chosen = np.setdiff1d(chosen, rows, assume_unique=True)
                        left = len(chosen)
                    if not left:
                        break
            if chosen is None:
                return _Selection(n, gone=gone)
        if chosen is None:
            return _Selection(n) if selects_all else _Selection(n, rows=_NO_ROWS)
        return _Selection(n, rows=chosen)

    # ---- hybrid rerank (vector_database.py:388-441): host-side string work, not on the GPU path ---------
    def _fetch_hash_text_features(self, text):
        if self.hash_vectorizer is None:
            from sklearn.feature_extraction.text import HashingVectorizer
            self.hash_vectorizer = HashingVectorizer(ngram_range=(1, 6), analyzer='char', n_features=64)
        counts = self.hash_vectorizer.fit_transform([text]).toarray()
        return np.sum(counts, axis=0).tolist()

    def _calculate_text_hash_scores(self, query, documents):
        """Cosine between the character n-gram hash vectors of the query and of each document."""
        if len(documents) == 0:
            return []
        unit = lambda v: np.asarray(v) / np.linalg.norm(v)  # noqa: E731
        q = unit(self._fetch_hash_text_features(query))
        return [np.dot(q, unit(self._fetch_hash_text_features(doc))) for doc in documents]

    def _calculate_fuzzy_ratios(self, query, documents):
        from ._fuzz import partial_ratio
        return [partial_ratio(query, doc) for doc in documents]

    def hybrid_rerank_results(self, sentences, search_scores, query, k=5, weights=(0.80, 0.15, 0.05)):
        """Blend the search scores with the two lexical scores and re-rank (vector_database.py:413-441).  Kept quirk:
        sentences and blended scores share ONE numpy string table, so the ranking sorts the scores AS STRINGS and the
        returned scores are strings; any failure falls back to the first k inputs."""
        try:
            lexical = self._calculate_text_hash_scores(query, sentences)
            fuzzy = self._calculate_fuzzy_ratios(query, sentences)
            if len(lexical) == 0:
                return sentences[:k], search_scores[:k]
            w_search, w_lexical, w_fuzzy = weights
            blended = w_search * np.array(search_scores) + w_lexical * np.array(lexical) + w_fuzzy * np.array(fuzzy)
            table = np.column_stack((np.array(sentences), np.array(blended)))
            table = table[table[:, 1].argsort()[::-1]]
            return tuple(table[:, 0])[:k], tuple(table[:, 1])[:k]
        except Exception:
            return sentences[:k], search_scores[:k]

    # ---- autocut (vector_database.py:443-464): numpy.float32 arithmetic element by element, as the reference -----------
    def autocut_scores(self, score_list):
        """Indices to drop: everything after the steepest relative drop between neighbours, if that drop exceeds 20 %."""
        drops = [(score_list[i - 1] - score_list[i]) / score_list[i - 1] for i in range(1, len(score_list))]
        steepest = max(drops)
        if steepest > 0.2:
            return list(range(drops.index(steepest) + 1, len(score_list)))
        return []


class UpdateMixin:
    """``update_embedding`` / ``update_embeddings_batch`` of the database classes that write (no reference counterpart: the
    reference raises on a duplicate id, and so does ``store_embedding`` here).  The id keeps its row, its handle and its
    place in its shard file; the embedding is overwritten where it lives (`_RowStore.replace`: the device row through
    ``set_rows``, which keeps every derived store of the index in step), the metadata dict is REPLACED, not merged.

    Needs what FilterAndRerankMixin needs; a class that persists per id overrides `_persist_update`."""

    def update_embedding(self, unique_id, embedding=None, metadata_dict=None):
        self.update_embeddings_batch([unique_id], None if embedding is None else [embedding],
                                     None if metadata_dict is None else [metadata_dict])

    def update_embeddings_batch(self, unique_ids, embeddings=None, metadata_dicts=None):
        """None means "keep"; both None is a ValueError.  All-or-nothing: every check runs before anything changes."""
        unique_ids = list(unique_ids)
        if embeddings is None and metadata_dicts is None:
            raise ValueError("Nothing to update: pass embeddings, metadata, or both.")
        with self.lock:
            if embeddings is not None and len(embeddings) != len(unique_ids):
                raise ValueError("Number of unique IDs must match number of embeddings.")
            if metadata_dicts is not None and len(metadata_dicts) != len(unique_ids):
                raise ValueError("Metadata dictionaries must be provided for all unique IDs.")
            if any(uid not in self._ids for uid in unique_ids):
                raise ValueError("Unique ID does not exist.")
            if len(set(unique_ids)) != len(unique_ids):
                raise ValueError("Unique ID listed more than once.")
            if metadata_dicts is not None:
                metadata_dicts = list(metadata_dicts)
                if any(not isinstance(m, dict) for m in metadata_dicts):
                    raise ValueError("Metadata must be a dictionary.")
            vectors = None
            if embeddings is not None and unique_ids:
                if isinstance(embeddings, np.ndarray) and embeddings.ndim == 2:
                    vectors = np.array(embeddings, dtype=np.float32)
                else:
                    rows = [np.array(e, dtype=np.float32) for e in embeddings]
                    if any(v.ndim != 1 or v.shape[0] != self._mat.d for v in rows):
                        raise ValueError(f"Embedding size must be {self._mat.d}.")
                    vectors = np.stack(rows)
                if vectors.shape[1] != self._mat.d:
                    raise ValueError(f"Embedding size must be {self._mat.d}.")
            if not unique_ids:
                return
            rows = [self._ids.row(uid) for uid in unique_ids]
            if vectors is not None:
                # Row numbers and filter results stay as they are, so the cached row sets and `_write_gen` stay too: a set a
                # concurrent search builds from rows it read before this call still names the right rows.  That search sees
                # either the old rows or the new ones — the index takes set_rows exclusively — and the two-call range search
                # notices counts that moved between its calls and runs both again.
                self._mat.replace(rows, vectors, self.index)
                self._partition_rows_changed(rows)
            if metadata_dicts is not None:
                values = self._live_value_index()
                inverted = self.inverted_index
                for uid, row, new in zip(unique_ids, rows, metadata_dicts):
                    old = self.metadata[row]
                    if values is not None:
                        values.note_update(self._ids.handle[uid], old, new)
                    for key in old:
                        holders = inverted.get(key)
                        if holders is not None:
                            holders.discard(uid)
                            if not holders:
                                del inverted[key]
                    self.metadata[row] = new
                    for key in new:
                        inverted[key].add(uid)
                self._note_write()   # filter results moved: cached row sets go, as after a store
            self._persist_update(unique_ids, vectors, metadata_dicts)

    def _persist_update(self, unique_ids, vectors, metadata_dicts):
        """Per-id storage of the class (shard files); nothing for a class that persists as a whole."""
