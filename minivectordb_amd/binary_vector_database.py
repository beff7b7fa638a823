"""BinaryVectorDatabase — 1-bit embeddings, exact Hamming search (faiss.IndexBinaryFlat's place in the flat family).

The models whose embeddings are 1024 to 4096 floats wide also publish them as sign bits ("ubinary": np.packbits(x > 0)), 32 times
smaller than fp32.  This class stores such rows packed on the device (`_native.BitsIndex`, include/mvdb.h "binary index") and
answers with integer Hamming distances, ascending, ties to the lower row.  An embedding is either a float vector of
``embedding_size`` — sign-packed on the device — or a uint8 vector of ``embedding_size / 8`` bytes, taken as packed.

A class of its own, not a subclass of the fp32 databases: no scores, no rerank, no autocut.  Ids, metadata and the metadata
filters are `_dbcore`'s, as they are: `_IdIndex`, `_ValueIndex` and `_get_filtered_indices` give the selected rows, which become
a bitmap uploaded with the call (no resident row sets here).
"""
import os
import pickle
import threading
from collections import defaultdict

import numpy as np

from ._dbcore import FilterAndRerankMixin, _IdIndex


class BinaryVectorDatabase:
    # the filter evaluation of the fp32 classes, unchanged: it needs _ids, metadata, inverted_index and the value index
    _get_filtered_indices = FilterAndRerankMixin._get_filtered_indices
    _rows_matching = FilterAndRerankMixin._rows_matching
    _live_value_index = FilterAndRerankMixin._live_value_index
    _row_count = FilterAndRerankMixin._row_count

    def __init__(self, embedding_size, storage_file=None, device=0):
        """embedding_size: bits per embedding, a multiple of 128 in [128, 4096].  storage_file: None keeps nothing on disk."""
        embedding_size = int(embedding_size)
        if embedding_size % 128 or not 128 <= embedding_size <= 4096:
            raise ValueError("embedding_size must be a multiple of 128 in [128, 4096]")
        self.embedding_size = embedding_size
        self.storage_file = storage_file
        self._device = device
        self.metadata = []
        self._ids = _IdIndex()
        self.inverted_index = defaultdict(set)
        self.index = None      # _native.BitsIndex, created with the first flush
        self._pending = []     # (is_float, [m, .] block) stored since the last flush, in order
        self.lock = threading.Lock()
        if storage_file is not None and os.path.exists(storage_file):
            with open(storage_file, 'rb') as f:
                data = pickle.load(f)
            if data['embedding_size'] != embedding_size:
                raise ValueError(f"{storage_file} holds embeddings of {data['embedding_size']} bits")
            self.metadata = data['metadata']
            self._ids = _IdIndex(data['unique_ids'])
            self.inverted_index = data['inverted_index']
            if len(data['rows']):
                self._pending.append((False, data['rows']))

    # ---- rows ------------------------------------------------------------------------------------------------
    def _classify(self, embedding):
        """(is_float, 1-D array): a uint8 vector of embedding_size / 8 is packed, anything of embedding_size is floats."""
        a = np.asarray(embedding)
        if a.dtype == np.uint8 and a.shape == (self.embedding_size // 8,):
            return False, a
        if a.shape == (self.embedding_size,):
            return True, a.astype(np.float32)
        raise ValueError(f"expected {self.embedding_size} floats or {self.embedding_size // 8} packed uint8, got "
                         f"{a.dtype} {a.shape}")

    def _blocks(self, embeddings):
        """Consecutive embeddings of one kind stacked: [(is_float, [m, .] array)], order kept."""
        blocks = []
        for is_float, a in map(self._classify, embeddings):
            if blocks and blocks[-1][0] == is_float:
                blocks[-1][1].append(a)
            else:
                blocks.append((is_float, [a]))
        return [(is_float, np.stack(rows)) for is_float, rows in blocks]

    def _flush(self):
        """Bring the device rows up to date (caller holds the lock)."""
        from . import _native
        if self.index is None:
            self.index = _native.BitsIndex(self.embedding_size, device=self._device)
        for is_float, block in self._pending:
            (self.index.add_float if is_float else self.index.add)(block)
        self._pending = []

    # ---- ingest / delete -----------------------------------------------------------------------------------------
    def store_embedding(self, unique_id, embedding, metadata_dict={}):
        self.store_embeddings_batch([unique_id], [embedding], [metadata_dict])

    def store_embeddings_batch(self, unique_ids, embeddings, metadata_dicts=[]):
        unique_ids = list(unique_ids)
        with self.lock:
            if len(set(unique_ids)) != len(unique_ids) or any(uid in self._ids for uid in unique_ids):
                raise ValueError("Unique ID already exists.")
            if len(embeddings) != len(unique_ids) or 0 < len(metadata_dicts) < len(unique_ids):
                raise ValueError("Embeddings and metadata dictionaries must be provided for all unique IDs.")
            metadata_dicts = list(metadata_dicts) or [{} for _ in unique_ids]
            self._pending.extend(self._blocks(embeddings))
            values = self._live_value_index()
            handle = self._ids.next
            self._ids.extend(unique_ids)
            self.metadata.extend(metadata_dicts)
            for uid, meta in zip(unique_ids, metadata_dicts):
                for key in meta:
                    self.inverted_index[key].add(uid)
                if values is not None and meta:
                    values.note_store(handle, meta)
                handle += 1

    def delete_embedding(self, unique_id):
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            self._flush()
            meta = self.metadata[self._ids.row(unique_id)]
            values = self._live_value_index()
            if values is not None and meta:
                values.note_delete(self._ids.handle[unique_id], meta)
            for key in meta:
                holders = self.inverted_index.get(key)
                if holders is not None:
                    holders.discard(unique_id)
                    if not holders:
                        del self.inverted_index[key]
            row = self._ids.pop(unique_id)
            del self.metadata[row]
            self.index.remove_rows([row])

    def get_vector(self, unique_id):
        """The stored row, packed: uint8 [embedding_size / 8]."""
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            self._flush()
            return self.index.get_rows(self._ids.row(unique_id), 1)[0]

    def persist_to_disk(self):
        if self.storage_file is None:
            raise ValueError("this database has no storage_file")
        with self.lock:
            self._flush()
            data = {'embedding_size': self.embedding_size, 'rows': self.index.get_rows(0, self.index.ntotal),
                    'unique_ids': list(self._ids.uids), 'metadata': self.metadata, 'inverted_index': self.inverted_index}
            with open(self.storage_file, 'wb') as f:
                pickle.dump(data, f)

    # ---- search ------------------------------------------------------------------------------------------------
    def find_most_similar(self, embedding, metadata_filter=None, exclude_filter=None, or_filters=None, k=5):
        """(ids, distances, metadatas) of the k rows nearest by Hamming distance, nearest first, ties to the earlier row."""
        return self.find_most_similar_batch([embedding], metadata_filter, exclude_filter, or_filters, k)[0]

    def find_most_similar_batch(self, embeddings, metadata_filter=None, exclude_filter=None, or_filters=None, k=5):
        """One (ids, distances, metadatas) per embedding; the filters apply to all of them."""
        from . import _native
        with self.lock:
            nq = len(embeddings)
            n = len(self._ids)
            if nq == 0 or n == 0:
                return [([], [], []) for _ in range(nq)]
            self._flush()
            mask, selected = None, n
            if metadata_filter or exclude_filter or or_filters:
                sel = self._get_filtered_indices(metadata_filter, exclude_filter, or_filters)
                selected = len(sel)
                if not sel.everything:
                    mask = _native.pack_row_mask(n, rows=sel.rows, excluded=sel.gone)
            k = min(int(k), selected)
            if k <= 0:
                return [([], [], []) for _ in range(nq)]
            D = np.empty((nq, k), dtype=np.int32)
            I = np.empty((nq, k), dtype=np.int64)
            at = 0
            for is_float, block in self._blocks(embeddings):   # queries of one kind travel together
                search = self.index.search_float if is_float else self.index.search
                D[at:at + len(block)], I[at:at + len(block)] = search(block, k, mask)
                at += len(block)
            uids, metadata = self._ids.uids, self.metadata
            return [([uids[r] for r in I[i]], [int(h) for h in D[i]], [metadata[r] for r in I[i]]) for i in range(nq)]
