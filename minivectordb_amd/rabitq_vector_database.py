"""RabitqVectorDatabase — embeddings stored at one bit per dimension plus two floats (faiss.IndexRaBitQ's place in the flat
family).

A row is centred, rotated by a seeded random rotation — `rounds` rounds of sign flips and a Walsh-Hadamard transform — and
kept as its sign bits, ``embedding_size / 8`` bytes, with two factors.  The codes live on the device (`_native.RabitqIndex`,
include/mvdb.h "RaBitQ index"); the original vectors are NOT kept.  The query is cut to 4 bits per dimension per call and the
scores are estimates of the inner product on its own scale, best first; every batch size returns the same answer and there is
no re-ranking.

`train` sets the centroid to the column mean (taken here in numpy float64) while nothing is stored; without it the centroid is
zero.  Ids, metadata and the metadata filters are `_dbcore`'s, as in SQ4VectorDatabase: the selected rows become a bitmap
uploaded with the call.
"""
import os
import pickle
import threading
from collections import defaultdict

import numpy as np

from ._dbcore import FilterAndRerankMixin, _IdIndex


class RabitqVectorDatabase:
    _get_filtered_indices = FilterAndRerankMixin._get_filtered_indices
    _rows_matching = FilterAndRerankMixin._rows_matching
    _live_value_index = FilterAndRerankMixin._live_value_index
    _row_count = FilterAndRerankMixin._row_count

    def __init__(self, embedding_size, storage_file=None, seed=0, rounds=4, device=0):
        """embedding_size: a multiple of 128 up to 4096.  storage_file: None keeps nothing on disk; a file that exists brings
        its own rotation and centroid.  seed, rounds: the rotation's sign bits are drawn from numpy.random.default_rng(seed),
        rounds in [0, 4]."""
        from . import _native
        self.embedding_size = int(embedding_size)
        self.storage_file = storage_file
        self.metadata = []
        self._ids = _IdIndex()
        self.inverted_index = defaultdict(set)
        self.lock = threading.Lock()
        self.index = _native.RabitqIndex(self.embedding_size, device=device)
        if storage_file is not None and os.path.exists(storage_file):
            with open(storage_file, 'rb') as f:
                data = pickle.load(f)
            if data['embedding_size'] != self.embedding_size:
                raise ValueError(f"{storage_file} holds a database of {data['embedding_size']} dimensions")
            self.metadata = data['metadata']
            self._ids = _IdIndex(data['unique_ids'])
            self.inverted_index = data['inverted_index']
            self.index.set_rotation(data['signs'])
            self.index.set_centroid(data['centroid'])
            if len(data['codes']):
                self.index.add_codes(data['codes'], data['factors'])
        else:
            bits = np.random.default_rng(seed).integers(0, 2, (int(rounds), self.embedding_size), dtype=np.uint8)
            self.index.set_rotation(np.packbits(bits, axis=1))

    # ---- training ------------------------------------------------------------------------------------------------
    def train(self, embeddings):
        """Set the centroid to the column mean of `embeddings` [n, embedding_size] while nothing is stored."""
        x = np.ascontiguousarray(embeddings, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.embedding_size or x.shape[0] < 1:
            raise ValueError(f"expected rows of {self.embedding_size} floats, got {x.shape}")
        with self.lock:
            if len(self._ids):
                raise ValueError("train before storing: the stored codes were coded with the present centroid")
            self.index.set_centroid(x.mean(axis=0, dtype=np.float64).astype(np.float32))

    # ---- ingest / delete / update --------------------------------------------------------------------------------
    def _vectors(self, embeddings, count):
        x = np.asarray(embeddings, dtype=np.float32).reshape(count, -1)
        if x.shape[1] != self.embedding_size:
            raise ValueError(f"Embedding size must be {self.embedding_size}.")
        return x

    def store_embedding(self, unique_id, embedding, metadata_dict={}):
        self.store_embeddings_batch([unique_id], [embedding], [metadata_dict])

    def store_embeddings_batch(self, unique_ids, embeddings, metadata_dicts=[]):
        unique_ids = list(unique_ids)
        with self.lock:
            if len(set(unique_ids)) != len(unique_ids) or any(uid in self._ids for uid in unique_ids):
                raise ValueError("Unique ID already exists.")
            if len(embeddings) != len(unique_ids) or 0 < len(metadata_dicts) < len(unique_ids):
                raise ValueError("Embeddings and metadata dictionaries must be provided for all unique IDs.")
            if not unique_ids:
                return
            metadata_dicts = list(metadata_dicts) or [{} for _ in unique_ids]
            self.index.add(self._vectors(embeddings, len(unique_ids)))
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

    def _drop_metadata(self, unique_id, meta, values):
        if values is not None and meta:
            values.note_delete(self._ids.handle[unique_id], meta)
        for key in meta:
            holders = self.inverted_index.get(key)
            if holders is not None:
                holders.discard(unique_id)
                if not holders:
                    del self.inverted_index[key]

    def delete_embedding(self, unique_id):
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            self._drop_metadata(unique_id, self.metadata[self._ids.row(unique_id)], self._live_value_index())
            row = self._ids.pop(unique_id)
            del self.metadata[row]
            self.index.remove_rows([row])

    def persist_to_disk(self):
        """Codes, factors, the rotation's sign bits and the centroid; the floats are not kept."""
        if self.storage_file is None:
            raise ValueError("this database has no storage_file")
        with self.lock:
            codes, factors = self.index.get_rows(0, self.index.ntotal)
            data = {'embedding_size': self.embedding_size, 'signs': self.index.get_rotation(),
                    'centroid': self.index.get_centroid(), 'codes': codes, 'factors': factors,
                    'unique_ids': list(self._ids.uids), 'metadata': self.metadata, 'inverted_index': self.inverted_index}
            with open(self.storage_file, 'wb') as f:
                pickle.dump(data, f)

    # ---- search ------------------------------------------------------------------------------------------------
    def find_most_similar(self, embedding, metadata_filter=None, exclude_filter=None, or_filters=None, k=5):
        """(ids, scores, metadatas) of the k best rows, best first, ties to the earlier row."""
        return self.find_most_similar_batch([embedding], metadata_filter, exclude_filter, or_filters, k)[0]

    def find_most_similar_batch(self, embeddings, metadata_filter=None, exclude_filter=None, or_filters=None, k=5):
        """One (ids, scores, metadatas) per embedding; the filters apply to all of them."""
        from . import _native
        with self.lock:
            nq = len(embeddings)
            n = len(self._ids)
            if nq == 0 or n == 0:
                return [([], [], []) for _ in range(nq)]
            mask, selected = None, n
            if metadata_filter or exclude_filter or or_filters:
                sel = self._get_filtered_indices(metadata_filter, exclude_filter, or_filters)
                selected = len(sel)
                if not sel.everything:
                    mask = _native.pack_row_mask(n, rows=sel.rows, excluded=sel.gone)
            k = min(int(k), selected)
            if k <= 0:
                return [([], [], []) for _ in range(nq)]
            D, I = self.index.search(self._vectors(embeddings, nq), k, mask)
            uids, metadata = self._ids.uids, self.metadata
            return [([uids[r] for r in I[i] if r >= 0], [float(s) for s, r in zip(D[i], I[i]) if r >= 0],
                     [metadata[r] for r in I[i] if r >= 0]) for i in range(nq)]
