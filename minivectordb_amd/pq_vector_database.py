"""PQVectorDatabase — product-quantised embeddings, ADC search (faiss.IndexPQ's place in the flat family).

Between one byte and one bit per dimension: a row is ``n_subvectors`` code bytes, each naming one of 256 centroids of its slice
of the embedding, so at 512 dimensions and 64 sub-vectors a row is the binary index's 64 bytes with a usable ranking.  The codes
live on the device (`_native.PQIndex`, include/mvdb.h "product-quantised index"); the original vectors are NOT kept, so scores
are estimates (inner products, best first, or squared distances, nearest first) and there is no re-ranking.

The codebooks come from `train` — Lloyd's algorithm per sub-space on the device, started from 256 seeded sample rows — and
must exist before anything is stored.  Ids, metadata and the metadata filters are `_dbcore`'s, as in BinaryVectorDatabase: the
selected rows become a bitmap uploaded with the call.
"""
import os
import pickle
import threading
from collections import defaultdict

import numpy as np

from ._dbcore import FilterAndRerankMixin, _IdIndex


def default_subvectors(embedding_size):
    """embedding_size // 8, raised to 16 and rounded up to the next multiple of 16 that divides the size."""
    for m in range(max(16, -(-(embedding_size // 8) // 16) * 16), min(embedding_size, 256) + 1, 16):
        if embedding_size % m == 0:
            return m
    raise ValueError(f"no multiple of 16 from {max(16, embedding_size // 8)} to 256 divides embedding_size {embedding_size}")


class PQVectorDatabase:
    _get_filtered_indices = FilterAndRerankMixin._get_filtered_indices
    _rows_matching = FilterAndRerankMixin._rows_matching
    _live_value_index = FilterAndRerankMixin._live_value_index
    _row_count = FilterAndRerankMixin._row_count

    def __init__(self, embedding_size, n_subvectors=None, metric="ip", storage_file=None, device=0):
        """metric: "ip" (scores are estimated inner products, best first) or "l2" (estimated squared distances, nearest
        first).  storage_file: None keeps nothing on disk."""
        from . import _native
        self.embedding_size = int(embedding_size)
        self.n_subvectors = default_subvectors(self.embedding_size) if n_subvectors is None else int(n_subvectors)
        if metric not in ("ip", "l2"):
            raise ValueError('metric must be "ip" or "l2"')
        self.metric = metric
        self.storage_file = storage_file
        self.metadata = []
        self._ids = _IdIndex()
        self.inverted_index = defaultdict(set)
        self.lock = threading.Lock()
        self.index = _native.PQIndex(self.embedding_size, self.n_subvectors,
                                     _native.METRIC_IP if metric == "ip" else _native.METRIC_L2, device=device)
        self.is_trained = False
        if storage_file is not None and os.path.exists(storage_file):
            with open(storage_file, 'rb') as f:
                data = pickle.load(f)
            if (data['embedding_size'], data['n_subvectors'], data['metric']) != (self.embedding_size, self.n_subvectors, metric):
                raise ValueError(f"{storage_file} holds a ({data['embedding_size']}, {data['n_subvectors']}, "
                                 f"{data['metric']}) database")
            self.metadata = data['metadata']
            self._ids = _IdIndex(data['unique_ids'])
            self.inverted_index = data['inverted_index']
            if data['codebooks'] is not None:
                self.index.set_codebooks(data['codebooks'])
                self.is_trained = True
                if len(data['codes']):
                    self.index.add_codes(data['codes'])

    # ---- training ------------------------------------------------------------------------------------------------
    def train(self, embeddings, iters=25, seed=0, max_samples=65536):
        """Learn the codebooks from `embeddings` [n >= 256, embedding_size] while nothing is stored: at most max_samples rows
        picked with a generator seeded by `seed`, the first 256 of them sliced into sub-vectors as the start."""
        x = np.ascontiguousarray(embeddings, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.embedding_size or x.shape[0] < 256:
            raise ValueError(f"expected at least 256 rows of {self.embedding_size} floats, got {x.shape}")
        with self.lock:
            if len(self._ids):
                raise ValueError("train before storing: the stored codes name the centroids they were coded with")
            rng = np.random.default_rng(seed)
            sample = x[rng.permutation(x.shape[0])[:max_samples]]
            start = sample[:256].reshape(256, self.n_subvectors, -1).transpose(1, 0, 2)
            self.index.set_codebooks(start)
            self.index.train(sample, iters)
            self.is_trained = True

    # ---- ingest / delete -----------------------------------------------------------------------------------------
    def store_embedding(self, unique_id, embedding, metadata_dict={}):
        self.store_embeddings_batch([unique_id], [embedding], [metadata_dict])

    def store_embeddings_batch(self, unique_ids, embeddings, metadata_dicts=[]):
        unique_ids = list(unique_ids)
        with self.lock:
            if not self.is_trained:
                raise ValueError("the database has no codebooks: call train first")
            if len(set(unique_ids)) != len(unique_ids) or any(uid in self._ids for uid in unique_ids):
                raise ValueError("Unique ID already exists.")
            if len(embeddings) != len(unique_ids) or 0 < len(metadata_dicts) < len(unique_ids):
                raise ValueError("Embeddings and metadata dictionaries must be provided for all unique IDs.")
            if not unique_ids:
                return
            metadata_dicts = list(metadata_dicts) or [{} for _ in unique_ids]
            self.index.add(np.asarray(embeddings, dtype=np.float32).reshape(len(unique_ids), -1))
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

    def reconstruct(self, unique_id):
        """The centroids the stored codes name, joined: float32 [embedding_size]."""
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            codes = self.index.get_codes(self._ids.row(unique_id), 1)[0]
            return self.index.get_codebooks()[np.arange(self.n_subvectors), codes].reshape(-1)

    def persist_to_disk(self):
        if self.storage_file is None:
            raise ValueError("this database has no storage_file")
        with self.lock:
            data = {'embedding_size': self.embedding_size, 'n_subvectors': self.n_subvectors, 'metric': self.metric,
                    'codebooks': self.index.get_codebooks() if self.is_trained else None,
                    'codes': self.index.get_codes(0, self.index.ntotal), 'unique_ids': list(self._ids.uids),
                    'metadata': self.metadata, 'inverted_index': self.inverted_index}
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
            D, I, _ = self.index.search(np.asarray(embeddings, dtype=np.float32).reshape(nq, -1), k, mask)
            uids, metadata = self._ids.uids, self.metadata
            return [([uids[r] for r in I[i] if r >= 0], [float(s) for s, r in zip(D[i], I[i]) if r >= 0],
                     [metadata[r] for r in I[i] if r >= 0]) for i in range(nq)]
