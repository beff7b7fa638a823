"""MXVectorDatabase — embeddings stored as OCP microscaling blocks: MXFP4 (4.25 bits per dimension) or MXFP8 (8.25).

A block of 32 dimensions is 32 small floats (E2M1 or E4M3) under one power-of-two scale byte, so there are no ranges and nothing
is trained.  The rows live on the device (`_native.MxIndex`, include/mvdb.h "MX INDEX") and are scored by CDNA4's scaled matrix
instruction, which takes the stored blocks as its operands.  The original vectors are NOT kept, so scores are estimates of the
inner product, best first.  The query is encoded as MXFP8 per call, and a query's answer does not depend on how many queries
share its call.

With `refine=True` the database also keeps every row as IEEE binary16 (`_native.RefineStore`, include/mvdb.h "REFINE STORE":
2 more bytes per dimension), and a search takes `fetch_k` candidates by the MX score and returns their best k by the fp32 inner
product with those rows: the scores are then products with the binary16 rows, not estimates.

Ids, metadata and the metadata filters are `_dbcore`'s, as in SQ4VectorDatabase: the selected rows become a bitmap uploaded with
the call.
"""
import os
import pickle
import threading
from collections import defaultdict

import numpy as np

from ._dbcore import FilterAndRerankMixin, _IdIndex


class MXVectorDatabase:
    _get_filtered_indices = FilterAndRerankMixin._get_filtered_indices
    _rows_matching = FilterAndRerankMixin._rows_matching
    _live_value_index = FilterAndRerankMixin._live_value_index
    _row_count = FilterAndRerankMixin._row_count

    def __init__(self, embedding_size, element_bits=4, storage_file=None, device=0, refine=False, fetch_k=None):
        """embedding_size: a multiple of 128 up to 4096.  element_bits: 4 (MXFP4) or 8 (MXFP8).  storage_file: None keeps
        nothing on disk.  refine: keep binary16 rows and re-rank every search against them.  fetch_k: candidates per query of a
        refined search, at most 1024 (None: max(64, 4 k))."""
        from . import _native
        self.embedding_size = int(embedding_size)
        self.element_bits = int(element_bits)
        self.storage_file = storage_file
        self.metadata = []
        self._ids = _IdIndex()
        self.inverted_index = defaultdict(set)
        self.lock = threading.Lock()
        self.index = _native.MxIndex(self.embedding_size, self.element_bits, device=device)
        self.fetch_k = fetch_k
        self.refine = _native.RefineStore(self.embedding_size, device=device) if refine else None
        if storage_file is not None and os.path.exists(storage_file):
            with open(storage_file, 'rb') as f:
                data = pickle.load(f)
            if (data['embedding_size'], data['element_bits']) != (self.embedding_size, self.element_bits):
                raise ValueError(f"{storage_file} holds a database of {data['embedding_size']} dimensions at "
                                 f"{data['element_bits']} bits")
            self.metadata = data['metadata']
            self._ids = _IdIndex(data['unique_ids'])
            self.inverted_index = data['inverted_index']
            if self.refine is not None and 'refine_rows' not in data:
                raise ValueError(f"{storage_file} was written without refine rows; open it with refine=False")
            if len(data['codes']):
                self.index.add_codes(data['codes'], data['scales'])
                if self.refine is not None:   # (binary16 -> fp32 -> binary16 is the identity)
                    self.refine.add(data['refine_rows'].view(np.float16).astype(np.float32))

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
            x = self._vectors(embeddings, len(unique_ids))
            self.index.add(x)
            if self.refine is not None:
                self.refine.add(x)
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
            if self.refine is not None:
                self.refine.remove_rows([row])

    def update_embedding(self, unique_id, embedding=None, metadata_dict=None):
        """Replace the stored vector (encoded in place, the row keeps its number), the metadata, or both; None means "keep"."""
        if embedding is None and metadata_dict is None:
            raise ValueError("Nothing to update: pass an embedding, metadata, or both.")
        if metadata_dict is not None and not isinstance(metadata_dict, dict):
            raise ValueError("Metadata must be a dictionary.")
        with self.lock:
            if unique_id not in self._ids:
                raise ValueError("Unique ID does not exist.")
            row = self._ids.row(unique_id)
            if embedding is not None:
                self.index.set_rows([row], self._vectors([embedding], 1))
                if self.refine is not None:
                    self.refine.set_rows([row], self._vectors([embedding], 1))
            if metadata_dict is not None:
                values = self._live_value_index()
                if values is not None:
                    values.note_update(self._ids.handle[unique_id], self.metadata[row], metadata_dict)
                self._drop_metadata(unique_id, self.metadata[row], None)
                self.metadata[row] = metadata_dict
                for key in metadata_dict:
                    self.inverted_index[key].add(unique_id)

    def persist_to_disk(self):
        if self.storage_file is None:
            raise ValueError("this database has no storage_file")
        with self.lock:
            codes, scales = self.index.get_codes(0, self.index.ntotal)
            data = {'embedding_size': self.embedding_size, 'element_bits': self.element_bits, 'codes': codes, 'scales': scales,
                    'unique_ids': list(self._ids.uids), 'metadata': self.metadata, 'inverted_index': self.inverted_index}
            if self.refine is not None:
                data['refine_rows'] = self.refine.get_rows(0, self.refine.ntotal)
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
            if self.refine is not None:
                fetch_k = min(max(k, min(1024, self.fetch_k or max(64, 4 * k))), selected)
                D, I = self.index.search_refined(self._vectors(embeddings, nq), k, self.refine, fetch_k, mask)
            else:
                D, I = self.index.search(self._vectors(embeddings, nq), k, mask)
            uids, metadata = self._ids.uids, self.metadata
            return [([uids[r] for r in I[i] if r >= 0], [float(s) for s, r in zip(D[i], I[i]) if r >= 0],
                     [metadata[r] for r in I[i] if r >= 0]) for i in range(nq)]
