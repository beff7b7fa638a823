"""ShardedVectorDatabaseUsearch — drop-in for ``minivectordb.sharded_vector_database_usearch.ShardedVectorDatabaseUsearch``.

The reference stores the same shard pickles as ``ShardedVectorDatabase`` (raw fp32 rows: this class never normalises a
stored row) and, for EVERY query, builds a usearch ``Index(metric='cos', dtype='int8')`` over the filtered rows and asks
its HNSW graph for the k nearest (sharded_vector_database_usearch.py:598-662).  Here the rows' int8 codes stay resident
on the device (``_native.Cos8Index``, csrc/cos8.hip) and every query is an EXACT scan under the same quantisation and
distance (include/mvdb.h "int8 cosine index"): what HNSW returns whenever HNSW is exact.  The fp32 rows stay on the host,
where ``get_vector``, ``embeddings`` and the shard files need them.

Deliberate deviations:
  - the query is quantised straight from fp32; the reference normalises it in fp32 first (faiss.normalize_L2, :602),
    and the quantiser normalises again in fp64, so the two differ only at the rounding level;
  - results are exact, not HNSW-approximate; ties go to the lower stacked row;
  - ``get_vector`` indexes the shard with the row's position inside that shard (the reference uses the stacked row
    number, :84-95), as ``ShardedVectorDatabase`` does.
"""
import numpy as np

from .sharded_vector_database import ShardedVectorDatabase

_WARNING = """
            Warning: You are using the `usearch` version of MiniVectorDB.
            This version is focused on being lightweight, that uses uint8 instead of float32 for embeddings.
            This version does not keep an index active at all times, it always creates the index on demand (per query).
        """


class _HostRows:
    """The stacked fp32 rows on the HOST (unnormalised, as stored); rows [0, synced) also live, quantised, in the device
    index.  Same interface as ``_dbcore._RowStore``."""

    def __init__(self, d):
        self.d = d
        self.synced = 0
        self._blocks = []
        self._n = 0

    @classmethod
    def adopt(cls, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        m = cls(arr.shape[1])
        if arr.shape[0]:
            m._blocks.append(arr)
            m._n = arr.shape[0]
        return m

    @property
    def n(self):
        return self._n

    def _matrix(self):
        if len(self._blocks) != 1:
            self._blocks = [np.concatenate(self._blocks, axis=0) if self._blocks else np.zeros((0, self.d), np.float32)]
        return self._blocks[0]

    def append(self, rows):
        rows = np.asarray(rows, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.shape[1] != self.d:
            raise ValueError(
                f"all the input array dimensions except for the concatenation axis must match exactly, "
                f"but along dimension 1, the array at index 0 has size {self.d} and the array at index 1 "
                f"has size {rows.shape[1]}")
        self._blocks.append(np.array(rows, dtype=np.float32))
        self._n += rows.shape[0]

    def flush(self, index):
        """Quantise and upload the rows stored since the last build (the host keeps them)."""
        if self.synced < self._n:
            index.add(self._matrix()[self.synced:])
            self.synced = self._n

    def delete(self, rows, index):
        rows = sorted(int(r) for r in rows)
        dev = [r for r in rows if r < self.synced]
        if dev:
            index.remove_rows(dev)
            self.synced -= len(dev)
        self._blocks = [np.delete(self._matrix(), rows, axis=0)]
        self._n = self._blocks[0].shape[0]

    def replace(self, rows, vectors, index):
        """Overwrite the stacked rows `rows` (distinct): the codes of the rows already flushed through ONE
        `Cos8Index.set_rows`, then the host matrix.  The device goes first: if it refuses, nothing changed."""
        rows = np.asarray(rows, dtype=np.int64)
        vectors = np.asarray(vectors, dtype=np.float32)
        on_device = rows < self.synced
        if on_device.any():
            index.set_rows(rows[on_device], vectors[on_device])
        self._matrix()[rows] = vectors

    def row(self, r, index=None):
        return self._matrix()[r].copy()

    def materialize(self, index=None):
        return self._matrix()


class ShardedVectorDatabaseUsearch(ShardedVectorDatabase):
    _row_store = _HostRows

    def __init__(self, storage_dir='db_shards_usearch', shard_size=5000, device=0):
        """storage_dir, shard_size: as in the reference (sharded_vector_database_usearch.py:10).  device: the GPU that
        holds the codes."""
        print(_WARNING)
        super().__init__(storage_dir=storage_dir, shard_size=shard_size, device=device)

    def _build_index(self):
        """Quantise the rows stored since the last build into the device index (caller holds the lock)."""
        from . import _native
        if self.index is None:
            self.index = _native.Cos8Index(self.embedding_size, device=self._device)
        if self._mat.n > 0:
            self._mat.flush(self.index)
            self._embeddings_changed = False

    def autocut_distances(self, distance_list):
        """Indices to drop: everything after the steepest relative INCREASE between neighbours, if it exceeds 20 %
        (sharded_vector_database_usearch.py:565-585).  Distances are numpy float32 as usearch returns them: a zero
        previous distance gives inf (or nan) with a RuntimeWarning, not an exception."""
        distance_increases = []
        for i in range(1, len(distance_list)):
            distance_increases.append((distance_list[i] - distance_list[i - 1]) / distance_list[i - 1])
        max_distance_increase = max(distance_increases)
        if max_distance_increase > 0.2:
            return list(range(distance_increases.index(max_distance_increase) + 1, len(distance_list)))
        return []

    def _package(self, hits, autocut):
        """[(id, distance, metadata)] -> (ids, distances, metadatas) as the reference's find_most_similar (:650-662)."""
        if not hits:
            return [], [], []
        ids, distances, metadatas = zip(*hits)
        if autocut and len(distances) > 1:
            remove = self.autocut_distances(distances)
            if remove:
                ids = [ids[i] for i in range(len(ids)) if i not in remove]
                distances = [distances[i] for i in range(len(distances)) if i not in remove]
                metadatas = [metadatas[i] for i in range(len(metadatas)) if i not in remove]
        return ids, distances, metadatas

    # ---- range search: not on the int8 cosine index --------------------------------------------------------------
    _NO_RANGE = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: a range search over int8 cosine "
                 "distances is not implemented (use ShardedVectorDatabase)")

    def find_all_similar(self, *args, **kwargs):
        raise NotImplementedError(self._NO_RANGE)

    def find_all_similar_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_RANGE)

    def count_similar(self, *args, **kwargs):
        raise NotImplementedError(self._NO_RANGE)

    def count_similar_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_RANGE)

    # ---- MMR search: not on the int8 cosine index -----------------------------------------------------------------
    _NO_MMR = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: MMR search, whose selection takes "
               "inner products of stored fp32 rows, is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_mmr(self, *args, **kwargs):
        raise NotImplementedError(self._NO_MMR)

    def find_most_similar_mmr_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_MMR)

    # ---- distinct search: not here ---------------------------------------------------------------------------------
    _NO_DISTINCT = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: distinct search, whose second tier is an exact fp32 pass with a per-group maximum, "
                   "is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_distinct(self, *args, **kwargs):
        raise NotImplementedError(self._NO_DISTINCT)

    def find_most_similar_distinct_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_DISTINCT)

    # ---- group hits search: not here -------------------------------------------------------------------------------
    _NO_GROUPS = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: group hits search, whose member pass scores "
                 "the rows of the winning groups in exact fp32, is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_groups(self, *args, **kwargs):
        raise NotImplementedError(self._NO_GROUPS)

    def find_most_similar_groups_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_GROUPS)

    # ---- MaxSim search: not on the int8 cosine index ----------------------------------------------------------------
    _NO_MAXSIM = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: MaxSim search, an exact fp32 pass "
                  "with a per-group maximum for every query vector, is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_maxsim(self, *args, **kwargs):
        raise NotImplementedError(self._NO_MAXSIM)

    def find_most_similar_maxsim_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_MAXSIM)

    # ---- clustering (assign_to_nearest, cluster_embeddings): not here ------------------------------------------------------------
    _NO_CLUSTERING = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: clustering, exact fp32 passes that label "
                      "every row by its nearest centre, is not implemented (use ShardedVectorDatabase)")

    def assign_to_nearest(self, *args, **kwargs):
        raise NotImplementedError(self._NO_CLUSTERING)

    def cluster_embeddings(self, *args, **kwargs):
        raise NotImplementedError(self._NO_CLUSTERING)

    # ---- probed search (build_partition, find_most_similar_approx): not here ---------------------------------------------------
    _NO_PROBE = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: probed search, whose partition is built by "
                 "the exact fp32 passes of clustering, is not implemented (use ShardedVectorDatabase)")

    def build_partition(self, *args, **kwargs):
        raise NotImplementedError(self._NO_PROBE)

    def drop_partition(self, *args, **kwargs):
        raise NotImplementedError(self._NO_PROBE)

    def partition_centroids(self, *args, **kwargs):
        raise NotImplementedError(self._NO_PROBE)

    def find_most_similar_approx(self, *args, **kwargs):
        raise NotImplementedError(self._NO_PROBE)

    def find_most_similar_approx_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_PROBE)

    # ---- search by examples: not on the int8 cosine index -------------------------------------------------------------
    _NO_EXAMPLES = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: search by examples, an exact fp32 pass "
                    "that keeps every row's best positive and best negative score, is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_by_examples(self, *args, **kwargs):
        raise NotImplementedError(self._NO_EXAMPLES)

    # ---- boosted search: not on the int8 cosine index ------------------------------------------------------------------
    _NO_BOOST = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: boosted search, an exact fp32 pass that "
                 "adds a per-row term to every score, is not implemented (use ShardedVectorDatabase)")

    def find_most_similar_boosted(self, *args, **kwargs):
        raise NotImplementedError(self._NO_BOOST)

    def find_most_similar_boosted_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_BOOST)

    # ---- sparse vectors and hybrid search: not on the int8 cosine index ---------------------------------------------
    _NO_SPARSE = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: sparse vectors, whose hybrid search "
                  "adds a column of sparse scores to an exact fp32 pass, are not implemented (use ShardedVectorDatabase)")

    def set_sparse_dim(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def set_sparse_vector(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def set_sparse_vectors_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def get_sparse_vector(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def find_most_similar_sparse(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def find_most_similar_sparse_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def find_most_similar_hybrid(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def find_most_similar_hybrid_batch(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def build_sparse_postings(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def drop_sparse_postings(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    def sparse_postings_info(self, *args, **kwargs):
        raise NotImplementedError(self._NO_SPARSE)

    # ---- duplicate-pair search: not on the int8 cosine index ---------------------------------------------------------
    _NO_JOIN = ("ShardedVectorDatabaseUsearch keeps int8 codes on the device, not fp32 rows: the duplicate-pair search, a range "
                "search of stored fp32 rows against each other, is not implemented (use ShardedVectorDatabase)")

    def find_duplicate_pairs(self, *args, **kwargs):
        raise NotImplementedError(self._NO_JOIN)

    def count_duplicate_pairs(self, *args, **kwargs):
        raise NotImplementedError(self._NO_JOIN)

    def find_duplicate_groups(self, *args, **kwargs):
        raise NotImplementedError(self._NO_JOIN)
