"""Sparse postings without a device (include/mvdb.h "SPARSE POSTINGS"): the posting route's arithmetic — term at a time, the
query's terms in ascending index order — gives the bits and the matched counts of the CSR contract (tests/sparse_oracle.py),
the header declares the new symbols and _native.py binds them, and the database classes carry the new methods."""
import os
import re

import numpy as np
import pytest

from postings_oracle import scores_by_postings, transpose
from sparse_oracle import scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mvdb_sparse_build_postings", "mvdb_sparse_drop_postings", "mvdb_sparse_has_postings", "mvdb_sparse_postings_geometry",
               "mvdb_sparse_postings_read", "mvdb_index_sparse_postings_counters"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_store(rng, n, dim, mean):
    """CSR rows with empty rows, negative values, signed zeros, infinities and NaN; index dim - 1 is held by no row."""
    lengths = rng.poisson(mean, n)
    lengths[rng.random(n) < 0.15] = 0
    lengths = np.minimum(lengths, dim - 1)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(dim - 1, int(m), replace=False)) for m in lengths] + [np.empty(0, np.int64)]).astype(np.int64)
    values = rng.standard_normal(len(indices)).astype(np.float32)
    special = rng.random(len(indices))
    for lo, v in ((0.00, 0.0), (0.02, -0.0), (0.04, np.inf), (0.05, -np.inf), (0.06, np.nan)):
        values[(special >= lo) & (special < lo + 0.01 + 0.01 * (v == 0.0))] = np.float32(v)
    return indptr, indices, values


def same_columns(got, want, what):
    (T, matched), (T0, matched0) = got, want
    assert np.array_equal(matched, matched0), (what, np.flatnonzero(matched != matched0)[:10])
    nan = T0 != T0
    assert np.array_equal(T != T, nan), (what, "NaN rows")
    diff = np.flatnonzero((bits(T) != bits(T0)) & ~nan)
    assert len(diff) == 0, (what, diff[:10], T[diff[:10]], T0[diff[:10]])


@pytest.mark.parametrize("n,dim,mean", [(1, 8, 3), (40, 12, 5), (300, 50, 8), (200, 4000, 30)])
def test_the_posting_route_is_the_csr_contract_bit_for_bit(n, dim, mean):
    rng = np.random.default_rng(100 * n + dim)
    indptr, indices, values = random_store(rng, n, dim, mean)
    post_ptr, rows, vals = transpose(indptr, indices, values, dim)
    assert post_ptr[0] == 0 and post_ptr[-1] == len(indices) and post_ptr[dim - 1] == post_ptr[dim]      # the index no row holds
    for t in range(dim):
        assert (np.diff(rows[post_ptr[t]:post_ptr[t + 1]].astype(np.int64)) > 0).all()                  # rows ascending within a list
    assert (np.diff(indptr) == 0).any() or n == 1
    for m in (1, 2, min(dim, 7), min(dim, 64)):
        q_idx = np.sort(rng.choice(dim, m, replace=False))
        if m > 1:
            q_idx[-1] = dim - 1                                                                          # a term no row holds
        q_val = rng.standard_normal(m).astype(np.float32)
        q_val[rng.random(m) < 0.3] *= -1
        for name, order in (("ascending", np.arange(m)), ("descending", np.arange(m)[::-1]), ("shuffled", rng.permutation(m))):
            want = scores(indptr, indices, values, q_idx[order], q_val[order])
            got = scores_by_postings(post_ptr, rows, vals, n, q_idx[order], q_val[order])
            same_columns(got, want, (n, dim, m, name))


def test_cancellation_signed_zeros_and_non_finite_values():
    """Row 0 cancels to +0.0, row 1 is -0.0 + +0.0, row 2 meets inf - inf, row 3 holds a NaN, row 4 is +inf, row 5 empty, row 6
    matches nothing.  The query gives two indices one weight, in descending order."""
    indptr = np.array([0, 2, 4, 6, 8, 9, 9, 10])
    indices = np.array([3, 11, 3, 11, 3, 11, 3, 19, 3, 40])
    values = np.array([2.5, -2.5, -0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, np.inf, 7.0], np.float32)
    q_idx, q_val = np.array([19, 11, 3]), np.array([-1.3, 0.75, 0.75], np.float32)
    want = scores(indptr, indices, values, q_idx, q_val)
    got = scores_by_postings(*transpose(indptr, indices, values, 50), 7, q_idx, q_val)
    same_columns(got, want, "special rows")
    T, matched = got
    assert matched.tolist() == [2, 2, 2, 2, 1, 0, 0]
    assert bits(T[:2]).tolist() == [0, 0] and T[2] != T[2] and T[3] != T[3] and T[4] == np.inf and bits(T[5:]).tolist() == [0, 0]


def test_the_header_declares_the_new_symbols_and_native_binds_them():
    from minivectordb_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvdb.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mvdb_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mvdb.h"
        assert name in _native.PROTOTYPES, f"{name} has no ctypes prototype"
    for name in ("build_postings", "drop_postings", "has_postings", "postings"):
        assert hasattr(_native.SparseStore, name), name
    assert hasattr(_native.FlatIndex, "sparse_postings_counters") and callable(_native.sparse_postings_geometry)


def test_the_classes_carry_the_methods_and_a_fresh_database_is_disabled(tmp_path):
    from minivectordb_amd import ShardedVectorDatabase, ShardedVectorDatabaseUsearch, VectorDatabase
    for cls in (VectorDatabase, ShardedVectorDatabase):
        for name in ("build_sparse_postings", "drop_sparse_postings", "sparse_postings_info"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    assert db.sparse_postings_info() == {'enabled': False, 'built': False, 'nnz': 0, 'dim': 0, 'bytes': 0}
    rows = np.random.default_rng(1).standard_normal((5, 16)).astype(np.float32)
    db.store_embeddings_batch(list(range(5)), rows, [{} for _ in range(5)])
    db.set_sparse_vector(2, {9: 0.5})
    info = db.sparse_postings_info()
    assert info['enabled'] is False and info['built'] is False and info['dim'] == 16 and info['bytes'] == 0
    # a class without sparse vectors refuses them as it refuses the vectors themselves
    u = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    for name in ("build_sparse_postings", "drop_sparse_postings", "sparse_postings_info"):
        with pytest.raises(NotImplementedError, match="sparse"):
            getattr(u, name)()


def test_build_sparse_postings_does_not_hold_the_lock_over_the_store(tmp_path):
    """The database lock is not re-entrant and `_resident_sparse_store` takes it: building at once, with sparse vectors present,
    must return.  The device index is a stand-in that records what it was asked for."""
    import threading
    from minivectordb_amd import VectorDatabase

    class Store:
        dim, nnz, has_postings = 16, 1, False

        def build_postings(self):
            self.has_postings = True

    class Index:
        def sparse(self, indptr, indices, values, dim):
            self.store = Store()
            return self.store

    db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    db.store_embeddings_batch(list(range(5)), np.random.default_rng(1).standard_normal((5, 16)).astype(np.float32), [{} for _ in range(5)])
    db.set_sparse_vector(2, {9: 0.5})
    db.index, db._embeddings_changed = Index(), False
    worker = threading.Thread(target=db.build_sparse_postings, daemon=True)
    worker.start()
    worker.join(20)
    assert not worker.is_alive(), "build_sparse_postings never returned: it waits for a lock it holds"
    assert db.index.store.has_postings
    info = db.sparse_postings_info()
    assert info == {'enabled': True, 'built': True, 'nnz': 1, 'dim': 16, 'bytes': 8 + 8 * 17}
