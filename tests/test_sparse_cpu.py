"""Sparse vectors without a GPU: tests/sparse_oracle.py (the contract in numpy float32) against scipy.sparse in float64, the
host helpers of the database mixin (normalising a sparse vector, the dimension, the CSR assembly in row order), the host state
through real stores and deletes, the sidecar file, and the classes that refuse."""
import os

import numpy as np
import pytest

from maxsim_oracle import MISSING
from sparse_oracle import scores, sparse_term, sparse_topk

D = 16


def random_csr(rng, n, dim, mean):
    lengths = np.minimum(rng.poisson(mean, n), dim)
    lengths[[0, n - 1]] = 0
    indices = [np.sort(rng.choice(dim, int(m), replace=False)) for m in lengths]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate(indices).astype(np.int32)
    return indptr, indices, rng.standard_normal(len(indices)).astype(np.float32)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,mean,m", [(50, 12, 7), (50, 30, 50), (1 << 14, 40, 300), (50, 12, 1)])
def test_the_oracle_against_scipy_in_float64(dim, mean, m):
    """fp32 products are exact in float64; the fp32 chain of `matched` sums is within matched * 2^-23 * sum|products| of the
    exact sum (each partial sum is bounded by sum|products|, each rounding by 2^-24 of it), and so is scipy's float64 result."""
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(dim + mean + m)
    n = 400
    indptr, indices, values = random_csr(rng, n, dim, mean)
    q_idx = rng.permutation(dim)[:m]
    q_val = rng.standard_normal(m).astype(np.float32)
    T, matched = scores(indptr, indices, values, q_idx, q_val)
    assert T.dtype == np.float32 and matched.dtype == np.int32
    csr = sp.csr_matrix((values.astype(np.float64), indices, indptr), shape=(n, dim))
    q = np.zeros(dim)
    q[q_idx] = q_val
    want = csr @ q
    present = np.zeros(dim, bool)
    present[q_idx] = True
    pattern = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, dim))
    assert np.array_equal(matched, (pattern @ present.astype(np.float64)).astype(np.int32))
    mass = abs(csr) @ np.abs(q)
    assert (np.abs(T.astype(np.float64) - want) <= matched * 2.0**-23 * mass).all()
    assert (T[matched == 0] == 0).all() and not np.signbit(T[matched == 0]).any()
    assert (matched == 0).any() and (m < 7 or (matched > 1).any())


def test_the_oracle_orders_and_drops_as_the_contract_says():
    indptr = np.array([0, 2, 3, 3, 5, 6, 8, 9])
    indices = np.array([1, 4, 1, 1, 4, 4, 1, 4, 7])
    values = np.array([2.5, -2.5, 1.0, np.inf, -np.inf, np.nan, 1.0, 0.0, 3.0], np.float32)
    T, matched = scores(indptr, indices, values, [4, 1], [2.0, 2.0])
    assert matched.tolist() == [2, 1, 0, 2, 1, 2, 0]
    assert T[0] == 0 and not np.signbit(T[0]) and T[1] == 2 and T[2] == 0 and T[3] != T[3] and T[4] != T[4] and T[5] == 2 and T[6] == 0
    D_, I_ = sparse_topk(T, matched, np.arange(7), 5)
    assert I_.tolist() == [1, 5, 0, -1, -1] and D_[:3].tolist() == [2.0, 2.0, 0.0] and (D_[3:] == MISSING).all()     # ties: the lower row
    D_, I_ = sparse_topk(T, matched, [5, 0, 6], 1)
    assert I_.tolist() == [5]
    # stored order matters in fp32: (1e8 + 1) - 1e8 is 0, (1e8 - 1e8) + 1 is 1
    T, _ = scores([0, 3, 6], [1, 2, 3, 1, 2, 3], np.array([1e8, 1.0, -1e8, 1e8, -1e8, 1.0], np.float32), [3, 2, 1], [1.0, 1.0, 1.0])
    assert T.tolist() == [0.0, 1.0]
    assert sparse_term(np.array([0.0, 3.0], np.float32), -0.7).view(np.uint32).tolist() == \
        (np.float32(-0.7) * np.array([0.0, 3.0], np.float32)).view(np.uint32).tolist()


# ---- the mixin's host helpers ---------------------------------------------------------------------------------------------------

def test_sparse_vectors_are_normalised_sorted_and_checked():
    from minivectordb_amd._dbcore import FilterAndRerankMixin as M
    idx, val = M._sparse_pair({9: 0.5, 2: -1.0, 40: 3})
    assert idx.dtype == np.int64 and val.dtype == np.float32 and idx.tolist() == [2, 9, 40] and val.tolist() == [-1.0, 0.5, 3.0]
    idx, val = M._sparse_pair(([9, 2, 40], [0.5, -1.0, 3]))
    assert idx.tolist() == [2, 9, 40] and val.tolist() == [-1.0, 0.5, 3.0]
    idx, val = M._sparse_pair((np.array([7, 3], np.uint32), np.array([1, 2], np.float64)))
    assert idx.tolist() == [3, 7] and val.tolist() == [2.0, 1.0]
    assert M._sparse_pair(([4.0], [1.0]))[0].tolist() == [4]
    assert M._sparse_pair(None) is None and M._sparse_pair({}) is None and M._sparse_pair(([], [])) is None
    for bad, msg in ((([1, 2, 1], [1, 2, 3]), "index 1 is listed twice"), (([1, 2], [1.0]), "one value per index"),
                     (([-1], [1.0]), "index -1 is outside"), (([2**31 - 1], [1.0]), "outside"), (([1.5], [1.0]), "must be integers"),
                     ((["a"], [1.0]), "must be integers"), (5, r"\{index: weight\} or \(indices, values\)")):
        with pytest.raises(ValueError, match=msg):
            M._sparse_pair(bad)
    assert [M._sparse_dim_for(i) for i in (0, 1, 3, 4, 1023, 1024, 2**31 - 2)] == [1, 2, 4, 8, 1024, 2048, 2**31 - 1]
    vectors = {"b": M._sparse_pair({5: 1.0, 1: 2.0}), "d": M._sparse_pair({0: 3.0})}
    indptr, indices, values = M._sparse_csr(["a", "b", "c", "d"], vectors)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
    assert indptr.tolist() == [0, 0, 2, 2, 3] and indices.tolist() == [1, 5, 0] and values.tolist() == [2.0, 1.0, 3.0]
    indptr, indices, values = M._sparse_csr(["a"], {})
    assert indptr.tolist() == [0, 0] and len(indices) == len(values) == 0


def make_db(tmp_path, n=20, name="db.pkl"):
    from minivectordb_amd import VectorDatabase
    db = VectorDatabase(storage_file=str(tmp_path / name))
    rows = np.random.default_rng(1).standard_normal((n, D)).astype(np.float32)
    db.store_embeddings_batch(list(range(n)), rows, [{"rank": i} for i in range(n)])
    return db, rows


def test_set_get_replace_remove_and_the_dimension(tmp_path):
    db, rows = make_db(tmp_path)
    assert db.sparse_dim is None and db.get_sparse_vector(3) is None
    db.set_sparse_vector(3, {9: 0.5, 2: -1.0})
    assert db.sparse_dim == 16                                       # the smallest power of two above 9
    got = db.get_sparse_vector(3)
    assert got[0].tolist() == [2, 9] and got[1].tolist() == [-1.0, 0.5]
    db.set_sparse_vector(3, ([1], [4.0]))                            # replaces
    assert db.get_sparse_vector(3)[0].tolist() == [1] and db.sparse_dim == 16
    db.set_sparse_vectors_batch([4, 5], [{16: 1.0}, ([70, 3], [1.0, 2.0])])
    assert db.sparse_dim == 128 and db.get_sparse_vector(5)[0].tolist() == [3, 70]
    db.set_sparse_vector(4, None)
    db.set_sparse_vector(5, {})
    assert db.get_sparse_vector(4) is None and db.get_sparse_vector(5) is None and db.sparse_dim == 128
    with pytest.raises(ValueError, match="does not exist"):
        db.set_sparse_vector("nobody", {1: 1.0})
    with pytest.raises(ValueError, match="does not exist"):
        db.get_sparse_vector("nobody")
    with pytest.raises(ValueError, match="listed twice"):
        db.set_sparse_vectors_batch([6, 7], [{1: 1.0}, ([2, 2], [1.0, 1.0])])
    assert db.get_sparse_vector(6) is None                            # nothing of a refused batch is stored
    with pytest.raises(ValueError, match="for all unique IDs"):
        db.set_sparse_vectors_batch([6, 7], [{1: 1.0}])
    # a fixed dimension refuses what it does not cover, and must cover what is stored
    with pytest.raises(ValueError, match="does not cover the stored index 1"):
        db.set_sparse_dim(1)
    db.set_sparse_dim(1000)
    assert db.sparse_dim == 1000
    db.set_sparse_vector(6, {999: 1.0})
    with pytest.raises(ValueError, match=r"index 1000 is outside \[0, 1000\)"):
        db.set_sparse_vector(7, {1000: 1.0})
    # a deleted id loses its vector: a store of the same id starts without one
    db.delete_embedding(3)
    db.store_embedding(3, rows[3], {"rank": 3})
    assert db.get_sparse_vector(3) is None and db.get_sparse_vector(6)[0].tolist() == [999]
    indptr, indices, values = db._sparse_csr(db._ids.uids, db._sparse_vectors())
    assert len(indptr) == 21 and indices.tolist() == [999] and indptr[db._ids.row(6) + 1] - indptr[db._ids.row(6)] == 1


def test_the_sidecar_round_trips_and_the_main_file_keeps_its_bytes(tmp_path):
    from minivectordb_amd import VectorDatabase
    plain, _ = make_db(tmp_path, name="plain.pkl")
    plain.persist_to_disk()
    assert not os.path.exists(plain.storage_file + ".sparse")
    db, _ = make_db(tmp_path, name="sparse.pkl")
    db.set_sparse_vectors_batch([2, 11], [{5: 1.5, 300: -2.0}, ([7], [0.25])])
    db.persist_to_disk()
    assert os.path.exists(db.storage_file + ".sparse")
    assert open(db.storage_file, "rb").read() == open(plain.storage_file, "rb").read()
    # (loading a stored database builds the device index: tests/test_sparse_db_gpu.py reloads through the constructor; here the
    # reader alone, on a database that holds the same ids but for one)
    again, _ = make_db(tmp_path, n=11, name="again.pkl")
    assert isinstance(again, VectorDatabase)
    again._sparse_load(db.storage_file + ".sparse")
    assert again.get_sparse_vector(2)[0].tolist() == [5, 300] and again.sparse_dim == 512
    with pytest.raises(ValueError, match="does not exist"):
        again.get_sparse_vector(11)
    assert 11 not in again._sparse_vectors()                          # an entry of an id that is not stored is dropped
    again, _ = make_db(tmp_path, name="again2.pkl")
    again._sparse_load(db.storage_file + ".sparse")
    assert again.sparse_dim == 512 and again.get_sparse_vector(2)[0].tolist() == [5, 300] and again.get_sparse_vector(11)[1].tolist() == [0.25]
    assert again.get_sparse_vector(3) is None


def test_a_leftover_sidecar_is_removed(tmp_path):
    db, _ = make_db(tmp_path)
    db.set_sparse_vector(2, {5: 1.5})
    db.persist_to_disk()
    assert os.path.exists(db.storage_file + ".sparse")
    db.set_sparse_vector(2, None)
    db.persist_to_disk()
    assert not os.path.exists(db.storage_file + ".sparse")


def test_classes_without_sparse_vectors_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        obj = obj if obj is not None else object.__new__(cls)
        for name, args in (("set_sparse_dim", (16,)), ("set_sparse_vector", (1, {1: 1.0})), ("set_sparse_vectors_batch", ([1], [{1: 1.0}])),
                           ("get_sparse_vector", (1,)), ("find_most_similar_sparse", ({1: 1.0},)),
                           ("find_most_similar_sparse_batch", ([{1: 1.0}],)),
                           ("find_most_similar_hybrid", (np.zeros(D, np.float32), {1: 1.0})),
                           ("find_most_similar_hybrid_batch", (np.zeros((1, D), np.float32), [{1: 1.0}]))):
            with pytest.raises(NotImplementedError, match="sparse vectors"):
                getattr(cls, name)(obj, *args)
