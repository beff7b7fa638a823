"""build_sparse_postings on the database classes: B + 100 rows (B = block_rows of mvdb_sparse_postings_geometry, so the rows
span two workgroups' blocks) at d = 32, two thirds of them with a sparse vector.  A twin database holds the same rows and
sparse vectors and never builds postings.  After every write the sparse and the hybrid search and their batch forms, under
every filter, return the same ids, scores (as float32 values) and metadata on both; the index's posting counters show that
the first database really answered through the posting lists and the twin never did."""
import os

import numpy as np
import pytest

from test_sparse_db_gpu import FILTERS, make_sparse

pytestmark = pytest.mark.gpu

D = 32


def n_rows():
    from minivectordb_amd import _native
    return _native.sparse_postings_geometry()[0] + 100


def make_rows(n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def make_db(kind, tmp_path, name):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    n = n_rows()
    if kind == "plain":
        db = VectorDatabase(storage_file=str(tmp_path / f"{name}.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / f"{name}_shards"), shard_size=1024)
    db.store_embeddings_batch(list(range(n)), make_rows(n), [{"bucket": i % 7, "rank": i} for i in range(n)])
    rng = np.random.default_rng(5)
    ids = [u for u in range(n) if u % 3]
    db.set_sparse_vectors_batch(ids, [make_sparse(rng) for _ in ids])
    return db


def both(db, twin, call):
    call(db)
    call(twin)


def same_answers(db, twin, what):
    """Every search form under every filter on both databases; returns how many non-empty sparse results were compared."""
    rng = np.random.default_rng(77)
    queries = [{3: 1.2, 0: -0.4, 1: 0.8, 17: 2.0, 250: -1.0, 5000: 9.0}] + [make_sparse(rng) for _ in range(3)] + [{9999: 1.0}, None]
    dense = make_rows(len(queries), 31)
    compared = 0
    for f in FILTERS:
        for k in (1, 10):
            got = db.find_most_similar_sparse(queries[0], k=k, **f)
            assert got == twin.find_most_similar_sparse(queries[0], k=k, **f), (what, f, k, "sparse")
            compared += bool(len(got[0]))
            args = dict(k=k, dense_weight=0.3, sparse_weight=-0.7, **f)
            assert db.find_most_similar_hybrid(dense[0], queries[0], **args) == twin.find_most_similar_hybrid(dense[0], queries[0], **args), (what, f, k)
        batch = db.find_most_similar_sparse_batch(queries, k=8, **f)
        assert batch == twin.find_most_similar_sparse_batch(queries, k=8, **f), (what, f, "sparse batch")
        args = dict(k=8, dense_weight=0.75, sparse_weight=1.3, **f)
        assert db.find_most_similar_hybrid_batch(dense, queries, **args) == twin.find_most_similar_hybrid_batch(dense, queries, **args), (what, f)
        assert batch[4] == batch[5] == ([], [], [])
    return compared


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_postings_follow_real_writes_and_change_no_result(gpu, tmp_path, kind):
    n = n_rows()
    db, twin = make_db(kind, tmp_path, "db"), make_db(kind, tmp_path, "twin")
    assert db.sparse_postings_info() == {'enabled': False, 'built': False, 'nnz': 0, 'dim': 512, 'bytes': 0}
    db.build_sparse_postings()                                                       # sparse vectors exist: the first store at once
    info = db.sparse_postings_info()
    assert info['enabled'] and info['built'] and info['dim'] == 512 and info['nnz'] > n and info['bytes'] == 8 * info['nnz'] + 8 * 513
    builds = db.__dict__["_sparse_builds"]
    assert same_answers(db, twin, "fresh") >= 8
    assert db.__dict__["_sparse_builds"] == builds                                   # that store served every search above
    served = db.index.sparse_postings_counters()
    assert served[0] > 0 and served[1] > 0 and served[2] > 0 and twin.index.sparse_postings_counters() == (0, 0, 0)
    assert db.index.sparse_counters()[1] == 0 and twin.index.sparse_counters()[1] > 0        # no CSR launch here, only CSR launches there
    assert not twin.sparse_postings_info()['enabled'] and not twin.sparse_postings_info()['built']
    # set_sparse_vector: replace and remove
    rng = np.random.default_rng(6)
    for u in (1, 2, 100, n - 2):
        vec = make_sparse(rng)
        both(db, twin, lambda d: d.set_sparse_vector(u, vec))
    both(db, twin, lambda d: d.set_sparse_vector(4, None))
    both(db, twin, lambda d: d.set_sparse_vector(5, {}))
    both(db, twin, lambda d: d.set_sparse_vector(0, {3: 50.0}))
    assert not db.sparse_postings_info()['built'] and db.sparse_postings_info()['enabled']      # outdated until the next search
    assert same_answers(db, twin, "replaced") >= 8
    assert db.sparse_postings_info()['built'] and db.__dict__["_sparse_builds"] == builds + 1  # rebuilt once
    assert db.find_most_similar_sparse({3: 1.0}, k=1)[0] == (0,)
    # delete, store, update
    doomed = [0, 7, 100, n - 1]
    if kind == "plain":
        for u in doomed:
            both(db, twin, lambda d: d.delete_embedding(u))
    else:
        both(db, twin, lambda d: d.delete_embeddings_batch(doomed))
    assert not db.sparse_postings_info()['built']
    assert same_answers(db, twin, "deleted") >= 8 and db.sparse_postings_info()['built']
    both(db, twin, lambda d: d.store_embedding(100, make_rows(1, 40)[0], {"bucket": 2, "rank": 100}))
    both(db, twin, lambda d: d.set_sparse_vector(100, {3: 0.25, 17: -1.0}))
    assert same_answers(db, twin, "stored again") >= 8
    target = make_rows(1, 41)[0]
    both(db, twin, lambda d: d.update_embedding(150, embedding=target))
    both(db, twin, lambda d: d.update_embedding(151, metadata_dict={"bucket": 2, "rank": 151}))
    assert same_answers(db, twin, "updated") >= 8 and db.sparse_postings_info()['built']
    assert db.find_most_similar_hybrid(target, {3: 1.0}, k=1, sparse_weight=0.0)[0][0] == 150
    assert twin.index.sparse_postings_counters() == (0, 0, 0) and db.index.sparse_postings_counters()[0] > served[0]
    # back to the CSR pass
    csr_launches = db.index.sparse_counters()[1]
    db.drop_sparse_postings()
    assert db.sparse_postings_info() == {'enabled': False, 'built': False, 'nnz': 0, 'dim': 512, 'bytes': 0}
    assert same_answers(db, twin, "dropped") >= 8
    assert db.index.sparse_counters()[1] > csr_launches and not db.sparse_postings_info()['built']


def test_postings_are_not_persisted(gpu, tmp_path):
    from minivectordb_amd import VectorDatabase
    plain = make_db("plain", tmp_path, "plain")
    plain.find_most_similar_sparse({3: 1.0}, k=3)
    plain.persist_to_disk()
    db = make_db("plain", tmp_path, "posted")
    db.build_sparse_postings()
    query = {3: 1.2, 0: -0.4, 1: 0.8, 17: 2.0}
    dense = make_rows(1, 31)[0]
    want = (db.find_most_similar_sparse(query, k=10), db.find_most_similar_hybrid(dense, query, k=10, sparse_weight=0.4))
    db.persist_to_disk()
    for suffix in ("", ".sparse"):
        assert open(db.storage_file + suffix, "rb").read() == open(plain.storage_file + suffix, "rb").read(), suffix
    assert not [name for name in os.listdir(tmp_path) if "post" in name and not name.startswith("posted.pkl")]      # no file of their own
    again = VectorDatabase(storage_file=db.storage_file)
    assert again.sparse_postings_info() == {'enabled': False, 'built': False, 'nnz': 0, 'dim': 512, 'bytes': 0}
    got = (again.find_most_similar_sparse(query, k=10), again.find_most_similar_hybrid(dense, query, k=10, sparse_weight=0.4))
    assert got == want and again.index.sparse_postings_counters() == (0, 0, 0)
    again.build_sparse_postings()
    assert again.sparse_postings_info()['built'] and again.find_most_similar_sparse(query, k=10) == want[0]
    assert again.index.sparse_postings_counters()[0] == 1


def test_a_dimension_above_the_cap_names_set_sparse_dim(gpu, tmp_path):
    from minivectordb_amd import VectorDatabase, _native
    cap = _native.sparse_postings_geometry()[2]
    db = VectorDatabase(storage_file=str(tmp_path / "wide.pkl"))
    db.store_embeddings_batch(list(range(10)), make_rows(10), [{"rank": i} for i in range(10)])
    db.set_sparse_vector(3, {cap + 5: 1.0, 2: 0.5})                                # sparse_dim grows to the next power of two: above the cap
    assert db.sparse_dim > cap
    with pytest.raises(ValueError, match="set_sparse_dim"):
        db.build_sparse_postings()
    assert not db.sparse_postings_info()['enabled']
    assert db.find_most_similar_sparse({2: 1.0}, k=3)[0] == (3,)                    # the CSR pass still answers
