"""find_most_similar_sparse and find_most_similar_hybrid on the device, both database classes: 300 rows at d = 64, two thirds
of them with a sparse vector.  After every step the results are compared with tests/sparse_oracle.py over the surviving rows:
ids exactly, scores as bits.  The test keeps its own record of which id holds which sparse vector; the dense scores the hybrid
oracle takes are the index's own single-query bits (the full ranking, as tests/test_boost_gpu.py takes them)."""
import os

import numpy as np
import pytest

from boost_oracle import boosted
from sparse_oracle import scores, sparse_term, sparse_topk
from test_assign_gpu import bits

pytestmark = pytest.mark.gpu

N, D, VOCAB = 300, 64, 500
FILTERS = [{}, {"metadata_filter": {"bucket": 2}}, {"exclude_filter": {"bucket": 3}}, {"or_filters": [{"bucket": 4}, {"bucket": 5}]},
           {"metadata_filter": {"bucket": 99}}]


def make_rows(n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def make_sparse(rng, most=30):
    m = int(rng.integers(1, most))
    idx = np.unique(np.minimum((rng.zipf(1.3, m) - 1), VOCAB - 1))
    return {int(i): float(np.float32(v)) for i, v in zip(idx, rng.standard_normal(len(idx)))}


def make_db(kind, tmp_path, name="db"):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "plain":
        db = VectorDatabase(storage_file=str(tmp_path / f"{name}.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / f"{name}_shards"), shard_size=128)
    db.store_embeddings_batch(list(range(N)), make_rows(N), [{"bucket": i % 7, "rank": i} for i in range(N)])
    return db


def give_sparse(db, seed=5):
    """Sparse vectors for two ids in three; returns the test's own record {id: {index: weight}}."""
    rng = np.random.default_rng(seed)
    truth = {u: make_sparse(rng) for u in range(N) if u % 3}
    ids = sorted(truth)
    db.set_sparse_vectors_batch(ids[:-5], [truth[u] for u in ids[:-5]])
    for u in ids[-5:]:
        vec = truth[u]
        db.set_sparse_vector(u, (list(vec)[::-1], list(vec.values())[::-1]))       # the pair form, indices descending
    return truth


def csr_of(db, truth):
    indptr, indices, values = [0], [], []
    for u in db._ids.uids:
        vec = sorted(truth.get(u, {}).items())
        indices += [i for i, _ in vec]
        values += [v for _, v in vec]
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int64), np.array(values, np.float32)


def selected_rows(db, f):
    n = len(db._ids.uids)
    ids = db.find_most_similar(make_rows(1, 9)[0], k=n + 10, **f)[0]
    return np.array(sorted(db._ids.row(u) for u in ids), np.int64)


def held(got, D_, I_, db, what):
    ids, got_scores, metas = got
    keep = I_ >= 0
    uids = db._ids.uids
    assert list(ids) == [uids[r] for r in I_[keep]], (what, ids, I_)
    assert [type(s) for s in got_scores] == [np.float32] * int(keep.sum()), what
    assert bits(np.array(got_scores, np.float32)).tolist() == bits(D_[keep]).tolist(), (what, got_scores, D_)
    assert [m["rank"] for m in metas] == list(ids), what


def check(db, truth, what, ks=(10,)):
    """Sparse and hybrid search under every filter against the oracle; returns how many non-empty results were compared."""
    indptr, indices, values = csr_of(db, truth)
    n = len(db._ids.uids)
    query = {3: 1.2, 0: -0.4, 1: 0.8, 17: 2.0, 250: -1.0, 5000: 9.0}               # 5000: beyond sparse_dim, dropped
    q_idx, q_val = [i for i in query if i < VOCAB], [v for i, v in query.items() if i < VOCAB]
    T, matched = scores(indptr, indices, values, q_idx, q_val)
    dense = make_rows(1, 31)[0]
    db.find_most_similar(dense, k=1)                                               # (brings the device index up to date)
    Dn, In = db.index.search(dense[None], n, normalize_q=True)
    s = np.full(n, np.nan, np.float32)
    s[In[0]] = Dn[0]
    compared = 0
    for f in FILTERS:
        rows = selected_rows(db, f)
        for k in ks:
            take = min(k, len(rows))
            got = db.find_most_similar_sparse(query, k=k, **f)
            got_h = db.find_most_similar_hybrid(dense, query, k=k, dense_weight=0.3, sparse_weight=-0.7, **f)
            if not len(rows):
                assert got == ([], [], []) and got_h == ([], [], [])
                continue
            held(got, *sparse_topk(T, matched, rows, take), db, (what, f, k, "sparse"))
            s_sel = np.full(n, np.nan, np.float32)
            s_sel[rows] = s[rows]
            held(got_h, *boosted(s_sel, sparse_term(T, -0.7), 0.3, take), db, (what, f, k, "hybrid"))
            assert len(got_h[0]) == take
            compared += 1
    return compared


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_sparse_vectors_follow_real_writes(gpu, tmp_path, kind):
    db = make_db(kind, tmp_path)
    truth = give_sparse(db)
    assert db.sparse_dim == 512
    assert check(db, truth, "fresh", ks=(1, 10, 64)) == 12
    builds = db.__dict__["_sparse_builds"]
    assert builds == 1                                                              # one upload served every search above
    # replace, remove, add
    rng = np.random.default_rng(6)
    for u in (1, 2, 100, 200):
        truth[u] = make_sparse(rng)
        db.set_sparse_vector(u, truth[u])
    for u in (4, 5):
        del truth[u]
    db.set_sparse_vector(4, None)
    db.set_sparse_vector(5, {})
    truth[0] = {3: 50.0}
    db.set_sparse_vector(0, truth[0])
    assert check(db, truth, "replaced") == 4 and db.__dict__["_sparse_builds"] == builds + 1
    assert db.find_most_similar_sparse({3: 1.0}, k=1)[0] == (0,)
    # the batch equals the singles; an empty query has no sparse result and ranks a hybrid search by the dense score
    queries = [make_sparse(rng) for _ in range(4)] + [{9999: 1.0}, None]
    dense = make_rows(6, 33)
    for f in FILTERS[:3]:
        batch = db.find_most_similar_sparse_batch(queries, k=8, **f)
        batch_h = db.find_most_similar_hybrid_batch(dense, queries, k=8, dense_weight=0.75, sparse_weight=1.3, **f)
        for i in range(6):
            assert batch[i] == db.find_most_similar_sparse(queries[i], k=8, **f), (kind, f, i)
            assert batch_h[i] == db.find_most_similar_hybrid(dense[i], queries[i], k=8, dense_weight=0.75, sparse_weight=1.3, **f), (kind, f, i)
        assert batch[4] == batch[5] == ([], [], [])
        for i in (4, 5):
            plain = db.find_most_similar(dense[i], k=8, **f)
            assert batch_h[i][0] == plain[0]
            assert np.allclose(batch_h[i][1], np.float32(0.75) * np.array(plain[1], np.float32), rtol=0, atol=1e-6)
    # autocut: the packaging of find_most_similar
    plain = db.find_most_similar_sparse({3: 1.2, 1: 0.8, 17: 2.0}, k=20)
    assert db.find_most_similar_sparse({3: 1.2, 1: 0.8, 17: 2.0}, k=20, autocut=True) == db._package(list(zip(*plain)), True)
    plain = db.find_most_similar_hybrid(dense[0], {3: 1.2}, k=20)
    assert db.find_most_similar_hybrid(dense[0], {3: 1.2}, k=20, autocut=True) == db._package(list(zip(*plain)), True)
    # delete, then store the same id again: it has no sparse vector
    doomed = [0, 7, 100]
    if kind == "plain":
        for u in doomed:
            db.delete_embedding(u)
    else:
        db.delete_embeddings_batch(doomed)
    for u in doomed:
        truth.pop(u, None)
    assert check(db, truth, "deleted") == 4
    db.store_embedding(100, make_rows(1, 40)[0], {"bucket": 2, "rank": 100})
    assert db.get_sparse_vector(100) is None
    assert check(db, truth, "stored again") == 4
    assert 100 not in db.find_most_similar_sparse({i: 1.0 for i in range(40)}, k=64)[0]
    # an embedding-only update keeps the store; the hybrid search follows the new row
    builds = db.__dict__["_sparse_builds"]
    target = make_rows(1, 41)[0]
    db.update_embedding(150, embedding=target)
    got = db.find_most_similar_hybrid(target, {3: 1.0}, k=1, sparse_weight=0.0)
    assert got[0][0] == 150 and abs(float(got[1][0]) - 1.0) < 1e-5
    assert check(db, truth, "embedding updated") == 4 and db.__dict__["_sparse_builds"] == builds
    # a metadata update moves the row between filters
    db.update_embedding(151, metadata_dict={"bucket": 2, "rank": 151})
    assert check(db, truth, "metadata updated") == 4
    assert 151 in db.find_most_similar_sparse(truth[151], k=64, metadata_filter={"bucket": 2})[0]
    for call in (lambda: db.find_most_similar_sparse({1: 1.0}, k=65), lambda: db.find_most_similar_hybrid(target, {1: 1.0}, k=65)):
        with pytest.raises(ValueError, match="exceeds 64"):
            call()


def test_the_sidecar_round_trips_and_the_main_file_keeps_its_bytes(gpu, tmp_path):
    from minivectordb_amd import VectorDatabase
    bare = make_db("plain", tmp_path, "bare")
    bare.find_most_similar(make_rows(1, 9)[0])
    bare.persist_to_disk()
    assert not os.path.exists(bare.storage_file + ".sparse")
    db = make_db("plain", tmp_path, "sparse")
    truth = give_sparse(db)
    query = {3: 1.2, 0: -0.4, 1: 0.8, 17: 2.0}
    dense = make_rows(1, 31)[0]
    want = (db.find_most_similar_sparse(query, k=10), db.find_most_similar_hybrid(dense, query, k=10, sparse_weight=0.4))
    db.persist_to_disk()
    assert open(db.storage_file, "rb").read() == open(bare.storage_file, "rb").read()
    again = VectorDatabase(storage_file=db.storage_file)
    assert again.sparse_dim == db.sparse_dim == 512
    for u in (0, 1, 2, 299):
        a, b = again.get_sparse_vector(u), db.get_sparse_vector(u)
        assert (a is None and b is None and u not in truth) or (np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])))
    got = (again.find_most_similar_sparse(query, k=10), again.find_most_similar_hybrid(dense, query, k=10, sparse_weight=0.4))
    assert got == want
    assert check(again, truth, "reloaded") == 4
    # no sparse vector left: the leftover file goes
    again.set_sparse_vectors_batch(sorted(truth), [None] * len(truth))
    again.persist_to_disk()
    assert not os.path.exists(again.storage_file + ".sparse")
    assert VectorDatabase(storage_file=db.storage_file).get_sparse_vector(1) is None


def test_classes_without_sparse_vectors_refuse(gpu, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    db.store_embeddings_batch(list(range(20)), make_rows(20), [{"rank": i} for i in range(20)])
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, object.__new__(DistributedShardedVectorDatabase))):
        with pytest.raises(NotImplementedError, match="sparse vectors"):
            cls.set_sparse_vector(obj, 1, {1: 1.0})
        with pytest.raises(NotImplementedError, match="sparse vectors"):
            cls.find_most_similar_sparse(obj, {1: 1.0})
        with pytest.raises(NotImplementedError, match="sparse vectors"):
            cls.find_most_similar_hybrid(obj, np.zeros(D, np.float32), {1: 1.0})
