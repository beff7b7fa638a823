"""assign_to_nearest / cluster_embeddings on the CPU oracle stand-in: the host half (the vectors' shape, filters, id mapping,
pending stores, deletes, the seeded initial centres, argument errors, the classes that refuse) — and the checks of
tests/kmeans_oracle.py, the contract the GPU tests hold the device to."""
import numpy as np
import pytest

from kmeans_oracle import CHUNK, KmeansOracleIndex, assign, kmeans, update, vectors_per_pass
from maxsim_oracle import MISSING
from oracle import flat
from test_distinct_cpu import make_db
from test_grouped_cpu import FILTERS

N, D = 300, 16
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", KmeansOracleIndex)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---- the oracle -------------------------------------------------------------------------------------------------------------

def test_oracle_assign_ties_nan_and_signed_zero():
    S = np.array([[.5, .2, NAN, NAN, -0.0, -INF, .3],
                  [.5, .9, NAN, .1, 0.0, -INF, NAN],
                  [.1, .9, NAN, INF, -0.0, NAN, .3]], np.float32)
    labels, scores = assign(S)
    assert labels.dtype == np.int32 and scores.dtype == np.float32
    #        tie -> 0, tie -> 1, all NaN, +inf wins, +0.0 above -0.0, -inf is a candidate (lower j), NaN skipped: tie 0 / 2 -> 0
    assert labels.tolist() == [0, 1, -1, 2, 1, 0, 0]
    assert np.array_equal(bits(scores), bits([.5, .9, MISSING, INF, 0.0, -INF, .3]))
    # one vector: every row that scores is labelled 0
    labels, scores = assign(S[1:2])
    assert labels.tolist() == [0, 0, -1, 0, 0, 0, -1] and scores[2] == MISSING and scores[6] == MISSING
    # no row at all
    labels, scores = assign(np.zeros((3, 0), np.float32))
    assert labels.shape == (0,) and scores.shape == (0,)
    # a vector that is NaN everywhere never wins, wherever it stands
    S2 = np.array([[NAN, NAN], [-1.0, -2.0]], np.float32)
    assert assign(S2)[0].tolist() == [1, 1] and assign(S2[::-1])[0].tolist() == [0, 0]


def naive_update(rows, members):
    """The order rule with Python floats (IEEE doubles), element by element."""
    d = rows.shape[1]
    partials = []
    for i in range(0, len(members), CHUNK):
        acc = [float(v) for v in rows[members[i]]]
        for r in members[i + 1:i + CHUNK]:
            acc = [a + float(v) for a, v in zip(acc, rows[r])]
        partials.append(acc)
    tot = partials[0]
    for p in partials[1:]:
        tot = [a + b for a, b in zip(tot, p)]
    mean = [t / float(len(members)) for t in tot]
    ss = mean[0] * mean[0]
    for e in range(1, d):
        ss = ss + mean[e] * mean[e]
    norm = np.sqrt(np.float64(ss))
    return np.array([np.float32(np.float64(m) / norm) for m in mean], np.float32)


def test_oracle_update_is_the_chunked_sequential_sum():
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((700, 3)) * 10.0 ** rng.integers(-3, 4, (700, 1))).astype(np.float32)
    labels = np.full(700, 1, np.int32)
    labels[[5, 77, 300]] = 0                      # cluster 0: three members; cluster 1: 697 = 256 + 256 + 185; cluster 2: none
    labels[[6, 8]] = -1                           # rows of no cluster
    centres = flat.synth(4, 3, 1)
    labels[9] = 3
    rows[9] = 0                                   # cluster 3: a zero mean
    got = update(rows, labels, centres)
    assert np.array_equal(bits(got[0]), bits(naive_update(rows, [5, 77, 300])))
    assert np.array_equal(bits(got[1]), bits(naive_update(rows, np.flatnonzero(labels == 1).tolist())))
    assert np.array_equal(bits(got[2]), bits(centres[2])) and np.array_equal(bits(got[3]), bits(centres[3]))   # kept
    assert got.dtype == np.float32 and abs(np.linalg.norm(got[1].astype(np.float64)) - 1) < 1e-6
    # a mean that is not finite keeps its centre too; a sum that starts at -0.0 keeps the sign
    rows[5, 0] = INF
    assert np.array_equal(bits(update(rows, labels, centres)[0]), bits(centres[0]))
    z = np.array([[-0.0, 1.0], [-0.0, 1.0]], np.float32)
    assert bits(update(z, np.zeros(2, np.int32), centres[:1, :2]))[0].tolist() == [0x80000000, 0x3F800000]


def planted(n_clusters, per, d, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    true = unit(rng.standard_normal((n_clusters, d)))
    owner = np.repeat(np.arange(n_clusters), per)
    rng.shuffle(owner)
    x = unit(true[owner] + noise * rng.standard_normal((len(owner), d))).astype(np.float32)
    return x, owner


def test_oracle_loop_recovers_planted_clusters_like_a_float64_lloyd():
    x, owner = planted(5, 60, D, 11)
    first = np.array([np.flatnonzero(owner == c)[0] for c in range(5)])
    init = x[first[::-1]].copy()                                   # one row of every cluster, in another order
    centres, labels, scores, counts, its = kmeans(lambda c: (c @ x.T).astype(np.float32), x, init, 25)
    # float64 brute force
    c64 = init.astype(np.float64)
    for _ in range(25):
        l64 = np.argmax(c64 @ x.astype(np.float64).T, axis=0)
        c64 = unit(np.stack([x[l64 == c].astype(np.float64).mean(axis=0) for c in range(5)]))
    l64 = np.argmax(c64 @ x.astype(np.float64).T, axis=0)
    assert np.array_equal(labels, l64)
    perm = owner[first[::-1]]                                      # cluster j grew from a row of planted cluster perm[j]
    assert np.array_equal(perm[labels], owner)                     # the partition, up to that permutation
    assert counts.tolist() == [60] * 5 and counts.dtype == np.int64
    assert 1 <= its < 25 and np.abs(centres - c64).max() < 1e-6
    again = assign((centres @ x.T).astype(np.float32))
    assert np.array_equal(again[0], labels) and np.array_equal(bits(again[1]), bits(scores))
    # max_iter = 1: one update, then the labels of the updated centres
    c1, l1, s1, n1, it1 = kmeans(lambda c: (c @ x.T).astype(np.float32), x, init, 1)
    assert it1 == 1 and np.array_equal(l1, assign((c1 @ x.T).astype(np.float32))[0])


def test_vectors_per_pass_rule():
    assert vectors_per_pass(1, 512) == 1 and vectors_per_pass(7, 512) == 7
    assert vectors_per_pass(33, 512) == 32 and vectors_per_pass(4096, 32) == 32
    assert vectors_per_pass(70, 1024) == 32 and vectors_per_pass(70, 2048) == 16 and vectors_per_pass(70, 4096) == 8
    assert vectors_per_pass(7, 512, knob=5) == 5 and vectors_per_pass(7, 512, knob=1) == 1 and vectors_per_pass(3, 512, knob=5) == 3


# ---- the Python layer -------------------------------------------------------------------------------------------------------

def selected_ids(db, f):
    return sorted(db.find_most_similar(flat.synth(1, D, 2)[0], k=10 ** 6, **(f or {}))[0])


def brute_assign(db, ids, vectors):
    x = unit(np.stack([db.get_vector(u) for u in ids]))
    s = x @ unit(vectors).T
    return np.argmax(s, axis=1), s.max(axis=1)


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_assign_to_nearest_filters_and_id_mapping(backend, tmp_path, kind):
    db = make_db(kind, tmp_path)
    vectors = flat.synth(5, D, 77)
    for f in FILTERS:
        ids, labels, scores = db.assign_to_nearest(vectors, **(f or {}))
        want = selected_ids(db, f)
        assert list(ids) == want, f                                        # the selected ids, in storage order
        assert labels.dtype == np.int32 and scores.dtype == np.float32 and labels.shape == scores.shape == (len(want),)
        if want:
            wl, ws = brute_assign(db, want, vectors)
            assert np.array_equal(labels, wl) and np.abs(scores - ws).max() < 1e-5, f
    calls = [c for c in db.index.calls if c[0] == "assign"]
    assert calls and all(c[1] == 5 for c in calls) and any(c[2] for c in calls) and not all(c[2] for c in calls)


def test_pending_stores_and_deletes_are_seen(backend, tmp_path):
    db = make_db("flat", tmp_path, n=60)
    vectors = flat.synth(3, D, 5)
    assert len(db.assign_to_nearest(vectors)[0]) == 60
    extra = flat.synth(4, D, 99)
    for i in range(4):
        db.store_embedding(1000 + i, extra[i], {"bucket": 50})
    ids, labels, scores = db.assign_to_nearest(vectors)                     # the pending rows are uploaded first
    assert list(ids) == list(range(60)) + [1000, 1001, 1002, 1003]
    assert np.array_equal(labels[60:], brute_assign(db, ids[60:], vectors)[0])
    only = db.assign_to_nearest(vectors, metadata_filter={"bucket": 50})
    assert list(only[0]) == [1000, 1001, 1002, 1003] and np.array_equal(only[1], labels[60:]) and np.array_equal(bits(only[2]), bits(scores[60:]))
    # delete, then cluster: the row is gone from the result and the labels still belong to their ids
    db.delete_embedding(3)
    db.delete_embedding(1001)
    ids, labels, scores, centroids = db.cluster_embeddings(3, seed=1)
    assert list(ids) == [i for i in range(60) if i != 3] + [1000, 1002, 1003]
    wl, ws = brute_assign(db, list(ids), centroids)
    assert np.array_equal(labels, wl) and np.abs(scores - ws).max() < 1e-5
    assert centroids.shape == (3, D) and centroids.dtype == np.float32


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_cluster_embeddings_seeded_init_restated(backend, tmp_path, kind):
    db = make_db(kind, tmp_path)
    for f in (None, {"metadata_filter": {"bucket": 2}}, {"exclude_filter": {"bucket": 3}}):
        kw = f or {}
        got = db.cluster_embeddings(4, max_iter=7, seed=5, **kw)
        ids = selected_ids(db, f)
        rows = np.array(ids, dtype=np.int64)                                 # (ids are the row numbers here: stored in order)
        picked = np.random.default_rng(5).choice(rows, 4, replace=False)
        init = db.index.x[picked]
        assert np.array_equal(bits(db.index.last_init), bits(init))          # those stored rows were the initial centres
        assert [c for c in db.index.calls if c[0] == "kmeans"][-1] == ("kmeans", 4, 7, f is not None)
        same = db.cluster_embeddings(4, max_iter=7, init=init, **kw)         # init= an array: the same run
        assert list(got[0]) == list(same[0]) == ids
        for a, b in zip(got[1:], same[1:]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # the result is an assignment to the returned centroids
        again = db.assign_to_nearest(got[3], **kw)
        assert list(again[0]) == ids and np.array_equal(again[1], got[1])
        assert set(got[1].tolist()) <= set(range(4)) and got[3].shape == (4, D)
        other = db.cluster_embeddings(4, max_iter=7, seed=6, **kw)
        assert not np.array_equal(bits(db.index.last_init), bits(init)) and list(other[0]) == ids


def test_argument_errors(backend, tmp_path):
    db = make_db("flat", tmp_path, n=50)
    v = flat.synth(3, D, 1)
    with pytest.raises(ValueError, match="2-D"):
        db.assign_to_nearest(v[0])
    with pytest.raises(ValueError, match="dimension"):
        db.assign_to_nearest(flat.synth(3, D + 1, 1))
    with pytest.raises(ValueError, match="1 to 4096"):
        db.assign_to_nearest(np.zeros((0, D), np.float32))
    with pytest.raises(ValueError, match="1 to 4096"):
        db.assign_to_nearest(np.zeros((4097, D), np.float32))
    with pytest.raises(ValueError, match="fewer rows selected \\(50\\) than n_clusters \\(51\\)"):
        db.cluster_embeddings(51)
    with pytest.raises(ValueError, match="fewer rows selected \\(8\\) than n_clusters \\(9\\)"):
        db.cluster_embeddings(9, metadata_filter={"bucket": 0})            # rows 0, 7, ..., 49
    with pytest.raises(ValueError, match="fewer rows selected \\(0\\)"):
        db.cluster_embeddings(2, metadata_filter={"bucket": 99})
    with pytest.raises(ValueError, match="n_clusters"):
        db.cluster_embeddings(0)
    with pytest.raises(ValueError, match="max_iter"):
        db.cluster_embeddings(2, max_iter=0)
    with pytest.raises(ValueError, match="init holds 3 centres"):
        db.cluster_embeddings(2, init=v)
    with pytest.raises(ValueError, match="dimension"):
        db.cluster_embeddings(3, init=flat.synth(3, D + 1, 1))
    assert len(db.cluster_embeddings(50)[0]) == 50 and len(db.cluster_embeddings(8, metadata_filter={"bucket": 0})[0]) == 8
    # nothing selected / nothing stored: an empty assignment
    ids, labels, scores = db.assign_to_nearest(v, metadata_filter={"bucket": 99})
    assert ids == [] and labels.shape == (0,) and labels.dtype == np.int32 and scores.dtype == np.float32
    from minivectordb_amd import VectorDatabase
    empty = VectorDatabase(storage_file=str(tmp_path / "empty.pkl"))
    assert empty.assign_to_nearest(v)[0] == []
    with pytest.raises(ValueError, match="fewer rows selected \\(0\\)"):
        empty.cluster_embeddings(2)
    # an index without the methods is told so
    from oracle_backend import OracleIndex
    db.index.__class__ = OracleIndex
    with pytest.raises(NotImplementedError, match="clustering"):
        db.assign_to_nearest(v)
    with pytest.raises(NotImplementedError, match="clustering"):
        db.cluster_embeddings(2)


def test_classes_without_clustering_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    v = flat.synth(3, D, 23)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("assign_to_nearest", (v,)), ("cluster_embeddings", (3,))):
            with pytest.raises(NotImplementedError, match="clustering"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_index_assign", "mvdb_index_assign_device", "mvdb_index_assign_counters", "mvdb_index_kmeans"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    for name in ("assign", "assign_device", "kmeans", "assign_counters"):
        assert callable(getattr(_native.FlatIndex, name))
