"""Probed search through the database classes (build_partition, find_most_similar_approx): exact comparisons against a model
built from partition_centroids(), the partition's current labels and the library's existing routes, as in
tests/test_probe_gpu.py — and the upkeep after stores, updates and deletes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D_, CLUSTERS = 1500, 100, 24


def make_rows(n, seed=77):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((CLUSTERS, D_)).astype(np.float32)
    return centres[np.arange(n) % CLUSTERS] + np.float32(0.35) * rng.standard_normal((n, D_)).astype(np.float32)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "plain":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=512)
    x = make_rows(n)
    db.store_embeddings_batch([f"id{i}" for i in range(n)], x, [{"bucket": i % 7, "half": int(i >= n // 2)} for i in range(n)])
    return db, x


def queries(nq=6):
    return make_rows(nq, seed=5) + np.float32(0.05)


def same_results(got, want, what):
    assert list(got[0]) == list(want[0]), (what, got[0], want[0])
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), what
    assert list(got[2]) == list(want[2]), what


def model(db, q, k, nprobe, selected=None):
    """(ids, scores) from the centroids, the partition's labels as they stand and the exact routes, for ONE query."""
    from minivectordb_amd import _native
    state = db.__dict__["_partition"]
    part = state["part"]
    labels = part.labels()
    assert len(part) == db.index.ntotal == len(db._ids.uids)
    centroids = db.partition_centroids()
    assert np.array_equal(labels, db.index.assign(centroids, normalize_c=False)[0])   # every row in the list of its nearest centre
    cidx = _native.FlatIndex(D_)
    cidx.add(centroids, normalize=False)
    _, Ic = cidx.search(q[None, :], min(nprobe, centroids.shape[0]), normalize_q=True)
    cidx.close()
    rows = np.flatnonzero(np.isin(labels, Ic[0][Ic[0] >= 0])).astype(np.int64)
    if selected is not None:
        rows = np.intersect1d(rows, selected)
    if not len(rows):
        return [], []
    take = min(k, db.index.ntotal if selected is None else len(selected))              # the k clamp of find_most_similar
    Dm, Im = db.index.search_rowset(q[None, :], take, db.index.rowset(rows), normalize_q=True)
    hit = Im[0] >= 0
    return [db._ids.uids[int(r)] for r in Im[0][hit]], Dm[0][hit]


def check_against_model(db, k, nprobe, what, **filters):
    selected = None
    if filters:
        with db.lock:
            selected = db._get_filtered_indices(filters.get("metadata_filter"), filters.get("exclude_filter"), None).materialize()
    for q in queries():
        ids, dist, meta = db.find_most_similar_approx(q, k=k, nprobe=nprobe, **filters)
        want_ids, want_d = model(db, q, k, nprobe, selected)
        assert list(ids) == want_ids, (what, ids, want_ids)
        assert np.array_equal(np.asarray(dist, np.float32).view(np.uint32), np.asarray(want_d, np.float32).view(np.uint32)), what
        assert [m["bucket"] for m in meta] == [int(i[2:]) % 7 if not i.startswith("new") else -1 for i in ids]


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_build_and_probe_every_list_equals_the_exact_search(gpu, tmp_path, kind):
    db, x = make_db(kind, tmp_path)
    with pytest.raises(ValueError, match="build_partition"):
        db.find_most_similar_approx(x[0])
    with pytest.raises(ValueError, match="build_partition"):
        db.partition_centroids()
    sizes = db.build_partition()
    C = min(4096, max(1, round(np.sqrt(N))))
    assert sizes.shape == (C,) and sizes.dtype == np.int64 and sizes.sum() == N
    cent = db.partition_centroids()
    assert cent.shape == (C, D_) and np.allclose(np.linalg.norm(cent, axis=1), 1, atol=1e-5)
    for q in queries():
        for k in (1, 5, 64):
            same_results(db.find_most_similar_approx(q, k=k, nprobe=C), db.find_most_similar(q, k=k), ("all lists", k))
            same_results(db.find_most_similar_approx(q, k=k, nprobe=10 ** 6), db.find_most_similar(q, k=k), ("clipped", k))
        same_results(db.find_most_similar_approx(q, k=5, nprobe=C, autocut=True), db.find_most_similar(q, k=5, autocut=True), "autocut")
    check_against_model(db, 10, 3, "fresh")
    assert np.array_equal(db.build_partition(n_clusters=C), sizes)                      # bit-identical run to run
    assert np.array_equal(db.partition_centroids().view(np.uint32), cent.view(np.uint32))
    # centroids=: the same partition without k-means
    calls = db.index.assign_counters()[0]
    again = db.build_partition(centroids=cent)
    assert again.shape == (C,) and again.sum() == N and db.index.assign_counters()[0] == calls + 1
    assert np.allclose(db.partition_centroids(), cent, atol=1e-6)
    check_against_model(db, 10, 3, "from centroids")
    sizes7 = db.build_partition(n_clusters=7, max_iter=3, seed=4, train_rows=300)
    assert sizes7.shape == (7,) and sizes7.sum() == N
    check_against_model(db, 10, 2, "seven lists")
    with pytest.raises(ValueError, match="64"):
        db.find_most_similar_approx(x[0], k=65)
    with pytest.raises(ValueError):
        db.find_most_similar_approx(x[0], nprobe=0)
    with pytest.raises(ValueError):
        db.build_partition(n_clusters=0)
    with pytest.raises(ValueError):
        db.build_partition(n_clusters=N + 1)
    db.drop_partition()
    with pytest.raises(ValueError, match="build_partition"):
        db.find_most_similar_approx(x[0])


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_store_update_delete_sequence(gpu, tmp_path, kind):
    db, x = make_db(kind, tmp_path)
    db.build_partition(n_clusters=16, seed=1)
    check_against_model(db, 10, 3, "built")
    extra = make_rows(200, seed=9)
    db.store_embeddings_batch([f"new{i}" for i in range(200)], extra, [{"bucket": -1, "half": 2} for _ in range(200)])
    check_against_model(db, 10, 3, "stored")
    moved = [f"id{i}" for i in (4, 5, 700, 1499)] + ["new7"]
    db.update_embeddings_batch(moved, embeddings=-x[[40, 50, 60, 70, 80]])             # opposite directions: other lists
    check_against_model(db, 10, 3, "updated")
    db.update_embedding("id9", embedding=x[333])
    if kind == "plain":
        db.delete_embedding("id3")
        db.delete_embedding("new0")
    else:
        db.delete_embeddings_batch(["id3", "new0"])
    assign_calls = db.index.assign_counters()[0]
    check_against_model(db, 10, 3, "deleted")                                           # (the update of "id9" is carried across the delete)
    # re-created from the labels: one assign, of the row that changed, not of every row; no k-means
    state = db.__dict__["_partition"]
    assert len(state["part"]) == N + 200 - 2
    db.store_embedding("new_late", extra[3] * 2, {"bucket": -1, "half": 2})
    if kind == "plain":
        db.delete_embedding("id100")
    else:
        db.delete_embeddings_batch(["id100"])
    check_against_model(db, 64, 16, "stored then deleted before a search")
    for q in queries(3):
        same_results(db.find_most_similar_approx(q, k=10, nprobe=16), db.find_most_similar(q, k=10), "all lists after the sequence")
    assert db.index.assign_counters()[0] > assign_calls


def test_filters_and_the_batch_call(gpu, tmp_path):
    db, x = make_db("plain", tmp_path, n=4400)                                          # a sorted list becomes a bitmap from 4,096 rows on
    db.build_partition(n_clusters=20)
    qs = queries(5)
    calls0 = db.index.probe_counters()[0]
    # a list-form filter: the exact search under the filter
    for q in qs:
        same_results(db.find_most_similar_approx(q, k=10, nprobe=1, metadata_filter={"bucket": 3}),
                     db.find_most_similar(q, k=10, metadata_filter={"bucket": 3}), "list-form filter")
    assert db.index.probe_counters()[0] == calls0
    # bitmap-form filters: probed under the bitmap
    check_against_model(db, 10, 3, "excluded", exclude_filter={"bucket": 3})
    check_against_model(db, 10, 20, "excluded, all lists", exclude_filter={"bucket": 3})
    for q in qs:
        same_results(db.find_most_similar_approx(q, k=10, nprobe=20, exclude_filter={"bucket": 3}),
                     db.find_most_similar(q, k=10, exclude_filter={"bucket": 3}), "excluded equals exact")
    assert db.index.probe_counters()[0] > calls0
    assert db.find_most_similar_approx(qs[0], metadata_filter={"bucket": 99}) == ([], [], [])
    # the batch call equals a loop of single calls
    for kw in ({}, {"exclude_filter": {"bucket": 3}}, {"metadata_filter": {"bucket": 3}}):
        batch = db.find_most_similar_approx_batch(qs, k=7, nprobe=4, **kw)
        assert len(batch) == len(qs)
        for q, got in zip(qs, batch):
            same_results(got, db.find_most_similar_approx(q, k=7, nprobe=4, **kw), ("batch", kw))
    assert db.find_most_similar_approx_batch(np.empty((0, D_), np.float32)) == []


def test_the_int8_cosine_class_refuses(gpu, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=512)
    for call in (db.build_partition, db.drop_partition, db.partition_centroids):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        db.find_most_similar_approx(np.ones(D_, np.float32))
    with pytest.raises(NotImplementedError):
        db.find_most_similar_approx_batch(np.ones((2, D_), np.float32))
