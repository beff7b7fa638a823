"""Search by examples through the database classes (find_most_similar_by_examples): exact comparisons against the native call
for the same rows (tests/test_examples_gpu.py holds that call to the contract) — examples by id and by vector, filters, the
average-vector strategy against find_most_similar, and stores, updates and deletes between two calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D_, CLUSTERS = 600, 100, 24


def make_rows(n, seed=78):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((CLUSTERS, D_)).astype(np.float32)
    return centres[np.arange(n) % CLUSTERS] + np.float32(0.35) * rng.standard_normal((n, D_)).astype(np.float32)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "plain":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=256)
    x = make_rows(n)
    db.store_embeddings_batch([f"id{i}" for i in range(n)], x, [{"bucket": i % 7, "half": int(i >= n // 2)} for i in range(n)])
    db.find_most_similar(x[0], k=1)                                                 # (the device index is built by the first search)
    return db, x


def same_results(got, want, what):
    assert list(got[0]) == list(want[0]), (what, got[0], want[0])
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), what
    assert list(got[2]) == list(want[2]), what


def native(db, pos, neg, skip_ids, k, **filters):
    """(ids, scores, metadatas) of the native call for the rows the filters select, the ids' rows skipped."""
    with db.lock:
        selected = db._get_filtered_indices(filters.get("metadata_filter"), filters.get("exclude_filter"), filters.get("or_filters")).materialize()
        skip = [db._ids.row(u) for u in skip_ids]
    n = db.index.ntotal
    assert n == len(db._ids.uids)
    if not len(selected):
        return [], [], []
    rs = None if len(selected) == n else db.index.rowset(np.asarray(selected, np.int64))
    D, I = db.index.search_examples(pos, neg, min(k, len(selected)), rowset=rs, skip_rows=skip, normalize=True)
    hit = I >= 0
    return [db._ids.uids[int(r)] for r in I[hit]], D[hit], [db.metadata[int(r)] for r in I[hit]]


FILTERS = [{}, {"metadata_filter": {"bucket": 3}}, {"exclude_filter": {"half": 1}}, {"or_filters": [{"bucket": 1}, {"bucket": 5}]},
           {"metadata_filter": {"bucket": 99}}]


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_results_equal_the_native_call_and_examples_by_id_are_absent(gpu, tmp_path, kind):
    db, x = make_db(kind, tmp_path)
    pos_ids, neg_ids = ["id3", "id40", "id77"], ["id5", "id130"]
    pos = np.stack([np.asarray(db.get_vector(u), np.float32) for u in pos_ids])
    neg = np.stack([np.asarray(db.get_vector(u), np.float32) for u in neg_ids])
    calls0 = db.index.examples_counters()[0]
    for f in FILTERS:
        for k in (5, 64):
            got = db.find_most_similar_by_examples(pos_ids, neg_ids, k=k, **f)
            same_results(got, native(db, pos, neg, pos_ids + neg_ids, k, **f), ("ids", f, k))
            assert not set(got[0]) & set(pos_ids + neg_ids)
            by_vec = db.find_most_similar_by_examples(positive_embeddings=pos, negative_embeddings=neg, k=k, **f)
            same_results(by_vec, native(db, pos, neg, [], k, **f), ("vectors", f, k))
            mixed = db.find_most_similar_by_examples(pos_ids[:2], None, pos[2:], neg, k=k, **f)
            same_results(mixed, native(db, pos, neg, pos_ids[:2], k, **f), ("mixed", f, k))
        if f != FILTERS[-1]:
            assert len(got[0]) == 64
            if "id3" in db.find_most_similar(pos[0], k=1, **f)[0]:                  # a selected positive given by vector is its own best match
                assert "id3" in by_vec[0]
    assert db.index.examples_counters()[0] > calls0                                 # the native route served them
    got = db.find_most_similar_by_examples(pos_ids, k=60)                           # 3 x 24 cluster mates: 60 of them cannot leave a topic out
    assert all(float(s) > 0.5 for s in got[1]) and len({int(u[2:]) % CLUSTERS for u in got[0]}) == 3   # every topic is answered
    assert isinstance(got[0], tuple) and type(got[1][0]) is np.float32
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        db.find_most_similar_by_examples(["id3", "nobody"])
    with pytest.raises(ValueError, match="exceeds 64"):
        db.find_most_similar_by_examples(["id3"], k=65)
    rare = {"metadata_filter": {"bucket": 3}, "exclude_filter": {"half": 1}}
    small = native(db, pos, neg, [], N, **rare)[0]
    assert 0 < len(small) <= 64 and "id3" in small
    got = db.find_most_similar_by_examples(pos_ids, neg_ids, k=200, **rare)        # k clamped; the examples eat into the selection
    assert sorted(got[0]) == sorted(set(small) - set(pos_ids + neg_ids)) and len(got[0]) < len(small)


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_average_vector_agrees_with_find_most_similar(gpu, tmp_path, kind):
    db, x = make_db(kind, tmp_path)
    pos_ids, neg_ids = ["id3", "id40", "id77"], ["id5", "id130"]
    pos = np.stack([np.asarray(db.get_vector(u), np.float32) for u in pos_ids])
    neg = np.stack([np.asarray(db.get_vector(u), np.float32) for u in neg_ids])
    for f in FILTERS[:4]:
        for ids, nids, q in ((pos_ids, [], pos.mean(axis=0, dtype=np.float32)),
                             (pos_ids, neg_ids, np.float32(2) * pos.mean(axis=0, dtype=np.float32) - neg.mean(axis=0, dtype=np.float32))):
            got = db.find_most_similar_by_examples(ids, nids, k=8, strategy="average_vector", **f)
            full = db.find_most_similar(q, k=8 + len(ids + nids), **f)
            want = [(u, s, m) for u, s, m in zip(*full) if u not in ids + nids][:8]
            same_results(got, tuple(zip(*want)), ("average", f, len(nids)))


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_a_store_an_update_and_a_delete_between_two_calls_are_followed(gpu, tmp_path, kind):
    db, x = make_db(kind, tmp_path)
    pos_ids, neg_ids = ["id3", "id40"], ["id5"]

    def check(what, **f):
        pos = np.stack([np.asarray(db.get_vector(u), np.float32) for u in pos_ids])
        neg = np.stack([np.asarray(db.get_vector(u), np.float32) for u in neg_ids])
        got = db.find_most_similar_by_examples(pos_ids, neg_ids, k=12, **f)
        same_results(got, native(db, pos, neg, pos_ids + neg_ids, 12, **f), what)
        return got

    f = {"metadata_filter": {"bucket": 3}}
    check("before")
    first = check("before, filtered", **f)
    twin = np.asarray(db.get_vector("id3"), np.float32)
    db.store_embedding("new", twin, {"bucket": 3, "half": 0})                       # a copy of a positive: the new best match
    assert check("stored")[0][0] == "new" and check("stored, filtered", **f)[0][0] == "new"
    db.update_embedding("new", embedding=np.asarray(db.get_vector("id5"), np.float32))   # now a copy of the negative: it sinks
    got = check("updated", **f)
    assert "new" not in got[0][:3] and list(got[0][:3]) == list(first[0][:3])
    victim = first[0][0]
    if kind == "plain":
        db.delete_embedding(victim)
        db.delete_embedding("id0")                                                  # rows renumber: the skip rows follow
    else:
        db.delete_embeddings_batch([victim, "id0"])
    got = check("deleted", **f)
    assert victim not in got[0] and got[0][0] == first[0][1]
    assert victim not in check("deleted, everything")[0]
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        db.find_most_similar_by_examples([victim])
