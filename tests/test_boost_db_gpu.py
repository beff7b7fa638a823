"""find_most_similar_boosted on the device, both database classes: about 600 rows at d = 64 whose metadata holds integer and
float keys, rows without a key and rows with values that are no numbers (tests/test_boost_cpu.py: metadata).  Results are held
to a float64 brute force under the project's 1e-4 parity rule, with inputs whose float64 ranking has no near-tie at the cut;
the column cache is driven through real writes."""
import numpy as np
import pytest

from test_boost_cpu import brute, column, metadata, separated
from test_examples_cpu import agrees

pytestmark = pytest.mark.gpu

N, D = 601, 64


def make_rows(n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "plain":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=256)
    db.store_embeddings_batch(list(range(n)), make_rows(n), metadata(n))
    return db


FILTERS = [{}, {"metadata_filter": {"bucket": 2}}, {"exclude_filter": {"bucket": 3}}, {"or_filters": [{"bucket": 4}, {"bucket": 5}]},
           {"metadata_filter": {"rare": "yes"}}, {"metadata_filter": {"bucket": 99}}]


def allowed_ids(db, f):
    return set(db.find_most_similar(make_rows(1, 9)[0], k=N + 10, **f)[0])


def column_object(db, key, missing=0.0):
    return db.__dict__["_boost_columns"][(key, float(missing))][2]


BOOSTS = {"age": 0.013, "rating": -0.21}


def float64_cases(db):
    """(filter, query, k, score_weight, missing, {id: S in float64}) of the parity test; tests/test_boost_cpu.py checks on the
    CPU that none of them has a near-tie around position k."""
    queries = make_rows(3, 31)   # (seeds 11 and 21 put a pair within 2e-4 at position 64 or 7: tests/test_boost_cpu.py checks)
    for f in FILTERS:
        allowed = allowed_ids(db, f)
        for j, q in enumerate(queries):
            for k, w_s, missing in ((7, 0.8, 0.5), (64, 1.0, 0.0)):
                if k == 64 and (j or f not in FILTERS[:3]):
                    continue
                yield f, q, k, w_s, missing, brute(db, q, BOOSTS, None, w_s, missing, allowed)


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_boosts_against_float64_under_filters(gpu, tmp_path, kind):
    db = make_db(kind, tmp_path)
    n = 0
    for f, q, k, w_s, missing, want in float64_cases(db):
        got = db.find_most_similar_boosted(q, BOOSTS, k=k, score_weight=w_s, missing=missing, **f)
        if not want:
            assert got == ([], [], [])
            continue
        separated(want, k)
        agrees(got, want, k, (kind, f, k))
        n += 1
    assert n == 18
    # the resident columns hold what the metadata says
    meta = metadata(N)
    T = db.index.boost_combine([column_object(db, "age", 0.5), column_object(db, "rating", 0.5)], [1.0, 0.0])
    assert np.array_equal(T, column(meta, "age", 0.5))
    T = db.index.boost_combine([column_object(db, "rating", 0.0)], [1.0])
    assert np.array_equal(T, column(meta, "rating", 0.0))


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_id_boosts_as_a_hybrid_and_the_batch(gpu, tmp_path, kind):
    db = make_db(kind, tmp_path)
    q = make_rows(1, 12)[0]
    k = 10
    plain = db.find_most_similar(q, k=N)
    rng = np.random.default_rng(5)
    # a lexical engine's hits: 18 of them with middling scores, two strong ones the dense ranking has at 150 and 200
    outsiders = [plain[0][150], plain[0][200]]
    hits = [u for u in rng.permutation(N).tolist() if u not in outsiders][:18]
    lexical = {u: float(s) for u, s in zip(hits, rng.uniform(0.2, 0.6, 18))}
    lexical.update({u: 1.0 for u in outsiders})
    alpha = 0.7
    id_boosts = {u: (1 - alpha) * s for u, s in lexical.items()}
    id_boosts["not stored"] = 9.0
    got = db.find_most_similar_boosted(q, id_boosts=id_boosts, k=k, score_weight=alpha)
    want = brute(db, q, None, id_boosts, alpha, 0.0, set(range(N)))
    separated(want, k)
    agrees(got, want, k, (kind, "hybrid"))
    assert set(outsiders) <= set(got[0]) and not set(outsiders) & set(plain[0][:100])
    # together with a metadata boost, under a filter that excludes one of the two
    f = {"exclude_filter": {"bucket": db.metadata[db._ids.row(outsiders[0])]["bucket"]}}
    allowed = allowed_ids(db, f)
    got = db.find_most_similar_boosted(q, {"age": 0.01}, id_boosts, k=k, score_weight=alpha, **f)
    want = brute(db, q, {"age": 0.01}, id_boosts, alpha, 0.0, allowed)
    separated(want, k)
    agrees(got, want, k, (kind, "hybrid, filtered"))
    assert outsiders[0] not in got[0] and set(got[0]) <= allowed
    # the batch equals the singles
    queries = make_rows(5, 13)
    boosts = {"rating": 0.3, "age": -0.02}
    for f in FILTERS:
        batch = db.find_most_similar_boosted_batch(queries, boosts, k=8, score_weight=0.9, missing=0.25, **f)
        assert len(batch) == 5
        for i in range(5):
            single = db.find_most_similar_boosted(queries[i], boosts, k=8, score_weight=0.9, missing=0.25, **f)
            assert batch[i] == single, (kind, f, i)


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_the_columns_follow_real_writes(gpu, tmp_path, kind):
    db = make_db(kind, tmp_path)
    q = make_rows(1, 14)[0]
    first = db.find_most_similar_boosted(q, {"age": 0.02})
    col = column_object(db, "age")
    assert len(col) == N
    assert db.find_most_similar_boosted(q, {"age": 0.02}) == first and column_object(db, "age") is col
    # an embedding-only update keeps the column; the search follows the new row
    db.update_embedding(300, embedding=q)
    got = db.find_most_similar_boosted(q, {"age": 0.0}, k=1)
    assert got[0][0] == 300 and abs(float(got[1][0]) - 1.0) < 1e-5 and column_object(db, "age") is col
    # a metadata update rebuilds it on next use
    db.update_embedding(17, metadata_dict={"bucket": 3, "rank": 17, "age": 500})
    got = db.find_most_similar_boosted(q, {"age": 0.02}, k=2)
    assert got[0][0] == 17 and column_object(db, "age") is not col
    agrees(got, brute(db, q, {"age": 0.02}, None, 1.0, 0.0, set(range(N))), 2, (kind, "metadata update"))
    # a store and a delete too
    col = column_object(db, "age")
    db.store_embedding(10_000, make_rows(1, 15)[0], {"bucket": 1, "rank": 10_000, "age": 2000})
    got = db.find_most_similar_boosted(q, {"age": 0.02}, k=2)
    assert list(got[0]) == [10_000, 17] and len(column_object(db, "age")) == N + 1 and column_object(db, "age") is not col
    if kind == "plain":
        db.delete_embedding(5)
    else:
        db.delete_embeddings_batch([5])
    got = db.find_most_similar_boosted(q, {"age": 0.02}, id_boosts={5: 99.0}, k=3)
    assert list(got[0][:2]) == [10_000, 17] and 5 not in got[0] and len(column_object(db, "age")) == N
    want = brute(db, q, {"age": 0.02}, None, 1.0, 0.0, (set(range(N)) - {5}) | {10_000})
    agrees(got, want, 3, (kind, "after the delete"))
    with pytest.raises(ValueError, match="exceeds 64"):
        db.find_most_similar_boosted(q, {"age": 0.02}, k=65)
