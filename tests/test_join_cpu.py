"""find_duplicate_pairs / count_duplicate_pairs / find_duplicate_groups on the CPU oracle stand-in (join_oracle.py): the host
half — filter semantics, first_row, limit, the order of the pairs, the union-find, the resident row-set cache, the behaviour
after a delete and an update — against a brute-force float64 answer over the stored rows."""
import numpy as np
import pytest

from join_oracle import JoinOracleIndex
from oracle import flat
from test_grouped_cpu import FILTERS
from test_update_cpu import UpdatableOracleIndex

N, D = 300, 16
MIN_SCORE = 0.95
ID0 = 1000   # ids are not row numbers


class JoinIndex(JoinOracleIndex, UpdatableOracleIndex):
    pass


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", JoinIndex)


def corpus():
    """300 rows; planted: per bucket b (rows b + 7 j) an exact copy, a near copy and a near copy OF the near copy (a chain, inside
    the bucket and from row 250 on), an exact copy across buckets, a near pair among the three `rare` rows, a pair beyond row 250."""
    x = flat.synth(N, D, 5)
    flat.normalize_l2(x)
    noise = flat.synth(N, D, 6)
    flat.normalize_l2(noise)
    for b in range(7):
        src = b + 7
        x[src + 140] = x[src]
        x[src + 210] = x[src] + 0.03 * noise[src + 210]
        x[src + 245] = x[src + 210] + 0.03 * noise[src + 245]
    x[201] = x[100]
    x[200] = x[0] + 0.03 * noise[200]
    x[280] = x[252]
    return x


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=64)
    meta = [{"bucket": i % 7, "rank": i, "rare": "yes"} if i % 100 == 0 else {"bucket": i % 7, "rank": i} for i in range(n)]
    db.store_embeddings_batch([ID0 + i for i in range(n)], corpus()[:n], meta)
    return db


def brute(db, min_score, f, first_row=0):
    """[(score64, later row, earlier row)] of every pair inside the filter, from the rows as they are stored, in float64."""
    db.find_most_similar(np.ones(D, np.float32), k=1)           # (brings the stand-in's matrix up to date)
    x = db.index.x.astype(np.float64)
    f = f or {}
    sel = db._get_filtered_indices(f.get("metadata_filter"), f.get("exclude_filter"), f.get("or_filters")).materialize()
    s = x @ x.T
    near = np.abs(s - min_score) < 1e-5
    assert not near.any(), "a pair sits on the threshold: the float32 and the float64 answer may differ"
    return sorted((-s[i, j], int(i), int(j)) for i in sel if i >= first_row for j in sel if j < i and s[i, j] >= min_score)


def check(db, got, want):
    a, b, scores = got
    assert type(a) is list and type(b) is list and type(scores) is list and len(a) == len(b) == len(scores)
    row = {uid: r for r, uid in enumerate(db._ids.uids)}
    pairs = [(row[late], row[early]) for early, late in zip(a, b)]
    assert sorted(pairs) == sorted((i, j) for _, i, j in want)
    assert len(set(pairs)) == len(pairs) and all(j < i for i, j in pairs)
    want_score = {(i, j): -s for s, i, j in want}
    assert all(abs(float(s) - want_score[p]) < 1e-5 for s, p in zip(scores, pairs))
    keys = [(-float(s), i, j) for s, (i, j) in zip(scores, pairs)]
    assert keys == sorted(keys)                                  # best first, ties by (later position, earlier position)


def groups_of(db, want):
    """connected components of the brute-force pairs, as find_duplicate_groups documents them"""
    comp = {}
    for _, i, j in want:
        a, b = comp.setdefault(i, {i}), comp.setdefault(j, {j})
        if a is not b:
            a |= b
            for r in b:
                comp[r] = a
    uids = db._ids.uids
    return [[uids[r] for r in sorted(g)] for g in sorted({id(g): g for g in comp.values()}.values(), key=min)]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_pairs_counts_and_groups_under_every_filter(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    nonempty = 0
    for f in FILTERS:
        want = brute(db, MIN_SCORE, f)
        got = db.find_duplicate_pairs(MIN_SCORE, **(f or {}))
        check(db, got, want)
        count = db.count_duplicate_pairs(MIN_SCORE, **(f or {}))
        assert count == len(want) and isinstance(count, int), f
        assert db.find_duplicate_groups(MIN_SCORE, **(f or {})) == groups_of(db, want), f
        nonempty += bool(want)
    assert nonempty >= 9
    everything = brute(db, MIN_SCORE, None)
    assert len(everything) >= 7 * 4 + 3                          # per bucket: copy, near copy, chain (2 pairs or more); the three singles
    groups = db.find_duplicate_groups(MIN_SCORE)
    assert [ID0 + 7, ID0 + 147, ID0 + 217, ID0 + 252, ID0 + 280] in groups   # the chain of bucket 0, in storage order
    assert groups == sorted(groups, key=lambda g: g[0]) and all(len(g) >= 2 and g == sorted(g) for g in groups)
    # a floor below every cosine: every pair of the selection
    assert db.count_duplicate_pairs(-2.0, metadata_filter={"rare": "yes"}) == 3
    assert db.count_duplicate_pairs(2.0) == 0 and db.find_duplicate_pairs(2.0) == ([], [], [])
    assert db.find_duplicate_groups(2.0) == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_first_row_and_limit(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    for f in (None, {"metadata_filter": {"bucket": 0}}, {"exclude_filter": {"bucket": 3}}):
        kw = f or {}
        for first_row in (0, 150, N, N + 5):
            want = brute(db, MIN_SCORE, f, first_row)
            assert (len(want) > 0) == (first_row < N)
            check(db, db.find_duplicate_pairs(MIN_SCORE, first_row=first_row, **kw), want)
            assert db.count_duplicate_pairs(MIN_SCORE, first_row=first_row, **kw) == len(want)
        full = db.find_duplicate_pairs(MIN_SCORE, **kw)
        for limit in (0, 1, 3, len(full[0]), len(full[0]) + 5):
            cut = db.find_duplicate_pairs(MIN_SCORE, limit=limit, **kw)
            assert cut == tuple(v[:limit] for v in full)
            assert db.count_duplicate_pairs(MIN_SCORE, limit=limit, **kw) == min(limit, len(full[0]))
    # a bulk add checked against what was there: pairs whose later member is new
    size = len(db._ids)
    y = corpus()[[7, 8, 50]].copy()
    db.store_embeddings_batch([5000, 5001, 5002], y, [{"bucket": 0, "rank": 900 + i} for i in range(3)])
    early, late, _ = db.find_duplicate_pairs(MIN_SCORE, first_row=size)
    assert set(late) <= {5000, 5001, 5002} and {(ID0 + 7, 5000), (ID0 + 8, 5001)} <= set(zip(early, late))
    check(db, db.find_duplicate_pairs(MIN_SCORE, first_row=size), brute(db, MIN_SCORE, None, size))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_after_a_delete_and_an_update(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    before = db.count_duplicate_pairs(MIN_SCORE)
    if kind == "flat":
        db.delete_embedding(ID0 + 147)
    else:
        db.delete_embeddings_batch([ID0 + 147])
    want = brute(db, MIN_SCORE, None)
    assert 0 < len(want) < before
    got = db.find_duplicate_pairs(MIN_SCORE)
    check(db, got, want)
    assert ID0 + 147 not in got[0] + got[1]
    assert db.find_duplicate_groups(MIN_SCORE) == groups_of(db, want)
    db.update_embedding(ID0 + 5, embedding=db.get_vector(ID0 + 6))   # row 5 becomes a copy of row 6
    want = brute(db, MIN_SCORE, None)
    got = db.find_duplicate_pairs(MIN_SCORE)
    check(db, got, want)
    assert (ID0 + 5, ID0 + 6) in set(zip(got[0], got[1]))
    assert db.count_duplicate_pairs(MIN_SCORE, metadata_filter={"bucket": 5}) == len(brute(db, MIN_SCORE, {"metadata_filter": {"bucket": 5}}))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_empty_store_and_argument_errors(tmp_path, backend, monkeypatch, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    db = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
          else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    assert db.find_duplicate_pairs(0.5) == ([], [], [])
    assert db.find_duplicate_pairs(0.5, metadata_filter={"a": 1}) == ([], [], [])
    assert db.count_duplicate_pairs(0.5) == 0 and db.find_duplicate_groups(0.5) == []
    for db in (db, make_db(kind, tmp_path)):
        for name in ("find_duplicate_pairs", "count_duplicate_pairs", "find_duplicate_groups"):
            for kw in ({"min_score": float("nan")}, {"min_score": 0.5, "first_row": -1}, {"min_score": 0.5, "limit": -1}):
                with pytest.raises(ValueError):
                    getattr(db, name)(**kw)


def test_a_filter_is_evaluated_once_per_call_and_its_row_set_is_kept(tmp_path, backend, monkeypatch):
    db = make_db("flat", tmp_path)
    db.find_most_similar(np.ones(D, np.float32), k=1)
    evaluated = []
    inner = db._get_filtered_indices
    monkeypatch.setattr(db, "_get_filtered_indices", lambda *a: evaluated.append(a) or inner(*a))
    f = {"metadata_filter": {"bucket": 2}}
    db.index.calls.clear()
    first = db.find_duplicate_pairs(MIN_SCORE, **f)
    kinds = [c[0] for c in db.index.calls]
    assert len(evaluated) == 1 and kinds.count("rowset") == 1 and kinds.count("range_join") == 1
    db.index.calls.clear()
    assert db.find_duplicate_pairs(MIN_SCORE, **f) == first
    assert db.count_duplicate_pairs(MIN_SCORE, first_row=100, **f) == sum(1 for uid in first[1] if uid - ID0 >= 100)
    db.find_duplicate_groups(MIN_SCORE, **f)
    db.find_most_similar(np.ones(D, np.float32), k=3, **f)       # the same cache serves the top-k search
    kinds = [c[0] for c in db.index.calls]
    assert len(evaluated) == 1 and kinds.count("rowset") == 0, db.index.calls   # resident: no evaluation, no upload
    assert kinds.count("range_join") == 2 and kinds.count("range_join_count") == 1
    assert all(c[1] for c in db.index.calls if c[0].startswith("range_join"))    # ... and every call went under the set
    db.index.calls.clear()
    db.find_duplicate_pairs(MIN_SCORE)                           # unfiltered: no set is built
    assert [c for c in db.index.calls if c[0] in ("rowset", "range_join")] == [("range_join", False)]
    # a stale set (rows deleted between the filter and the join) is evaluated again, as every search under a filter
    db.index.fail_next_join = 1
    assert db.find_duplicate_pairs(MIN_SCORE, **f) == first
    db.index.fail_next_join = 3
    with pytest.raises(ValueError):
        db.find_duplicate_pairs(MIN_SCORE, **f)
    db.index.fail_next_join = 0


def test_classes_without_a_range_join_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name in ("find_duplicate_pairs", "count_duplicate_pairs", "find_duplicate_groups"):
            with pytest.raises(NotImplementedError, match="duplicate-pair search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), 0.9)


def test_the_wrapper_works_in_blocks_and_asks_overflowed_rows_once_more():
    """FlatIndex.range_join over a scripted range_join_raw: blocks of `block` query rows under a small cap, the rows of a block
    that overflowed once more with the largest count seen; [N, cap] arrays for the whole corpus never exist."""
    from minivectordb_amd import _native

    class Scripted(_native.FlatIndex):
        def __init__(self, n):
            self.d, self.n, self.raw_calls = 4, n, []

        def __del__(self):
            pass

        ntotal = property(lambda self: self.n)

        def range_join_raw(self, qrows, threshold, cap, rowset=None):
            qrows = np.asarray(qrows, np.int64)
            self.raw_calls.append((qrows.tolist(), cap))
            counts = np.minimum(qrows, 5)                        # row i matches rows 0 .. min(i, 5) - 1
            if cap == 0:
                return counts, None, None
            D = np.full((len(qrows), cap), -3.4028234663852886e38, np.float32)
            I = np.full((len(qrows), cap), -1, np.int64)
            for r, c in enumerate(counts):
                if c <= cap:
                    D[r, :c], I[r, :c] = 1.0 - 0.1 * np.arange(c), np.arange(c)
            return counts, D, I

    idx = Scripted(9)
    qrows, lims, D, I = idx.range_join(0.5, cap=2, block=4)
    assert idx.raw_calls == [([0, 1, 2, 3], 2), ([3], 3), ([4, 5, 6, 7], 2), ([4, 5, 6, 7], 5), ([8], 2), ([8], 5)]
    assert qrows.tolist() == list(range(9)) and lims.tolist() == [0, 0, 1, 3, 6, 10, 15, 20, 25, 30]
    assert all(I[lims[i]:lims[i + 1]].tolist() == list(range(min(i, 5))) for i in range(9))
    assert D.dtype == np.float32 and I.dtype == np.int64 and (I >= 0).all()
    idx.raw_calls.clear()
    assert idx.range_join_count(0.5, first_row=2, block=4) == 2 + 3 + 4 + 5 * 4
    assert idx.raw_calls == [([2, 3, 4, 5], 0), ([6, 7, 8], 0)]
    qrows, lims, D, I = idx.range_join(0.5, rows=[7, 1, 7], cap=8)
    assert qrows.tolist() == [7, 1, 7] and lims.tolist() == [0, 5, 6, 11]
    assert Scripted(0).range_join(0.5)[1].tolist() == [0] and Scripted(0).range_join_count(0.5) == 0
