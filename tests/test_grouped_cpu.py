"""find_most_similar_each — a batch in which every query has its own filter — on the CPU oracle stand-in: the host half
(filter evaluation once per distinct filter, routing, the byte-bounded row-set cache, the retry after a concurrent delete).
Element i must equal find_most_similar(embeddings[i], **filters[i]) exactly: the same oracle arithmetic runs on both sides."""
import numpy as np
import pytest

from oracle import flat
from oracle_backend import OracleIndex

N, D, NQ = 300, 16, 40


class GroupedOracleIndex(OracleIndex):
    """OracleIndex + search_grouped: a loop over the oracle's search_rowset / search, as the contract of the C-ABI states it."""
    fail_next_grouped = 0

    def search_grouped(self, q, k, rowsets, normalize_q=False):
        rowsets = list(rowsets)
        self.calls.append(("search_grouped", k, len(rowsets)))
        if self.fail_next_grouped:
            self.fail_next_grouped -= 1
            raise ValueError("the row set was built for another state of the index")
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        assert len(rowsets) == q.shape[0]
        Ds = np.empty((q.shape[0], k), np.float32)
        Is = np.empty((q.shape[0], k), np.int64)
        for i, rs in enumerate(rowsets):
            if rs is None:
                Ds[i:i + 1], Is[i:i + 1] = OracleIndex.search(self, q[i:i + 1], k, normalize_q=normalize_q)
            elif len(rs) == 0:
                if rs.n > self.x.shape[0] or rs.gen != getattr(self, "renumbered", 0):
                    raise ValueError("the row set was built for another state of the index")
                Ds[i], Is[i] = -3.4028234663852886e38, -1
            else:
                Ds[i:i + 1], Is[i:i + 1] = OracleIndex.search_rowset(self, q[i:i + 1], k, rs, normalize_q=normalize_q)
        return Ds, Is


@pytest.fixture(params=["grouped", "plain"])
def backend(request, monkeypatch):
    from minivectordb_amd import _native
    cls = GroupedOracleIndex if request.param == "grouped" else OracleIndex
    monkeypatch.setattr(_native, "FlatIndex", cls)
    return request.param


@pytest.fixture
def grouped_backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", GroupedOracleIndex)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=64)
    x = flat.synth(n, D, 5)
    meta = [{"bucket": i % 7, "rank": i, "rare": "yes"} if i % 100 == 0 else {"bucket": i % 7, "rank": i} for i in range(n)]
    db.store_embeddings_batch(list(range(n)), x, meta)
    return db


FILTERS = [
    None,
    {"metadata_filter": {"bucket": 0}},
    {"metadata_filter": {"bucket": 1}},
    {"metadata_filter": {"bucket": 2}},
    {"exclude_filter": {"bucket": 3}},
    {"or_filters": [{"bucket": 4}, {"bucket": 5}]},
    {"metadata_filter": {"rank": {"$gte": 250}}},
    {"metadata_filter": {"bucket": 99}},                      # matches nothing
    {"metadata_filter": {"rank": {"$gte": 0}}},               # matches everything
    {"metadata_filter": {"rare": "yes"}},                     # three rows: fewer than k
    {"metadata_filter": {"bucket": 1}},                       # a repeat
    {"metadata_filter": {"bucket": 6}, "exclude_filter": {"rare": "yes"}},
    {},
]


def filters_for(nq):
    return [FILTERS[i % len(FILTERS)] for i in range(nq)]


def assert_same_result(got, want, what):
    assert type(got) is type(want) and len(got) == 3, what
    for a, b in zip(got, want):
        assert type(a) is type(b), (what, type(a), type(b))
    assert list(got[0]) == list(want[0]), what
    assert list(got[2]) == list(want[2]), what
    assert len(got[1]) == len(want[1]) and all(x == y for x, y in zip(got[1], want[1])), what


@pytest.mark.parametrize("autocut", [False, True])
@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_each_equals_the_loop_of_single_calls(tmp_path, backend, kind, autocut):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 6)
    filters = filters_for(NQ)
    many = db.find_most_similar_each(q, filters, k=5, autocut=autocut)
    assert len(many) == NQ
    for i, f in enumerate(filters):
        one = db.find_most_similar(q[i], k=5, autocut=autocut, **(f or {}))
        assert_same_result(many[i], one, (i, f))
    assert many[7] == ([], [], [])                             # the filter that matches nothing
    assert len(many[9][0]) in ((3,) if not autocut else (1, 2, 3))   # min(k, rows selected)


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_empty_database_and_argument_errors(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    db = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
          else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(3, D, 7)
    assert db.find_most_similar_each(q, [None, {"metadata_filter": {"a": 1}}, None]) == [([], [], [])] * 3
    db = make_db(kind, tmp_path)
    with pytest.raises(ValueError):
        db.find_most_similar_each(q, [None, None])             # wrong length
    with pytest.raises(ValueError):
        db.find_most_similar_each(q[0], [None])                # 1-D embeddings
    with pytest.raises(ValueError):
        db.find_most_similar_each(q, [None, {"filter": {}}, None])   # not one of the three names
    db.find_most_similar_each(q, [None] * 3)
    db.index.calls.clear()
    with pytest.raises(ValueError):
        db.find_most_similar_each(flat.synth(3, D + 1, 7), [{"metadata_filter": {"bucket": 1}}] * 3)   # wrong width
    assert db.index.calls == []                                  # refused before any filter or search
    assert db.find_most_similar_each(np.empty((0, D), np.float32), []) == []


def searches(calls):
    return [c for c in calls if c[0] in ("search", "subset", "search_grouped")]


def test_one_grouped_call_when_every_filter_is_in_list_form(tmp_path, grouped_backend):
    db = make_db("flat", tmp_path)
    q = flat.synth(NQ, D, 8)
    filters = [{"metadata_filter": {"bucket": i % 7}} for i in range(NQ)]
    db.find_most_similar_each(q[:1], filters[:1])              # builds the index
    db.index.calls.clear()
    db.find_most_similar_each(q, filters, k=5)
    kinds = [c[0] for c in db.index.calls]
    assert kinds.count("search_grouped") == 1 and db.index.calls[kinds.index("search_grouped")][2] == NQ
    assert kinds.count("rowset") == 6                          # one set per distinct filter not yet resident
    db.index.calls.clear()
    db.find_most_similar_each(q, filters, k=5)                 # everything resident now
    assert [c[0] for c in db.index.calls if c[0] != "subset"] == ["search_grouped"]   # ("subset": the stand-in's own inner loop)
    # unfiltered queries travel as ONE batch beside the grouped call
    db.index.calls.clear()
    db.find_most_similar_each(q, [None if i % 2 else filters[i] for i in range(NQ)], k=5)
    kinds = [c[0] for c in db.index.calls]
    assert kinds.count("search_grouped") == 1 and kinds.count("search") == 1


def test_an_index_without_search_grouped_is_served_per_filter(tmp_path, monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", OracleIndex)
    db = make_db("flat", tmp_path)
    q = flat.synth(NQ, D, 9)
    filters = filters_for(NQ)
    db.find_most_similar_each(q[:1], [None])
    db.index.calls.clear()
    db.find_most_similar_each(q, filters, k=5)
    made = searches(db.index.calls)
    # FILTERS holds 13 entries, 11 of them distinct after None == {} and the repeat; the one that matches nothing is never
    # searched, and the unfiltered queries share ONE batch with the filter that matches everything: 11 - 1 - 1 = 9 searches
    assert len({repr(f or None) for f in filters}) == 11
    assert len(made) == 9, made                                  # one search per distinct filter, not one per query
    assert [c[0] for c in made].count("search") == 1


def held_bytes(db):
    cache = db.__dict__["_rowsets_each"]
    total = sum(entry[4] for entry in cache.values())
    assert total == db.__dict__["_rowsets_each_bytes"]
    return total


def test_the_row_set_cache_is_bounded_by_bytes(tmp_path, grouped_backend):
    n = 400
    db = make_db("flat", tmp_path, n=n)
    q = flat.synth(4, D, 10)
    bound = 2 * 8 * n
    requested, lo, seen_nonempty = 0, 0, False
    while requested <= 2 * n + 100:
        # four overlapping tenants of 3n/100 rows each, new ones every call
        filters = [{"metadata_filter": {"rank": {"$gte": lo + 2 * j}}, "exclude_filter": None,
                    "or_filters": [{"rank": r} for r in range(lo + 2 * j, lo + 2 * j + 3 * n // 100)]} for j in range(4)]
        out = db.find_most_similar_each(q, filters, k=5)
        assert all(len(ids) == 5 for ids, _, _ in out)
        requested += 4 * (3 * n // 100)
        lo += 8
        total = held_bytes(db)
        assert total <= bound, (total, bound)
        seen_nonempty = seen_nonempty or total > 0
    assert seen_nonempty and requested > 2 * n
    assert len(db.__dict__["_rowsets_each"]) < requested // (3 * n // 100)       # something was evicted
    assert list(db.__dict__["_rowsets_each"])[-1] == repr(tuple(filters[-1][name] for name in db._EACH_FILTER_KEYS))
    assert len(db.__dict__.get("_rowsets", {})) == 0                           # the single-filter cache is not this method's
    db.store_embedding(10_000, flat.synth(1, D, 11)[0], {"bucket": 0})
    assert held_bytes(db) == 0 and len(db.__dict__["_rowsets_each"]) == 0      # a write empties the cache


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_deletes_between_and_inside_calls(tmp_path, grouped_backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 12)
    filters = filters_for(NQ)
    db.find_most_similar_each(q, filters, k=5)
    if kind == "flat":
        db.delete_embedding(14)
    else:
        db.delete_embeddings_batch([14])
    many = db.find_most_similar_each(q, filters, k=5)
    for i, f in enumerate(filters):
        assert_same_result(many[i], db.find_most_similar(q[i], k=5, **(f or {})), (i, f))
        assert 14 not in many[i][0]
    # a delete between filter evaluation and search: the first grouped call reports stale sets once
    db.index.fail_next_grouped = 1
    db.index.calls.clear()
    again = db.find_most_similar_each(q, filters, k=5)
    assert [c[0] for c in db.index.calls].count("search_grouped") == 2
    for i in range(NQ):
        assert_same_result(again[i], many[i], i)
    db.index.fail_next_grouped = 3
    with pytest.raises(ValueError):
        db.find_most_similar_each(q, filters, k=5)
    db.index.fail_next_grouped = 0
