"""find_most_similar_groups / find_most_similar_groups_batch on the CPU oracle stand-in: the host half (grouping by a
metadata key, missing-key singletons, short groups, filters, clamps, argument errors, packaging and order, the grouping
cache across writes, the retry after a stale-object ValueError) — and the checks of tests/groups_oracle.py, the contract the
GPU tests hold the device to."""
import numpy as np
import pytest

from distinct_oracle import MISSING
from groups_oracle import member_rows, members
from oracle import flat
from oracle_backend import OracleIndex
from test_distinct_cpu import D, N, NQ, DistinctOracleIndex, group_of, make_db
from test_grouped_cpu import FILTERS


class GroupsOracleIndex(DistinctOracleIndex):
    """DistinctOracleIndex + search_groups: the contract of mvdb_index_search_groups as a loop — the groups of
    search_distinct, the members from each query's full ranking of the selected rows."""
    fail_next_groups = 0

    def search_groups(self, q, k, group_size, fetch_k, grouping, rowset=None, normalize_q=False):
        self.calls.append(("search_groups", int(k), int(group_size), int(fetch_k), rowset is not None))
        if self.fail_next_groups:
            self.fail_next_groups -= 1
            raise ValueError("the grouping was built for another state of the index")
        if not 1 <= group_size <= 16:
            raise ValueError("group hits search needs 1 <= group_size <= 16")
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        _, _, G = DistinctOracleIndex.search_distinct(self, q, k, fetch_k, grouping, rowset=rowset, normalize_q=normalize_q)
        m = self.x.shape[0] if rowset is None else len(rowset)
        Dm = np.empty((q.shape[0], k, group_size), np.float32)
        Im = np.empty((q.shape[0], k, group_size), np.int64)
        for i in range(q.shape[0]):
            if rowset is None:
                Df, If = OracleIndex.search(self, q[i:i + 1], m, normalize_q=normalize_q)
            else:
                Df, If = OracleIndex.search_rowset(self, q[i:i + 1], m, rowset, normalize_q=normalize_q)
            Dm[i], Im[i] = members(Df[0], If[0], grouping.codes, G[i], group_size)
        return Dm, Im, G


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", GroupsOracleIndex)


def brute(db, q, key, k, group_size, f):
    """The answer from find_most_similar over everything the filter selects: groups in the order of their first hit, the
    first k of them, each with its first group_size hits."""
    ids, dist, metas = db.find_most_similar(q, k=10 ** 6, **f)
    order, hits = [], {}
    for u, s, m in zip(ids, dist, metas):
        g = group_of(m, key, u)
        if g not in hits:
            hits[g] = []
            order.append(g)
        if len(hits[g]) < group_size:
            hits[g].append((u, s, m))
    return [(tuple(h[0] for h in hits[g]), [h[1] for h in hits[g]], [h[2] for h in hits[g]]) for g in order[:k]]


def same(got, want, what):
    assert isinstance(got, list) and len(got) == len(want), (what, len(got), len(want))
    for j, (a, b) in enumerate(zip(got, want)):
        assert len(a) == 3 and isinstance(a[0], tuple) and list(a[0]) == list(b[0]) and list(a[2]) == list(b[2]), (what, j, a[0], b[0])
        assert len(a[1]) == len(b[1]) and all(x == y and type(x) is np.float32 for x, y in zip(a[1], b[1])), (what, j)


def group_calls(db):
    return [c for c in db.index.calls if c[0] == "search_groups"]


# ---- the helper -------------------------------------------------------------------------------------------------------------

def test_members_take_the_ranking_order_pad_and_skip_missing_groups():
    codes = np.array([0, 0, 1, 2, 1, 3, 3, 0, 0], np.int32)
    # rows 1 and 0 tie at .9, rows 7 and 8 tie at .5: a ranking lists equal scores by ascending position, and members keep it
    Df = np.array([.9, .9, .7, .6, .5, .5, .4, .3, 0], np.float32)
    If = np.array([0, 1, 4, 2, 7, 8, 6, 5, -1], np.int64)       # row 3 (group 2) scored NaN: it is in no ranking
    d, i = members(Df, If, codes, np.array([0, 3, -1, 1], np.int32), 3)
    assert i.tolist() == [[0, 1, 7], [6, 5, -1], [-1, -1, -1], [4, 2, -1]]
    assert d[0].tolist() == [Df[0], Df[1], Df[4]] and d[1].tolist()[:2] == [Df[6], Df[7]] and d[3].tolist()[:2] == [Df[2], Df[3]]
    assert (d[i == -1] == MISSING).all() and d.dtype == np.float32 and i.dtype == np.int64 and d.shape == i.shape == (4, 3)
    d, i = members(Df, If, codes, np.array([2], np.int32), 2)    # the group's only row is NaN: all padding
    assert i.tolist() == [[-1, -1]] and (d == MISSING).all()
    d, i = members(Df, If, codes, np.array([0], np.int32), 1)
    assert i.tolist() == [[0]]
    d, i = members(Df[:0], If[:0], codes, np.array([-1, -1], np.int32), 2)
    assert (i == -1).all() and (d == MISSING).all()
    with pytest.raises(AssertionError):
        members(Df, If, codes, np.array([1, 1], np.int32), 2)


def test_member_rows_counts_selected_rows_of_the_chosen_groups():
    codes = np.array([0, 0, 1, 2, 1, 3, 3, 0, 0], np.int32)
    assert member_rows(None, codes, np.array([[0, 3, -1]])) == 6          # NaN or not: every row of groups 0 and 3
    assert member_rows(None, codes, np.array([[0, 3, -1], [2, -1, -1]])) == 7
    assert member_rows([8, 2, 0, 5], codes, np.array([[0, 1]])) == 3      # of the selected rows only
    assert member_rows([], codes, np.array([[0, 1]])) == 0
    assert member_rows(None, codes, np.array([[-1, -1]])) == 0


# ---- the Python layer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_groups_and_members_under_every_filter(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 6)
    q[0] = db.get_vector(39)
    several = 0
    for i, f in enumerate(FILTERS):
        f = f or {}
        allowed = set(db.find_most_similar(q[i], k=N, **f)[0])
        db.index.calls.clear()
        got = db.find_most_similar_groups(q[i], "doc", k=5, group_size=3, fetch_k=30, **f)
        if not allowed:
            assert got == [] and db.index.calls == []                  # zero matches: nothing is searched
            continue
        (call,) = group_calls(db)
        assert call == ("search_groups", min(5, len(allowed)), 3, max(min(5, len(allowed)), min(30, len(allowed))), len(allowed) != N)
        same(got, brute(db, q[i], "doc", 5, 3, f), (i, f))
        # the groups, and their heads, are distinct search's
        heads = db.find_most_similar_distinct(q[i], "doc", k=5, fetch_k=30, **f)
        assert [g[0][0] for g in got] == list(heads[0]) and [g[1][0] for g in got] == list(heads[1])
        for ids, dist, metas in got:
            assert set(ids) <= allowed and [m["rank"] for m in metas] == list(ids) and 1 <= len(ids) <= 3
            assert len({group_of(m, "doc", u) for u, m in zip(ids, metas)}) == 1          # one group
            assert list(dist) == sorted(dist, reverse=True)
        assert len({group_of(g[2][0], "doc", g[0][0]) for g in got}) == len(got)          # every group once
        several += any(len(g[0]) > 1 for g in got)
    assert several >= 1
    # the query on two documents of near-copies, which fill the fetch: 5 documents all the same, 3 chunks of each
    got = db.find_most_similar_groups(q[0], "doc", k=5, group_size=3, fetch_k=8)
    assert db.index.fallback_queries >= 1 and len(got) == 5 and got[0][0][0] == 39 and [len(g[0]) for g in got] == [3] * 5
    same(got, brute(db, q[0], "doc", 5, 3, {}), "tier 2")


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_missing_keys_short_groups_and_the_unhashable_value(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 7)
    # rows without the key are groups of their own — one row each —, documents have 6 rows (5 where one row lost its key)
    got = db.find_most_similar_groups(q[0], "doc", k=64, group_size=16, fetch_k=N)
    assert len(got) == 50 + 6
    sizes = {(g[2][0].get("doc"), len(g[0])) for g in got}
    assert {n for d, n in sizes if d is None} == {1} and {n for d, n in sizes if d is not None} == {5, 6}
    same(got, brute(db, q[0], "doc", 64, 16, {}), "whole groups")
    # "rare": 3 rows share "yes", 297 stand alone; group_size 2 cuts the one group that has more
    got = db.find_most_similar_groups_batch(q[:1], "rare", k=64, group_size=2, fetch_k=N)[0]
    assert len(got) == 64 and sorted({len(g[0]) for g in got}) in ([1], [1, 2])
    same(got, brute(db, q[0], "rare", 64, 2, {}), "rare")
    f = {"metadata_filter": {"rare": "yes"}}
    got = db.find_most_similar_groups(q[0], "rare", k=5, group_size=2, **f)
    assert len(got) == 1 and len(got[0][0]) == 2                        # one group of three rows, the best two
    same(got, brute(db, q[0], "rare", 5, 2, f), "rare only")
    # 1, 1.0 and True are one dict key; "1" is another: two groups
    got = db.find_most_similar_groups(q[1], "mixed", k=10, group_size=4)
    assert len(got) == 2 and [len(g[0]) for g in got] == [4, 4]
    same(got, brute(db, q[1], "mixed", 10, 4, {}), "mixed")
    # a key nobody has: every row its own group — the plain search, one row per group
    plain = db.find_most_similar(q[1], k=7)
    got = db.find_most_similar_groups(q[1], "nobody", k=7, group_size=3)
    assert [g[0] for g in got] == [(u,) for u in plain[0]] and [g[1][0] for g in got] == list(plain[1])
    # group_size = 1 is distinct search
    heads = db.find_most_similar_distinct(q[0], "doc", k=9)
    got = db.find_most_similar_groups(q[0], "doc", k=9, group_size=1)
    assert [g[0] for g in got] == [(u,) for u in heads[0]] and [g[2][0] for g in got] == list(heads[2])
    # an unhashable value is a TypeError naming the id; raised once, not retried as a stale object
    db.update_embedding(11, metadata_dict={"doc": ["a", "list"], "bucket": 4, "rank": 11})
    db.index.calls.clear()
    with pytest.raises(TypeError, match=r"id 11\b"):
        db.find_most_similar_groups(q[0], "doc", k=3)
    assert group_calls(db) == []
    with pytest.raises(TypeError):
        db.find_most_similar_groups(q[0], ["unhashable", "key"], k=3)
    assert len(db.find_most_similar_groups(q[0], "bucket", k=10)) == 7   # other keys are unaffected


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_clamps_defaults_and_argument_errors(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
             else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(3, D, 8)
    assert empty.find_most_similar_groups(q[0], "doc") == []
    assert empty.find_most_similar_groups_batch(q, "doc", metadata_filter={"a": 1}) == [[], [], []]
    for bad in (dict(k=0), dict(group_size=0), dict(group_size=17)):
        with pytest.raises(ValueError):
            empty.find_most_similar_groups(q[0], "doc", **bad)         # a bad argument is an error whatever the database holds
    db = make_db(kind, tmp_path)
    assert db.GROUPS_MAX_SIZE == 16 and db.DISTINCT_MAX_K == 64
    db.find_most_similar(q[1], k=1)

    def shape(**kw):
        db.index.calls.clear()
        got = db.find_most_similar_groups(q[0], "doc", **kw)
        (call,) = group_calls(db)
        return call[1:4], got

    assert shape()[0] == (5, 3, 32)                                     # k = 5, group_size = 3, fetch_k=None: max(4 k, 32)
    assert shape(k=3, group_size=16)[0] == (3, 16, 32)
    assert shape(k=30, group_size=1)[0] == (30, 1, 120)
    assert shape(k=64, fetch_k=2000)[0] == (64, 3, N)                   # fetch_k clamped to the rows selected
    rare = {"metadata_filter": {"rare": "yes"}}
    (take, gs, fetch), got = shape(k=5, group_size=2, fetch_k=40, **rare)
    assert (take, gs, fetch) == (3, 2, 3)                               # k and fetch_k clamped to the selected count, group_size is not
    assert [list(g[0]) for g in got] == [[u] for u in got[0][0] + got[1][0] + got[2][0]] and sorted(u for g in got for u in g[0]) == [0, 100, 200]
    big = make_db(kind, tmp_path / "big", n=1100)
    big.find_most_similar_groups(q[0], "doc", k=4, fetch_k=5000)
    assert [c[1:4] for c in group_calls(big)] == [(4, 3, 1024)]         # fetch_k clamped to 1024
    big.index.calls.clear()
    with pytest.raises(ValueError, match="exceeds 64"):
        big.find_most_similar_groups(q[0], "doc", k=65, fetch_k=100)
    assert big.index.calls == []                                        # raised once: nothing searched, no retry
    assert len(db.find_most_similar_groups(q[0], "doc", k=200, fetch_k=500, **rare)) == 3           # k = 200 clamps to 3 rows: fine
    db.index.calls.clear()
    wrong = flat.synth(3, D + 1, 8)
    for bad in (dict(embedding=wrong[0]), dict(embedding=q[0], k=0), dict(embedding=q[0], k=-2), dict(embedding=q[0], fetch_k=0),
                dict(embedding=q[0], k=5, fetch_k=4), dict(embedding=q[0], group_size=0), dict(embedding=q[0], group_size=-1),
                dict(embedding=q[0], group_size=17)):
        with pytest.raises(ValueError):
            db.find_most_similar_groups(group_by="doc", **bad)
    with pytest.raises(ValueError, match=r"group_size must lie in \[1, 16\]"):
        db.find_most_similar_groups_batch(q, "doc", group_size=17)
    with pytest.raises(ValueError):
        db.find_most_similar_groups_batch(wrong, "doc")
    with pytest.raises(ValueError):
        db.find_most_similar_groups_batch(q[0], "doc")                  # 1-D embeddings
    assert db.index.calls == []                                         # nothing reached the index
    assert db.find_most_similar_groups_batch(np.empty((0, D), np.float32), "doc") == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_batch_equals_the_loop_of_single_calls(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 9)
    q[3] = db.get_vector(40)
    for f in FILTERS:
        f = f or {}
        many = db.find_most_similar_groups_batch(q, "doc", k=4, group_size=3, fetch_k=9, **f)
        assert len(many) == NQ
        for i in range(NQ):
            same(many[i], db.find_most_similar_groups(q[i], "doc", k=4, group_size=3, fetch_k=9, **f), (i, f))
            same(many[i], brute(db, q[i], "doc", 4, 3, f), (i, f))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_the_grouping_cache_follows_every_write(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(4, D, 10)

    def uploads():
        return [c for c in db.index.calls if c[0] == "grouping"]

    db.find_most_similar_groups(q[0], "doc")
    db.index.calls.clear()
    db.find_most_similar_groups(q[1], "doc", group_size=5)
    db.find_most_similar_distinct(q[1], "doc")                          # one cache for both searches
    db.find_most_similar_groups_batch(q, "doc", metadata_filter={"bucket": 2})
    assert uploads() == []                                              # resident: no pass over the metadata, no upload
    # a store: the new row joins document d6
    db.store_embedding(10_000, db.get_vector(39), {"doc": "d6", "bucket": 2, "rank": 10_000})
    db.index.calls.clear()
    got = db.find_most_similar_groups(db.get_vector(39), "doc", k=8, group_size=16)
    assert len(uploads()) == 1 and uploads()[0][1] == N + 1
    assert got[0][2][0]["doc"] == "d6" and len(got[0][0]) == 7 and {39, 10_000} == set(got[0][0][:2])
    same(got, brute(db, db.get_vector(39), "doc", 8, 16, {}), "store")
    # a delete
    if kind == "flat":
        db.delete_embedding(39)
    else:
        db.delete_embeddings_batch([39])
    db.index.calls.clear()
    got = db.find_most_similar_groups(q[0], "doc", k=8, group_size=16)
    assert len(uploads()) == 1 and uploads()[0][1] == N and all(39 not in g[0] for g in got)
    same(got, brute(db, q[0], "doc", 8, 16, {}), "delete")
    # a metadata update: rows 40 .. 44 leave document d6 / d7 for one of their own
    db.update_embeddings_batch([40, 41, 42, 43, 44], metadata_dicts=[{"doc": "moved", "bucket": 1, "rank": u} for u in range(40, 45)])
    db.index.calls.clear()
    got = db.find_most_similar_groups(db.get_vector(41), "doc", k=8, group_size=16)
    assert len(uploads()) == 1
    assert got[0][2][0]["doc"] == "moved" and sorted(got[0][0]) == [40, 41, 42, 43, 44]
    assert sum(g[2][0].get("doc") == "moved" for g in got) == 1
    db.index.calls.clear()
    same(db.find_most_similar_groups(q[0], "doc", k=8), brute(db, q[0], "doc", 8, 3, {}), "update")
    assert uploads() == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_object_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 12)
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_most_similar_groups(q[0], "doc", **f)
    db.index.fail_next_groups = 1
    db.index.calls.clear()
    same(db.find_most_similar_groups(q[0], "doc", **f), want, "retried")
    assert len(group_calls(db)) == 2
    db.index.fail_next_groups = 3
    with pytest.raises(ValueError):
        db.find_most_similar_groups(q[0], "doc", **f)
    db.index.fail_next_groups = 0
    # an index without the method is told so, not retried
    db.index.__class__ = DistinctOracleIndex
    with pytest.raises(NotImplementedError, match="group hits search"):
        db.find_most_similar_groups(q[0], "doc")


def test_classes_without_a_group_hits_search_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    q = flat.synth(2, D, 14)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("find_most_similar_groups", (q[0], "doc")), ("find_most_similar_groups_batch", (q, "doc"))):
            with pytest.raises(NotImplementedError, match="group hits search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_index_search_groups", "mvdb_index_search_groups_device", "mvdb_index_groups_counters"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    assert callable(_native.FlatIndex.search_groups) and callable(_native.FlatIndex.search_groups_device)
    assert callable(_native.FlatIndex.groups_counters)
