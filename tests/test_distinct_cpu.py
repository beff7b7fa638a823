"""find_most_similar_distinct / find_most_similar_distinct_batch on the CPU oracle stand-in: the host half (grouping by a
metadata key, missing-key singletons, the unhashable value, filters, clamps, argument errors, packaging and order, the
grouping cache across writes, the retry after a stale-object ValueError) — and the checks of tests/distinct_oracle.py, the
contract the GPU tests hold the device to."""
import numpy as np
import pytest

from distinct_oracle import MISSING, collapse, tier
from oracle import flat
from oracle_backend import OracleIndex
from test_grouped_cpu import FILTERS

N, D, NQ = 300, 16, 13


class _OracleGrouping:
    def __init__(self, codes, n_groups, gen):
        self.codes, self.n_groups, self.gen = codes, int(n_groups), gen

    def __len__(self):
        return len(self.codes)

    def free(self):
        pass


class DistinctOracleIndex(OracleIndex):
    """OracleIndex + grouping / search_distinct: the contract of mvdb_index_search_distinct as a loop — the oracle's
    top-fetch_k search of the selected rows collapsed (tier 1), or the full ranking collapsed (tier 2)."""
    fail_next_distinct = 0
    fallback_queries = 0

    def grouping(self, codes, n_groups):
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        self.calls.append(("grouping", len(codes), int(n_groups)))
        if len(codes) != self.x.shape[0]:
            raise ValueError("a grouping needs one code per stored row")
        if len(codes) and (n_groups < 1 or n_groups > len(codes) or codes.min() < 0 or codes.max() >= n_groups):
            raise ValueError("group code out of range")
        return _OracleGrouping(codes, n_groups, getattr(self, "renumbered", 0))

    def search_distinct(self, q, k, fetch_k, grouping, rowset=None, normalize_q=False):
        self.calls.append(("search_distinct", int(k), int(fetch_k), rowset is not None))
        if self.fail_next_distinct:
            self.fail_next_distinct -= 1
            raise ValueError("the grouping was built for another state of the index")
        if not (1 <= k <= 64 and k <= fetch_k <= 1024):
            raise ValueError("distinct search needs 1 <= k <= 64 and k <= fetch_k <= 1024")
        if len(grouping) != self.x.shape[0] or grouping.gen != getattr(self, "renumbered", 0):
            raise ValueError("the grouping was built for another state of the index")
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        m = self.x.shape[0] if rowset is None else len(rowset)

        def ranking(qq, kk):
            if rowset is None:
                return OracleIndex.search(self, qq, kk, normalize_q=normalize_q)
            return OracleIndex.search_rowset(self, qq, kk, rowset, normalize_q=normalize_q)

        Dc, Ic = ranking(q, fetch_k)
        out = [np.empty((q.shape[0], k), t) for t in (np.float32, np.int64, np.int32)]
        for i in range(q.shape[0]):
            Dr, Ir = Dc[i], Ic[i]
            if tier(Ir, grouping.codes, k, m) == 2:
                self.fallback_queries += 1
                Df, If = ranking(q[i:i + 1], m)
                Dr, Ir = Df[0], If[0]
            out[0][i], out[1][i], out[2][i] = collapse(Dr, Ir, grouping.codes, k)
        return tuple(out)


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", DistinctOracleIndex)


def metadata(n):
    """bucket / rank / rare as tests/test_grouped_cpu.py's filters expect; "doc": chunks of 6 rows, except that rows with
    rank % 50 == 7 carry no "doc" key; "mixed": values that are equal as dict keys (1, 1.0 and True)."""
    out = []
    for i in range(n):
        m = {"bucket": i % 7, "rank": i, "mixed": (1, 1.0, True, "1")[i % 4]}
        if i % 100 == 0:
            m["rare"] = "yes"
        if i % 50 != 7:
            m["doc"] = f"d{i // 6}"
        out.append(m)
    return out


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=64)
    x = flat.synth(n, D, 5)
    x[36:48] = x[39] + 0.01 * flat.synth(12, D, 55)          # two whole documents (d6, d7) of near-copies: a plain top-k is one of them
    db.store_embeddings_batch(list(range(n)), x, metadata(n))
    return db


def group_of(meta, key, uid):
    return ("value", meta[key]) if key in meta else ("row", uid)


def brute(db, q, key, k, f):
    """The answer from find_most_similar over everything the filter selects: the first hit of every group, k of them."""
    ids, dist, metas = db.find_most_similar(q, k=10 ** 6, **f)
    seen, out = set(), []
    for u, s, m in zip(ids, dist, metas):
        g = group_of(m, key, u)
        if g not in seen:
            seen.add(g)
            out.append((u, s, m))
    out = out[:k]
    return tuple(o[0] for o in out), [o[1] for o in out], [o[2] for o in out]


def same(got, want, what):
    assert len(got) == 3 and list(got[0]) == list(want[0]) and list(got[2]) == list(want[2]), (what, got[0], want[0])
    assert len(got[1]) == len(want[1]) and all(x == y and type(x) is np.float32 for x, y in zip(got[1], want[1])), what


# ---- the helper -------------------------------------------------------------------------------------------------------------

def test_collapse_keeps_the_first_entry_of_every_group_and_pads():
    codes = np.array([0, 0, 1, 2, 1, 3, 3, 0], np.int32)
    D = np.array([.9, .8, .7, .6, .5, .4, .3], np.float32)
    I = np.array([1, 0, 4, 7, 2, 6, -1], np.int64)
    d, i, g = collapse(D, I, codes, 3)
    assert i.tolist() == [1, 4, 6] and g.tolist() == [0, 1, 3] and d.tolist() == [D[0], D[2], D[5]]
    assert i.dtype == np.int64 and g.dtype == np.int32 and d.dtype == np.float32
    d, i, g = collapse(D, I, codes, 5)
    assert i.tolist() == [1, 4, 6, -1, -1] and g.tolist() == [0, 1, 3, -1, -1] and (d[3:] == MISSING).all()
    d, i, g = collapse(D[:0], I[:0], codes, 2)
    assert i.tolist() == [-1, -1] and (d == MISSING).all() and g.tolist() == [-1, -1]
    assert collapse(D, I, codes, 1)[1].tolist() == [1]


def test_tier_rule():
    codes = np.array([0, 0, 0, 1, 2, 0], np.int32)
    assert tier(np.array([0, 1, 2]), codes, 2, 6) == 2            # full, one group, does not cover
    assert tier(np.array([0, 1, 3]), codes, 2, 6) == 1            # g >= k
    assert tier(np.array([0, 1, -1]), codes, 2, 6) == 1           # not full: the whole ranking
    assert tier(np.array([0, 1, 2]), codes, 2, 3) == 1            # covers the selection
    assert tier(np.array([0, 1, 2, 5]), codes, 1, 6) == 1


# ---- the Python layer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_grouping_by_key_under_every_filter(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 6)
    q[0] = db.get_vector(39)
    collapsed = 0
    for i, f in enumerate(FILTERS):
        f = f or {}
        allowed = set(db.find_most_similar(q[i], k=N, **f)[0])
        db.index.calls.clear()
        got = db.find_most_similar_distinct(q[i], "doc", k=5, fetch_k=30, **f)
        if not allowed:
            assert got == ([], [], []) and db.index.calls == []      # zero matches: nothing is searched
            continue
        (call,) = [c for c in db.index.calls if c[0] == "search_distinct"]
        assert call == ("search_distinct", min(5, len(allowed)), max(min(5, len(allowed)), min(30, len(allowed))), len(allowed) != N)
        want = brute(db, q[i], "doc", 5, f)
        same(got, want, (i, f))
        ids, dist, metas = got
        assert isinstance(ids, tuple) and set(ids) <= allowed and [m["rank"] for m in metas] == list(ids)
        assert len({group_of(m, "doc", u) for u, m in zip(ids, metas)}) == len(ids)       # one row per group
        assert list(dist) == sorted(dist, reverse=True)
        collapsed += list(ids) != list(db.find_most_similar(q[i], k=5, **f)[0])
    assert collapsed >= 1
    # the query on a document of near-copies: the plain search returns 5 rows of two documents, the distinct search 5 documents
    plain = db.find_most_similar(q[0], k=5)
    assert {m["doc"] for m in plain[2]} <= {"d6", "d7"}
    got = db.find_most_similar_distinct(q[0], "doc", k=5, fetch_k=8)                      # the two documents fill the fetch: tier 2
    assert db.index.fallback_queries >= 1 and len({m["doc"] for m in got[2]}) == 5 and got[0][0] == 39
    same(got, brute(db, q[0], "doc", 5, {}), "tier 2")


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_missing_keys_equal_values_and_the_unhashable_value(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 7)
    # rows without the key are groups of their own: with k = everything, every such row is returned
    ids, _, metas = db.find_most_similar_distinct(q[0], "doc", k=64, fetch_k=N)
    assert len(ids) == 50 + 6 and {u for u in range(N) if u % 50 == 7} <= set(ids)       # 50 documents and the 6 rows without one
    every = db.find_most_similar_distinct_batch(q[:1], "rare", k=64, fetch_k=N)[0]       # 3 rows share "yes", 297 stand alone
    assert len(every[0]) == 64 and sum("rare" in m for m in every[2]) <= 1
    same(every, brute(db, q[0], "rare", 64, {}), "rare")
    lone = [u for u in range(N) if u % 50 == 7]
    got = db.find_most_similar_distinct(q[0], "doc", k=64, fetch_k=N, metadata_filter={"rank": {"$gte": 0}}, exclude_filter={"bucket": 3})
    same(got, brute(db, q[0], "doc", 64, {"exclude_filter": {"bucket": 3}}), "lone")
    assert all("doc" in m or m["rank"] in lone for m in got[2])
    # 1, 1.0 and True are one dict key; "1" is another: two groups
    ids, _, metas = db.find_most_similar_distinct(q[1], "mixed", k=10)
    assert len(ids) == 2 and {type(m["mixed"]) is str for m in metas} == {True, False}
    same((ids, _, metas), brute(db, q[1], "mixed", 10, {}), "mixed")
    # a key nobody has: every row its own group — the plain search
    same(db.find_most_similar_distinct(q[1], "nobody", k=7), db.find_most_similar(q[1], k=7), "nobody")
    # an unhashable value is a TypeError naming the id; raised once, not retried as a stale object
    db.update_embedding(11, metadata_dict={"doc": ["a", "list"], "bucket": 4, "rank": 11})
    db.index.calls.clear()
    with pytest.raises(TypeError, match=r"id 11\b"):
        db.find_most_similar_distinct(q[0], "doc", k=3)
    assert [c for c in db.index.calls if c[0] == "search_distinct"] == []
    with pytest.raises(TypeError):
        db.find_most_similar_distinct(q[0], ["unhashable", "key"], k=3)
    assert len(db.find_most_similar_distinct(q[0], "bucket", k=10)[0]) == 7              # other keys are unaffected


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_clamps_defaults_and_argument_errors(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
             else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(3, D, 8)
    assert empty.find_most_similar_distinct(q[0], "doc") == ([], [], [])
    assert empty.find_most_similar_distinct_batch(q, "doc", metadata_filter={"a": 1}) == [([], [], [])] * 3
    with pytest.raises(ValueError):
        empty.find_most_similar_distinct(q[0], "doc", k=0)          # a bad argument is an error whatever the database holds
    db = make_db(kind, tmp_path)
    db.find_most_similar(q[1], k=1)

    def shape(**kw):
        db.index.calls.clear()
        got = db.find_most_similar_distinct(q[0], "doc", **kw)
        (call,) = [c for c in db.index.calls if c[0] == "search_distinct"]
        return call[1:3], got

    assert shape()[0] == (5, 32)                                        # fetch_k=None: max(4 k, 32)
    assert shape(k=3)[0] == (3, 32)
    assert shape(k=30)[0] == (30, 120)
    assert shape(k=64, fetch_k=2000)[0] == (64, N)                      # fetch_k clamped to the rows selected
    rare = {"metadata_filter": {"rare": "yes"}}
    (take, fetch), got = shape(k=5, fetch_k=40, **rare)
    assert (take, fetch) == (3, 3) and sorted(got[0]) == [0, 100, 200]  # k and fetch_k clamped to the selected count
    big = make_db(kind, tmp_path / "big", n=1100)
    big.find_most_similar_distinct(q[0], "doc", k=4, fetch_k=5000)
    assert [c[1:3] for c in big.index.calls if c[0] == "search_distinct"] == [(4, 1024)]       # fetch_k clamped to 1024
    big.index.calls.clear()
    with pytest.raises(ValueError, match="exceeds 64"):
        big.find_most_similar_distinct(q[0], "doc", k=65, fetch_k=100)
    assert big.index.calls == []                                        # raised once: nothing searched, no retry
    assert len(db.find_most_similar_distinct(q[0], "doc", k=200, fetch_k=500, **rare)[0]) == 3      # k = 200 clamps to 3 rows: fine
    db.index.calls.clear()
    wrong = flat.synth(3, D + 1, 8)
    for bad in (dict(embedding=wrong[0]), dict(embedding=q[0], k=0), dict(embedding=q[0], k=-2), dict(embedding=q[0], fetch_k=0),
                dict(embedding=q[0], k=5, fetch_k=4)):
        with pytest.raises(ValueError):
            db.find_most_similar_distinct(group_by="doc", **bad)
    with pytest.raises(ValueError):
        db.find_most_similar_distinct_batch(wrong, "doc")
    with pytest.raises(ValueError):
        db.find_most_similar_distinct_batch(q[0], "doc")                # 1-D embeddings
    assert db.index.calls == []                                         # nothing reached the index
    assert db.find_most_similar_distinct_batch(np.empty((0, D), np.float32), "doc") == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_batch_equals_the_loop_of_single_calls(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 9)
    q[3] = db.get_vector(40)
    for f in FILTERS:
        f = f or {}
        many = db.find_most_similar_distinct_batch(q, "doc", k=4, fetch_k=9, **f)
        assert len(many) == NQ
        for i in range(NQ):
            same(many[i], db.find_most_similar_distinct(q[i], "doc", k=4, fetch_k=9, **f), (i, f))
            same(many[i], brute(db, q[i], "doc", 4, f), (i, f))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_the_grouping_cache_follows_every_write(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(4, D, 10)

    def uploads():
        return [c for c in db.index.calls if c[0] == "grouping"]

    def fresh_answer(key, **kw):
        """The same rows and metadata in a database built from scratch."""
        other = type(db)(**({"storage_file": str(tmp_path / f"f{len(list(tmp_path.iterdir()))}.pkl")} if kind == "flat"
                            else {"storage_dir": str(tmp_path / f"f{len(list(tmp_path.iterdir()))}"), "shard_size": 64}))
        uids = list(db._ids.uids)
        other.store_embeddings_batch(uids, np.stack([raw[u] for u in uids]), [dict(m) for m in db.metadata])
        return other.find_most_similar_distinct(q[0], key, **kw)

    raw = dict(enumerate(flat.synth(N, D, 5)))              # what make_db stored, as it was handed in
    for u, v in zip(range(36, 48), raw[39] + 0.01 * flat.synth(12, D, 55)):
        raw[u] = v
    raw[10_000] = db.get_vector(39)

    db.find_most_similar_distinct(q[0], "doc")
    db.index.calls.clear()
    db.find_most_similar_distinct(q[1], "doc")
    db.find_most_similar_distinct_batch(q, "doc", metadata_filter={"bucket": 2})
    assert uploads() == []                                              # resident: no pass over the metadata, no upload
    # a store
    db.store_embedding(10_000, raw[10_000], {"doc": "d6", "bucket": 2, "rank": 10_000})
    db.index.calls.clear()
    got = db.find_most_similar_distinct(q[0], "doc", k=8)
    assert len(uploads()) == 1 and uploads()[0][1] == N + 1
    same(got, fresh_answer("doc", k=8), "store")
    # a delete
    if kind == "flat":
        db.delete_embedding(39)
    else:
        db.delete_embeddings_batch([39])
    db.index.calls.clear()
    got = db.find_most_similar_distinct(q[0], "doc", k=8)
    assert len(uploads()) == 1 and uploads()[0][1] == N and 39 not in got[0]
    same(got, fresh_answer("doc", k=8), "delete")
    # a metadata update: rows 40 .. 44 leave document d6 / d7 for one of their own
    db.update_embeddings_batch([40, 41, 42, 43, 44], metadata_dicts=[{"doc": "moved", "bucket": 1, "rank": u} for u in range(40, 45)])
    db.index.calls.clear()
    got = db.find_most_similar_distinct(db.get_vector(41), "doc", k=8)
    assert len(uploads()) == 1
    assert got[2][0]["doc"] == "moved" and sum(m.get("doc") == "moved" for m in got[2]) == 1
    db.index.calls.clear()
    same(db.find_most_similar_distinct(q[0], "doc", k=8), fresh_answer("doc", k=8), "update")
    assert uploads() == []
    # at most four keys stay resident; the least recently used goes
    for key in ("bucket", "rank", "mixed", "rare"):
        db.find_most_similar_distinct(q[0], key)
    assert list(db.__dict__["_groupings"]) == ["bucket", "rank", "mixed", "rare"]
    db.index.calls.clear()
    db.find_most_similar_distinct(q[0], "rare")
    assert uploads() == []
    db.find_most_similar_distinct(q[0], "doc")
    assert len(uploads()) == 1 and list(db.__dict__["_groupings"]) == ["rank", "mixed", "rare", "doc"]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_object_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 12)
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_most_similar_distinct(q[0], "doc", **f)
    db.index.fail_next_distinct = 1
    db.index.calls.clear()
    same(db.find_most_similar_distinct(q[0], "doc", **f), want, "retried")
    assert [c[0] for c in db.index.calls].count("search_distinct") == 2
    db.index.fail_next_distinct = 3
    with pytest.raises(ValueError):
        db.find_most_similar_distinct(q[0], "doc", **f)
    db.index.fail_next_distinct = 0
    # an index without the method is told so, not retried
    db.index.__class__ = OracleIndex
    with pytest.raises(NotImplementedError, match="distinct search"):
        db.find_most_similar_distinct(q[0], "doc")


def test_classes_without_a_distinct_search_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    q = flat.synth(2, D, 14)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("find_most_similar_distinct", (q[0], "doc")), ("find_most_similar_distinct_batch", (q, "doc"))):
            with pytest.raises(NotImplementedError, match="distinct search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_grouping_create", "mvdb_grouping_rows", "mvdb_grouping_groups", "mvdb_grouping_free",
                 "mvdb_index_search_distinct", "mvdb_index_search_distinct_device", "mvdb_index_distinct_counters"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    assert callable(_native.FlatIndex.search_distinct) and callable(_native.Grouping.free)
