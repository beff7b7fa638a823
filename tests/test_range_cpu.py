"""find_all_similar / find_all_similar_batch / count_similar on the CPU oracle stand-in: the host half (filter semantics,
packaging, limit, the resident row-set cache, the retry after a concurrent delete).  The stand-in's range_search states the
contract of mvdb_index_range_search as a loop over the oracle's search: everything at or above the threshold, best first."""
import numpy as np
import pytest

from oracle import flat
from oracle_backend import OracleIndex
from test_grouped_cpu import FILTERS

N, D, NQ = 300, 16, 13


class RangeOracleIndex(OracleIndex):
    """OracleIndex + range_search / range_count: the top-n search of the selected rows, cut where the score falls below the
    threshold (the contract: the leading `count` entries of the search with k = count)."""
    fail_next_range = 0

    def _range(self, q, threshold, rowset, normalize_q):
        if self.fail_next_range:
            self.fail_next_range -= 1
            raise ValueError("the row set was built for another state of the index")
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        if q.shape[1] != self.d:
            raise ValueError("query dimension")
        out = []
        for i in range(q.shape[0]):
            if rowset is None:
                k = self.x.shape[0]
                Ds, Is = OracleIndex.search(self, q[i:i + 1], max(k, 1), normalize_q=normalize_q)
            else:
                k = len(rowset)
                if k == 0:
                    out.append((np.empty(0, np.float32), np.empty(0, np.int64)))
                    continue
                Ds, Is = OracleIndex.search_rowset(self, q[i:i + 1], k, rowset, normalize_q=normalize_q)
            keep = (Is[0] >= 0) & (Ds[0] >= np.float32(threshold))
            assert not keep.any() or keep[:keep.sum()].all()      # sorted: the matches lead
            out.append((Ds[0][keep], Is[0][keep]))
        return out

    def range_search(self, q, threshold, rowset=None, normalize_q=False, cap=None):
        self.calls.append(("range_search", rowset is not None))
        per = self._range(q, threshold, rowset, normalize_q)
        lims = np.zeros(len(per) + 1, np.int64)
        np.cumsum([len(d) for d, _ in per], out=lims[1:])
        return lims, np.concatenate([d for d, _ in per]), np.concatenate([i for _, i in per])

    def range_count(self, q, threshold, rowset=None, normalize_q=False):
        self.calls.append(("range_count", rowset is not None))
        return np.array([len(d) for d, _ in self._range(q, threshold, rowset, normalize_q)], np.int64)


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", RangeOracleIndex)


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


def same(got, want, what):
    assert type(got) is type(want) and len(got) == 3, what
    for a, b in zip(got, want):
        assert type(a) is type(b), (what, type(a), type(b))
    assert list(got[0]) == list(want[0]), what
    assert list(got[2]) == list(want[2]), what
    assert len(got[1]) == len(want[1]) and all(x == y and type(x) is type(y) for x, y in zip(got[1], want[1])), what


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_filters_select_what_find_most_similar_selects(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 6)
    nonempty = 0
    for min_score in (-2.0, 0.0, 0.3):
        for i, f in enumerate(FILTERS):
            f = f or {}
            got = db.find_all_similar(q[i], min_score, **f)
            count = db.count_similar(q[i], min_score, **f)
            assert count == len(got[0]) and isinstance(count, int), (i, f)
            if count == 0:
                assert got == ([], [], [])
                wider = db.find_most_similar(q[i], k=N, **f)     # nothing selected, or nothing reaches the floor
                assert all(s < min_score for s in wider[1])
                continue
            nonempty += 1
            want = db.find_most_similar(q[i], k=count, **f)
            same(got, want, (min_score, i, f))
            assert all(type(s) is np.float32 and s >= min_score for s in got[1])
            more = db.find_most_similar(q[i], k=count + 1, **f)
            assert len(more[0]) == count or more[1][count] < min_score
            for limit in (0, 1, count, count + 5):
                cut = db.find_all_similar(q[i], min_score, limit=limit, **f)
                if min(limit, count) == 0:
                    assert cut == ([], [], [])
                else:
                    same(cut, db.find_most_similar(q[i], k=min(limit, count), **f), (limit, i, f))
    assert nonempty >= 20
    # min_score = -2 is below every cosine: everything the filter selects
    assert len(db.find_all_similar(q[0], -2.0)[0]) == N
    assert db.count_similar(q[0], -2.0, metadata_filter={"bucket": 1}) == len(range(1, N, 7))
    assert db.count_similar(q[0], 2.0) == 0


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_batch_equals_the_loop_of_single_calls(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 7)
    for f in FILTERS:
        f = f or {}
        many = db.find_all_similar_batch(q, 0.1, **f)
        assert len(many) == NQ
        for i in range(NQ):
            same(many[i], db.find_all_similar(q[i], 0.1, **f), (i, f))
        cut = db.find_all_similar_batch(q, 0.1, limit=2, **f)
        for i in range(NQ):
            same(cut[i], db.find_all_similar(q[i], 0.1, limit=2, **f), (i, f))
    assert db.find_all_similar_batch(np.empty((0, D), np.float32), 0.1) == []


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_empty_database_and_argument_errors(tmp_path, backend, monkeypatch, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    db = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
          else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(3, D, 8)
    assert db.find_all_similar(q[0], 0.0) == ([], [], [])
    assert db.find_all_similar_batch(q, 0.0, metadata_filter={"a": 1}) == [([], [], [])] * 3
    assert db.count_similar(q[0], 0.0) == 0
    db = make_db(kind, tmp_path)
    db.find_all_similar(q[0], 0.0)
    db.index.calls.clear()
    evaluated = []
    inner = db._get_filtered_indices
    monkeypatch.setattr(db, "_get_filtered_indices", lambda *a: evaluated.append(a) or inner(*a))
    wrong = flat.synth(3, D + 1, 8)
    with pytest.raises(ValueError):
        db.find_all_similar(wrong[0], 0.0, metadata_filter={"bucket": 1})
    with pytest.raises(ValueError):
        db.find_all_similar_batch(wrong, 0.0, metadata_filter={"bucket": 1})
    with pytest.raises(ValueError):
        db.count_similar(wrong[0], 0.0, metadata_filter={"bucket": 1})
    assert evaluated == [] and db.index.calls == []              # refused before any filter is evaluated, any search made
    with pytest.raises(ValueError):
        db.find_all_similar_batch(q[0], 0.0)                     # 1-D embeddings
    with pytest.raises(ValueError):
        db.find_all_similar(q[0], float("nan"))
    with pytest.raises(ValueError):
        db.find_all_similar(q[0], 0.0, limit=-1)
    assert evaluated == [] and db.index.calls == []
    db.find_all_similar(q[0], 0.0, metadata_filter={"bucket": 1})
    assert len(evaluated) == 1                                   # (the spy does see an evaluation)


def test_the_row_set_cache_is_reused_and_dropped_by_a_write(tmp_path, backend):
    db = make_db("flat", tmp_path)
    q = flat.synth(4, D, 9)
    f = {"metadata_filter": {"bucket": 2}}
    db.find_all_similar(q[0], 0.0, **f)
    kinds = [c[0] for c in db.index.calls]
    assert kinds.count("rowset") == 1 and kinds.count("range_search") == 1
    db.index.calls.clear()
    db.find_all_similar(q[1], 0.2, **f)
    db.count_similar(q[2], 0.1, **f)
    db.find_all_similar_batch(q, 0.1, **f)
    db.find_most_similar(q[3], k=3, **f)                         # the same cache serves the top-k search
    kinds = [c[0] for c in db.index.calls]
    assert kinds.count("rowset") == 0, db.index.calls            # resident: no filter evaluation, no upload
    assert kinds.count("range_search") == 2 and kinds.count("range_count") == 1
    assert all(c[1] for c in db.index.calls if c[0].startswith("range"))   # ... and every call went under the set
    db.store_embedding(10_000, flat.synth(1, D, 10)[0], {"bucket": 2})
    assert db.__dict__["_rowsets"] == {}                         # a write empties the cache
    db.index.calls.clear()
    got = db.find_all_similar(q[0], -2.0, **f)
    assert [c[0] for c in db.index.calls].count("rowset") == 1 and 10_000 in got[0]
    # an unfiltered query never builds a set
    db.index.calls.clear()
    db.find_all_similar(q[0], 0.0)
    assert [c for c in db.index.calls if c[0] == "rowset"] == []
    assert [c for c in db.index.calls if c[0] == "range_search"] == [("range_search", False)]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_set_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 11)
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_all_similar(q[0], 0.0, **f)
    if kind == "flat":
        db.delete_embedding(3)
    else:
        db.delete_embeddings_batch([3])
    after = db.find_all_similar(q[0], -2.0, **f)
    assert 3 not in after[0] and len(after[0]) == len(range(3, N, 7)) - 1
    want = db.find_all_similar(q[0], 0.0, **f)
    db.index.fail_next_range = 1
    db.index.calls.clear()
    same(db.find_all_similar(q[0], 0.0, **f), want, "retried")
    assert [c[0] for c in db.index.calls].count("range_search") == 2
    db.index.fail_next_range = 1
    assert db.count_similar(q[0], 0.0, **f) == len(want[0])
    db.index.fail_next_range = 3
    with pytest.raises(ValueError):
        db.find_all_similar(q[0], 0.0, **f)
    db.index.fail_next_range = 3
    with pytest.raises(ValueError):
        db.count_similar(q[0], 0.0, **f)
    db.index.fail_next_range = 0


def test_classes_without_a_range_search_say_so(tmp_path, monkeypatch):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    q = flat.synth(2, D, 12)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("find_all_similar", (q[0], 0.5)), ("find_all_similar_batch", (q, 0.5)), ("count_similar", (q[0], 0.5))):
            with pytest.raises(NotImplementedError, match="range search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


def test_the_wrapper_repeats_both_calls_when_the_index_changes_between_them():
    """FlatIndex.range_search over a scripted range_search_raw: the second (larger) call reporting other counts than the
    first — rows added or removed in between — makes the wrapper start over; an index that keeps changing is a ValueError,
    the class the database layer retries."""
    from minivectordb_amd import _native

    class Scripted(_native.FlatIndex):
        def __init__(self, script):
            self.d, self.script, self.raw_calls = 4, list(script), []

        def __del__(self):
            pass

        def range_search_raw(self, q, threshold, cap, rowset=None, normalize_q=False, out=None):
            counts = np.asarray(self.script.pop(0), np.int64)
            self.raw_calls.append((q.shape[0], cap))
            D = np.tile(np.arange(cap, 0, -1, dtype=np.float32), (len(counts), 1))
            I = np.tile(np.arange(cap, dtype=np.int64), (len(counts), 1))
            for i, c in enumerate(counts):
                if c > cap:
                    D[i], I[i] = -3.4028234663852886e38, -1
            return counts, D, I

    q = np.zeros((2, 4), np.float32)
    idx = Scripted([[2, 5], [6], [2, 6], [6]])                  # 5 matches, then 6 in the larger call: both calls again
    lims, D, I = idx.range_search(q, 0.0, cap=3)
    assert idx.raw_calls == [(2, 3), (1, 5), (2, 3), (1, 6)]
    assert lims.tolist() == [0, 2, 8] and I.tolist() == [0, 1, 0, 1, 2, 3, 4, 5] and (I >= 0).all()
    idx = Scripted([[2, 5], [6], [2, 6], [7], [2, 7], [8]])
    with pytest.raises(ValueError, match="kept changing"):
        idx.range_search(q, 0.0, cap=3)
    assert len(idx.raw_calls) == 6
