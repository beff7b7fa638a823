"""find_most_similar_boosted on the CPU oracle stand-in: the host half (value extraction, the chain order, id_boosts, the
filters, clamps, argument errors, packaging, the column cache, the retry after a stale-object ValueError) — and the checks of
tests/boost_oracle.py, the contract the GPU tests hold the device to."""
import numpy as np
import pytest

from boost_oracle import boosted, combine
from maxsim_oracle import MISSING
from oracle import flat
from oracle_backend import OracleIndex
from test_examples_cpu import agrees, bits, unit
from test_grouped_cpu import FILTERS
from test_update_cpu import UpdatableOracleIndex

N, D = 300, 16
NAN, INF = np.float32(np.nan), np.float32(np.inf)


class _OracleTerm:
    def __init__(self, values, gen):
        self.values, self.gen = values, gen

    def __len__(self):
        return len(self.values)

    def free(self):
        pass


class BoostOracleIndex(UpdatableOracleIndex):
    """OracleIndex + rowterm / search_boosted: the contract of mvdb_index_search_boosted as a loop — per query the oracle's
    full ranking of the selected rows, scattered by row number, then tests/boost_oracle.py."""
    fail_next_boosted = 0

    def rowterm(self, values):
        values = np.ascontiguousarray(values, dtype=np.float32).copy()
        self.calls.append(("rowterm", len(values)))
        if values.shape != (self.x.shape[0],):
            raise ValueError(f"a row term needs one value per stored row ({len(values)} values, {self.x.shape[0]} rows)")
        return _OracleTerm(values, getattr(self, "renumbered", 0))

    def search_boosted(self, q, k, terms, weights, score_weight=1.0, sparse_rows=None, sparse_values=None, rowset=None, normalize_q=False):
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        terms, weights = list(terms), [float(w) for w in np.asarray(weights, dtype=np.float32).reshape(-1)]
        rows = [] if sparse_rows is None else [int(r) for r in sparse_rows]
        values = [] if sparse_values is None else [float(v) for v in sparse_values]
        self.calls.append(("search_boosted", q.shape[0], int(k), [t.values for t in terms], weights, dict(zip(rows, values)), rowset is not None))
        if self.fail_next_boosted:
            self.fail_next_boosted -= 1
            raise ValueError("the row set was built for another state of the index")
        n = self.x.shape[0]
        if not 1 <= k <= 64 or len(terms) > 4 or len(terms) != len(weights) or len(rows) != len(values) or not (terms or rows):
            raise ValueError("boosted search needs 1 <= k <= 64, 0 to 4 terms, something to boost by")
        if rows and (q.shape[0] != 1 or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= n):
            raise ValueError("boosted search: sparse entries belong to a single query, their rows are distinct and inside the index")
        for t in terms:
            if len(t) != n or t.gen != getattr(self, "renumbered", 0):
                raise ValueError(f"boosted search: term holds {len(t)} rows, the index {n}")
        if rowset is not None and (rowset.n > n or rowset.gen != getattr(self, "renumbered", 0)):
            raise ValueError("the row set was built for another state of the index")
        T = combine([t.values for t in terms], weights, n, (rows, values) if rows else None)
        count = n if rowset is None else len(rowset)
        Ds = np.full((q.shape[0], k), MISSING, np.float32)
        Is = np.full((q.shape[0], k), -1, np.int64)
        for i in range(q.shape[0] if count else 0):
            if rowset is None:
                Dr, Ir = OracleIndex.search(self, q[i:i + 1], count, normalize_q=normalize_q)
            else:
                Dr, Ir = OracleIndex.search_rowset(self, q[i:i + 1], count, rowset, normalize_q=normalize_q)
            s = np.full(n, np.nan, np.float32)
            s[Ir[0][Ir[0] >= 0]] = Dr[0][Ir[0] >= 0]
            Ds[i], Is[i] = boosted(s, T, score_weight, k)
        return Ds, Is


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", BoostOracleIndex)


# ---- the oracle's own properties ----------------------------------------------------------------------------------------------

def test_oracle_negative_zero_column_changes_no_bit():
    rng = np.random.default_rng(1)
    s = rng.standard_normal(500).astype(np.float32)
    s[:6] = [0.0, -0.0, INF, -INF, 1e-45, -1e-45]
    T = combine([np.full(500, -0.0, np.float32)], [1.0], 500)
    assert (bits(T) == 0x80000000).all()
    D, I = boosted(s, T, 1.0, 500)
    assert np.array_equal(bits(D), bits(s[I])) and sorted(I.tolist()) == list(range(500))
    assert bits(D[I == 0]).tolist() == [0] and bits(D[I == 1]).tolist() == [0x80000000]      # +0.0 stays +0.0, -0.0 stays -0.0
    assert I[0] == 2 and I[-1] == 3


def test_oracle_chain_order_rounding_and_sparse():
    t = [np.array([0.1, 3.0, 1e8], np.float32), np.array([0.2, -1.0, 1.0], np.float32), np.array([0.3, 7.0, -1e8], np.float32)]
    w = np.array([0.3, -0.7, 1.1], np.float32)
    T = combine(t, w, 3)
    want = [np.float32(np.float32(w[0] * t[0][r]) + np.float32(w[1] * t[1][r])) + np.float32(w[2] * t[2][r]) for r in range(3)]
    assert T.dtype == np.float32 and np.array_equal(bits(T), bits(np.array(want, np.float32)))
    # the order of the chain matters in float32, and the oracle follows the order given
    big = [np.array([1e8], np.float32), np.array([-1e8], np.float32), np.array([1.0], np.float32)]
    assert combine(big, [1.0, 1.0, 1.0], 1)[0] == 1.0 and combine(big[::-1], [1.0, 1.0, 1.0], 1)[0] == 0.0
    # an unfused multiply: the product is rounded before the add (a fused one would differ here)
    a, b = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12)
    fused = np.float32(np.float64(a) * np.float64(b) - 1.0)
    T = combine([np.array([-1.0], np.float32), np.array([b], np.float32)], [1.0, a], 1)
    assert T[0] == np.float32(np.float32(a * b) - np.float32(1.0)) and T[0] != fused
    # sparse entries: added as they are, after the terms; alone they start from +0.0
    T = combine(t[:1], w[:1], 3, ([2, 0], [0.5, -0.25]))
    assert np.array_equal(bits(T), bits(np.array([np.float32(w[0] * t[0][0]) + np.float32(-0.25), w[0] * t[0][1],
                                                  np.float32(w[0] * t[0][2]) + np.float32(0.5)], np.float32)))
    T = combine([], [], 4, ([1], [-0.0]))
    assert bits(T).tolist() == [0, 0, 0, 0]                                            # +0.0 + -0.0 = +0.0


def test_oracle_ties_nan_and_infinities():
    s = np.array([.5, .5, .25, .5, NAN, .75], np.float32)
    T = np.array([0, 0, .25, 0, 9, -.25], np.float32)
    D, I = boosted(s, T, 1.0, 8)
    assert I.tolist() == [0, 1, 2, 3, 5, -1, -1, -1]                                   # every S is 0.5: the lower row; NaN never comes back
    assert bits(D[:5]).tolist() == [bits(np.float32(.5))[()]] * 5 and (D[5:] == MISSING).all()
    assert D.dtype == np.float32 and I.dtype == np.int64
    s = np.array([.1, .2, .3, .4, .5, .6], np.float32)
    T = np.array([INF, -INF, NAN, 0, INF, -INF], np.float32)
    D, I = boosted(s, T, 1.0, 6)
    assert I.tolist() == [0, 4, 3, 1, 5, -1]                                           # +inf first (ties: lower row), -inf last, ahead of padding
    assert bits(D[:5]).tolist() == bits(np.array([INF, INF, .4, -INF, -INF], np.float32)).tolist()
    T = combine([np.array([INF, 1], np.float32), np.array([-INF, 1], np.float32)], [1.0, 1.0], 2)
    assert T[0] != T[0] and boosted(np.array([.9, .1], np.float32), T, 1.0, 2)[1].tolist() == [1, -1]
    D, I = boosted(s, np.zeros(6, np.float32), -1.0, 2)                                # a negative score weight turns the ranking round
    assert I.tolist() == [0, 1] and bits(D).tolist() == bits(np.array([-.1, -.2], np.float32)).tolist()
    assert boosted(s, np.zeros(6, np.float32), 0.5, 1)[0][0] == np.float32(.3)         # (w_s * s) is one float32 multiply


# ---- the Python layer -------------------------------------------------------------------------------------------------------

def metadata(n):
    """`age`: ints and numpy ints, absent on every 11th row; `rating`: floats, numpy floats, and things that are no numbers."""
    out = []
    for i in range(n):
        m = {"bucket": i % 7, "rank": i}
        if i % 100 == 0:
            m["rare"] = "yes"
        if i % 11:
            m["age"] = np.int64(i % 13) if i % 2 else i % 13
        r = i % 9
        m["rating"] = (True if r == 0 else "4.5" if r == 1 else None if r == 2 else np.float32(0.1 * r) if r == 3
                       else np.float64(0.1 * r) if r == 4 else 0.1 * r)
        if i % 17 == 0:
            del m["rating"]
        out.append(m)
    return out


def column(meta, key, missing):
    """What the issue says a row's value is, spelled out a second time."""
    out = []
    for m in meta:
        v = m.get(key)
        real = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
        out.append(np.float32(v) if real else np.float32(missing))
    return np.array(out, np.float32)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=64)
    db.store_embeddings_batch(list(range(n)), flat.synth(n, D, 5), metadata(n))
    return db


def brute(db, q, boosts, id_boosts, score_weight, missing, allowed):
    """float64: {id: S} over the stored ids in `allowed`."""
    ids = sorted(allowed)
    if not ids:
        return {}
    x = unit(np.stack([db.get_vector(u) for u in ids]))
    S = float(np.float32(score_weight)) * (x @ unit(q))
    metas = [db.metadata[db._ids.row(u)] for u in ids]
    for key, w in (boosts or {}).items():
        S = S + float(np.float32(w)) * column(metas, key, missing).astype(np.float64)
    for i, u in enumerate(ids):
        if id_boosts and u in id_boosts:
            S[i] += float(np.float32(id_boosts[u]))
    return dict(zip(ids, S.tolist()))


def separated(want, k):
    """The float64 ranking has no pair closer than 2e-4 around position k: the float32 answer has the same ids."""
    S = np.sort(np.array(list(want.values())))[::-1]
    lo, hi = max(0, min(k, len(S)) - 2), min(len(S), k + 2)
    gaps = -np.diff(S[lo:hi])
    assert not len(gaps) or gaps.min() > 2e-4, ("choose other values: a near-tie at the cut", k, gaps)


def allowed_ids(db, f):
    return set(db.find_most_similar(flat.synth(1, D, 1)[0], k=N, **f)[0])


def boosted_calls(db):
    return [c for c in db.index.calls if c[0] == "search_boosted"]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_boosts_under_every_filter_against_float64(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(1, D, 77)[0]
    boosts = {"age": 0.013, "rating": -0.21}
    id_boosts = {5: 0.31, 77: 0.29, 140: -0.4, 216: 0.33, "nobody": 5.0, 10 ** 6: 5.0}
    for i, f in enumerate(FILTERS):
        f = f or {}
        allowed = allowed_ids(db, f)
        db.index.calls.clear()
        got = db.find_most_similar_boosted(q, boosts, k=6, score_weight=0.8, missing=0.5, **f)
        both = db.find_most_similar_boosted(q, boosts, id_boosts, k=6, missing=0.5, **f)
        ids_only = db.find_most_similar_boosted(q, id_boosts=id_boosts, k=6, **f)
        if not allowed:
            assert got == both == ids_only == ([], [], []) and db.index.calls == []    # zero matches: nothing is searched
            continue
        for res, args in ((got, (boosts, None, 0.8, 0.5)), (both, (boosts, id_boosts, 1.0, 0.5)), (ids_only, (None, id_boosts, 1.0, 0.0))):
            want = brute(db, q, *args, allowed)
            separated(want, 6)
            agrees(res, want, 6, (i, f, args))
            assert set(res[0]) <= allowed                                              # an id the filters exclude is never a result
        calls = boosted_calls(db)
        take = min(6, len(allowed))
        assert [(c[1], c[2], len(c[3]), c[6]) for c in calls] == [(1, take, 2, len(allowed) != N), (1, take, 2, len(allowed) != N),
                                                                 (1, take, 0, len(allowed) != N)]
        assert calls[0][4] == [float(np.float32(0.013)), float(np.float32(-0.21))] and calls[0][5] == {}
        # unknown ids are ignored; the known ones travel as rows, whether the filter selects them or not
        assert calls[1][5] == calls[2][5] == {db._ids.row(u): float(np.float32(v)) for u, v in id_boosts.items() if isinstance(u, int) and u < N}
    assert isinstance(got[0], tuple) and isinstance(got[1], tuple)
    # the boost reaches past any fetched top-k: a row far down the plain ranking wins on S
    plain = db.find_most_similar(q, k=N)
    loser = plain[0][-1]
    got = db.find_most_similar_boosted(q, id_boosts={loser: 3.0}, k=3)
    assert got[0][0] == loser and list(got[0][1:]) == list(plain[0][:2])


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_value_extraction_and_chain_order(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(1, D, 78)[0]
    meta = metadata(N)
    db.find_most_similar_boosted(q, {"rating": 2.0, "age": 0.5, "absent": 1.0}, missing=-1.5)
    (call,) = boosted_calls(db)
    cols = call[3]
    assert call[4] == [2.0, 0.5, 1.0]                                                  # dict order is the order of the chain
    for got, key in zip(cols, ("rating", "age", "absent")):
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(column(meta, key, -1.5))), key
    rating = cols[0]
    assert rating[0] == np.float32(-1.5) and rating[1] == np.float32(-1.5) and rating[2] == np.float32(-1.5)   # bool, str, None
    assert rating[3] == np.float32(0.1 * 3) and rating[4] == np.float32(np.float64(0.1 * 4)) and rating[5] == np.float32(0.5)
    assert rating[17] == np.float32(-1.5) and cols[1][11] == np.float32(-1.5) and cols[1][3] == np.float32(3)   # absent keys
    assert (cols[2] == np.float32(-1.5)).all()
    db.index.calls.clear()
    a = db.find_most_similar_boosted(q, {"age": 0.5, "rating": 2.0}, missing=-1.5)
    (call,) = boosted_calls(db)
    assert call[4] == [0.5, 2.0] and np.array_equal(call[3][0], cols[1]) and np.array_equal(call[3][1], cols[0])
    assert all(type(s) is np.float32 for s in a[1])
    # the scores are the contract's bits: S from the stand-in's own arithmetic
    T = combine([cols[1], cols[0]], [0.5, 2.0], N)
    Dr, Ir = OracleIndex.search(db.index, q[None], N, normalize_q=True)
    s = np.empty(N, np.float32)
    s[Ir[0]] = Dr[0]
    Dw, Iw = boosted(s, T, 1.0, 5)
    assert list(a[0]) == Iw.tolist() and np.array_equal(bits(np.array(a[1], np.float32)), bits(Dw))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_argument_errors_clamp_autocut_and_batch(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
             else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(4, D, 31)
    assert empty.find_most_similar_boosted(q[0], {"age": 1.0}) == ([], [], [])
    assert empty.find_most_similar_boosted_batch(q, {"age": 1.0}) == [([], [], [])] * 4
    with pytest.raises(ValueError):
        empty.find_most_similar_boosted(q[0])
    db = make_db(kind, tmp_path)
    db.find_most_similar(q[0], k=1)
    db.index.calls.clear()
    five = {"a": 1.0, "b": 1.0, "c": 1.0, "d": 1.0, "e": 1.0}
    for bad in (dict(), dict(boosts={}), dict(id_boosts={}), dict(boosts={}, id_boosts={}),            # nothing to boost by
                dict(boosts=five), dict(boosts={"age": 1.0}, k=0), dict(boosts={"age": 1.0}, k=-2),
                dict(boosts={"age": 1.0}, missing=float("nan"))):
        with pytest.raises(ValueError):
            db.find_most_similar_boosted(q[0], **bad)
    with pytest.raises(ValueError, match="exceeds 64"):
        db.find_most_similar_boosted(q[0], {"age": 1.0}, k=65)
    with pytest.raises(ValueError, match="dimension"):
        db.find_most_similar_boosted(np.zeros(D + 1, np.float32), {"age": 1.0})
    with pytest.raises(ValueError):
        db.find_most_similar_boosted_batch(q[0], {"age": 1.0})                         # not [nq, d]
    with pytest.raises(ValueError):
        db.find_most_similar_boosted_batch(q, {})
    with pytest.raises(TypeError):
        db.find_most_similar_boosted_batch(q, {"age": 1.0}, id_boosts={1: 1.0})        # the batch takes no id_boosts
    assert db.index.calls == []                                                        # nothing reached the index, nothing was retried
    # k is clamped to the rows selected
    rare = {"metadata_filter": {"rare": "yes"}}
    got = db.find_most_similar_boosted(q[0], {"age": 0.1}, k=40, **rare)
    assert boosted_calls(db)[-1][2] == 3 and sorted(got[0]) == [0, 100, 200]
    assert db.find_most_similar_boosted(q[0], {"age": 0.1}, k=64)[0].__len__() == 64
    # every boosted id is unknown, or outside the filter: the plain ranking
    plain = db.find_most_similar(q[0], k=5)
    got = db.find_most_similar_boosted(q[0], id_boosts={"nobody": 1.0}, k=5)
    assert list(got[0]) == list(plain[0]) and np.allclose(got[1], plain[1], atol=1e-6)
    got = db.find_most_similar_boosted(q[0], id_boosts={7: 50.0}, k=3, **rare)         # 7 is outside the filter: still never a result
    assert sorted(got[0]) == [0, 100, 200]
    # autocut: a cliff behind two boosted rows
    base = db.find_most_similar_boosted(q[0], id_boosts={20: 5.0, 21: 8.0}, k=10)
    cut = db.find_most_similar_boosted(q[0], id_boosts={20: 5.0, 21: 8.0}, k=10, autocut=True)
    assert isinstance(cut[0], list) and cut[0] == [21, 20] == list(base[0][:2]) and cut[1] == list(base[1][:2]) and cut[2] == list(base[2][:2])
    # the batch equals the singles
    boosts = {"age": 0.02, "rating": 0.3}
    for f in (FILTERS[0], FILTERS[1], FILTERS[4], FILTERS[7], FILTERS[9]):
        f = f or {}
        db.index.calls.clear()
        batch = db.find_most_similar_boosted_batch(q, boosts, k=7, score_weight=0.9, missing=0.25, **f)
        assert len(boosted_calls(db)) == (1 if allowed_ids(db, f) else 0) and len(batch) == 4
        for i in range(4):
            single = db.find_most_similar_boosted(q[i], boosts, k=7, score_weight=0.9, missing=0.25, **f)
            assert batch[i] == single and type(batch[i][0]) is type(single[0]), (f, i)
    assert db.find_most_similar_boosted_batch(np.zeros((0, D), np.float32), boosts) == []


def rowterm_calls(db):
    return [c for c in db.index.calls if c[0] == "rowterm"]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_the_column_cache_follows_the_writes(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(1, D, 79)[0]
    first = db.find_most_similar_boosted(q, {"age": 0.02, "rating": 0.1})
    assert [c[1] for c in rowterm_calls(db)] == [N, N]
    assert db.find_most_similar_boosted(q, {"age": 0.02, "rating": 0.1}) == first      # a repeated call uploads nothing
    db.find_most_similar_boosted(q, {"rating": -1.0}, k=9, metadata_filter={"bucket": 2})
    assert len(rowterm_calls(db)) == 2
    db.find_most_similar_boosted(q, {"age": 0.02}, missing=1.0)                        # another `missing` is another column
    assert len(rowterm_calls(db)) == 3
    # an embedding-only update keeps the columns, and the search sees the new row
    db.update_embedding(250, embedding=q)
    got = db.find_most_similar_boosted(q, {"age": 0.0}, k=1)
    assert got[0][0] == 250 and len(rowterm_calls(db)) == 3
    # a metadata update, a store and a delete each rebuild a column on its next use — once
    db.update_embedding(250, metadata_dict={"bucket": 5, "rank": 250, "age": 1000})
    got = db.find_most_similar_boosted(flat.synth(1, D, 80)[0], {"age": 0.02}, k=1)
    assert got[0][0] == 250 and len(rowterm_calls(db)) == 4
    db.find_most_similar_boosted(q, {"age": 0.02}, k=1)
    assert len(rowterm_calls(db)) == 4
    db.store_embedding(10_000, flat.synth(1, D, 81)[0], {"bucket": 1, "rank": 10_000, "age": 2000})
    got = db.find_most_similar_boosted(q, {"age": 0.02}, k=2)
    assert list(got[0]) == [10_000, 250] and [c[1] for c in rowterm_calls(db)][4:] == [N + 1]
    if kind == "flat":
        db.delete_embedding(10_000)
    else:
        db.delete_embeddings_batch([10_000])
    got = db.find_most_similar_boosted(q, {"age": 0.02}, id_boosts={10_000: 9.0}, k=2)
    assert got[0][0] == 250 and [c[1] for c in rowterm_calls(db)][5:] == [N]
    # at most eight columns stay: the ninth key evicts the least recently used one
    n0 = len(rowterm_calls(db))
    for j in range(8):
        db.find_most_similar_boosted(q, {f"key{j}": 1.0}, k=1)
    assert len(rowterm_calls(db)) == n0 + 8 and len(db.__dict__["_boost_columns"]) == 8
    db.find_most_similar_boosted(q, {"key7": 1.0, "key0": 1.0}, k=1)
    assert len(rowterm_calls(db)) == n0 + 8                                            # both still resident
    db.find_most_similar_boosted(q, {"age": 0.02}, k=1)                                # evicted by the eight: built again
    assert len(rowterm_calls(db)) == n0 + 9


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_object_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(1, D, 82)[0]
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_most_similar_boosted(q, {"age": 0.02}, {5: 1.0}, **f)
    db.index.fail_next_boosted = 1
    db.index.calls.clear()
    got = db.find_most_similar_boosted(q, {"age": 0.02}, {5: 1.0}, **f)
    assert got == want and len(boosted_calls(db)) == 2 and not rowterm_calls(db)        # the terms are looked up again, not rebuilt
    db.index.fail_next_boosted = 3
    with pytest.raises(ValueError):
        db.find_most_similar_boosted(q, {"age": 0.02}, **f)
    db.index.fail_next_boosted = 0
    # a term that the index refuses as stale (rows were added behind the database's back) is a ValueError after the retries
    stale = db.__dict__["_boost_columns"][("age", 0.0)]
    db.index.x = np.vstack([db.index.x, db.index.x[:1]])
    with pytest.raises(ValueError, match=f"holds {N} rows, the index {N + 1}"):
        db.index.search_boosted(q, 1, [stale[2]], [1.0])
    db.index.x = db.index.x[:N].copy()
    # an index without the method is told so, not retried
    db.index.__class__ = OracleIndex
    with pytest.raises(NotImplementedError, match="boosted search"):
        db.find_most_similar_boosted(q, {"age": 0.02})


@pytest.mark.parametrize("kind", ["plain", "sharded"])
def test_the_gpu_parity_cases_have_no_near_tie_at_the_cut(tmp_path, backend, kind):
    """tests/test_boost_db_gpu.py holds the device to a float64 brute force; its inputs are chosen so that the float64 ranking
    has no pair closer than 2e-4 around position k.  Checked here, where no GPU is needed — and the stand-in passes them."""
    import test_boost_db_gpu as G
    db = G.make_db(kind, tmp_path)
    n = 0
    for f, q, k, w_s, missing, want in G.float64_cases(db):
        if want:
            separated(want, k)
            agrees(db.find_most_similar_boosted(q, G.BOOSTS, k=k, score_weight=w_s, missing=missing, **f), want, k, (f, k))
            n += 1
    assert n == 18


def test_classes_without_a_boosted_search_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        obj = obj if obj is not None else object.__new__(cls)
        with pytest.raises(NotImplementedError, match="boosted search"):
            cls.find_most_similar_boosted(obj, np.zeros(D, np.float32), {"age": 1.0})
        with pytest.raises(NotImplementedError, match="boosted search"):
            cls.find_most_similar_boosted_batch(obj, np.zeros((2, D), np.float32), {"age": 1.0})


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_rowterm_create", "mvdb_rowterm_rows", "mvdb_rowterm_free", "mvdb_index_search_boosted",
                 "mvdb_index_search_boosted_device", "mvdb_index_boost_combine", "mvdb_index_boost_counters"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    for name in ("rowterm", "search_boosted", "search_boosted_device", "boost_combine", "boost_counters"):
        assert callable(getattr(_native.FlatIndex, name))
    assert callable(_native.RowTerm.free)
