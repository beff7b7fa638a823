"""find_most_similar_by_examples on the CPU oracle stand-in: the host half (examples by id and by vector, the skip rows, the
filters, clamps, argument errors, packaging, the average-vector strategy, the retry after a stale-object ValueError) — and the
checks of tests/examples_oracle.py, the contract the GPU tests hold the device to."""
import numpy as np
import pytest

from examples_oracle import branches, examples
from maxsim_oracle import MISSING
from oracle import flat
from oracle_backend import OracleIndex
from test_distinct_cpu import make_db
from test_grouped_cpu import FILTERS

N, D = 300, 16
NAN, INF = np.float32(np.nan), np.float32(np.inf)


class ExamplesOracleIndex(OracleIndex):
    """OracleIndex + search_examples: the contract of mvdb_index_search_examples as a loop — per example the oracle's full
    ranking of the selected rows, scattered into a [P + N, n] matrix, then tests/examples_oracle.py."""
    fail_next_examples = 0

    def search_examples(self, positives, negatives, k, rowset=None, skip_rows=None, normalize=False):
        p = np.asarray(positives, dtype=np.float32)
        m = np.empty((0, self.d), np.float32) if negatives is None or not len(negatives) else np.asarray(negatives, dtype=np.float32)
        skip = [] if skip_rows is None else [int(r) for r in skip_rows]
        self.calls.append(("search_examples", p.shape[0], m.shape[0], int(k), rowset is not None, sorted(skip)))
        if self.fail_next_examples:
            self.fail_next_examples -= 1
            raise ValueError("the row set was built for another state of the index")
        if p.ndim != 2 or p.shape[1] != self.d or p.shape[0] < 1 or p.shape[0] + m.shape[0] > 256 or not 1 <= k <= 64:
            raise ValueError("search by examples needs 1 <= P, P + N <= 256, 1 <= k <= 64")
        n = self.x.shape[0]
        if any(r < 0 or r >= n for r in skip) or len(skip) > 1024:
            raise ValueError("search by examples: skip row outside the index")
        if rowset is not None and (rowset.n > n or rowset.gen != getattr(self, "renumbered", 0)):
            raise ValueError("the row set was built for another state of the index")
        v = np.concatenate([p, m])
        count = n if rowset is None else len(rowset)
        scores = np.full((v.shape[0], n), np.nan, np.float32)
        for j in range(v.shape[0] if count else 0):
            if rowset is None:
                Dr, Ir = OracleIndex.search(self, v[j:j + 1], count, normalize_q=normalize)
            else:
                Dr, Ir = OracleIndex.search_rowset(self, v[j:j + 1], count, rowset, normalize_q=normalize)
            scores[j, Ir[0][Ir[0] >= 0]] = Dr[0][Ir[0] >= 0]
        return examples(scores, p.shape[0], k, skip)


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", ExamplesOracleIndex)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def brute(db, pos, neg, allowed, excluded=()):
    """float64: {id: S} over the stored ids in `allowed` minus `excluded`, by the rule."""
    ids = [u for u in allowed if u not in set(excluded)]
    if not ids:
        return {}
    x = unit(np.stack([db.get_vector(u) for u in ids]))
    bp = (x @ unit(pos).T).max(axis=1)
    bn = (x @ unit(neg).T).max(axis=1) if neg is not None and len(neg) else np.full(len(ids), -np.inf)
    S = np.where(bp > bn, bp, -(bn * bn))
    return dict(zip(ids, S.tolist()))


def agrees(got, want, k, what):
    """`got` is the top k of `want` ({id: S}) up to the 1e-4 parity rule: each score within 1e-4 of its id's S, no id left
    out that beats the last one by more than 2e-4, best first."""
    ids, scores, metas = got
    assert len(ids) == len(scores) == len(metas) == min(k, len(want)), (what, len(ids), len(want))
    for u, s, m in zip(ids, scores, metas):
        assert u in want and abs(float(s) - want[u]) < 1e-4 and m["rank"] == u and type(s) is np.float32, (what, u, s, want.get(u))
    assert all(float(a) >= float(b) for a, b in zip(scores, scores[1:])), what
    assert len(set(ids)) == len(ids), what
    if ids:
        floor = float(scores[-1])
        assert not [u for u, s in want.items() if u not in ids and s > floor + 2e-4], what


# ---- the helper -------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_oracle_rule_order_skip_and_padding():
    s = np.array([[.5, .1, .3, .9, .2, NAN],      # positives
                  [.4, .6, .1, .2, .2, .7],
                  [.3, .7, .2, .1, .8, .1]], np.float32)   # one negative
    D, I = examples(s, 2, 6)
    # row 0: bp .5 > bn .3; row 1: bp .6 <= .7 -> -(.49); row 2: .3 > .2; row 3: .9; row 4: .2 <= .8 -> -(.64); row 5: .7 > .1
    want = [np.float32(.9), np.float32(.7), np.float32(.5), np.float32(.3), -(np.float32(.7) * np.float32(.7)), -(np.float32(.8) * np.float32(.8))]
    assert I.tolist() == [3, 5, 0, 2, 1, 4] and np.array_equal(bits(D), bits(want))
    assert D.dtype == np.float32 and I.dtype == np.int64
    D, I = examples(s, 2, 4, skip=[3, 3, 0])
    assert I.tolist() == [5, 2, 1, 4]                                                  # skip rows are never results, duplicates allowed
    D, I = examples(s, 2, 8, skip=[1])
    assert I.tolist() == [3, 5, 0, 2, 4, -1, -1, -1] and (D[5:] == MISSING).all()
    D, I = examples(s[:2], 2, 3)                                                       # N = 0: the per-row maximum over the positives
    assert I.tolist() == [3, 5, 1] and np.array_equal(bits(D), bits([.9, .7, .6]))
    D, I = examples(s[:1], 1, 6)                                                       # a NaN score: no offer, never a result
    assert I.tolist() == [3, 0, 2, 4, 1, -1]
    assert examples(np.full((2, 4), NAN, np.float32), 1, 2)[1].tolist() == [-1, -1]


def test_oracle_ties_nan_infinities_and_signed_zero():
    s = np.array([[.5, .5, .5, .25], [.5, .5, .1, .25]], np.float32)
    D, I = examples(s, 1, 4)
    # rows 0, 1, 3: bp == bn, not greater -> -(bn * bn); equal S: the lower row
    assert I.tolist() == [2, 3, 0, 1] and np.array_equal(bits(D), bits([.5, -np.float32(.0625), -np.float32(.25), -np.float32(.25)]))
    z = np.array([[-0.0, 0.0, 0.0, -INF, INF, INF, NAN],
                  [0.0, -0.0, NAN, -INF, INF, NAN, .5]], np.float32)
    bp, bn, has = branches(z, 1)
    assert has.tolist() == [True] * 6 + [False] and bn[2] == -INF and bn[5] == -INF
    D, I = examples(z, 1, 7)
    # row 0: -0.0 > 0.0 is false -> -(0 * 0) = -0.0; row 1: 0.0 > -0.0 is false as IEEE -> -(-0.0 * -0.0) = -0.0;
    # row 2: no negative offers, 0.0 > -inf -> +0.0; row 3: -inf > -inf false -> -(inf) = -inf, still a result;
    # row 4: inf > inf false -> -inf; row 5: +inf; row 6: no positive offers — never a result
    assert I.tolist() == [5, 2, 0, 1, 3, 4, -1]
    assert bits(D[:6]).tolist() == bits([INF, 0.0, -0.0, -0.0, -INF, -INF]).tolist() and D[6] == MISSING
    # the maximum over the positives is by order image: +0.0 beats -0.0
    D, I = examples(np.array([[-0.0], [0.0]], np.float32), 2, 1)
    assert bits(D).tolist() == [0]


def test_oracle_against_float64_brute_force():
    rng = np.random.default_rng(3)
    n, d = 400, 24
    x = unit(rng.standard_normal((n, d))).astype(np.float32)
    for P, Nn in ((1, 0), (3, 2), (5, 5), (1, 1)):
        v = unit(x[rng.permutation(n)[:P + Nn]] + 0.4 * rng.standard_normal((P + Nn, d))).astype(np.float32)
        s32 = np.stack([(x * v[j]).sum(axis=1, dtype=np.float32) for j in range(P + Nn)]).astype(np.float32)
        s64 = v.astype(np.float64) @ x.astype(np.float64).T
        bp = s64[:P].max(axis=0)
        bn = s64[P:].max(axis=0) if Nn else np.full(n, -np.inf)
        S = np.where(bp > bn, bp, -(bn * bn))
        D, I = examples(s32, P, 20)
        assert (I >= 0).all() and len(set(I.tolist())) == 20
        assert np.abs(D.astype(np.float64) - S[I]).max() < 1e-4                        # the project's parity rule
        order = np.argsort(-S, kind="stable")
        gaps = np.abs(np.diff(S[order][:21]))
        for j in range(20):                                                            # ids equal away from near-ties
            if (j == 0 or gaps[j - 1] > 1e-5) and gaps[j] > 1e-5:
                assert I[j] == order[j], (P, Nn, j)


# ---- the Python layer -------------------------------------------------------------------------------------------------------

def allowed_ids(db, f):
    return set(db.find_most_similar(flat.synth(1, D, 1)[0], k=N, **f)[0])


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_examples_by_id_and_by_vector_under_every_filter(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    pos_ids, neg_ids = [39, 120, 7], [200, 13]
    pos = np.stack([db.get_vector(u) for u in pos_ids])
    neg = np.stack([db.get_vector(u) for u in neg_ids])
    took_other_branch = 0
    for i, f in enumerate(FILTERS):
        f = f or {}
        allowed = allowed_ids(db, f)
        db.index.calls.clear()
        by_id = db.find_most_similar_by_examples(pos_ids, neg_ids, k=6, **f)
        by_vec = db.find_most_similar_by_examples(positive_embeddings=pos, negative_embeddings=neg, k=6, **f)
        mixed = db.find_most_similar_by_examples(pos_ids[:1], neg_ids[:1], pos[1:], neg[1:], k=6, **f)
        if not allowed:
            assert by_id == by_vec == mixed == ([], [], []) and db.index.calls == []   # zero matches: nothing is searched
            continue
        calls = [c for c in db.index.calls if c[0] == "search_examples"]
        take = min(6, len(allowed))
        rows = sorted(db._ids.row(u) for u in pos_ids + neg_ids)
        assert [c[1:] for c in calls] == [(3, 2, take, len(allowed) != N, rows), (3, 2, take, len(allowed) != N, []),
                                          (3, 2, take, len(allowed) != N, sorted(db._ids.row(u) for u in (39, 200)))]
        # the examples by id never come back — also when the filter would not select them; by vector nothing is excluded
        agrees(by_id, brute(db, pos, neg, allowed, pos_ids + neg_ids), 6, (i, f, "ids"))
        agrees(by_vec, brute(db, pos, neg, allowed), 6, (i, f, "vectors"))
        agrees(mixed, brute(db, pos, neg, allowed, [39, 200]), 6, (i, f, "mixed"))
        assert not set(by_id[0]) & set(pos_ids + neg_ids) and set(by_id[0]) <= allowed
        if set(pos_ids) & allowed:
            assert set(by_vec[0]) & set(pos_ids)                                       # a stored positive is its own best match
        took_other_branch += any(float(s) < 0 for s in by_vec[1])
    # positives alone: the per-row maximum, every topic is answered
    got = db.find_most_similar_by_examples(pos_ids, k=9)
    agrees(got, brute(db, pos, None, set(range(N)), pos_ids), 9, "positives only")
    assert isinstance(got[0], tuple) and isinstance(got[1], tuple)
    # rows near a negative sink: ask for everything a small filter selects
    f = {"metadata_filter": {"bucket": 4}}
    got = db.find_most_similar_by_examples(pos_ids, [200, 11], k=64, **f)
    want = brute(db, pos, np.stack([db.get_vector(200), db.get_vector(11)]), allowed_ids(db, f), pos_ids + [200, 11])
    agrees(got, want, 64, "all of a bucket")
    assert any(float(s) < 0 for s in got[1]) and any(float(s) > 0 for s in got[1])     # both branches of the rule


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_unknown_ids_argument_errors_clamp_and_short_results(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
             else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    v = flat.synth(3, D, 31)
    assert empty.find_most_similar_by_examples(positive_embeddings=v) == ([], [], [])
    with pytest.raises(ValueError):
        empty.find_most_similar_by_examples(positive_embeddings=v, k=0)
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        empty.find_most_similar_by_examples([5])
    db = make_db(kind, tmp_path)
    db.find_most_similar(v[0], k=1)
    db.index.calls.clear()
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        db.find_most_similar_by_examples([39, 10_000])                                 # what get_vector raises
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        db.find_most_similar_by_examples([39], negative_ids=["nobody"])
    for bad in (dict(), dict(negative_ids=[3]), dict(negative_embeddings=v),                                  # no positive
                dict(positive_embeddings=v[0]), dict(positive_embeddings=v[None]),                            # not [m, d]
                dict(positive_embeddings=flat.synth(3, D + 1, 1)), dict(positive_ids=[1], negative_embeddings=flat.synth(2, D + 1, 1)),
                dict(positive_embeddings=np.zeros((257, D), np.float32)),
                dict(positive_ids=[1], negative_embeddings=np.zeros((256, D), np.float32)),                   # P + N = 257
                dict(positive_ids=[1], k=0), dict(positive_ids=[1], k=-3),
                dict(positive_ids=[1], strategy="mean"), dict(positive_ids=[1], strategy=None)):
        with pytest.raises(ValueError):
            db.find_most_similar_by_examples(**bad)
    with pytest.raises(ValueError, match="exceeds 64"):
        db.find_most_similar_by_examples([1], k=65)
    assert db.index.calls == []                                                        # nothing reached the index, nothing was retried
    db.find_most_similar_by_examples(positive_embeddings=np.tile(v, (86, 1))[:200], negative_embeddings=np.tile(v, (20, 1))[:56], k=2)
    assert [c[1:3] for c in db.index.calls if c[0] == "search_examples"] == [(200, 56)]                       # 256 examples are accepted

    def shape(*a, **kw):
        db.index.calls.clear()
        got = db.find_most_similar_by_examples(*a, **kw)
        (call,) = [c for c in db.index.calls if c[0] == "search_examples"]
        return call[3], got

    assert shape([1])[0] == 5 and shape([1], k=64)[0] == 64
    rare = {"metadata_filter": {"rare": "yes"}}
    take, got = shape([1], k=40, **rare)
    assert take == 3 and sorted(got[0]) == [0, 100, 200]                               # k clamped to the rows selected
    take, got = shape([100], [5], k=200, **rare)
    assert take == 3 and sorted(got[0]) == [0, 200]                                    # the skip rows eat into it: a short result
    take, got = shape([0, 100], [200], k=3, **rare)
    assert take == 3 and got == ([], [], [])                                           # every selected row is an example
    take, got = shape([5], [6], k=3, **rare)                                           # examples outside the filter steer it all the same
    assert sorted(got[0]) == [0, 100, 200]
    agrees(got, brute(db, [db.get_vector(5)], [db.get_vector(6)], [0, 100, 200]), 3, "outside")
    take, got = shape([1, 1, 2], [2], k=4)                                             # an id twice, on both sides: skipped once each
    assert not {1, 2} & set(got[0]) and len(got[0]) == 4
    assert [c[5] for c in db.index.calls if c[0] == "search_examples"] == [sorted(db._ids.row(u) for u in (1, 2))]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_autocut_and_writes_are_followed(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    base = db.find_most_similar_by_examples([39], k=30)                                # 36..47 are near-copies of 39: a cliff behind them
    cut = db.find_most_similar_by_examples([39], k=30, autocut=True)
    assert isinstance(cut[0], list) and 0 < len(cut[0]) < 30 and list(base[0][:len(cut[0])]) == cut[0]
    assert set(cut[0]) <= set(range(36, 48)) - {39}
    assert list(base[1][:len(cut[1])]) == cut[1] and list(base[2][:len(cut[2])]) == cut[2]
    # a store, a delete: the next call sees them, and the skip rows follow the renumbering
    db.store_embedding(10_000, db.get_vector(120), {"bucket": 2, "rank": 10_000})
    got = db.find_most_similar_by_examples([120], k=3)
    assert got[0][0] == 10_000 and abs(float(got[1][0]) - 1.0) < 1e-5
    if kind == "flat":
        db.delete_embedding(3)
    else:
        db.delete_embeddings_batch([3])
    db.index.calls.clear()
    got = db.find_most_similar_by_examples([120, 10_000], [200], k=5)
    assert [c[5] for c in db.index.calls if c[0] == "search_examples"] == [[119, 199, N - 1]]
    assert not {120, 10_000, 200, 3} & set(got[0])
    with pytest.raises(ValueError, match="Unique ID does not exist"):
        db.find_most_similar_by_examples([3])


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_average_vector_is_find_most_similar_of_the_mean_minus_the_examples(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    pos_ids, neg_ids = [39, 120, 7], [200, 13]
    db.find_most_similar(flat.synth(1, D, 2)[0], k=1)                                  # (the device index is built by the first search,
    pos = np.stack([np.asarray(db.get_vector(u), np.float32) for u in pos_ids])        #  and get_vector reads the rows as stored from then on)
    neg = np.stack([np.asarray(db.get_vector(u), np.float32) for u in neg_ids])
    for f in (FILTERS[0], FILTERS[1], FILTERS[4], FILTERS[9]):
        f = f or {}
        for ids, nids, q in ((pos_ids, [], pos.mean(axis=0, dtype=np.float32)),
                             (pos_ids, neg_ids, np.float32(2) * pos.mean(axis=0, dtype=np.float32) - neg.mean(axis=0, dtype=np.float32))):
            db.index.calls.clear()
            got = db.find_most_similar_by_examples(ids, nids, k=5, strategy="average_vector", **f)
            (call,) = [c for c in db.index.calls if c[0] == "search_examples"]
            assert call[1:3] == (1, 0) and call[5] == sorted(db._ids.row(u) for u in ids + nids)     # the SAME device call, P = 1, N = 0
            full = db.find_most_similar(q, k=N, **f)
            want = [(u, s, m) for u, s, m in zip(*full) if u not in ids + nids][:5]
            assert list(got[0]) == [w[0] for w in want] and list(got[2]) == [w[2] for w in want], f
            assert all(a == b and type(a) is np.float32 for a, b in zip(got[1], [w[1] for w in want])), f
            by_vec = db.find_most_similar_by_examples(positive_embeddings=pos, negative_embeddings=neg if nids else None, k=5,
                                                      strategy="average_vector", **f)
            assert list(by_vec[0]) == list(full[0][:5])                                # examples by vector exclude nothing
    # the two rules differ: three positives from three topics — the mean sits near none of them
    best = db.find_most_similar_by_examples(pos_ids, k=6)
    mean = db.find_most_similar_by_examples(pos_ids, k=6, strategy="average_vector")
    assert min(float(s) for s in best[1]) > max(float(s) for s in mean[1][1:])


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_object_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_most_similar_by_examples([39, 7], [200], **f)
    db.index.fail_next_examples = 1
    db.index.calls.clear()
    got = db.find_most_similar_by_examples([39, 7], [200], **f)
    assert got == want and [c[0] for c in db.index.calls].count("search_examples") == 2
    db.index.fail_next_examples = 3
    with pytest.raises(ValueError):
        db.find_most_similar_by_examples([39, 7], [200], **f)
    db.index.fail_next_examples = 0
    # an index without the method is told so, not retried
    db.index.__class__ = OracleIndex
    with pytest.raises(NotImplementedError, match="search by examples"):
        db.find_most_similar_by_examples([39])


def test_classes_without_a_search_by_examples_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        with pytest.raises(NotImplementedError, match="search by examples"):
            cls.find_most_similar_by_examples(obj if obj is not None else object.__new__(cls), [1], [2])


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_index_search_examples", "mvdb_index_search_examples_device", "mvdb_index_examples_counters"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    for name in ("search_examples", "search_examples_device", "examples_counters"):
        assert callable(getattr(_native.FlatIndex, name))
