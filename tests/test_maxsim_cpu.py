"""find_most_similar_maxsim / find_most_similar_maxsim_batch on the CPU oracle stand-in: the host half (the question's shape,
grouping by a metadata key, missing-key singletons, filters, clamps, argument errors, packaging, the grouping cache, the retry
after a stale-object ValueError) — and the checks of tests/maxsim_oracle.py, the contract the GPU tests hold the device to."""
import numpy as np
import pytest

from maxsim_oracle import MISSING, maxsim, order_image
from oracle import flat
from oracle_backend import OracleIndex
from test_distinct_cpu import DistinctOracleIndex, group_of, make_db
from test_grouped_cpu import FILTERS

N, D, T = 300, 16, 3
NAN, INF = np.float32(np.nan), np.float32(np.inf)


class MaxsimOracleIndex(DistinctOracleIndex):
    """DistinctOracleIndex + search_maxsim: the contract of mvdb_index_search_maxsim as a loop — per query vector the
    oracle's full ranking of the selected rows, scattered into a [T, n] matrix, then tests/maxsim_oracle.py."""
    fail_next_maxsim = 0

    def search_maxsim(self, q, k, grouping, rowset=None, normalize_q=False, with_tokens=True):
        q = np.asarray(q, dtype=np.float32)
        self.calls.append(("search_maxsim", q.shape[0], int(k), rowset is not None))
        if self.fail_next_maxsim:
            self.fail_next_maxsim -= 1
            raise ValueError("the grouping was built for another state of the index")
        if q.ndim != 2 or q.shape[1] != self.d or not 1 <= q.shape[0] <= 256 or not 1 <= k <= 64:
            raise ValueError("MaxSim search needs a [T, d] question, 1 <= T <= 256, 1 <= k <= 64")
        if len(grouping) != self.x.shape[0] or grouping.gen != getattr(self, "renumbered", 0):
            raise ValueError("the grouping was built for another state of the index")
        n = self.x.shape[0]
        selection = np.arange(n, dtype=np.int64) if rowset is None else np.asarray(rowset.rows, dtype=np.int64)
        scores = np.full((q.shape[0], n), np.nan, np.float32)
        for t in range(q.shape[0]):
            if rowset is None:
                Dr, Ir = OracleIndex.search(self, q[t:t + 1], len(selection), normalize_q=normalize_q)
            else:
                Dr, Ir = OracleIndex.search_rowset(self, q[t:t + 1], len(selection), rowset, normalize_q=normalize_q)
            scores[t, Ir[0][Ir[0] >= 0]] = Dr[0][Ir[0] >= 0]
        Dm, G, I_tok, D_tok = maxsim(scores, grouping.codes, selection, k)
        return (Dm, G, I_tok, D_tok) if with_tokens else (Dm, G, None, None)


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", MaxsimOracleIndex)


def brute(db, q, key, k, f):
    """float64 over the stored rows the filter selects: [(sum, [row of each vector])] of the k best groups, best first."""
    allowed = sorted(db.find_most_similar(q[0], k=10 ** 6, **f)[0])
    if not allowed:
        return []
    x = np.stack([db.get_vector(u) for u in allowed]).astype(np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    s = qn @ x.T                                                          # [T, rows]
    meta = dict(zip(db._ids.uids, db.metadata))
    groups = {}
    for j, u in enumerate(allowed):
        groups.setdefault(group_of(meta[u], key, u), []).append(j)
    out = []
    for members in groups.values():
        pick = [members[int(np.argmax(s[t, members]))] for t in range(len(q))]
        out.append((float(sum(s[t, j] for t, j in enumerate(pick))), [allowed[j] for j in pick]))
    out.sort(key=lambda e: -e[0])
    return out[:k]


def same_as_brute(got, want, what):
    ids, scores, metas = got
    assert len(ids) == len(want) == len(scores) == len(metas), (what, ids, want)
    for j, (s, picked) in enumerate(want):
        assert list(ids[j]) == picked and isinstance(ids[j], tuple), (what, j, ids[j], picked)
        assert type(scores[j]) is np.float32 and abs(float(scores[j]) - s) < 1e-5, (what, j, scores[j], s)
        assert [m["rank"] for m in metas[j]] == picked and isinstance(metas[j], list), (what, j)
    assert [float(s) for s in scores] == sorted((float(s) for s in scores), reverse=True), what


def identical(a, b, what):
    assert len(a) == 3 and len(b) == 3 and list(a[0]) == list(b[0]) and list(a[2]) == list(b[2]), (what, a[0], b[0])
    assert len(a[1]) == len(b[1]) and all(x == y and type(x) is np.float32 for x, y in zip(a[1], b[1])), what


# ---- the helper -------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_oracle_maxima_sums_order_and_padding():
    codes = np.array([0, 0, 1, 1, 2, 3], np.int32)
    s = np.array([[.5, .7, .2, .1, .9, .3],
                  [.4, .1, .6, .8, .0, .3]], np.float32)
    D, G, I, Dt = maxsim(s, codes, np.arange(6), 3)
    want = [np.float32(.7) + np.float32(.4), np.float32(.2) + np.float32(.8), np.float32(.9) + np.float32(.0)]
    assert G.tolist() == [0, 1, 2] and np.array_equal(bits(D), bits(want))
    assert I.tolist() == [[1, 0], [2, 3], [4, 4]] and np.array_equal(bits(Dt[1]), bits([.2, .8]))
    assert D.dtype == np.float32 and G.dtype == np.int32 and I.dtype == np.int64 and Dt.dtype == np.float32
    # fewer groups than k: padding; a selection leaves rows (and whole groups) out
    D, G, I, Dt = maxsim(s, codes, np.array([5, 3]), 4)
    assert G.tolist() == [1, 3, -1, -1] and I.tolist() == [[3, 3], [5, 5], [-1, -1], [-1, -1]]
    assert (D[2:] == MISSING).all() and (Dt[2:] == MISSING).all() and np.array_equal(bits(D[:2]), bits([np.float32(.1) + np.float32(.8), np.float32(.6)]))
    D, G, I, Dt = maxsim(s, codes, np.empty(0, np.int64), 2)
    assert G.tolist() == [-1, -1] and (I == -1).all() and (D == MISSING).all() and (Dt == MISSING).all()
    assert maxsim(s[:1], codes, np.arange(6), 1)[1].tolist() == [2]                  # T = 1: the best row's group


def test_oracle_ties_go_to_the_lower_code_and_the_lower_position():
    codes = np.array([2, 2, 0, 1, 1], np.int32)
    s = np.array([[.5, .5, .5, .5, .25], [.25, .25, .25, .25, .25]], np.float32)
    D, G, I, Dt = maxsim(s, codes, np.arange(5), 3)
    assert G.tolist() == [0, 1, 2] and len(set(bits(D).tolist())) == 1               # equal sums: code order
    assert I.tolist() == [[2, 2], [3, 3], [0, 0]]                                    # equal rows of a group: the lower row
    D, G, I, Dt = maxsim(s, codes, np.array([4, 3, 1, 0, 2]), 3)                     # a list: the lower LIST position
    assert G.tolist() == [0, 1, 2] and I.tolist() == [[2, 2], [3, 4], [1, 1]]


def test_oracle_nan_infinities_and_signed_zero():
    codes = np.array([0, 1, 1, 2, 3, 4], np.int32)
    s = np.array([[NAN, NAN, .5, INF, INF, -INF],
                  [.1, .2, NAN, .3, -INF, -INF]], np.float32)
    D, G, I, Dt = maxsim(s, codes, np.arange(6), 6)
    # group 0 has no offer for vector 0; group 1 takes each vector from the row that is not NaN; group 3 sums to NaN
    assert G.tolist() == [2, 1, 4, -1, -1, -1] and D[0] == INF and D[2] == -INF and not np.isnan(D).any()
    assert I[1].tolist() == [2, 1] and np.array_equal(bits(D[1]), bits([np.float32(.5) + np.float32(.2)]))
    s1 = s.copy()
    s1[1] = NAN                                                                       # a vector nobody is offered for: nothing
    assert maxsim(s1, codes, np.arange(6), 2)[1].tolist() == [-1, -1]
    # -0.0 ranks below +0.0, inside a group and between groups; sums keep their sign (-0.0 + -0.0 = -0.0)
    z = np.array([[-0.0, 0.0, -0.0], [-0.0, 0.0, -0.0]], np.float32)
    D, G, I, Dt = maxsim(z, np.array([0, 0, 1], np.int32), np.arange(3), 2)
    assert G.tolist() == [0, 1] and I.tolist() == [[1, 1], [2, 2]] and bits(D).tolist() == [0, 0x80000000]
    assert order_image(np.array([-INF, -1, -0.0, 0.0, 1, INF], np.float32)).tolist() == sorted(
        order_image(np.array([-INF, -1, -0.0, 0.0, 1, INF], np.float32)).tolist())


# ---- the Python layer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_maxsim_by_key_under_every_filter(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    pool = flat.synth(len(FILTERS) * T, D, 16).reshape(len(FILTERS), T, D)
    pool[0, 0] = db.get_vector(39)
    pool[0, 1] = db.get_vector(200)
    spread = 0
    for i, f in enumerate(FILTERS):
        f = f or {}
        q = pool[i]
        allowed = set(db.find_most_similar(q[0], k=N, **f)[0])
        db.index.calls.clear()
        got = db.find_most_similar_maxsim(q, "doc", k=5, **f)
        if not allowed:
            assert got == ([], [], []) and db.index.calls == []                       # zero matches: nothing is searched
            continue
        (call,) = [c for c in db.index.calls if c[0] == "search_maxsim"]
        assert call == ("search_maxsim", T, min(5, len(allowed)), len(allowed) != N)
        same_as_brute(got, brute(db, q, "doc", 5, f), (i, f))
        for ids, metas in zip(got[0], got[2]):
            assert set(ids) <= allowed and len({group_of(m, "doc", u) for u, m in zip(ids, metas)}) == 1     # chunks of ONE group
            spread += len(set(ids)) > 1
        assert len({group_of(m[0], "doc", u[0]) for u, m in zip(got[0], got[2])}) == len(got[0])            # one entry per group
    assert spread >= 1                                                                # some group answered two vectors with two rows


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_missing_keys_are_singletons_and_the_unhashable_value(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(T, D, 17)
    ids, scores, metas = db.find_most_similar_maxsim(q, "doc", k=64)
    assert len(ids) == 50 + 6                                                         # 50 documents and the 6 rows without one
    lone = {u for u in range(N) if u % 50 == 7}
    assert {u[0] for u in ids if len(set(u)) == 1 and u[0] in lone} == lone           # each is a group of its own row
    same_as_brute((ids, scores, metas), brute(db, q, "doc", 64, {}), "doc")
    # a key nobody has: every row its own group — one row answers every vector
    ids, scores, metas = db.find_most_similar_maxsim(q, "nobody", k=7)
    assert all(len(set(u)) == 1 for u in ids)
    same_as_brute((ids, scores, metas), brute(db, q, "nobody", 7, {}), "nobody")
    db.update_embedding(11, metadata_dict={"doc": ["a", "list"], "bucket": 4, "rank": 11})
    db.index.calls.clear()
    with pytest.raises(TypeError, match=r"id 11\b"):
        db.find_most_similar_maxsim(q, "doc", k=3)
    assert [c for c in db.index.calls if c[0] == "search_maxsim"] == []
    with pytest.raises(TypeError):
        db.find_most_similar_maxsim(q, ["unhashable", "key"], k=3)
    assert len(db.find_most_similar_maxsim(q, "bucket", k=10)[0]) == 7               # other keys are unaffected


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_clamps_and_argument_errors(tmp_path, backend, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    empty = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
             else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(T, D, 18)
    assert empty.find_most_similar_maxsim(q, "doc") == ([], [], [])
    assert empty.find_most_similar_maxsim_batch([q, q[:1]], "doc", metadata_filter={"a": 1}) == [([], [], [])] * 2
    with pytest.raises(ValueError):
        empty.find_most_similar_maxsim(q, "doc", k=0)                                 # a bad argument is an error whatever the database holds
    db = make_db(kind, tmp_path)
    db.find_most_similar(q[1], k=1)

    def shape(**kw):
        db.index.calls.clear()
        got = db.find_most_similar_maxsim(q, "doc", **kw)
        (call,) = [c for c in db.index.calls if c[0] == "search_maxsim"]
        return call[1:3], got

    assert shape()[0] == (T, 5)
    assert shape(k=64)[0] == (T, 64)
    rare = {"metadata_filter": {"rare": "yes"}}
    (t, take), got = shape(k=40, **rare)
    assert (t, take) == (T, 3) and sorted(u for ids in got[0] for u in set(ids)) == [0, 100, 200]      # k clamped to the rows selected
    assert len(db.find_most_similar_maxsim(q, "doc", k=200, **rare)[0]) == 3
    db.index.calls.clear()
    with pytest.raises(ValueError, match="exceeds 64"):
        db.find_most_similar_maxsim(q, "doc", k=65)
    assert db.index.calls == []                                                       # raised once: nothing searched, no retry
    wrong = flat.synth(T, D + 1, 18)
    for bad in (dict(embeddings=wrong), dict(embeddings=q[0]), dict(embeddings=q[None]), dict(embeddings=np.empty((0, D), np.float32)),
                dict(embeddings=np.zeros((257, D), np.float32)), dict(embeddings=q, k=0), dict(embeddings=q, k=-2)):
        with pytest.raises(ValueError):
            db.find_most_similar_maxsim(group_by="doc", **bad)
    with pytest.raises(ValueError):
        db.find_most_similar_maxsim_batch([q, wrong], "doc")
    with pytest.raises(ValueError):
        db.find_most_similar_maxsim_batch(q, "doc")                                   # a 2-D array is a list of 1-D "questions"
    assert db.index.calls == []                                                       # nothing reached the index
    assert db.find_most_similar_maxsim_batch([], "doc") == []
    db.index.calls.clear()
    db.find_most_similar_maxsim(np.tile(q, (86, 1))[:256], "doc", k=2)                # T = 256 is accepted
    assert [c[1] for c in db.index.calls if c[0] == "search_maxsim"] == [256]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_batch_equals_the_loop_of_single_calls(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    questions = [flat.synth(t, D, 20 + t) for t in (1, 3, 2, 7)]
    questions[1][0] = db.get_vector(40)
    db.find_most_similar(questions[0][0], k=1)                                        # (the device index is built by the first search)
    for f in FILTERS:
        f = f or {}
        db.index.calls.clear()
        many = db.find_most_similar_maxsim_batch(questions, "doc", k=4, **f)
        assert len(many) == len(questions)
        assert [c[1] for c in db.index.calls if c[0] == "search_maxsim"] in ([], [1, 3, 2, 7])       # one device call per question
        for i, q in enumerate(questions):
            identical(many[i], db.find_most_similar_maxsim(q, "doc", k=4, **f), (i, f))
            same_as_brute(many[i], brute(db, q, "doc", 4, f), (i, f))


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_the_grouping_cache_is_shared_with_distinct_search(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(T, D, 21)

    def uploads():
        return [c for c in db.index.calls if c[0] == "grouping"]

    db.find_most_similar_maxsim(q, "doc")
    assert len(uploads()) == 1
    db.index.calls.clear()
    db.find_most_similar_maxsim(q[:2], "doc", metadata_filter={"bucket": 2})
    db.find_most_similar_distinct(q[0], "doc")                                        # the same resident codes serve both searches
    db.find_most_similar_maxsim_batch([q, q[:1]], "doc")
    assert uploads() == []
    db.store_embedding(10_000, db.get_vector(39), {"doc": "d6", "bucket": 2, "rank": 10_000})
    db.index.calls.clear()
    got = db.find_most_similar_maxsim(q, "doc", k=8)
    assert len(uploads()) == 1 and uploads()[0][1] == N + 1
    same_as_brute(got, brute(db, q, "doc", 8, {}), "store")
    if kind == "flat":
        db.delete_embedding(39)
    else:
        db.delete_embeddings_batch([39])
    db.index.calls.clear()
    got = db.find_most_similar_maxsim(q, "doc", k=8)
    assert len(uploads()) == 1 and uploads()[0][1] == N and all(39 not in u for u in got[0])
    same_as_brute(got, brute(db, q, "doc", 8, {}), "delete")


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_object_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(T, D, 22)
    f = {"metadata_filter": {"bucket": 3}}
    want = db.find_most_similar_maxsim(q, "doc", **f)
    db.index.fail_next_maxsim = 1
    db.index.calls.clear()
    identical(db.find_most_similar_maxsim(q, "doc", **f), want, "retried")
    assert [c[0] for c in db.index.calls].count("search_maxsim") == 2
    db.index.fail_next_maxsim = 3
    with pytest.raises(ValueError):
        db.find_most_similar_maxsim(q, "doc", **f)
    db.index.fail_next_maxsim = 0
    # an index without the method is told so, not retried
    db.index.__class__ = DistinctOracleIndex
    with pytest.raises(NotImplementedError, match="MaxSim search"):
        db.find_most_similar_maxsim(q, "doc")


def test_classes_without_a_maxsim_search_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    q = flat.synth(T, D, 23)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("find_most_similar_maxsim", (q, "doc")), ("find_most_similar_maxsim_batch", ([q], "doc"))):
            with pytest.raises(NotImplementedError, match="MaxSim search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


def test_native_bindings_exist():
    from minivectordb_amd import _native
    for name in ("mvdb_index_search_maxsim", "mvdb_index_search_maxsim_device", "mvdb_index_maxsim_counters"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    for name in ("search_maxsim", "search_maxsim_device", "maxsim_counters"):
        assert callable(getattr(_native.FlatIndex, name))
