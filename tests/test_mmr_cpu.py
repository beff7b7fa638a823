"""find_most_similar_mmr / find_most_similar_mmr_batch on the CPU oracle stand-in: the host half (clamps, argument errors,
filter semantics, packaging in selection order, the resident row-set cache, the retry after a concurrent delete) — and the
checks of the float64 oracle itself (tests/mmr_oracle.py), which the GPU tests adjudicate the device with."""
import numpy as np
import pytest

import mmr_oracle
from oracle import flat
from oracle_backend import OracleIndex
from test_grouped_cpu import FILTERS

N, D, NQ = 300, 16, 13
MISSING = np.float32(-3.4028234663852886e38)


class MmrOracleIndex(OracleIndex):
    """OracleIndex + search_mmr: the oracle's top-fetch_k search of the selected rows, then mmr_oracle.select over the
    stored rows of those candidates (the contract of mvdb_index_search_mmr as a loop)."""
    fail_next_mmr = 0

    def search_mmr(self, q, k, fetch_k, lambda_mult, rowset=None, normalize_q=False, out=None):
        self.calls.append(("search_mmr", int(k), int(fetch_k), float(lambda_mult), rowset is not None))
        if self.fail_next_mmr:
            self.fail_next_mmr -= 1
            raise ValueError("the row set was built for another state of the index")
        if not (1 <= k <= fetch_k <= 1024) or not (0.0 <= lambda_mult <= 1.0):
            raise ValueError("MMR search needs 1 <= k <= fetch_k <= 1024 and lambda in [0, 1]")
        q = np.atleast_2d(np.asarray(q, dtype=np.float32))
        if rowset is None:
            Dc, Ic = OracleIndex.search(self, q, fetch_k, normalize_q=normalize_q)
        else:
            Dc, Ic = OracleIndex.search_rowset(self, q, fetch_k, rowset, normalize_q=normalize_q)
        Dm = np.full((q.shape[0], k), MISSING, np.float32)
        Im = np.full((q.shape[0], k), -1, np.int64)
        for i in range(q.shape[0]):
            nv = int((Ic[i] >= 0).sum())
            picks = mmr_oracle.select(Dc[i, :nv], self.x[Ic[i, :nv]], k, lambda_mult)
            Dm[i, :len(picks)] = Dc[i, picks]
            Im[i, :len(picks)] = Ic[i, picks]
        return Dm, Im


@pytest.fixture
def backend(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "FlatIndex", MmrOracleIndex)


def make_db(kind, tmp_path, n=N):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=64)
    x = flat.synth(n, D, 5)
    x[40:48] = x[39]                                   # near-copies a plain top-k returns together
    meta = [{"bucket": i % 7, "rank": i, "rare": "yes"} if i % 100 == 0 else {"bucket": i % 7, "rank": i} for i in range(n)]
    db.store_embeddings_batch(list(range(n)), x, meta)
    return db


def same(got, want, what):
    assert type(got) is type(want) and len(got) == 3, what
    assert list(got[0]) == list(want[0]), what
    assert list(got[2]) == list(want[2]), what
    assert len(got[1]) == len(want[1]) and all(x == y and type(x) is type(y) for x, y in zip(got[1], want[1])), what


def selected_ids(db, f):
    f = f or {}
    return set(db.find_most_similar(flat.synth(1, D, 1)[0], k=N, **f)[0])


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_filters_packaging_and_selection_order(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 6)
    q[0] = db.get_vector(39)
    diversified = 0
    for i, f in enumerate(FILTERS):
        f = f or {}
        allowed = selected_ids(db, f)
        db.index.calls.clear()
        got = db.find_most_similar_mmr(q[i], k=5, fetch_k=30, lambda_mult=0.5, **f)
        if not allowed:
            assert got == ([], [], []) and db.index.calls == []      # zero matches: nothing is searched
            continue
        call = [c for c in db.index.calls if c[0] == "search_mmr"]
        assert call == [("search_mmr", min(5, len(allowed)), min(30, len(allowed)), 0.5, len(allowed) != N)], (i, f, call)
        ids, dist, metas = got
        assert isinstance(ids, tuple) and len(ids) == min(5, len(allowed)) == len(set(ids)) and set(ids) <= allowed, (i, f)
        assert all(type(s) is np.float32 for s in dist) and [m["rank"] for m in metas] == list(ids)
        # the candidates are find_most_similar's: the first pick is its best hit, every pick carries that search's score
        wide = db.find_most_similar(q[i], k=30, **f)
        assert ids[0] == wide[0][0]
        score_of = dict(zip(wide[0], wide[1]))
        assert all(score_of[u] == s for u, s in zip(ids, dist)), (i, f)
        # lambda_mult = 1 is the plain search; selection order is not score order once diversity counts
        same(db.find_most_similar_mmr(q[i], k=5, fetch_k=30, lambda_mult=1.0, **f), db.find_most_similar(q[i], k=5, **f), (i, f))
        diversified += list(dist) != sorted(dist, reverse=True) or list(ids) != list(wide[0][:len(ids)])
    assert diversified >= 5
    # the query that sits on 9 identical rows: the plain search returns 5 of them, MMR one
    plain = db.find_most_similar(q[0], k=5)[0]
    mmr = db.find_most_similar_mmr(q[0], k=5, fetch_k=30)[0]
    assert set(plain) <= set(range(39, 48)) and mmr[0] == 39 and len(set(mmr) & set(range(39, 48))) == 1


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_clamps_and_the_default_fetch_k(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 7)

    db.find_most_similar(q[1], k=1)                                     # (the index exists from the first search on)

    def shape(**kw):
        db.index.calls.clear()
        got = db.find_most_similar_mmr(q[0], **kw)
        (call,) = [c for c in db.index.calls if c[0] == "search_mmr"]
        return call[1:3], got

    assert shape()[0] == (5, 20)                                        # fetch_k=None: max(4 k, 20)
    assert shape(k=3)[0] == (3, 20)
    assert shape(k=30)[0] == (30, 120)
    assert shape(k=100)[0] == (100, N)                                  # fetch_k clamped to the rows selected
    assert shape(k=N + 50, fetch_k=2000)[0] == (N, N)                   # ... and k
    rare = {"metadata_filter": {"rare": "yes"}}
    (take, fetch), got = shape(k=5, fetch_k=40, **rare)
    assert (take, fetch) == (3, 3) and sorted(got[0]) == [0, 100, 200]
    big = make_db(kind, tmp_path / "big", n=1100)
    big.find_most_similar_mmr(q[0], k=4, fetch_k=5000)
    assert [c[1:3] for c in big.index.calls if c[0] == "search_mmr"] == [(4, 1024)]       # fetch_k clamped to 1024
    big.index.calls.clear()
    with pytest.raises(ValueError, match="exceeds fetch_k"):
        big.find_most_similar_mmr(q[0], k=1050, fetch_k=1100)           # k stays above the clamped fetch_k
    assert big.index.calls == []                                        # raised once: nothing searched, no retry


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_empty_database_and_argument_errors(tmp_path, backend, monkeypatch, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    db = (VectorDatabase(storage_file=str(tmp_path / "e.pkl")) if kind == "flat"
          else ShardedVectorDatabase(storage_dir=str(tmp_path / "e"), shard_size=64))
    q = flat.synth(3, D, 8)
    assert db.find_most_similar_mmr(q[0]) == ([], [], [])
    assert db.find_most_similar_mmr_batch(q, metadata_filter={"a": 1}) == [([], [], [])] * 3
    with pytest.raises(ValueError):
        db.find_most_similar_mmr(q[0], lambda_mult=2.0)                  # a bad argument is an error whatever the database holds
    db = make_db(kind, tmp_path)
    db.find_most_similar_mmr(q[0])
    db.index.calls.clear()
    evaluated = []
    inner = db._get_filtered_indices
    monkeypatch.setattr(db, "_get_filtered_indices", lambda *a: evaluated.append(a) or inner(*a))
    f = {"metadata_filter": {"bucket": 1}}
    wrong = flat.synth(3, D + 1, 8)
    for bad in (dict(embedding=wrong[0]), dict(embedding=q[0], k=0), dict(embedding=q[0], k=-2), dict(embedding=q[0], fetch_k=0),
                dict(embedding=q[0], k=5, fetch_k=4), dict(embedding=q[0], lambda_mult=-0.1), dict(embedding=q[0], lambda_mult=1.5),
                dict(embedding=q[0], lambda_mult=float("nan"))):
        with pytest.raises(ValueError):
            db.find_most_similar_mmr(**bad, **f)
    with pytest.raises(ValueError):
        db.find_most_similar_mmr_batch(wrong, **f)
    with pytest.raises(ValueError):
        db.find_most_similar_mmr_batch(q[0], **f)                        # 1-D embeddings
    assert db.index.calls == []                                          # nothing reached the index
    assert db.find_most_similar_mmr_batch(np.empty((0, D), np.float32)) == []
    db.find_most_similar_mmr(q[0], **f)
    assert len(evaluated) >= 1                                           # (the spy does see an evaluation)


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_batch_equals_the_loop_of_single_calls(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(NQ, D, 9)
    for f in FILTERS:
        f = f or {}
        many = db.find_most_similar_mmr_batch(q, k=4, fetch_k=25, lambda_mult=0.4, **f)
        assert len(many) == NQ
        for i in range(NQ):
            same(many[i], db.find_most_similar_mmr(q[i], k=4, fetch_k=25, lambda_mult=0.4, **f), (i, f))


def test_the_row_set_cache_is_shared_with_the_other_searches(tmp_path, backend):
    db = make_db("flat", tmp_path)
    q = flat.synth(4, D, 10)
    f = {"metadata_filter": {"bucket": 2}}
    db.find_most_similar(q[0], k=3, **f)
    db.index.calls.clear()
    db.find_most_similar_mmr(q[1], **f)
    db.find_most_similar_mmr_batch(q, **f)
    kinds = [c[0] for c in db.index.calls]
    assert kinds.count("rowset") == 0 and kinds.count("search_mmr") == 2          # resident: no filter evaluation, no upload
    assert all(c[4] for c in db.index.calls if c[0] == "search_mmr")              # ... and both calls went under the set
    db.store_embedding(10_000, flat.synth(1, D, 11)[0], {"bucket": 2})
    db.index.calls.clear()
    db.find_most_similar_mmr(q[0], **f)
    assert [c[0] for c in db.index.calls].count("rowset") == 1
    db.index.calls.clear()
    db.find_most_similar_mmr(q[0])                                                # unfiltered: never a set
    assert [c for c in db.index.calls if c[0] in ("rowset", "search_mmr")] == [("search_mmr", 5, 20, 0.5, False)]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_a_stale_set_is_retried_once_and_raised_after_three(tmp_path, backend, kind):
    db = make_db(kind, tmp_path)
    q = flat.synth(2, D, 12)
    f = {"metadata_filter": {"bucket": 3}}
    db.find_most_similar_mmr(q[0], **f)
    if kind == "flat":
        db.delete_embedding(3)
    else:
        db.delete_embeddings_batch([3])
    after = db.find_most_similar_mmr(q[0], k=N, fetch_k=N, **f)
    assert 3 not in after[0] and len(after[0]) == len(range(3, N, 7)) - 1
    want = db.find_most_similar_mmr(q[0], **f)
    db.index.fail_next_mmr = 1
    db.index.calls.clear()
    same(db.find_most_similar_mmr(q[0], **f), want, "retried")
    assert [c[0] for c in db.index.calls].count("search_mmr") == 2
    db.index.fail_next_mmr = 3
    with pytest.raises(ValueError):
        db.find_most_similar_mmr(q[0], **f)
    db.index.fail_next_mmr = 0


def test_the_factored_loop_still_serves_the_plain_and_the_range_search(tmp_path, backend):
    """_search_selected is shared by find_most_similar and find_all_similar: a stand-in without search_mmr / range_search
    is told so, not retried."""
    db = make_db("flat", tmp_path)
    q = flat.synth(1, D, 13)
    assert len(db.find_most_similar(q[0], k=4, metadata_filter={"bucket": 1})[0]) == 4
    with pytest.raises(NotImplementedError, match="range search"):
        db.find_all_similar(q[0], 0.0)
    db.index.__class__ = OracleIndex
    with pytest.raises(NotImplementedError, match="MMR search"):
        db.find_most_similar_mmr(q[0])


def test_classes_without_an_mmr_search_say_so(tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=64)
    q = flat.synth(2, D, 14)
    for cls, obj in ((ShardedVectorDatabaseUsearch, db), (DistributedShardedVectorDatabase, None)):
        for name, args in (("find_most_similar_mmr", (q[0],)), ("find_most_similar_mmr_batch", (q,))):
            with pytest.raises(NotImplementedError, match="MMR search"):
                getattr(cls, name)(obj if obj is not None else object.__new__(cls), *args)


# ---- the oracle's own checks ---------------------------------------------------------------------------------------------

def clustered(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((8, d))
    x = centres[rng.integers(0, 8, n)] + 0.35 * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def near(x, r, seed):
    """A perturbed copy of row r (cosine ~0.96): a query ON a stored row makes step 1 a tie of rounding errors — then
    rel[j] and s(first pick, j) are the same number and every objective is lambda * rel - (1 - lambda) * rel."""
    q = x[r] + 0.3 / np.sqrt(x.shape[1]) * np.random.default_rng(seed).standard_normal(x.shape[1]).astype(np.float32)
    return (q / np.linalg.norm(q)).astype(np.float32)


def candidates(x, q, F):
    rel = x @ q
    order = np.lexsort((np.arange(len(rel)), -rel))[:F]
    return rel[order].astype(np.float32), x[order]


def test_oracle_lambda_one_is_the_identity_and_sequences_pass_their_own_adjudicator():
    x = clustered(400, 24, 1)
    for qi in range(5):
        rel, rows = candidates(x, near(x, qi * 7, qi), 40)
        assert mmr_oracle.select(rel, rows, 10, 1.0) == list(range(10))
        for lam in (0.0, 0.3, 0.5, 0.7):
            picks = mmr_oracle.select(rel, rows, 10, lam)
            assert picks[0] == 0 and len(set(picks)) == 10
            ok, msg, worst = mmr_oracle.adjudicate(rel, rows, picks, 10, lam)
            assert ok and worst == 0.0, msg
            assert mmr_oracle.select(rel, rows, 10, lam, dtype=np.float32) == picks      # fp32 numpy agrees on this corpus
            ok, msg, _ = mmr_oracle.adjudicate(rel, rows, list(range(10)), 10, lam)
            assert not ok, (qi, lam)                                                  # the plain top-k is not an MMR answer
    assert mmr_oracle.select(rel, rows, 100, 0.5)[:1] == [0] and len(mmr_oracle.select(rel, rows, 100, 0.5)) == 40
    assert mmr_oracle.select(rel[:0], rows[:0], 3, 0.5) == []
    ok, msg, _ = mmr_oracle.adjudicate(rel, rows, mmr_oracle.select(rel, rows, 9, 0.5), 10, 0.5)
    assert not ok and "picks for k" in msg


def test_oracle_duplicate_ties_go_to_the_lower_position():
    x = clustered(200, 24, 2)
    x[50:58] = x[49]
    rel, rows = candidates(x, near(x, 49, 7), 30)
    assert np.array_equal(rows[:9], np.repeat(x[49:50], 9, 0))                        # nine identical candidates lead
    picks = mmr_oracle.select(rel, rows, 30, 0.5)
    copies = [p for p in picks if p < 9]
    assert picks[0] == 0 and copies == list(range(9))                                 # copies come in position order
    assert picks[1] >= 9                                                              # ... and never back to back at the start
    assert mmr_oracle.adjudicate(rel, rows, picks, 30, 0.5)[0]
    swapped = [copies[1] if p == copies[2] else copies[2] if p == copies[1] else p for p in picks]
    assert mmr_oracle.adjudicate(rel, rows, swapped, 30, 0.5)[0]                      # (exact ties: tau cannot tell; the GPU test checks the order)


def test_adjudicator_rejects_a_swap_across_a_margin_and_accepts_one_inside_it():
    x = clustered(400, 24, 3)
    rel, rows = candidates(x, near(x, 5, 8), 40)
    picks = mmr_oracle.select(rel, rows, 10, 0.5)
    trace = mmr_oracle.objective_trace(rel, rows, picks, 0.5)
    t_ = mmr_oracle.tau(rows)
    assert t_ == pytest.approx(28 * 2.0 ** -23, rel=1e-5)                             # unit rows: (d + 4) 2^-23
    rejected = 0
    for t in range(1, 9):
        swapped = list(picks)
        swapped[t], swapped[t + 1] = swapped[t + 1], swapped[t]
        # float64 margin of the swap at step t: the objective of the later pick, under the same prefix, against the best
        later = mmr_oracle.objective_trace(rel, rows, swapped[:t + 1], 0.5)[-1]
        margin = trace[t - 1] - later
        ok, msg, worst = mmr_oracle.adjudicate(rel, rows, swapped, 10, 0.5)
        assert ok == (margin <= t_), (t, margin, msg)
        rejected += not ok
    assert rejected >= 6
    # a tie inside tau may go either way: two candidates 1e-9 apart
    rows2 = rows.copy()
    rows2[7] = rows2[6]
    rel2 = rel.copy()
    rel2[7] = rel2[6]
    a = mmr_oracle.select(rel2, rows2, 40, 0.5)
    i6, i7 = a.index(6), a.index(7)
    assert i6 < i7
    b = list(a)
    b[i6], b[i7] = 7, 6
    if i7 == i6 + 1:
        assert mmr_oracle.adjudicate(rel2, rows2, b, 40, 0.5)[0]                      # exact tie: the adjudicator takes both orders
    assert not mmr_oracle.adjudicate(rel, rows, [1] + picks[1:], 10, 0.5)[0]          # step 0 must be position 0
    assert not mmr_oracle.adjudicate(rel, rows, picks[:5] + picks[:5], 10, 0.5)[0]    # distinct


def test_oracle_non_finite_objectives_rank_last():
    x = clustered(60, 24, 4).astype(np.float64).astype(np.float32)
    rel, rows = candidates(x, near(x, 0, 9), 12)
    rows = rows.copy()
    rows[11, 3] = -np.inf
    rel = rel.copy()
    rel[11] = -np.inf
    picks = mmr_oracle.select(rel, rows, 12, 0.5)
    assert picks[-1] == 11 and mmr_oracle.adjudicate(rel, rows, picks, 12, 0.5)[0]
    trace = mmr_oracle.objective_trace(rel, rows, picks, 0.5)
    assert all(np.isfinite(v) for v in trace[:-1]) and trace[-1] == -np.inf
