"""The range join on the device (mvdb_index_range_join): query i is stored row qrows[i], matched against the rows below it.

The main claim is BIT IDENTITY: with option "join_shared" = 2 (the triangular shared pass wherever the shape is eligible) a call
returns the counts, D.view(uint32) and I of the same call with "join_shared" = 0 (one bounded fp32 pass per query row), and both
equal `range_search(get_rows(i), thr, normalize_q=False)` on the per-query route, cut to the rows below i.  The corpus is the one
of test_range_batch_gpu.py: a cluster whose pairs straddle 0.8, exact duplicates at rows 299 .. 309 and in the last three rows."""
import ctypes

import numpy as np
import pytest

from test_range_batch_gpu import FMAX, corpus

pytestmark = pytest.mark.gpu

THR = 0.8


def build(native, n, d, x=None, metric=None):
    idx = native.FlatIndex(d) if metric is None else native.FlatIndex(d, metric=metric)
    idx.add(corpus(n, d) if x is None else x)
    return idx


def both_routes(idx, qrows, thr, cap, rowset=None, expect_shared=True):
    """(counts, D, I) of range_join_raw on the shared route, asserted equal to the per-query route's."""
    idx.set_option("join_shared", 0)
    before = idx.join_counters()[0]
    want = idx.range_join_raw(qrows, thr, cap, rowset)
    assert idx.join_counters()[0] == before
    idx.set_option("join_shared", 2)
    got = idx.range_join_raw(qrows, thr, cap, rowset)
    assert idx.join_counters()[0] - before == (1 if expect_shared else 0)
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    if cap:
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(got[2], want[2])
    return got


def by_range_search(idx, i, thr, rowset=None):
    """(D, I) of row i as an uploaded query on the per-query route, cut to the rows below i."""
    idx.set_option("range_shared", 0)
    lims, D, I = idx.range_search(idx.get_rows(int(i), 1), thr, rowset=rowset, normalize_q=False)
    keep = I < i
    return D[keep], I[keep]


def check_rows_against_range_search(idx, qrows, counts, D, I, thr, rows, rowset=None):
    for r in rows:
        i = int(qrows[r])
        Dw, Iw = by_range_search(idx, i, thr, rowset)
        c = int(counts[r])
        assert c == len(Iw), (i, c, len(Iw))
        assert np.array_equal(I[r, :c], Iw) and np.array_equal(D[r, :c].view(np.uint32), Dw.view(np.uint32)), i
        assert (I[r, c:] == -1).all()


@pytest.mark.parametrize("n,d", [(4_999, 128), (4_999, 384), (20_001, 512), (4_999, 1024)])
def test_shared_join_is_bit_identical(gpu, n, d):
    from minivectordb_amd import _native
    idx = build(_native, n, d)
    calls0 = idx.join_counters()[0]
    idx.set_option("join_shared", 0)
    want = idx.range_join(THR)
    assert idx.join_counters()[0] == calls0
    idx.set_option("join_shared", 2)
    qrows, lims, D, I = idx.range_join(THR)
    assert idx.join_counters()[0] > calls0                       # the shared pass ran
    assert np.array_equal(qrows, np.arange(n)) and np.array_equal(qrows, want[0])
    assert np.array_equal(lims, want[1]) and np.array_equal(D.view(np.uint32), want[2].view(np.uint32)) and np.array_equal(I, want[3])
    assert lims[1] == 0                                          # row 0 has nothing before it
    assert idx.range_join_count(THR) == lims[-1] and lims[-1] > 1_000
    assert (I < np.repeat(qrows, np.diff(lims))).all() and (I >= 0).all() and (D >= np.float32(THR)).all()
    fixed = [0, 1, *range(299, 311), 599, 600, n - 3, n - 2, n - 1]
    rest = np.setdiff1d(np.arange(n), fixed)
    sample = fixed + np.random.default_rng(d).choice(rest, 64 - len(fixed), replace=False).tolist()
    for i in sample:
        Dw, Iw = by_range_search(idx, i, THR)
        assert np.array_equal(I[lims[i]:lims[i + 1]], Iw), i
        assert np.array_equal(D[lims[i]:lims[i + 1]].view(np.uint32), Dw.view(np.uint32)), i
    # the exact duplicates (rows 299 .. 309 and the last three): equal score bits, ascending rows, at the head of the list
    copies = list(range(299, 310)) + [n - 3, n - 2, n - 1]
    for i in (305, 309, n - 1):
        want_rows = [r for r in copies if r < i]
        assert I[lims[i]:lims[i] + len(want_rows)].tolist() == want_rows, i
        bits = D[lims[i]:lims[i] + len(want_rows)].view(np.uint32)
        assert (bits == bits[0]).all()
    idx.close()


def test_edges_of_the_triangle_and_of_the_chunks(gpu):
    from minivectordb_amd import _native
    n, d = 4_999, 512
    idx = build(_native, n, d)
    cap = 1024
    # consecutive rows (no copy), bounds inside 32-row tiles, a full 256-chunk and a ragged one
    qrows = np.arange(37, 37 + 300)
    counts, D, I = both_routes(idx, qrows, THR, cap)
    check_rows_against_range_search(idx, qrows, counts, D, I, THR, [0, 1, 27, 255, 256, 262, 263, 299])
    # unsorted and repeating: the gather path
    rng = np.random.default_rng(5)
    qrows = np.concatenate([rng.choice(n, 60, replace=False), [305, 305, 0, n - 1, 31, 32, 33, 305, 64, 1]])
    assert len(qrows) == 70
    counts, D, I = both_routes(idx, qrows, THR, cap)
    check_rows_against_range_search(idx, qrows, counts, D, I, THR, range(50, 70))
    assert counts[60] == counts[61] == counts[67] and np.array_equal(I[60], I[67])
    for single in ([0], [n - 1]):
        counts, D, I = both_routes(idx, np.array(single), THR, cap, expect_shared=False)   # (one query row: its own pass)
        check_rows_against_range_search(idx, single, counts, D, I, THR, [0])
    assert both_routes(idx, np.array([0]), THR, cap, expect_shared=False)[0][0] == 0
    # a cap far below the counts: missing markers, true counts
    qrows = np.arange(280, 340)
    full = both_routes(idx, qrows, THR, cap)
    small = both_routes(idx, qrows, THR, 8)
    assert np.array_equal(small[0], full[0]) and (full[0] > 8).sum() > 40
    for r in range(len(qrows)):
        if full[0][r] > 8:
            assert (small[2][r] == -1).all() and (small[1][r] == -FMAX).all()
        else:
            assert np.array_equal(small[2][r], full[2][r, :8])
    none = both_routes(idx, qrows, THR, 0)
    assert np.array_equal(none[0], full[0]) and none[1] is None and none[2] is None
    idx.close()


def test_overflow_goes_to_the_bounded_fallback(gpu):
    from minivectordb_amd import _native
    n, d = 4_999, 512
    idx = build(_native, n, d)
    idx.set_option("range_candidates", 64)
    qrows = np.arange(n - 700, n)[::-1].copy()                   # descending: gathered; then the cluster rows
    qrows[:400] = np.arange(200, 600)
    fb0 = idx.join_counters()[1]
    counts, D, I = both_routes(idx, qrows, THR, 1024)
    assert (counts[:400] > 64).sum() > 100                       # the cluster rows hold more pairs than a segment
    assert idx.join_counters()[1] - fb0 >= (counts > 64).sum()
    check_rows_against_range_search(idx, qrows, counts, D, I, THR, [0, 99, 100, 399, 400, 699])
    # -inf: every row below the bound matches
    qrows = np.concatenate([np.arange(0, 300), [n - 1, 1, 0, 33]])
    counts = both_routes(idx, qrows, -np.inf, 0)[0]
    assert np.array_equal(counts, qrows)
    assert idx.range_counters()[:2] == (0, 0)                    # the range calls' counters are not the join's
    idx.close()


def test_row_sets(gpu):
    from minivectordb_amd import _native
    n, d = 4_999, 512
    idx = build(_native, n, d)
    rng = np.random.default_rng(11)
    gone = np.concatenate([[299, 303, 600, 0], rng.choice(n, 96, replace=False)])
    listed = rng.permutation(np.concatenate([np.arange(250, 650), rng.choice(np.arange(650, n), 300, replace=False)]))
    cases = [("bitmap", idx.rowset(gone, excluded=True), np.setdiff1d(np.arange(n), gone), True),
             ("list", idx.rowset(listed), np.sort(listed), False),
             ("one row", idx.rowset(np.array([299])), np.array([299]), False)]
    assert cases[0][1].is_bitmap and not cases[1][1].is_bitmap and len(listed) == 700
    qrows = np.concatenate([np.arange(290, 330), [n - 1, n - 2, 601, 0, 299]])
    for name, rs, members, shared in cases:
        counts, D, I = both_routes(idx, qrows, THR, 1024, rowset=rs, expect_shared=shared)
        assert counts.sum() > 0, name
        for r in range(len(qrows)):
            got = I[r, :counts[r]]
            assert np.isin(got, members).all() and (got < qrows[r]).all(), (name, r)
        check_rows_against_range_search(idx, qrows, counts, D, I, THR, [0, 9, 10, 20, 39, 40, 42, 44], rowset=rs)
    # members of the set as query rows: both ends of every pair inside
    members = cases[0][2]
    q_in = members[(members >= 280) & (members < 340)]
    counts, D, I = both_routes(idx, q_in, THR, 1024, rowset=cases[0][1])
    assert all(np.isin(I[r, :counts[r]], members).all() for r in range(len(q_in)))
    # a set created before 500 more rows are added: the new rows are not in it, and may be query rows
    idx.add(corpus(n, d)[200:700])
    qrows = np.concatenate([np.arange(n + 90, n + 130), [310, n - 1]])
    counts, D, I = both_routes(idx, qrows, THR, 2048, rowset=cases[0][1])
    assert all((I[r, :counts[r]] < n).all() and np.isin(I[r, :counts[r]], members).all() for r in range(len(qrows)))
    assert counts[:40].min() >= 1                                # (the added rows repeat cluster rows)
    check_rows_against_range_search(idx, qrows, counts, D, I, THR, [0, 10, 39, 40, 41], rowset=cases[0][1])
    idx.close()


@pytest.mark.parametrize("what", ["l2", "d30", "d1536", "nonfinite"])
def test_indexes_the_shared_pass_does_not_take(gpu, what):
    from minivectordb_amd import _native
    n, d, thr, metric = 2_999, 512, THR, None
    if what == "l2":
        metric, thr = _native.METRIC_L2, 0.4                     # squared distance 0.4 = cosine 0.8 on unit rows
    elif what == "d30":
        d = 30
        thr = 0.7
    elif what == "d1536":
        d = 1536
    x = corpus(n, d).copy()
    if what == "nonfinite":
        x[301] = np.nan
        x[650, 3] = np.inf
    idx = build(_native, n, d, x, metric)
    qrows = np.concatenate([np.arange(280, 340), [n - 1, 650, 651, 0, 1]])
    counts, D, I = both_routes(idx, qrows, thr, 1024, expect_shared=False)
    assert idx.join_counters() == (0, 0)
    assert counts.sum() > 500 and counts[-2] == 0
    check_rows_against_range_search(idx, qrows, counts, D, I, thr, range(len(qrows)))
    if metric is not None:
        assert all((np.diff(D[r, :counts[r]]) >= 0).all() for r in range(len(qrows)))   # distances ascend
    if what == "nonfinite":
        r = int(np.flatnonzero(qrows == 301)[0])
        assert counts[r] == 0                                    # a NaN query row matches nothing ...
        assert not (I == 301).any()                              # ... and a NaN row is matched by nothing
        assert not np.isnan(D[I >= 0]).any()
    idx.close()


@pytest.mark.parametrize("d,thresholds", [(128, (0.78, 0.80)), (512, (0.78,))])
def test_against_the_float64_scores(gpu, d, thresholds):
    from minivectordb_amd import _native
    n = 6_001
    idx = build(_native, n, d)
    idx.set_option("join_shared", 2)
    x64 = idx.get_rows(0, n).astype(np.float64)
    delta = (d + 8) * 2.0 ** -24
    lo = min(thresholds) - delta
    s64 = {}
    for b0 in range(0, n, 1000):
        s = x64[b0:b0 + 1000] @ x64.T
        ii, jj = np.nonzero(s >= lo)
        keep = jj < ii + b0
        s64.update(zip(zip((ii[keep] + b0).tolist(), jj[keep].tolist()), s[ii[keep], jj[keep]].tolist()))
    for t in thresholds:
        calls0 = idx.join_counters()[0]
        qrows, lims, D, I = idx.range_join(t)
        assert idx.join_counters()[0] > calls0
        later = np.repeat(qrows, np.diff(lims))
        got = dict(zip(zip(later.tolist(), I.tolist()), D.tolist()))
        assert len(got) == len(I) and all(j < i for i, j in got)           # no pair twice, none as (i, i) or (earlier, later)
        must = {p for p, s in s64.items() if s >= t + delta}
        may = {p for p, s in s64.items() if s >= t - delta}
        at_or_above = sum(1 for s in s64.values() if s >= t)
        band = len(may) - len(must)
        print(f"d={d} t={t}: {len(got)} pairs returned, {at_or_above} at or above t in float64, {band} inside the band")
        assert must <= set(got) <= may
        assert max(abs(s - s64[p]) for p, s in got.items()) <= 1e-4
        assert at_or_above >= 10_000 and band <= 0.01 * at_or_above
    idx.close()


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_through_the_database_classes(gpu, tmp_path, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    n, d = 3_000, 128
    x = corpus(n, d)
    # a floor no pair score comes near: the class path re-normalises its query, the join does not
    x64 = x[:620].astype(np.float64)
    s = np.sort((x64 @ x64.T)[np.tril_indices(620, -1)])
    s = s[(s > 0.82) & (s < 0.83)]
    g = int(np.argmax(np.diff(s)))
    min_score = float((s[g] + s[g + 1]) / 2)
    assert s[g + 1] - s[g] > 4e-6
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "shards"), shard_size=1024)
    ids = [10_000 + i for i in range(n)]
    meta = [{"bucket": i % 3} for i in range(n)]
    db.store_embeddings_batch(ids[:2000], x[:2000], meta[:2000])
    assert db.count_duplicate_pairs(min_score) > 500
    db.store_embeddings_batch(ids[2000:], x[2000:], meta[2000:])
    position = {uid: i for i, uid in enumerate(ids)}

    def loop(later_ids, **f):
        pairs = {}
        for uid in later_ids:
            found, scores, _ = db.find_all_similar(db.get_vector(uid), min_score, **f)
            pairs.update({(e, uid): sc for e, sc in zip(found, scores) if position[e] < position[uid]})
        return pairs

    f = {"metadata_filter": {"bucket": 1}}
    for kw, later_ids in ((dict(first_row=2000, **f), [u for u in ids[2000:] if position[u] % 3 == 1]),
                          (dict(first_row=2700), ids[2700:]),
                          (f, [u for u in ids[:640] if position[u] % 3 == 1] + ids[2998:2999])):
        want = loop(later_ids, **{k: v for k, v in kw.items() if k != "first_row"})
        early, late, scores = db.find_duplicate_pairs(min_score, **kw)
        got = dict(zip(zip(early, late), scores))
        if "first_row" not in kw:                                # the loop covered the cluster's rows only: cut the join to them
            got = {p: sc for p, sc in got.items() if p[1] in set(later_ids)}
            assert len(got) > 50
        else:
            assert len(got) == len(early) == db.count_duplicate_pairs(min_score, **kw)
        assert set(got) == set(want) and len(got) > 0
        assert max(abs(got[p] - want[p]) for p in got) <= 1e-6
        keys = [(-sc, position[b], position[a]) for a, b, sc in zip(early, late, scores)]
        assert keys == sorted(keys)
    groups = db.find_duplicate_groups(min_score, first_row=2700)
    pairs = db.find_duplicate_pairs(min_score, first_row=2700)
    assert {u for g in groups for u in g} == set(pairs[0]) | set(pairs[1])
    assert any({ids[299], ids[305], ids[2999]} <= set(g) for g in groups)     # the exact duplicates end in one group
    assert all(g == sorted(g, key=position.get) for g in groups)


def test_argument_errors_write_nothing(gpu):
    from minivectordb_amd import _native
    n, d = 1_000, 128
    idx = build(_native, n, d)
    other = build(_native, n, d)
    foreign = other.rowset(np.arange(10))
    lib = _native.lib()
    cap = 4
    qrows = np.array([5, 6, 7], np.int64)

    def call(q=qrows, nq=3, thr=0.5, rs=None, cap=cap, counts=True, D=True, I=True):
        c = np.full(3, -7, np.int64)
        Dv = np.full((3, 4), 123.0, np.float32)
        Iv = np.full((3, 4), -7, np.int64)
        p = lambda a, use: a.ctypes.data_as(ctypes.c_void_p) if use else None
        rc = lib.mvdb_index_range_join(idx.handle, p(q, q is not None), nq, ctypes.c_float(thr), rs, cap, p(c, counts), p(Dv, D), p(Iv, I))
        return rc, c, Dv, Iv

    bad = [dict(q=None), dict(counts=False), dict(D=False), dict(I=False), dict(nq=0), dict(nq=-1), dict(thr=float("nan")),
           dict(cap=-1), dict(q=np.array([5, n, 7], np.int64)), dict(q=np.array([5, -1, 7], np.int64)), dict(rs=foreign._h)]
    for kw in bad:
        rc, c, Dv, Iv = call(**kw)
        assert rc == _native.ERR_ARG and _native.last_error(), kw
        assert (c == -7).all() and (Dv == 123.0).all() and (Iv == -7).all(), kw
    rc, c, Dv, Iv = call()
    assert rc == 0 and (c >= 0).all()
    rc, c, Dv, Iv = call(cap=0, D=False, I=False)                # cap == 0: D / I may be NULL
    assert rc == 0 and (c >= 0).all() and (Dv == 123.0).all()
    with pytest.raises(ValueError):
        idx.set_option("join_shared", 3)
    with pytest.raises(ValueError, match="join_shared"):
        idx.set_option("no_such_option", 1)
    idx.close()
    other.close()
