"""Boosted search on the device (mvdb_index_search_boosted, csrc/boost_scan.hpp): every comparison is exact.  The oracle's
s_row is the library's own single-query bits — `world(d, kind).scores(kind)[j]` of tests/test_assign_gpu.py, the full ranking
of query vector j over the selected rows scattered by row number — and tests/boost_oracle.py is the contract in numpy.
Scores are compared as bits, rows as integers.

Corpus and queries: that file's (2,051 rows, 4,099 for the dense bitmap, 70 perturbed stored rows as queries; vector ZERO
is all zeros, vector NANV holds a NaN).  Terms: four float32 columns per world drawn N(0, 0.05), at the weights 0.3, -0.7,
1.1 and 0.05 — no power of two, so a fused multiply-add would show; the sparse entries are 50 distinct rows with values
N(0, 0.2)."""
import numpy as np
import pytest

from boost_oracle import boosted, combine
from maxsim_oracle import MISSING
from test_assign_gpu import DIMS, KINDS, NANV, ZERO, bits, make_corpus, world

pytestmark = pytest.mark.gpu

WEIGHTS = np.array([0.3, -0.7, 1.1, 0.05], np.float32)
SCORE_WEIGHTS = [1.0, 0.75, 1.3, -0.6]
KS = (1, 10, 64)
INF = np.float32(np.inf)


def boost_state(w):
    """The world's term columns (host and resident) and sparse entries, made once."""
    if not hasattr(w, "boost"):
        rng = np.random.default_rng(4000 + w.d + w.n)
        cols = [(np.float32(0.05) * rng.standard_normal(w.n)).astype(np.float32) for _ in range(4)]
        rows = rng.permutation(w.n)[:50].astype(np.int64)
        vals = (np.float32(0.2) * rng.standard_normal(50)).astype(np.float32)
        w.boost = (cols, [w.idx.rowterm(c) for c in cols], (rows, vals))
    return w.boost


def same(got, want, what):
    D, I = got
    assert D.dtype == np.float32 and I.dtype == np.int64, what
    assert np.array_equal(I, want[1]), (what, "rows", I, want[1])
    assert np.array_equal(bits(D), bits(want[0])), (what, "scores", D, want[0])


def one(got):
    assert got[0].shape[0] == 1 and got[1].shape[0] == 1
    return got[0][0], got[1][0]


# ---- widths, row sets, k, term counts, sparse entries -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_every_width_row_set_k_and_term_count(gpu, d, kind):
    w = world(d, kind)
    rs, selected = w.rowset(kind)
    assert kind not in ("dense", "excluded") or rs.is_bitmap
    assert kind != "unsorted" or not rs.is_bitmap
    cols, terms, sparse = boost_state(w)
    s_all = w.scores(kind)
    for nt in (1, 2, 3, 4):
        for sp in (None, sparse):
            T = combine(cols[:nt], WEIGHTS[:nt], w.n, sp)
            got_T = w.idx.boost_combine(terms[:nt], WEIGHTS[:nt], *(sp or (None, None)))
            assert np.array_equal(bits(got_T), bits(T)), (d, kind, nt, sp is not None, np.flatnonzero(bits(got_T) != bits(T))[:10])
            for k in KS:
                j = 10 + 3 * nt + k % 7 + (sp is not None)          # a query of its own per cell; none of them ZERO or NANV
                w_s = SCORE_WEIGHTS[(nt + k) % 4]
                got = one(w.idx.search_boosted(w.c[j], k, terms[:nt], WEIGHTS[:nt], score_weight=w_s, sparse_rows=sp and sp[0],
                                               sparse_values=sp and sp[1], rowset=rs, normalize_q=True))
                want = boosted(s_all[j], T, w_s, k)
                same(got, want, (d, kind, nt, sp is not None, k, j, w_s))
                if kind == "empty":
                    assert (got[1] == -1).all() and (got[0] == MISSING).all()
                else:
                    assert (got[1] >= 0).all() and np.isin(got[1], selected).all()
    # sparse entries alone: T starts as +0.0
    T = combine([], [], w.n, sparse)
    assert np.array_equal(bits(w.idx.boost_combine([], [], *sparse)), bits(T))
    got = one(w.idx.search_boosted(w.c[20], 10, [], [], sparse_rows=sparse[0], sparse_values=sparse[1], rowset=rs, normalize_q=True))
    same(got, boosted(s_all[20], T, 1.0, 10), (d, kind, "sparse only"))


def test_the_term_takes_part_in_the_ranking(gpu):
    """A kernel that ignores T cannot pass: a N(0, 0.05) term changes the top 10, one huge value lifts the plain ranking's last
    row to the front — from a resident column and from a sparse entry."""
    w = world(512)
    cols, terms, _ = boost_state(w)
    changed = 0
    for j in (10, 11, 12, 13):
        D0, I0 = one(w.idx.search(w.c[j:j + 1], 10, normalize_q=True))
        D1, I1 = one(w.idx.search_boosted(w.c[j], 10, terms[:1], [1.0], normalize_q=True))
        same((D1, I1), boosted(w.scores()[j], combine(cols[:1], [1.0], w.n), 1.0, 10), ("term", j))
        assert set(I1.tolist()) != set(I0.tolist()), (j, I0, I1)
        changed += 1
        Dn, In = one(w.idx.search(w.c[j:j + 1], w.n, normalize_q=True))
        tail = int(In[-1])
        D2, I2 = one(w.idx.search_boosted(w.c[j], 10, [], [], sparse_rows=[tail], sparse_values=[1000.0], normalize_q=True))
        assert I2[0] == tail and I2[1:].tolist() == I0[:9].tolist()
        assert bits(D2[:1]).tolist() == bits(np.float32(Dn[-1]) + np.float32(1000.0)).tolist()
        col = np.zeros(w.n, np.float32)
        col[tail] = 1000.0
        D3, I3 = one(w.idx.search_boosted(w.c[j], 10, [w.idx.rowterm(col)], [1.0], normalize_q=True))
        assert np.array_equal(I3, I2) and np.array_equal(bits(D3), bits(D2))
    assert changed == 4


@pytest.mark.parametrize("d", DIMS)
def test_a_negative_zero_term_is_the_plain_search(gpu, d):
    for kind in (None, "dense", "excluded"):
        w = world(d, kind)
        rs, _ = w.rowset(kind)
        zero = w.idx.rowterm(np.full(w.n, -0.0, np.float32))
        for k in KS:
            for j in (9, 33, ZERO):
                q = w.c[j:j + 1]
                want = w.idx.search(q, k, normalize_q=True) if rs is None else w.idx.search_rowset(q, k, rs, normalize_q=True)
                got = w.idx.search_boosted(q, k, [zero], [1.0], score_weight=1.0, rowset=rs, normalize_q=True)
                same(one(got), one(want), (d, kind, k, j))


# ---- ties -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "unsorted", "dense", "excluded"])
@pytest.mark.parametrize("d", [100, 512])
def test_ties_go_to_the_lower_physical_row(gpu, d, kind):
    w = world(d, kind)
    rs, selected = w.rowset(kind)
    ascending = np.sort(selected)
    const = w.idx.rowterm(np.full(w.n, 0.25, np.float32))
    for k in KS:
        D, I = one(w.idx.search_boosted(w.c[ZERO], k, [const], [2.0], rowset=rs, normalize_q=True))
        assert I.tolist() == ascending[:k].tolist(), (d, kind, k)                 # the all-zero query: every row scores 0
        assert bits(D).tolist() == bits(np.full(k, 0.5, np.float32)).tolist()
    three = np.array([0.5, -1.0, 0.125], np.float32)[(np.arange(w.n) * 7 + 1) % 3]
    D, I = one(w.idx.search_boosted(w.c[ZERO], 64, [w.idx.rowterm(three)], [1.0], rowset=rs, normalize_q=True))
    same((D, I), boosted(w.scores(kind)[ZERO], three, 1.0, 64), (d, kind, "three values"))
    best = ascending[three[ascending] == 0.5]
    assert len(best) >= 64 and I.tolist() == best[:64].tolist()
    # a tie across the three values: with weights that map all of them to 0 the order is the rows' again
    D, I = one(w.idx.search_boosted(w.c[ZERO], 64, [w.idx.rowterm(three)], [0.0], rowset=rs, normalize_q=True))
    assert I.tolist() == ascending[:64].tolist()


# ---- non-finite values -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 512])
def test_non_finite_scores_and_terms(gpu, d):
    w = world(d)
    cols, terms, sparse = boost_state(w)
    D, I = one(w.idx.search_boosted(w.c[NANV], 10, terms[:2], WEIGHTS[:2], normalize_q=True))
    assert (I == -1).all() and (D == MISSING).all()                               # a NaN query: nothing has a score
    j = 15
    s = w.scores()[j]
    plain = np.argsort(-s, kind="stable")
    # NaN on the plain top three and on a stripe of rows: never returned
    col = cols[0].copy()
    nan_rows = np.union1d(plain[:3], np.arange(0, w.n, 5))
    col[nan_rows] = np.nan
    lifted = int(np.setdiff1d(plain[300:320], nan_rows)[0])
    col[lifted] = np.inf                                                          # +inf: first
    D, I = one(w.idx.search_boosted(w.c[j], 64, [w.idx.rowterm(col)], [1.0], normalize_q=True))
    same((D, I), boosted(s, combine([col], [1.0], w.n), 1.0, 64), (d, "nan and +inf"))
    assert I[0] == lifted and D[0] == INF and not np.isin(I, nan_rows).any() and (I >= 0).all()
    # -inf: last among the candidates, still ahead of the padding (a list of 20 rows, k = 64)
    rows = plain[[5, 900, 17, 3, 1200, 44, 8, 300, 2, 70, 1, 0, 1500, 61, 12, 2000, 9, 25, 33, 6]].astype(np.int64)
    rs = w.idx.rowset(rows)
    col = cols[1].copy()
    col[rows[4]] = -np.inf
    col[rows[9]] = np.inf
    s_sel = np.full(w.n, np.nan, np.float32)
    s_sel[rows] = s[rows]
    D, I = one(w.idx.search_boosted(w.c[j], 64, [w.idx.rowterm(col)], [1.0], rowset=rs, normalize_q=True))
    same((D, I), boosted(s_sel, combine([col], [1.0], w.n), 1.0, 64), (d, "-inf"))
    assert I[0] == rows[9] and D[0] == INF and I[19] == rows[4] and D[19] == -INF
    assert (I[20:] == -1).all() and (D[20:] == MISSING).all()
    # +inf and -inf on the same row meet as NaN: never returned
    up, down = np.zeros(w.n, np.float32), np.zeros(w.n, np.float32)
    up[rows[9]], down[rows[9]] = np.inf, -np.inf
    up[rows[2]] = np.inf
    D, I = one(w.idx.search_boosted(w.c[j], 64, [w.idx.rowterm(up), w.idx.rowterm(down)], [1.0, 1.0], rowset=rs, normalize_q=True))
    same((D, I), boosted(s_sel, combine([up, down], [1.0, 1.0], w.n), 1.0, 64), (d, "inf - inf"))
    assert rows[9] not in I and I[0] == rows[2] and (I[:19] >= 0).all() and (I[19:] == -1).all()


# ---- tails ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("d", [100, 512])
def test_small_indexes_and_padding(gpu, d, n):
    from minivectordb_amd import _native
    x, rng = make_corpus(d, n)
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    q = (x[n // 2] + np.float32(0.05) * rng.standard_normal(d)).astype(np.float32)
    col = (np.float32(0.05) * rng.standard_normal(n)).astype(np.float32)
    Dn, In = one(idx.search(q[None], n, normalize_q=True))
    s = np.full(n, np.nan, np.float32)
    s[In] = Dn
    term = idx.rowterm(col)
    assert len(term) == n
    assert np.array_equal(bits(idx.boost_combine([term], [-0.7])), bits(combine([col], [-0.7], n)))
    D, I = one(idx.search_boosted(q, 64, [term], [-0.7], score_weight=0.75, normalize_q=True))
    same((D, I), boosted(s, combine([col], [-0.7], n), 0.75, 64), (d, n))
    assert (I[:min(n, 64)] >= 0).all() and (I[n:] == -1).all() and (D[n:] == MISSING).all()
    sparse = (np.array([n - 1], np.int64), np.array([0.5], np.float32))
    D, I = one(idx.search_boosted(q, 64, [term], [-0.7], sparse_rows=sparse[0], sparse_values=sparse[1], normalize_q=True))
    same((D, I), boosted(s, combine([col], [-0.7], n, sparse), 1.0, 64), (d, n, "sparse"))
    idx.close()


# ---- batches and counters -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "unsorted", "dense", "empty"])
def test_a_batch_equals_its_single_calls_and_the_counters_count(gpu, kind):
    w = world(384, kind)
    rs, selected = w.rowset(kind)
    cols, terms, sparse = boost_state(w)
    scans = 1 if len(selected) else 0                   # one scan launch per call (the queries are the grid's y); none for an empty set
    calls0, launches0 = w.idx.boost_counters()
    Db, Ib = w.idx.search_boosted(w.c[20:23], 10, terms[:2], WEIGHTS[:2], score_weight=0.75, rowset=rs, normalize_q=True)
    assert w.idx.boost_counters() == (calls0 + 1, launches0 + scans)
    assert Db.shape == (3, 10) and Ib.shape == (3, 10)
    for i in range(3):
        single = one(w.idx.search_boosted(w.c[20 + i], 10, terms[:2], WEIGHTS[:2], score_weight=0.75, rowset=rs, normalize_q=True))
        same((Db[i], Ib[i]), single, (kind, i))
        same(single, boosted(w.scores(kind)[20 + i], combine(cols[:2], WEIGHTS[:2], w.n), 0.75, 10), (kind, i, "oracle"))
    assert w.idx.boost_counters() == (calls0 + 4, launches0 + 4 * scans)
    w.idx.boost_combine(terms[:1], [1.0])                                          # the combine alone is no search
    assert w.idx.boost_counters() == (calls0 + 4, launches0 + 4 * scans)


# ---- staleness and arguments ----------------------------------------------------------------------------------------------------

def test_stale_terms_and_argument_errors(gpu):
    from minivectordb_amd import _native
    d, n = 32, 100
    x, rng = make_corpus(d, n + 10)
    idx = _native.FlatIndex(d)
    idx.add(x[:n], normalize=True)
    q = x[7]
    col = np.zeros(n, np.float32)
    term = idx.rowterm(col)
    base = one(idx.search_boosted(q, 5, [term], [1.0], normalize_q=True))
    with pytest.raises(ValueError, match="one value per stored row .99 values, 100 rows"):
        idx.rowterm(col[:99])
    # set_rows keeps the row numbers: the term stays valid, and the result follows the new row
    idx.set_rows([50], x[7:8] * np.float32(3), normalize=True)
    D, I = one(idx.search_boosted(q, 5, [term], [1.0], normalize_q=True))
    assert base[1][0] == 7 and sorted(I[:2].tolist()) == [7, 50] and abs(float(D[1]) - 1.0) < 1e-5
    # rows added since: the term has no value for them
    idx.add(x[n:n + 5], normalize=True)
    with pytest.raises(ValueError, match="holds 100 rows, the index 105"):
        idx.search_boosted(q, 5, [term], [1.0])
    with pytest.raises(ValueError, match="holds 100 rows, the index 105"):
        idx.boost_combine([term], [1.0])
    # rows removed since: renumbered, whatever the count
    term = idx.rowterm(np.zeros(105, np.float32))
    idx.remove_rows([3])
    with pytest.raises(ValueError, match="holds 105 rows, the index 104"):
        idx.search_boosted(q, 5, [term], [1.0])
    idx.add(x[n + 5:n + 6], normalize=True)
    assert idx.ntotal == 105
    with pytest.raises(ValueError, match="before rows were removed"):
        idx.search_boosted(q, 5, [term], [1.0])
    term = idx.rowterm(np.zeros(105, np.float32))
    other = _native.FlatIndex(d)
    other.add(x[:105], normalize=True)
    with pytest.raises(ValueError, match="belongs to another index"):
        other.search_boosted(q, 5, [term], [1.0])
    calls = idx.boost_counters()
    for kw, msg in ((dict(k=65), "1 <= k <= 64"),
                    (dict(terms=[term] * 5, weights=[1.0] * 5), "0 to 4 terms"),
                    (dict(terms=[], weights=[]), "nothing to boost by"),
                    (dict(q=np.stack([q, q]), sparse_rows=[1], sparse_values=[1.0]), "single query"),
                    (dict(sparse_rows=[4, 9, 4], sparse_values=[1.0, 2.0, 3.0]), "sparse row 4 is listed twice"),
                    (dict(sparse_rows=[4, 105], sparse_values=[1.0, 2.0]), r"sparse row 105 is outside \[0, 105\)"),
                    (dict(sparse_rows=[-1], sparse_values=[1.0]), r"sparse row -1 is outside \[0, 105\)")):
        args = dict(q=q, k=5, terms=[term], weights=[1.0])
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            idx.search_boosted(**args)
    assert idx.boost_counters() == calls                                           # a refused call is not counted
    with pytest.raises(ValueError, match="1 terms, 2 weights"):
        idx.search_boosted(q, 5, [term], [1.0, 2.0])
    l2 = _native.FlatIndex(d, metric=_native.METRIC_L2)
    l2.add(x[:n])
    with pytest.raises(ValueError, match="inner-product index"):
        l2.search_boosted(q, 5, [l2.rowterm(col)], [1.0])
    # a stale row set is refused as every row-set search refuses it
    rs = idx.rowset(np.arange(10, dtype=np.int64))
    idx.remove_rows([0])
    term = idx.rowterm(np.zeros(104, np.float32))
    with pytest.raises(ValueError, match="another state of the index"):
        idx.search_boosted(q, 5, [term], [1.0], rowset=rs)
    for i in (idx, other, l2):
        i.close()
