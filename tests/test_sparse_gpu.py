"""Sparse and hybrid search on the device (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH", csrc/sparse_scan.hpp): every
comparison is exact — scores as bits, rows and matched counts as integers — against tests/sparse_oracle.py, the contract in
numpy float32.  One exception to "bits": where the contract's value is a NaN (a NaN weight, inf - inf) the device's value must
be a NaN too; which NaN is not part of the contract (numpy's and the device's default NaN differ in the sign bit).

Rows: the 2,051-row world of tests/test_assign_gpu.py and its 4,099-row world (the dense bitmap's).  Their sparse rows are built
around mvdb_sparse_geometry: lengths 0, 1, 63, 64, 65, span - 1, span, span + 1, 2 span + 3, a run of tile_rows + 5 empty rows,
the first and the last row empty, a few dozen entries elsewhere.  dim is 50 and 2^20; at dim 50 a row holds at most 50 entries
(its indices are distinct), so the long rows and the 1,024-term query exist at 2^20 only, and so does the query of indices
congruent modulo table_slots (50 < table_slots).  Rows 100 .. 105 hold the special values: products that cancel to +0.0, +inf,
a NaN weight, inf - inf, -0.0 / +0.0, -inf."""
import numpy as np
import pytest

from boost_oracle import boosted
from maxsim_oracle import MISSING
from sparse_oracle import scores, sparse_term, sparse_topk
from test_assign_gpu import KINDS, bits, make_corpus, world

pytestmark = pytest.mark.gpu

DIMS = [50, 1 << 20]
KS = (1, 10, 64)
D_DENSE = 100                       # width of the worlds the sparse tests ride on (the sparse side never reads the dense matrix)
HYBRID_WEIGHTS = [(0.3, -0.7), (1.1, 0.3), (-0.7, 1.1)]      # (dense, sparse): no power of two, a fused multiply-add would show
CANCEL, PINF, NANROW, INFINF, ZEROS, NINF = 100, 101, 102, 103, 104, 105
Q7 = np.array([3, 11, 19, 27, 35, 43, 49], np.int64)
Q7_VALUES = np.array([0.75, 0.75, -1.3, 0.4, 2.1, -0.6, 0.9], np.float32)       # q[3] == q[11]: row CANCEL cancels, row INFINF meets inf - inf


def geometry():
    from minivectordb_amd import _native
    return _native.sparse_geometry()


def build_rows(n, dim, seed):
    """(indptr, indices, values, unused): the CSR rows of an n-row index; `unused` are indices no row holds."""
    span, tile_rows, slots = geometry()
    rng = np.random.default_rng(seed)
    if dim == 50:
        unused = np.array([48], np.int64)
        pool = np.setdiff1d(np.arange(dim), unused)
    else:
        unused = dim - 1 - np.arange(5, dtype=np.int64)
        pool = np.unique(np.concatenate([np.arange(9000), 7 + slots * np.arange(400), rng.integers(9000, dim - 10, 600)]))
    lengths = rng.integers(0, 40, n)
    lengths[[0, n - 1]] = 0
    for row, length in zip(range(200, 209), (0, 1, 63, 64, 65, span - 1, span, span + 1, 2 * span + 3)):
        lengths[row] = length
    lengths[400:400 + tile_rows + 5] = 0
    lengths = np.minimum(lengths, len(pool))
    special = {CANCEL: ([3, 11], [2.5, -2.5]), PINF: ([3], [np.inf]), NANROW: ([3, 19], [np.nan, 1.0]), INFINF: ([3, 11], [np.inf, -np.inf]),
               ZEROS: ([3, 11], [-0.0, 0.0]), NINF: ([3], [-np.inf])}
    indptr, indices, values = [0], [], []
    for r in range(n):
        if r in special and n > NINF:
            idx, val = special[r]
            idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float32)
        else:
            idx = np.sort(rng.choice(pool, int(lengths[r]), replace=False))
            val = rng.standard_normal(len(idx)).astype(np.float32)
            val[rng.random(len(idx)) < 0.02] = np.float32(-0.0)
        indices.append(idx)
        values.append(val)
        indptr.append(indptr[-1] + len(idx))
    return (np.asarray(indptr, np.int64), np.concatenate(indices).astype(np.int32), np.concatenate(values).astype(np.float32), unused)


def build_queries(dim, unused, rng):
    """name -> (indices, values)."""
    slots = geometry()[2]
    q = {"m1": (np.array([3], np.int64), np.array([1.7], np.float32)),
         "m7": (Q7, Q7_VALUES),
         "none": (unused, np.ones(len(unused), np.float32))}
    desc = np.sort(rng.choice(np.arange(min(dim, 9000)), 20, replace=False))[::-1].copy()
    q["descending"] = (desc, rng.standard_normal(20).astype(np.float32))
    if dim == 50:
        q["m50"] = (rng.permutation(dim), rng.standard_normal(dim).astype(np.float32))          # every index there is
    else:
        big = rng.permutation(np.concatenate([np.arange(3, 900), 7 + slots * np.arange(1, 128)]))[:1024]
        assert len(big) == 1024
        q["m1024"] = (big, rng.standard_normal(1024).astype(np.float32))
        q["congruent"] = (7 + slots * np.arange(40)[::3], rng.standard_normal(14).astype(np.float32))   # one home slot: probing
    return q


class SparseState:
    def __init__(self, idx, n, dim):
        self.indptr, self.indices, self.values, unused = build_rows(n, dim, 5000 + n + dim % 97)
        self.store = idx.sparse(self.indptr, self.indices, self.values, dim)
        self.queries = build_queries(dim, unused, np.random.default_rng(6000 + n + dim % 97))
        self._oracle = {}

    def oracle(self, name):
        """(T, matched) of the contract, computed once per query."""
        if name not in self._oracle:
            T, matched = scores(self.indptr, self.indices, self.values, *self.queries[name])
            T.setflags(write=False)
            self._oracle[name] = (T, matched)
        return self._oracle[name]


def sparse_state(w, dim):
    if not hasattr(w, "sparse_states"):
        w.sparse_states = {}
    if dim not in w.sparse_states:
        w.sparse_states[dim] = SparseState(w.idx, w.n, dim)
    return w.sparse_states[dim]


def same_column(got, want, what):
    nan = want != want
    assert np.array_equal(got != got, nan), (what, "NaN rows", np.flatnonzero((got != got) != nan)[:10])
    diff = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert len(diff) == 0, (what, "rows", diff[:10], got[diff[:10]], want[diff[:10]])


def same(got, want, what):
    D, I = got
    assert D.dtype == np.float32 and I.dtype == np.int64, what
    assert np.array_equal(I, want[1]), (what, "rows", I, want[1])
    assert np.array_equal(bits(D), bits(want[0])), (what, "scores", D, want[0])


# ---- the scoring launch alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "dense"])
@pytest.mark.parametrize("dim", DIMS)
def test_scores_and_matched_counts_are_the_oracles(gpu, dim, kind):
    w = world(D_DENSE, kind)
    st = sparse_state(w, dim)
    assert (len(st.store), st.store.nnz, st.store.dim) == (w.n, len(st.indices), dim)
    span = geometry()[0]
    lengths = np.diff(st.indptr)
    assert dim == 50 or {0, 1, 63, 64, 65, span - 1, span, span + 1, 2 * span + 3} <= set(lengths.tolist())
    launches = w.idx.sparse_counters()[1]
    for name, (qi, qv) in st.queries.items():
        T, matched = st.oracle(name)
        got_T, got_m = w.idx.sparse_scores(st.store, qi, qv)
        assert got_m.dtype == np.int32 and np.array_equal(got_m, matched), (dim, kind, name, np.flatnonzero(got_m != matched)[:10])
        same_column(got_T, T, (dim, kind, name))
        same_column(w.idx.sparse_scores(st.store, qi, qv, with_matched=False), T, (dim, kind, name, "no matched"))
    assert w.idx.sparse_counters()[1] == launches + 2 * len(st.queries)
    # the values that must show: a query no row shares an index with, cancellation, the non-finite rows
    T, matched = st.oracle("none")
    assert not matched.any() and not T.any()
    T, matched = st.oracle("m7")
    assert matched[CANCEL] == 2 and bits(T[CANCEL:CANCEL + 1])[0] == 0 and T[PINF] == np.inf and T[NINF] == -np.inf
    assert T[NANROW] != T[NANROW] and T[INFINF] != T[INFINF] and matched[ZEROS] == 2 and bits(T[ZEROS:ZEROS + 1])[0] == 0
    assert matched.max() > 1 and (matched == 0).sum() > 300


# ---- sparse top-k ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_sparse_search_under_every_row_set(gpu, dim, kind):
    w = world(D_DENSE, kind)
    rs, selected = w.rowset(kind)
    st = sparse_state(w, dim)
    names = list(st.queries)
    for k in KS:
        Db, Ib = w.idx.search_sparse(st.store, [st.queries[name] for name in names], k, rowset=rs)       # the queries as the grid's y
        assert Db.shape == (len(names), k)
        for i, name in enumerate(names):
            want = sparse_topk(*st.oracle(name), selected, k)
            same((Db[i], Ib[i]), want, (dim, kind, k, name, "batch"))
            D1, I1 = w.idx.search_sparse(st.store, [st.queries[name]], k, rowset=rs)
            same((D1[0], I1[0]), want, (dim, kind, k, name))
            if kind == "empty" or name == "none":
                assert (Ib[i] == -1).all() and (Db[i] == MISSING).all()
    if kind is None:
        # the special rows alone, as an unsorted list: +inf first, the two rows that score 0 (products that cancel; -0.0 and +0.0)
        # are candidates and tie to the lower row, -inf is last, the NaN rows are no result, padding behind
        rows = np.array([NINF, ZEROS, INFINF, NANROW, PINF, CANCEL], np.int64)
        D, I = w.idx.search_sparse(st.store, [st.queries["m7"]], 64, rowset=w.idx.rowset(rows))
        same((D[0], I[0]), sparse_topk(*st.oracle("m7"), rows, 64), (dim, "special rows"))
        assert I[0][:4].tolist() == [PINF, CANCEL, ZEROS, NINF] and (I[0][4:] == -1).all() and (D[0][4:] == MISSING).all()
        assert bits(D[0][:4]).tolist() == bits(np.array([np.inf, 0.0, 0.0, -np.inf], np.float32)).tolist()


def test_ties_go_to_the_lower_row(gpu):
    """Every row holds index 5 with the same weight: the k best are the k lowest selected rows, in every row-set form."""
    for kind in (None, "unsorted", "dense", "excluded"):
        w = world(D_DENSE, kind)
        rs, selected = w.rowset(kind)
        n = w.n
        store = w.idx.sparse(np.arange(n + 1), np.full(n, 5), np.full(n, 0.5, np.float32), 50)
        for k in KS:
            D, I = w.idx.search_sparse(store, [([5], [3.0])], k, rowset=rs)
            assert I[0].tolist() == np.sort(selected)[:k].tolist(), (kind, k)
            assert bits(D[0]).tolist() == bits(np.full(k, 1.5, np.float32)).tolist()


# ---- hybrid search --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,dim", [(100, 1 << 20), (512, 50), (512, 1 << 20)])
def test_hybrid_is_the_oracle_and_the_boosted_search(gpu, d, dim, kind):
    w = world(d, kind)
    rs, selected = w.rowset(kind)
    st = sparse_state(w, dim)
    s_all = w.scores(kind)
    names = list(st.queries)
    terms = {name: w.idx.rowterm(w.idx.sparse_scores(st.store, *st.queries[name], with_matched=False)) for name in names}
    for c, (w_d, w_s) in enumerate(HYBRID_WEIGHTS):
        for k in KS:
            five = [names[(c + k + i) % len(names)] for i in range(5)]
            js = [10 + c + 2 * i for i in range(5)]
            Db, Ib = w.idx.search_hybrid(st.store, w.c[js], [st.queries[name] for name in five], k, dense_weight=w_d, sparse_weight=w_s,
                                         rowset=rs, normalize_q=True)
            for i, (j, name) in enumerate(zip(js, five)):
                want = boosted(s_all[j], sparse_term(st.oracle(name)[0], w_s), w_d, k)
                same((Db[i], Ib[i]), want, (d, dim, kind, w_d, w_s, k, name, "nq = 5"))
                D1, I1 = w.idx.search_hybrid(st.store, w.c[j], [st.queries[name]], k, dense_weight=w_d, sparse_weight=w_s, rowset=rs,
                                             normalize_q=True)
                same((D1[0], I1[0]), want, (d, dim, kind, w_d, w_s, k, name, "nq = 1"))
                D2, I2 = w.idx.search_boosted(w.c[j], k, [terms[name]], [w_s], score_weight=w_d, rowset=rs, normalize_q=True)
                same((D1[0], I1[0]), (D2[0], I2[0]), (d, dim, kind, w_d, w_s, k, name, "boosted"))
                if kind == "empty":
                    assert (I1 == -1).all() and (D1 == MISSING).all()


def test_the_sparse_side_takes_part_in_the_hybrid_ranking(gpu):
    """A kernel that wrote no column cannot pass: one huge sparse weight lifts the dense ranking's last row to the front."""
    w = world(512)
    j = 12
    Dn, In = w.idx.search(w.c[j:j + 1], w.n, normalize_q=True)
    tail = int(In[0][-1])
    indptr = np.zeros(w.n + 1, np.int64)
    indptr[tail + 1:] = 1
    store = w.idx.sparse(indptr, [9], [1000.0], 50)
    D, I = w.idx.search_hybrid(store, w.c[j], [([9, 4], [1.0, 5.0])], 10, normalize_q=True)
    assert I[0][0] == tail and I[0][1:].tolist() == In[0][:9].tolist()
    assert bits(D[0][:1]).tolist() == bits(np.float32(Dn[0][-1]) + np.float32(1000.0)).tolist()
    D, I = w.idx.search_sparse(store, [([9, 4], [1.0, 5.0])], 10)
    assert I[0].tolist() == [tail] + [-1] * 9


# ---- small and empty stores -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 65, 300])
def test_small_indexes_and_rows_that_are_all_empty(gpu, n):
    from minivectordb_amd import _native
    d = 32
    x, rng = make_corpus(d, n)
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    q = ([2, 7], [1.0, -2.0])
    # every row empty: nothing matches; the hybrid search is the dense ranking
    empty = idx.sparse(np.zeros(n + 1, np.int64), [], [], 50)
    assert (len(empty), empty.nnz) == (n, 0)
    T, matched = idx.sparse_scores(empty, *q)
    assert not matched.any() and (bits(T) == 0).all()
    D, I = idx.search_sparse(empty, [q], 10)
    assert (I == -1).all() and (D == MISSING).all()
    Dh, Ih = idx.search_hybrid(empty, x[0], [q], min(n, 10), sparse_weight=0.3, normalize_q=True)
    Dd, Id = idx.search(x[:1], min(n, 10), normalize_q=True)
    same((Dh[0], Ih[0]), (Dd[0], Id[0]), (n, "all empty"))
    # one entry per row
    vals = rng.standard_normal(n).astype(np.float32)
    store = idx.sparse(np.arange(n + 1), np.full(n, 7), vals, 8)
    indptr = np.arange(n + 1)
    T, matched = scores(indptr, np.full(n, 7), vals, *q)
    got = idx.sparse_scores(store, *q)
    assert np.array_equal(bits(got[0]), bits(T)) and np.array_equal(got[1], matched) and (matched == 1).all()
    D, I = idx.search_sparse(store, [q], 64)
    same((D[0], I[0]), sparse_topk(T, matched, np.arange(n), 64), (n, "one entry per row"))
    assert (I[0][n:] == -1).all()
    idx.close()


# ---- the device variants --------------------------------------------------------------------------------------------------------

def test_device_variants_agree_and_refuse_a_capturing_stream(gpu):
    import torch
    w = world(D_DENSE)
    st = sparse_state(w, 1 << 20)
    rs, _ = w.rowset("unsorted")
    qs = [st.queries["m7"], st.queries["descending"]]
    stream = torch.cuda.Stream()
    k, off = 10, 1 << 33
    qt = torch.from_numpy(w.c[20:22]).cuda()
    Dt = torch.zeros((2, k), dtype=torch.float32, device="cuda")
    It = torch.zeros((2, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for rowset in (None, rs):
        Dw, Iw = w.idx.search_sparse(st.store, qs, k, rowset=rowset)
        w.idx.search_sparse_device(st.store, qs, k, Dt.data_ptr(), It.data_ptr(), rowset=rowset, stream=stream.cuda_stream, label_offset=off)
        stream.synchronize()
        same((Dt.cpu().numpy(), It.cpu().numpy()), (Dw, np.where(Iw >= 0, Iw + off, -1)), ("sparse device", rowset is not None))
        Dw, Iw = w.idx.search_hybrid(st.store, w.c[20:22], qs, k, dense_weight=0.3, sparse_weight=-0.7, rowset=rowset, normalize_q=True)
        w.idx.search_hybrid_device(st.store, qt.data_ptr(), qs, k, Dt.data_ptr(), It.data_ptr(), dense_weight=0.3, sparse_weight=-0.7,
                                   rowset=rowset, stream=stream.cuda_stream, normalize_q=True, label_offset=off)
        stream.synchronize()
        same((Dt.cpu().numpy(), It.cpu().numpy()), (Dw, Iw + off), ("hybrid device", rowset is not None))
    counters = w.idx.sparse_counters()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        Dt.zero_()
        with pytest.raises(ValueError, match="sparse search cannot be captured"):
            w.idx.search_sparse_device(st.store, qs, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)
        with pytest.raises(ValueError, match="hybrid search cannot be captured"):
            w.idx.search_hybrid_device(st.store, qt.data_ptr(), qs, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)
    assert w.idx.sparse_counters() == counters


# ---- counters -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "unsorted", "dense", "empty"])
def test_the_counters_count(gpu, kind):
    w = world(D_DENSE, kind)
    rs, selected = w.rowset(kind)
    st = sparse_state(w, 50)
    some = 1 if len(selected) else 0                    # nothing selected: no launch
    qs = [st.queries["m7"], st.queries["m1"], st.queries["descending"]]
    calls, launches = w.idx.sparse_counters()
    boost_calls, boost_launches = w.idx.boost_counters()
    w.idx.search_sparse(st.store, qs, 10, rowset=rs)                                # one launch for the three queries
    assert w.idx.sparse_counters() == (calls + 1, launches + some)
    w.idx.search_hybrid(st.store, w.c[20:23], qs, 10, rowset=rs, normalize_q=True)   # one scoring launch and one scan per query
    assert w.idx.sparse_counters() == (calls + 2, launches + 4 * some)
    assert w.idx.boost_counters() == (boost_calls, boost_launches + 3 * some)
    w.idx.sparse_scores(st.store, *qs[0])                                            # the scoring launch alone is no search
    assert w.idx.sparse_counters() == (calls + 2, launches + 4 * some + 1)


# ---- staleness and arguments ----------------------------------------------------------------------------------------------------

def test_stale_stores_and_argument_errors(gpu):
    from minivectordb_amd import _native
    d, n = 32, 100
    x, rng = make_corpus(d, n + 10)
    idx = _native.FlatIndex(d)
    idx.add(x[:n], normalize=True)
    indptr = np.arange(n + 1, dtype=np.int64)
    cols = (np.arange(n) % 9).astype(np.int32)
    vals = rng.standard_normal(n).astype(np.float32)
    store = idx.sparse(indptr, cols, vals, 16)
    q = ([3, 8], [1.0, 0.5])
    dense = x[7]
    base = idx.search_sparse(store, [q], 5)
    # creation
    for args, msg in (((indptr[:-1], cols[:-1], vals[:-1], 16), "one sparse vector per stored row .99 vectors, 100 rows"),
                      ((indptr + 1, np.append(cols, 0), np.append(vals, 0), 16), "indptr starts at 1"),
                      ((np.r_[0, 2, 1, np.arange(3, n + 1)], cols, vals, 16), "indptr decreases at row 1"),
                      ((np.r_[0, np.arange(2, n + 2)], np.r_[5, 4, cols[1:]], np.r_[1, 1, vals[1:]], 16), "row 0 are not strictly ascending"),
                      ((np.r_[0, np.arange(2, n + 2)], np.r_[5, 5, cols[1:]], np.r_[1, 1, vals[1:]], 16), "row 0 are not strictly ascending"),
                      ((indptr, cols, vals, 8), r"holds index 8 outside \[0, 8\)"),
                      ((indptr, np.where(cols == 2, -1, cols), vals, 16), r"holds index -1 outside \[0, 16\)"),
                      ((indptr, cols, vals, 0), "dim must be in"),
                      ((indptr, cols, vals, 1 << 31), "dim must be in")):
        with pytest.raises(ValueError, match=msg):
            idx.sparse(*args)
    idx.sparse(indptr, cols, vals, (1 << 31) - 1).free()
    # queries and k
    counters = idx.sparse_counters()
    for query, msg in ((([3, 8, 3], [1.0, 2.0, 3.0]), "index 3 is listed twice"),
                       (([], []), "holds 0 terms: a query needs 1 to 1024"),
                       ((np.arange(1025) % 16, np.ones(1025)), "holds 1025 terms"),
                       (([3, 16], [1.0, 1.0]), r"index 16 is outside \[0, 16\)"),
                       (([-1], [1.0]), r"index -1 is outside \[0, 16\)")):
        with pytest.raises(ValueError, match=msg):
            idx.search_sparse(store, [query], 5)
        with pytest.raises(ValueError, match=msg):
            idx.search_hybrid(store, dense, [query], 5)
        with pytest.raises(ValueError, match=msg):
            idx.sparse_scores(store, *query)
    for k in (0, 65):
        with pytest.raises(ValueError, match="1 <= k <= 64|k must be positive"):
            idx.search_sparse(store, [q], k)
        with pytest.raises(ValueError, match="1 <= k <= 64|k must be positive"):
            idx.search_hybrid(store, dense, [q], k)
    with pytest.raises(ValueError, match="nq must be positive"):
        idx.search_sparse(store, [], 5)
    assert idx.sparse_counters() == counters                                       # a refused call counts nothing
    l2 = _native.FlatIndex(d, metric=_native.METRIC_L2)
    l2.add(x[:n])
    l2_store = l2.sparse(indptr, cols, vals, 16)
    with pytest.raises(ValueError, match="inner-product index"):
        l2.search_hybrid(l2_store, dense, [q], 5)
    same(l2.search_sparse(l2_store, [q], 5), base, "an L2 index: the sparse search never reads the dense matrix")
    with pytest.raises(ValueError, match="belongs to another index"):
        l2.search_sparse(store, [q], 5)
    # set_rows keeps the row numbers: the store stays valid
    idx.set_rows([50], x[7:8] * np.float32(3), normalize=True)
    same(idx.search_sparse(store, [q], 5), base, "after set_rows")
    D, I = idx.search_hybrid(store, dense, [q], 5, sparse_weight=0.0, normalize_q=True)
    assert sorted(I[0][:2].tolist()) == [7, 50]
    # rows added since
    idx.add(x[n:n + 5], normalize=True)
    for call in (lambda: idx.search_sparse(store, [q], 5), lambda: idx.search_hybrid(store, dense, [q], 5), lambda: idx.sparse_scores(store, *q)):
        with pytest.raises(ValueError, match="holds 100 rows, the index 105"):
            call()
    # rows removed since: renumbered, whatever the count
    store = idx.sparse(np.arange(106), np.arange(105) % 9, np.ones(105), 16)
    idx.remove_rows([3])
    with pytest.raises(ValueError, match="holds 105 rows, the index 104"):
        idx.search_sparse(store, [q], 5)
    idx.add(x[n + 5:n + 6], normalize=True)
    assert idx.ntotal == 105
    for call in (lambda: idx.search_sparse(store, [q], 5), lambda: idx.search_hybrid(store, dense, [q], 5)):
        with pytest.raises(ValueError, match="before rows were removed"):
            call()
    # a stale row set is refused as every row-set search refuses it
    store = idx.sparse(np.arange(106), np.arange(105) % 9, np.ones(105), 16)
    rs = idx.rowset(np.arange(10, dtype=np.int64))
    idx.search_sparse(store, [q], 5, rowset=rs)
    idx.remove_rows([0])
    store2 = idx.sparse(np.arange(105), np.arange(104) % 9, np.ones(104), 16)
    with pytest.raises(ValueError, match="another state of the index"):
        idx.search_sparse(store2, [q], 5, rowset=rs)
    # reset: every store is stale; an empty index takes an empty store
    idx.reset()
    with pytest.raises(ValueError, match="holds 104 rows, the index 0"):
        idx.search_sparse(store2, [q], 5)
    nothing = idx.sparse(np.zeros(1, np.int64), [], [], 16)
    D, I = idx.search_sparse(nothing, [q], 5)
    assert (I == -1).all() and (D == MISSING).all()
    idx.add(x[:104], normalize=True)
    with pytest.raises(ValueError, match="before rows were removed"):
        idx.search_sparse(store2, [q], 5)
    for i in (idx, l2):
        i.close()
