"""Search by examples on the device (mvdb_index_search_examples, csrc/examples_scan.hpp): every comparison is exact.  The
oracle's input is the library's own single-query bits, as in tests/test_assign_gpu.py — for each example j the full ranking of
the selected rows, idx.search / search_rowset of v[j] alone with k = the rows selected, scattered into a [P + N, n] matrix (a
row the ranking leaves out scored NaN) — and tests/examples_oracle.py is the contract in numpy.  Scores are compared as bits,
rows as integers.

Corpus, row sets and vectors are that file's World: 2,051 rows of 64 Gaussian clusters (4,099 for the dense-bitmap form), 70
perturbed stored rows of which vector 3 is all zeros, vector 6 holds a NaN and vector 40 is a copy of vector 5.  A call's
positives are the first P of them and its negatives the next N: (20, 12) and (20, 13) carry the zero and the NaN vector among
the positives, (3, 2) the zero vector among the negatives, (40, 30) the twin of positive 5 among the negatives.

Vectors per pass: Vp = min(P + N, 32, 128 KiB / (4 ld)) (include/mvdb.h), lowered by the index option
examples_vectors_per_pass: (20, 12) is exactly one pass of 32, (20, 13) the smallest two-pass call, and its first pass
straddles the positive / negative boundary."""
import numpy as np
import pytest

from examples_oracle import branches, examples
from kmeans_oracle import vectors_per_pass
from maxsim_oracle import MISSING
from test_assign_gpu import NANV, TWIN, TWIN_OF, ZERO, bits, make_corpus, world

pytestmark = pytest.mark.gpu

DIMS = [30, 100, 384, 512, 1024]
SHAPES = [(1, 0), (1, 1), (3, 2), (20, 12), (20, 13), (40, 30)]
KINDS = [None, "unsorted", "dense", "excluded", "empty"]


def same(got, want, what):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64, what
    assert np.array_equal(got[1], want[1]), (what, "rows", got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, "scores", got[0], want[0])


def run_and_check(w, P, N, k, kind=None, knob=0, skip=None, what=""):
    """One call against the contract, the counters included.  Returns what the call returned."""
    rs, selected = w.rowset(kind)
    want = examples(w.scores(kind)[:P + N], P, k, skip if skip is not None else ())
    calls0, passes0 = w.idx.examples_counters()
    got = w.idx.search_examples(w.c[:P], w.c[P:P + N], k, rowset=rs, skip_rows=skip, normalize=True)
    calls1, passes1 = w.idx.examples_counters()
    vp = vectors_per_pass(P + N, (w.d + 3) // 4 * 4, knob)
    expected = -(-(P + N) // vp) if len(selected) else 0
    print(f"{what} d={w.d} P={P} N={N} k={k} set={kind} knob={knob}: passes {passes1 - passes0} (expected {expected})")
    same(got, want, (what, w.d, P, N, k, kind, knob))
    assert calls1 - calls0 == 1 and passes1 - passes0 == expected, (what, passes1 - passes0, expected)
    hit = got[1] >= 0
    assert np.isin(got[1][hit], selected).all() and (got[0][~hit] == MISSING).all()
    return got


# ---- widths, example counts, k, row sets --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_every_width_shape_and_row_set(gpu, d, kind):
    w = world(d, kind)
    rs, selected = w.rowset(kind)
    assert kind not in ("dense", "excluded") or rs.is_bitmap
    assert kind != "unsorted" or not rs.is_bitmap
    for P, N in SHAPES:
        for k in ((1, 10, 64) if (P, N) in ((3, 2), (20, 13)) else (10,)):
            D, I = run_and_check(w, P, N, k, kind)
            if kind == "empty":
                assert (I == -1).all() and (D == MISSING).all()
            else:
                assert (I >= 0).all() and len(set(I.tolist())) == k


def test_results_do_not_depend_on_the_vectors_per_pass(gpu):
    from minivectordb_amd import _native
    for d in (100, 512):
        w = world(d)
        base = {s: run_and_check(w, *s, 64) for s in ((3, 2), (20, 13))}
        try:
            for knob in (1, 5):
                w.idx.set_option("examples_vectors_per_pass", knob)
                for kind in (None, "unsorted", "excluded"):
                    for s in ((3, 2), (20, 13)):                                   # 5 and 33 passes at 1, 1 and 7 at 5
                        got = run_and_check(w, *s, 64, kind, knob=knob)
                        if kind is None:
                            same(got, base[s], ("knob", d, knob, s))
            with pytest.raises(ValueError, match="examples_vectors_per_pass"):
                w.idx.set_option("examples_vectors_per_pass", 33)
            with pytest.raises(ValueError, match="examples_vectors_per_pass"):
                w.idx.set_option("examples_vectors_per_pass", -1)
            with pytest.raises(ValueError, match="examples_vectors_per_pass"):
                w.idx.set_option("no_such_option", 1)                              # the message names every option
        finally:
            w.idx.set_option("examples_vectors_per_pass", 0)
    # the option survives a reset, like its siblings
    x, _ = make_corpus(100, 200)
    idx = _native.FlatIndex(100)
    idx.set_option("examples_vectors_per_pass", 5)
    idx.add(x, normalize=True)
    idx.reset()
    idx.add(x, normalize=True)
    idx.search_examples(x[:4], x[4:7], 3, normalize=True)
    assert idx.examples_counters() == (1, 2)
    idx.close()


# ---- one positive is the single-query search ----------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_one_positive_is_the_single_query_search_minus_the_skip_rows(gpu, d):
    for kind in (None, "unsorted", "dense", "excluded"):
        w = world(d, kind)
        rs, selected = w.rowset(kind)
        for j in (0, ZERO, 11):
            if j == ZERO and kind == "unsorted":
                # every row scores 0: search_rowset breaks the tie by LIST position, this call by physical row number
                for k in (1, 64):
                    got = w.idx.search_examples(w.c[j:j + 1], None, k, rowset=rs, normalize=True)
                    same(got, examples(w.scores(kind)[j:j + 1], 1, k), ("ties in a list", d, k))
                    assert got[1].tolist() == np.sort(selected)[:k].tolist() and bits(got[0]).tolist() == [0] * k
                continue
            q = w.c[j:j + 1]
            for k in (1, 10, 64):
                want = w.idx.search(q, k, normalize_q=True) if rs is None else w.idx.search_rowset(q, k, rs, normalize_q=True)
                same(w.idx.search_examples(q, None, k, rowset=rs, normalize=True), (want[0][0], want[1][0]), ("search", d, kind, j, k))
            # skip the best three, the seventh and a row that is not selected anyway (twice: duplicates are allowed)
            full = w.idx.search(q, 70, normalize_q=True) if rs is None else w.idx.search_rowset(q, 70, rs, normalize_q=True)
            outside = np.setdiff1d(np.arange(w.n), selected)[:1]
            skip = np.concatenate([full[1][0][[0, 1, 2, 6]], outside, outside, full[1][0][[1]]]).astype(np.int64)
            keep = ~np.isin(full[1][0], skip)
            got = w.idx.search_examples(q, None, 64, rowset=rs, skip_rows=skip, normalize=True)
            same(got, (full[0][0][keep][:64], full[1][0][keep][:64]), ("skip", d, kind, j))
            same(got, examples(w.scores(kind)[j:j + 1], 1, 64, skip), ("skip oracle", d, kind, j))


# ---- both branches of the rule in one result ------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [30, 100, 512])
def test_both_branches_of_the_rule_in_one_result(gpu, d):
    w = world(d)
    for P, N in SHAPES[1:]:
        bp, bn, has = branches(w.scores()[:P + N], P)
        assert has.all()
        gap = bn.astype(np.float64) - bp.astype(np.float64)
        by_gap = np.argsort(gap, kind="stable")
        rows = np.concatenate([by_gap[-30:], by_gap[:30]]).astype(np.int64)       # the 30 most "negative" rows, the 30 most "positive"
        rows = rows[np.random.default_rng(P).permutation(60)]                      # a list-form set, unsorted
        rs = w.idx.rowset(rows)
        assert not rs.is_bitmap
        s = np.full((P + N, w.n), np.nan, np.float32)
        for j in range(P + N):
            Dj, Ij = w.idx.search_rowset(w.c[j:j + 1], 60, rs, normalize_q=True)
            s[j, Ij[0][Ij[0] >= 0]] = Dj[0][Ij[0] >= 0]
        want = examples(s, P, 64)
        closer = (bp > bn)[want[1][:60]]
        print(f"d={d} P={P} N={N}: {int(closer.sum())} rows score bp, {int((~closer).sum())} score -(bn * bn)")
        assert closer.sum() >= 10 and (~closer).sum() >= 10 and (want[1][60:] == -1).all() and (want[1][:60] >= 0).all()
        same(w.idx.search_examples(w.c[:P], w.c[P:P + N], 64, rowset=rs, normalize=True), want, ("branches", d, P, N))
        rs.close()


def test_a_negative_equal_to_the_only_positive_ranks_least_similar_first(gpu):
    for d in (100, 384):
        w = world(d)
        q = w.c[11:12]
        s = w.scores()[11]
        D, I = w.idx.search_examples(q, q, 64, normalize=True)
        same((D, I), examples(np.stack([s, s]), 1, 64), ("twin sides", d))
        assert np.array_equal(bits(D), bits(-(s[I] * s[I])))                       # bp == bn on every row: never greater
        assert I[0] == np.argmin(s * s) and (np.diff(np.abs(s[I])) >= 0).all()     # least similar first


# ---- NaN and zero vectors, equal rows -----------------------------------------------------------------------------------------

def test_nan_and_zero_vectors(gpu):
    w = world(100)
    c, s = w.c, w.scores()
    plain = w.idx.search_examples(c[10:13], c[20:22], 10, normalize=True)
    same(plain, examples(s[[10, 11, 12, 20, 21]], 3, 10), "plain")
    # a NaN vector among the positives and among the negatives never offers
    pos = c[[10, NANV, 11, 12]]
    neg = c[[20, NANV, 21]]
    got = w.idx.search_examples(pos, neg, 10, normalize=True)
    same(got, plain, "nan vectors change nothing")
    same(got, examples(s[[10, NANV, 11, 12, 20, NANV, 21]], 4, 10), "nan vectors, oracle")
    # the only positive holds a NaN: all padding, whatever the negatives
    for neg in (None, c[20:22]):
        D, I = w.idx.search_examples(c[NANV:NANV + 1], neg, 5, normalize=True)
        assert (I == -1).all() and (D == MISSING).all()
    # only NaN negatives: bn = -inf, the per-row maximum over the positives
    same(w.idx.search_examples(c[10:13], c[NANV:NANV + 1], 10, normalize=True), w.idx.search_examples(c[10:13], None, 10, normalize=True), "nan negative")
    # the zero vector is not normalised: it scores 0 on every row
    D, I = w.idx.search_examples(c[ZERO:ZERO + 1], None, 7, normalize=True)
    assert I.tolist() == list(range(7)) and bits(D).tolist() == [0] * 7           # equal S: the lower row
    same(w.idx.search_examples(c[10:13], c[ZERO:ZERO + 1], 64, normalize=True), examples(s[[10, 11, 12, ZERO]], 3, 64), "zero negative")
    # normalize = 0: the vectors as they are
    raw = np.full((3, w.n), np.nan, np.float32)
    for j in range(3):
        Dj, Ij = w.idx.search(c[j:j + 1], w.n, normalize_q=False)
        raw[j, Ij[0]] = Dj[0]
    same(w.idx.search_examples(c[:2], c[2:3], 10, normalize=False), examples(raw, 2, 10), "raw")
    # the twin of a positive among the negatives, in another pass (the (40, 30) shape): its rows take the other branch
    bp, bn, _ = branches(s[:70], 40)
    assert TWIN >= 40 and (bp == bn).any() and (s[TWIN_OF] == s[TWIN]).all()


def test_a_stored_row_with_a_nan_and_two_equal_rows(gpu):
    from minivectordb_amd import _native
    d, n = 100, 300
    x, rng = make_corpus(d, n)
    x[77, 3] = np.nan
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    stored = idx.get_rows(0, n)
    idx.set_rows(np.array([250], np.int64), stored[17:18])                          # a copy of row 17 at row 250
    v = np.ascontiguousarray(np.concatenate([stored[17:18], x[[5, 9]] + np.float32(0.01), x[[200, 201]] + np.float32(0.01)]))
    s = np.full((5, n), np.nan, np.float32)
    for j in range(5):
        Dj, Ij = idx.search(v[j:j + 1], n, normalize_q=True)
        s[j, Ij[0][Ij[0] >= 0]] = Dj[0][Ij[0] >= 0]
    assert np.isnan(s[:, 77]).all() and not np.isnan(np.delete(s, 77, axis=1)).any()
    for k in (2, 64):
        D, I = idx.search_examples(v[:3], v[3:], k, normalize=True)
        same((D, I), examples(s, 3, k), ("nan row", k))
        assert I[:2].tolist() == [17, 250] and bits(D[:1]) == bits(D[1:2]) and 77 not in I   # equal rows tie: the lower row first
    rs = idx.rowset(np.array([250, 30, 17, 77], np.int64))                          # a list that names the higher twin first
    D, I = idx.search_examples(v[:1], None, 4, rowset=rs, normalize=True)
    assert I.tolist() == [17, 250, 30, -1] and D[3] == MISSING                      # ... still the lower physical row
    idx.close()


def test_empty_index(gpu):
    from minivectordb_amd import _native
    idx = _native.FlatIndex(100)
    D, I = idx.search_examples(np.ones((3, 100), np.float32), np.ones((2, 100), np.float32), 4, normalize=True)
    assert (I == -1).all() and (D == MISSING).all() and idx.examples_counters() == (1, 0)
    idx.close()


# ---- the device variant -------------------------------------------------------------------------------------------------------

def _device_call(idx, v, P, N, k, rowset=None, skip=None, stream=0, label_offset=0):
    """search_examples_device on prefilled tensors: (error, D, I) as numpy, whatever the call did."""
    import torch
    vt = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(skip, dtype=np.int64)).cuda() if skip is not None and len(skip) else None
    Dt = torch.full((64,), 7.5, dtype=torch.float32, device="cuda")
    It = torch.full((64,), 777, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        idx.search_examples_device(vt.data_ptr(), P, N, k, Dt.data_ptr(), It.data_ptr(), rowset=rowset,
                                   skip_rows_ptr=st.data_ptr() if st is not None else 0, n_skip=len(skip) if st is not None else 0,
                                   stream=stream, normalize=True, label_offset=label_offset)
        err = None
    except ValueError as e:
        err = e
    torch.cuda.synchronize()
    return err, Dt.cpu().numpy(), It.cpu().numpy()


def _untouched(res):
    err, D, I = res
    return isinstance(err, ValueError) and (D == 7.5).all() and (I == 777).all()


def test_host_and_device_variants_agree(gpu):
    import torch
    stream = torch.cuda.Stream()
    for d, (P, N), k, kind in ((30, (3, 2), 10, None), (384, (20, 13), 64, "unsorted"), (512, (40, 30), 7, "dense"),
                               (100, (1, 1), 1, "excluded"), (100, (3, 2), 5, "empty")):
        w = world(d, kind)
        rs, selected = w.rowset(kind)
        skip = np.array([selected[0], selected[-1], selected[0]], np.int64) if len(selected) else np.array([4, 4], np.int64)
        host = w.idx.search_examples(w.c[:P], w.c[P:P + N], k, rowset=rs, skip_rows=skip, normalize=True)
        same(host, examples(w.scores(kind)[:P + N], P, k, skip), ("host", d, P, N, kind))
        for s in (0, stream.cuda_stream):
            err, D, I = _device_call(w.idx, w.c[:P + N], P, N, k, rs, skip, stream=s, label_offset=1000)
            assert err is None and (D[k:] == 7.5).all() and (I[k:] == 777).all()  # nothing behind the k results is written
            same((D[:k], np.where(I[:k] >= 0, I[:k] - 1000, -1)), host, ("device", d, P, N, kind, s))
            assert ((I[:k] >= 1000) | (I[:k] == -1)).all()                         # padding stays -1 under a label offset
        # a skip row outside the index: the device variant reads nothing back and ignores it
        err, D, I = _device_call(w.idx, w.c[:P + N], P, N, k, rs, np.concatenate([skip, [w.n, -1, 1 << 40]]))
        assert err is None
        same((D[:k], I[:k]), host, ("device, rows outside", d, kind))


# ---- argument errors ------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(gpu):
    from minivectordb_amd import _native
    w = world(100)
    other = world(384)
    v = w.c[:5]
    before = w.idx.examples_counters()
    assert _untouched(_device_call(w.idx, v, 0, 5, 3))                              # P = 0
    assert _untouched(_device_call(w.idx, v, 3, -1, 3))
    big = np.zeros((257, 100), np.float32)
    assert _untouched(_device_call(w.idx, big, 200, 57, 3))                         # P + N = 257
    assert _untouched(_device_call(w.idx, v, 3, 2, 65))                             # k = 65
    assert _untouched(_device_call(w.idx, v, 3, 2, 0))
    with pytest.raises(ValueError, match="at least one positive"):
        w.idx.search_examples(np.zeros((0, 100), np.float32), v, 3)
    with pytest.raises(ValueError, match="P \\+ N <= 256"):
        w.idx.search_examples(big[:200], big[:57], 3)
    w.idx.search_examples(big[:200] + 1, big[:56] + 1, 3)                           # 256 examples are accepted
    before = (before[0] + 1, before[1] + 8)
    with pytest.raises(ValueError, match="k <= 64"):
        w.idx.search_examples(v[:3], v[3:], 65)
    with pytest.raises(ValueError):
        w.idx.search_examples(np.zeros((3, 101), np.float32), None, 3)
    # a skip row out of range (the host variant checks them), too many skip rows
    for bad in ([5, w.n], [-1], [1 << 40]):
        with pytest.raises(ValueError, match="skip row"):
            w.idx.search_examples(v[:3], v[3:], 3, skip_rows=bad)
    with pytest.raises(ValueError, match="n_skip"):
        w.idx.search_examples(v[:3], v[3:], 3, skip_rows=np.zeros(1025, np.int64))
    assert _untouched(_device_call(w.idx, v, 3, 2, 3, skip=np.zeros(1025, np.int64)))
    w.idx.search_examples(v[:3], v[3:], 3, skip_rows=np.arange(1024))               # 1024 are accepted
    before = (before[0] + 1, before[1] + 1)
    # a foreign row set, and one the index has outgrown by an add
    foreign, _ = other.rowset("unsorted")
    res = _device_call(w.idx, v, 3, 2, 3, rowset=foreign)
    assert _untouched(res) and "another index" in str(res[0])
    with pytest.raises(ValueError, match="another index"):
        w.idx.search_examples(v[:3], v[3:], 3, rowset=foreign)
    x, _ = make_corpus(100, 200)
    idx = _native.FlatIndex(100)
    idx.add(x, normalize=True)
    # (rows appended behind a set are simply not part of it — the library's rule for every row-set search: an add alone
    #  outdates nothing; a removal or a reset renumbers the rows, and the set is stale from then on, whatever is added after)
    for excluded in (False, True):
        for shrink in ("remove", "reset"):
            held = idx.rowset(np.array([1, 5, 9], np.int64), excluded=excluded)
            idx.add(x[:3], normalize=True)
            n_then, n_now = idx.ntotal - 3, idx.ntotal
            calls = idx.examples_counters()[0]
            D, I = idx.search_examples(v[:3], v[3:], 64, rowset=held, normalize=True)
            assert idx.examples_counters()[0] == calls + 1 and (I < n_then).all()
            hits = I[I >= 0].tolist()
            assert sorted(hits) == [1, 5, 9] if not excluded else len(hits) == 64 and not set(hits) & {1, 5, 9}
            if shrink == "remove":
                idx.remove_rows(np.array([0], np.int64))
            else:
                idx.reset()
            idx.add(x[:5] if shrink == "remove" else x, normalize=True)             # a stale row set, after an add
            calls = idx.examples_counters()
            res = _device_call(idx, v, 3, 2, 3, rowset=held)
            assert _untouched(res) and "another state" in str(res[0])
            with pytest.raises(ValueError, match="another state"):
                idx.search_examples(v[:3], v[3:], 3, rowset=held)
            assert idx.examples_counters() == calls and n_now > 0
    idx.close()
    # an L2 index
    l2 = _native.FlatIndex(100, metric=1)
    l2.add(x)
    assert _untouched(_device_call(l2, v, 3, 2, 3))
    with pytest.raises(ValueError, match="inner-product"):
        l2.search_examples(v[:3], v[3:], 3)
    l2.close()
    assert w.idx.examples_counters() == before
