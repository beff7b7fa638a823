"""mvdb_index_range_search on the device: every selected row whose score reaches a threshold.

The core claim is BIT IDENTITY with the library's own top-k path: the results of a query are — D.view(uint32) and I element for
element — the leading `count` entries of search / search_rowset with nq = 1 and k = count + 8, and the entry behind them is
below the threshold, for every (G, C) shape choose_shape returns, both metrics, with and without the fused query
normalisation, under no set / a sorted list / an unsorted list / a bitmap / an excluded set, for data holding NaN, +-inf,
-0.0 and exact duplicate rows.  One convention of the k > 64 route is accounted for where the comparison is made
(`reference`): it reports a row whose score is NaN with score -inf, while a range search never returns such a row.
The independent float64 oracle bounds what may be returned and what may be missed around the threshold."""
import threading
import time

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

DIMS = [16, 30, 64, 100, 256, 384, 512, 640, 1024, 1280, 1536, 1792, 2048, 2304]   # tests/test_grouped_gpu.py's list
NQ = 8
FMAX = np.float32(3.4028234663852886e38)


def gaussian(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def spike(x, q):
    """NaN, +-inf, -0.0 and exact duplicate rows / queries (in place)."""
    n = x.shape[0]
    x[7, 3] = np.nan
    x[8, 0] = np.inf
    x[9, 1] = -np.inf
    x[10, :] = -0.0
    x[100:110] = x[99]
    x[n - 5:] = x[99]
    q[3, 2] = np.nan
    q[4, 0] = np.inf
    q[5, ::2] = -0.0
    q[6, :] = 0.0
    q[7] = x[99]


SPECIAL_ROWS = np.array([7, 8, 9, 10, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109])


def make_sets(idx, n, seed):
    """[(name, RowSet | None, the rows the set selects in tie order)]"""
    rng = np.random.default_rng(seed)
    tail = np.arange(n - 5, n)

    def pick(m):
        rows = np.union1d(np.union1d(rng.choice(n, m, replace=False), SPECIAL_ROWS), tail)
        return np.sort(rows).astype(np.int64)

    sorted_list = pick(5_000)
    unsorted = rng.permutation(pick(2_000))
    dense = np.setdiff1d(np.arange(n), rng.choice(n, n // 20, replace=False)).astype(np.int64)
    excluded = np.sort(rng.choice(np.arange(200, n - 10), 100, replace=False)).astype(np.int64)
    out = [("no set", None, np.arange(n, dtype=np.int64)),
           ("sorted list", idx.rowset(sorted_list), sorted_list),
           ("unsorted list", idx.rowset(unsorted), unsorted),
           ("dense bitmap", idx.rowset(dense), dense),
           ("excluded set", idx.rowset(excluded, excluded=True), np.setdiff1d(np.arange(n), excluded)),
           ("empty set", idx.rowset(np.empty(0, np.int64)), np.empty(0, np.int64))]
    assert [bool(rs is not None and rs.is_bitmap) for _, rs, _ in out] == [False, False, False, True, True, False]
    return out


def key_scores_f64(x, q, rows, metric, normalize_q):
    """Restatement of the key score (IP: q.x, L2: -|q - x|^2) of `rows` against q — used ONLY to tell which rows score NaN or
    -inf: NaN comes from NaN elements, inf * 0 and inf - inf, -inf from an infinite term, and neither depends on the summation
    order or the precision (Gaussian data does not overflow).  A finite query can only score so against a row that holds a
    non-finite element: the other rows are not computed (0 stands for "finite")."""
    q = q.astype(np.float64)
    with np.errstate(all="ignore"):
        if normalize_q:
            nr = (q * q).sum()
            if nr > 0:
                q = q * (1.0 / np.sqrt(nr))
        out = np.zeros(len(rows), np.float64)
        odd = np.flatnonzero(np.isin(rows, ODD_ROWS)) if np.isfinite(q).all() else np.arange(len(rows))
        for lo in range(0, len(odd), 4096):
            at = odd[lo:lo + 4096]
            xs = x[rows[at]].astype(np.float64)
            out[at] = (xs * q).sum(axis=1) if metric == flat.METRIC_IP else -((q - xs) ** 2).sum(axis=1)
        return out


ODD_ROWS = np.array([7, 8, 9])   # the rows spike() gives a non-finite element


def reference(idx, q1, rs, k, metric, normalize_q):
    """The single-query top-k of the existing path, nq = 1, without missing markers.  Rows whose score is NaN are in no top-k
    list at any k, and rows scoring -inf are listed last, under a bitmap too: the range result is
    compared with it as it stands."""
    if rs is None:
        D, I = idx.search(q1[None], int(k), normalize_q=normalize_q)
    else:
        D, I = idx.search_rowset(q1[None], int(k), rs, normalize_q=normalize_q)
    keep = I[0] >= 0
    return D[0][keep], I[0][keep]


def check_query(idx, x, q1, rs, rows, t, got_D, got_I, metric, normalize_q, what):
    s64 = key_scores_f64(x, q1, rows, metric, normalize_q)
    nan_set = set(rows[np.isnan(s64)].tolist())
    ip = metric == flat.METRIC_IP
    assert (got_D >= t).all() if ip else (got_D <= t).all(), what
    assert not (set(got_I.tolist()) & nan_set), what                  # rows with NaN scores never match
    count = len(got_D)
    Dw, Iw = reference(idx, q1, rs, count + 8, metric, normalize_q)
    assert not (set(Iw.tolist()) & nan_set), what                     # ... and are in no top-k list either
    assert len(Dw) >= count, (what, len(Dw), count)
    same = (got_I == Iw[:count]) & (got_D.view(np.uint32) == Dw[:count].view(np.uint32))
    if not same.all():
        j = int(np.flatnonzero(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {count} entries differ; first at {j}: range "
                             f"({got_D[j]!r}, {got_I[j]}) top-k ({Dw[j]!r}, {Iw[j]})")
    if len(Dw) > count:     # the entry behind the last match is on the other side of the threshold
        assert (Dw[count] < t) if ip else (Dw[count] > t), (what, Dw[count], t)


def rows_of(d):
    return 20_000 if d < 1280 else 8_000


@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2], ids=["ip", "l2"])
@pytest.mark.parametrize("d", DIMS)
def test_range_is_bit_identical_to_the_top_k_path(gpu, d, metric):
    from minivectordb_amd import _native
    n = rows_of(d)
    x = gaussian(n, d, 1000 + d)
    q = gaussian(NQ, d, 2000 + d)
    spike(x, q)
    idx = _native.FlatIndex(d, metric=metric)
    idx.add(x)
    ip = metric == flat.METRIC_IP
    everything, nothing = (-np.inf, np.inf) if ip else (np.inf, -np.inf)
    try:
        cases = make_sets(idx, n, 3000 + d)
        for name, rs, rows in cases:
            for normalize_q in (False, True):
                what = f"d={d} metric={metric} set={name} normalize_q={normalize_q}"
                if len(rows) == 0:
                    lims, D, I = idx.range_search(q, everything, rowset=rs, normalize_q=normalize_q)
                    assert lims.tolist() == [0] * (NQ + 1) and len(D) == 0 and len(I) == 0, what
                    assert idx.range_count(q, everything, rowset=rs, normalize_q=normalize_q).tolist() == [0] * NQ
                    continue
                # stored scores to aim at: each query's 20th and 37th best (NaN / inf queries have none)
                top = []
                for i in range(NQ):
                    top.append(reference(idx, q[i], rs, 64, metric, normalize_q)[0])
                aims = [float(t[19]) for t in top if len(t) > 36 and np.isfinite(t[19])]
                shared = float(np.median(aims))
                # above every finite score (rows 8 and 9 score +-inf against most queries: only the all-zero query 6 and the
                # NaN query 3 are sure to match nothing); L2: a negative distance
                beyond = (max(float(v) for t in top for v in t if np.isfinite(v)) + 1.0) if ip else -1.0
                for t in (shared, everything, nothing, beyond):
                    lims, D, I = idx.range_search(q, t, rowset=rs, normalize_q=normalize_q)
                    counts = idx.range_count(q, t, rowset=rs, normalize_q=normalize_q)
                    assert lims[0] == 0 and np.array_equal(np.diff(lims), counts), what
                    for i in range(NQ):
                        check_query(idx, x, q[i], rs, rows, np.float32(t), D[lims[i]:lims[i + 1]], I[lims[i]:lims[i + 1]], metric,
                                    normalize_q, f"{what} t={t} query {i}")
                    if t == shared:
                        assert (counts > 0).sum() >= 3, (what, counts)
                    if t == beyond:                                   # queries matching nothing
                        assert counts[3] == 0 and counts[6] == 0 and (ip or not counts.any()), (what, counts)
                    if t == everything:
                        bad = np.isnan(key_scores_f64(x, q[0], rows, metric, normalize_q)).sum()
                        assert counts[0] == len(rows) - bad and counts[3] == 0, (what, counts)   # query 3 holds a NaN
                # a threshold exactly equal to a stored score: >= (L2: <=) includes that row
                for i in (0, 7):
                    t = top[i][36]
                    assert np.isfinite(t), (what, i)
                    lims, D, I = idx.range_search(q[i:i + 1], float(t), rowset=rs, normalize_q=normalize_q)
                    assert lims[1] >= 37 and D[36:37].view(np.uint32)[0] == np.array([t]).view(np.uint32)[0], (what, i, lims)
                    check_query(idx, x, q[i], rs, rows, t, D, I, metric, normalize_q, f"{what} stored score, query {i}")
        for _, rs, _ in cases:
            if rs is not None:
                rs.close()
    finally:
        idx.close()


def test_ties_and_empty_index(gpu):
    from minivectordb_amd import _native
    d, n = 512, 4096
    x = np.tile(gaussian(1, d, 5), (n, 1))
    idx = _native.FlatIndex(d)
    q = np.tile(x[:1], (2, 1))
    lims, D, I = idx.range_search(q, -np.inf)                       # an empty index: counts 0
    assert lims.tolist() == [0, 0, 0] and len(D) == 0
    assert idx.range_count(q, 0.0).tolist() == [0, 0]
    idx.add(x)
    score = idx.search(q[:1], 1)[0][0, 0]
    rows = np.array([900, 17, 3000, 17, 5, 2222], np.int64)
    rs = idx.rowset(rows)
    lims, D, I = idx.range_search(q, float(score), rowset=rs)
    assert lims.tolist() == [0, 6, 12] and I[:6].tolist() == rows.tolist() and I[6:].tolist() == rows.tolist()   # list positions
    lims, D, I = idx.range_search(q[:1], float(score))
    assert lims.tolist() == [0, n] and I.tolist() == list(range(n)) and (D.view(np.uint32) == score.view(np.uint32)).all()
    assert idx.range_count(q, float(np.nextafter(score, np.float32(np.inf)))).tolist() == [0, 0]
    idx.close()


@pytest.mark.parametrize("d,thresholds", [(128, (0.10, 0.15, 0.20, 0.25)), (512, (0.10,))])
def test_range_against_the_float64_oracle(gpu, d, thresholds):
    """200,000 normalised synthetic rows, 16 queries (half of them perturbed corpus rows).  With s64 the float64 score and
    delta = (d + 8) * 2^-24 — the worst-case fp32 dot-product error for unit vectors in any summation order, plus the query
    normalisation — every row with s64 >= t + delta is returned, no row with s64 < t - delta is, every returned score is
    within 1e-4 of s64.  Rows inside the band may fall either way, but they must stay below 1 % of the rows at or above t,
    and at least 1,000 rows must be at or above t."""
    from minivectordb_amd import _native
    n, nq = 200_000, 16
    idx = _native.FlatIndex(d)
    idx.add(flat.synth(n, d, 71), normalize=True)
    x = idx.get_rows(0, n)
    q = flat.synth(nq, d, 73)
    q[::2] = x[np.arange(0, 8) * 20_011 + 5] + 0.3 * q[::2] / np.linalg.norm(q[::2], axis=1, keepdims=True)
    qn = q.copy()
    flat.normalize_l2(qn)
    every = np.arange(n, dtype=np.int64)
    s64 = np.stack([flat.scores_f64(x, qn[i], every) for i in range(nq)])
    delta = (d + 8) * 2.0 ** -24
    for t in thresholds:
        lims, D, I = idx.range_search(q, t, normalize_q=True)
        at_or_above = in_band = 0
        for i in range(nq):
            got_I, got_D = I[lims[i]:lims[i + 1]], D[lims[i]:lims[i + 1]]
            assert len(set(got_I.tolist())) == len(got_I)
            returned = np.zeros(n, bool)
            returned[got_I] = True
            must = s64[i] >= t + delta
            never = s64[i] < t - delta
            assert returned[must].all(), (d, t, i, int((must & ~returned).sum()))
            assert not returned[never].any(), (d, t, i, int((never & returned).sum()))
            assert np.abs(got_D.astype(np.float64) - s64[i][got_I]).max(initial=0.0) < 1e-4, (d, t, i)
            assert (np.diff(got_D) <= 0).all()
            at_or_above += int((s64[i] >= t).sum())
            in_band += int((~must & ~never).sum())
        print(f"[range vs oracle] d={d} t={t}: {at_or_above} rows at or above t, {in_band} inside the band "
              f"({100.0 * in_band / max(at_or_above, 1):.3f} %)")
        assert at_or_above >= 1_000, (d, t, at_or_above)
        assert in_band <= 0.01 * at_or_above, (d, t, in_band, at_or_above)
    idx.close()


def test_capacity(gpu):
    from minivectordb_amd import _native
    d, n = 64, 400_000
    idx = _native.FlatIndex(d)
    idx.add_synthetic(n, 31)
    q = flat.synth(5, d, 32)
    t = 0.3
    counts = idx.range_count(q, t, normalize_q=True)                 # cap = 0, D and I NULL
    assert (counts > 0).all() and len(set(counts.tolist())) > 1, counts
    full = idx.range_search(q, t, normalize_q=True, cap=int(counts.max()))
    assert np.array_equal(np.diff(full[0]), counts)
    cap = int(np.sort(counts)[2])                                    # the two largest overflow, three fit
    c, D, I = idx.range_search_raw(q, t, cap, normalize_q=True)
    assert np.array_equal(c, counts) and 1 <= (counts > cap).sum() <= 2 and (counts <= cap).sum() >= 3
    for i in range(5):
        if counts[i] > cap:                                          # only missing markers, the count still true
            assert (I[i] == -1).all() and (D[i] == -FMAX).all()
        else:                                                        # the neighbours are complete
            m = counts[i]
            assert np.array_equal(I[i, :m], full[2][full[0][i]:full[0][i + 1]])
            assert np.array_equal(D[i, :m].view(np.uint32), full[1][full[0][i]:full[0][i + 1]].view(np.uint32))
            assert (I[i, m:] == -1).all() and (D[i, m:] == -FMAX).all()
    for small in (1, 4, cap):                                        # the wrapper's second call returns everything
        got = idx.range_search(q, t, normalize_q=True, cap=small)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, full)), small
    # L2 markers
    l2 = _native.FlatIndex(d, metric=flat.METRIC_L2)
    l2.add(idx.get_rows(0, 1000))
    c, D, I = l2.range_search_raw(q[:1], 1e9, 10)
    assert c[0] == 1000 and (I == -1).all() and (D == FMAX).all()
    l2.close()
    # a dense result: more than 100,000 rows for one query, sorted and complete
    lims, D, I = idx.range_search(q[:2], 0.0, normalize_q=True)
    assert lims[1] >= 100_000 and lims[2] - lims[1] >= 100_000, lims
    for i in range(2):
        m = int(lims[i + 1] - lims[i])
        Dw, Iw = idx.search(q[i:i + 1], m + 8, normalize_q=True)
        assert np.array_equal(I[lims[i]:lims[i + 1]], Iw[0, :m])
        assert np.array_equal(D[lims[i]:lims[i + 1]].view(np.uint32), Dw[0, :m].view(np.uint32))
        assert Dw[0, m] < 0.0 and D[lims[i + 1] - 1] >= 0.0
    idx.close()


def _raw(_native, idx, q, t, cap, rs, counts, D, I, nq=None):
    return _native.lib().mvdb_index_range_search(idx._h, _native._ptr(q), q.shape[0] if nq is None else nq, t, 0,
                                                 rs._h if rs is not None else None, cap, _native._ptr(counts), _native._ptr(D),
                                                 _native._ptr(I))


def test_errors_leave_the_outputs_untouched(gpu):
    from minivectordb_amd import _native
    d, n = 64, 5_000
    x = gaussian(n, d, 11)
    q = gaussian(4, d, 12)
    idx, other = _native.FlatIndex(d), _native.FlatIndex(d)
    idx.add(x)
    other.add(x)
    stale = idx.rowset(np.arange(10, 500))
    idx.remove_rows([4999])
    other.remove_rows([4999])
    fresh = idx.rowset(np.arange(0, 1000, 3))
    foreign = other.rowset(np.arange(0, 1000, 3))
    foreign_bitmap = other.rowset(np.arange(5), excluded=True)

    def sentinel():
        return np.full(4, -55, np.int64), np.full((4, 5), 123.0, np.float32), np.full((4, 5), -77, np.int64)

    def untouched(c, D, I):
        return (c == -55).all() and (D == 123.0).all() and (I == -77).all()

    for t, cap, rs, nq in ((float("nan"), 5, None, 4), (0.0, -1, None, 4), (0.0, 5, stale, 4), (0.0, 5, foreign, 4),
                           (0.0, 5, foreign_bitmap, 4), (0.0, 5, fresh, 0), (0.0, 0, stale, 4)):
        c, D, I = sentinel()
        assert _raw(_native, idx, q, t, cap, rs, c, D, I, nq=nq) == _native.ERR_ARG, (t, cap, nq)
        assert untouched(c, D, I), (t, cap, nq)
    c, D, I = sentinel()
    assert _native.lib().mvdb_index_range_search(idx._h, _native._ptr(q), 4, 0.0, 0, None, 5, _native._ptr(c), None,
                                                 _native._ptr(I)) == _native.ERR_ARG          # cap > 0 needs D and I
    assert untouched(c, D, I)
    for call in (lambda: idx.range_search(gaussian(4, d + 1, 13), 0.0), lambda: idx.range_count(gaussian(4, d + 1, 13), 0.0),
                 lambda: idx.range_search(q, float("nan")), lambda: idx.range_search(q, 0.0, cap=-1),
                 lambda: idx.range_search(q, 0.0, rowset=stale), lambda: idx.range_search(q, 0.0, rowset=foreign)):
        with pytest.raises(ValueError):
            call()
    c, D, I = sentinel()
    idx.range_search_raw(q, 1e9, 5, rowset=fresh, out=(c, D, I))     # ... and a good call writes everything
    assert (c == 0).all() and (I == -1).all() and (D == -FMAX).all()
    assert np.diff(other.range_search(q, 0.0, rowset=foreign)[0]).sum() > 0     # each set still serves its own index
    idx.close()
    other.close()


def test_device_entry_stream_graph_and_label_offset(gpu):
    import torch
    from minivectordb_amd import _native
    d, n, nq, off = 512, 60_000, 6, 5_000_000
    idx = _native.FlatIndex(d)
    x = gaussian(n, d, 21)
    base = gaussian(1, d, 20)[0]
    x[:5000] += base                                                 # a cluster: the query `base` has a dense neighbourhood
    idx.add(x, normalize=True)
    rng = np.random.default_rng(22)
    listed = idx.rowset(rng.permutation(n)[:20_000].astype(np.int64))           # an unsorted list
    bitmap = idx.rowset(np.arange(5), excluded=True)
    stream = torch.cuda.Stream()
    qt = torch.zeros((nq, d), dtype=torch.float32, device="cuda")
    # (threshold, cap, set): one LDS tile; several tiles and global steps; a pure count
    for t, cap, rs in ((0.08, 3000, None), (0.02, 30_000, bitmap), (0.05, 5000, listed), (0.0, 0, listed)):
        ct = torch.zeros(nq, dtype=torch.int64, device="cuda")
        Dt = torch.zeros((nq, max(cap, 1)), dtype=torch.float32, device="cuda")
        It = torch.zeros((nq, max(cap, 1)), dtype=torch.int64, device="cuda")

        def enqueue():
            idx.range_search_device(qt.data_ptr(), nq, t, cap, ct.data_ptr(), Dt.data_ptr() if cap else 0,
                                    It.data_ptr() if cap else 0, rowset=rs, stream=stream.cuda_stream, normalize_q=True,
                                    label_offset=off)

        def check(q, what):
            cw, Dw, Iw = idx.range_search_raw(q, t, cap, rowset=rs, normalize_q=True)
            assert np.array_equal(ct.cpu().numpy(), cw), what
            assert (cw > 0).all() and (cap == 0 or ((cw <= cap).sum() >= 2 and (cw > 64).any())), (what, cw)
            assert rs is not None or cw[1] > cap, (what, cw)          # the clustered query overflows the small capacity
            if cap:
                assert np.array_equal(Dt.cpu().numpy().view(np.uint32), Dw.view(np.uint32)), what
                assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + off, -1)), what

        q0 = gaussian(nq, d, 23)
        q0[1] = base
        qt.copy_(torch.from_numpy(q0))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue()
        stream.synchronize()
        check(q0, f"eager, caller stream, cap={cap}")
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue()
        for r in range(2):
            qr = gaussian(nq, d, 30 + r)
            qr[1] = base + 0.1 * qr[1]
            qt.copy_(torch.from_numpy(qr))
            ct.fill_(-9)
            Dt.zero_()
            It.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            check(qr, f"replay {r}, cap={cap}")
    idx.close()


def _metadata(n):
    return [{"tenant": i % 50, "lang": ("en", "de", "fr")[i % 3]} for i in range(n)]


FILTERS = [{}, {"metadata_filter": {"tenant": 7}}, {"exclude_filter": {"lang": "de"}},
           {"or_filters": [{"tenant": 3}, {"tenant": 4}]}, {"metadata_filter": {"tenant": 21, "lang": "en"}},
           {"metadata_filter": {"tenant": 99}}]


def _check_drop_in(db, q, min_score):
    nonempty = 0
    for f in FILTERS:
        many = db.find_all_similar_batch(q, min_score, **f)
        for i in range(q.shape[0]):
            got = db.find_all_similar(q[i], min_score, **f)
            count = db.count_similar(q[i], min_score, **f)
            assert count == len(got[0]) and list(many[i][0]) == list(got[0])
            assert np.array_equal(np.asarray(many[i][1], np.float32).view(np.uint32), np.asarray(got[1], np.float32).view(np.uint32))
            if count == 0:
                assert got == ([], [], [])
                continue
            nonempty += 1
            want = db.find_most_similar(q[i], k=count, **f)
            assert type(got) is type(want) and all(type(a) is type(b) for a, b in zip(got, want))
            assert list(got[0]) == list(want[0]) and list(got[2]) == list(want[2]), (i, f)
            assert all(type(s) is np.float32 for s in got[1])
            assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), (i, f)
            more = db.find_most_similar(q[i], k=count + 1, **f)
            assert len(more[0]) == count or more[1][count] < min_score
            cut = db.find_all_similar(q[i], min_score, limit=3, **f)
            assert list(cut[0]) == list(want[0][:3]) and list(cut[2]) == list(want[2][:3])
    return nonempty


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_drop_in_classes(tmp_path, gpu, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    n, d = 200_000, 128
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "r.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=4096)
    x = flat.synth(n + 10, d, 51)
    db.store_embeddings_batch(list(range(n)), x[:n], _metadata(n))
    q = flat.synth(6, d, 52)
    q[0] = x[7] / np.linalg.norm(x[7]) + 0.05 * q[0] / np.linalg.norm(q[0])   # near tenant 7's row 7
    assert _check_drop_in(db, q, 0.25) >= 12
    assert 7 in db.find_all_similar(q[0], 0.9)[0]
    # after a store: the new rows are found (a near-duplicate check before a store)
    assert db.count_similar(x[n], 0.999) == 0
    db.store_embeddings_batch(list(range(n, n + 10)), x[n:], _metadata(n + 10)[n:])
    assert db.find_all_similar(x[n], 0.999)[0] == (n,)
    assert _check_drop_in(db, q, 0.25) >= 12
    # after a delete: the row is gone, everything else still agrees with find_most_similar
    if kind == "flat":
        db.delete_embedding(7)
    else:
        db.delete_embeddings_batch([7])
    assert 7 not in db.find_all_similar(q[0], 0.5)[0]
    assert _check_drop_in(db, q, 0.25) >= 12


def test_classes_without_a_range_search_say_so(tmp_path, gpu):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    from minivectordb_amd.distributed import DistributedShardedVectorDatabase
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=4096)
    x = flat.synth(2_000, 128, 55)
    db.store_embeddings_batch(list(range(2_000)), x, _metadata(2_000))
    assert len(db.find_most_similar(x[0], k=3)[0]) == 3
    for obj in (db, object.__new__(DistributedShardedVectorDatabase)):
        for call in (lambda: obj.find_all_similar(x[0], 0.5), lambda: obj.find_all_similar_batch(x[:2], 0.5),
                     lambda: obj.count_similar(x[0], 0.5)):
            with pytest.raises(NotImplementedError, match="range search"):
                call()


def test_threads_find_all_similar_while_storing_and_deleting(tmp_path, gpu):
    """Four threads call find_all_similar / count_similar while a fifth stores and deletes (the manner of
    test_threads_each_while_storing_and_deleting): no exception beyond the ValueError / IndexError a search racing a delete may
    raise there, every id returned existed."""
    from minivectordb_amd import VectorDatabase
    d, base, extra = 64, 4_000, 600
    x = flat.synth(base + extra, d, 61)
    db = VectorDatabase(storage_file=str(tmp_path / "t.pkl"))
    db.store_embeddings_batch(list(range(base)), x[:base], [{"tenant": i % 20} for i in range(base)])
    errs, stop, served, overflowed = [], threading.Event(), [0, 0, 0, 0], [0, 0, 0, 0]

    def searcher(s):
        try:
            q = flat.synth(32, d, 700 + s)
            i = 0
            while not stop.is_set():
                i += 1
                # every other call is unfiltered with a floor of 0: about half of the >= 4,000 rows match, more than the wrapper's
                # default capacity of 1,024, so its second call runs while the writer changes the index
                f, floor = ({}, 0.0) if i % 2 else ({"metadata_filter": {"tenant": (i + s) % 20}}, 0.1)
                try:
                    ids, dist, meta = db.find_all_similar(q[i % 32], floor, **f)
                    count = db.count_similar(q[i % 32], floor, **f)
                except (ValueError, IndexError):
                    continue
                served[s] += 1
                overflowed[s] += len(ids) > 1024
                assert len(ids) == len(dist) == len(meta) and count >= 0
                assert all(0 <= u < base + extra for u in ids)
                assert all(a >= b for a, b in zip(dist, dist[1:])) and all(v >= floor for v in dist)
        except Exception as e:  # pragma: no cover
            errs.append(("s", e))

    def writer():
        try:
            for i in range(extra):
                uid = base + i
                db.store_embedding(uid, x[uid], {"tenant": uid % 20})
                if i % 3 == 0:
                    db.delete_embedding(i)
                    time.sleep(0.01)
        except Exception as e:  # pragma: no cover
            errs.append(("w", e))
        finally:
            stop.set()

    ts = [threading.Thread(target=searcher, args=(s,)) for s in range(4)] + [threading.Thread(target=writer)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert all(c > 0 for c in served), f"calls answered per searcher while the writer ran: {served}"
    assert all(c > 0 for c in overflowed), f"calls that needed the second, larger call per searcher: {overflowed}"
    q = flat.synth(20, d, 800)
    for t in range(20):
        ids, dist, meta = db.find_all_similar(q[t], 0.1, metadata_filter={"tenant": t})
        assert all(m["tenant"] == t for m in meta)
        assert list(ids) == list(db.find_most_similar(q[t], k=max(len(ids), 1), metadata_filter={"tenant": t})[0][:len(ids)])
