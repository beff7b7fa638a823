"""Range search for batches on the device: the shared pass (fp16 nomination against per-query floors, exact re-score, gated
fallback) and per-query thresholds.

The claim is BIT IDENTITY: with option "range_shared" = 2 (the shape-eligible route whatever the sizes) a call returns the
counts, D.view(uint32) and I of the same call with "range_shared" = 0 (one fp32 pass per query), and those of the single-query
`search` with k = count.  Shapes are the smallest that reach every form: n no multiple of the 32-row tile, a partial 32-query
group, more than one 128 / 256-query chunk, a ragged last chunk."""
import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.4028234663852886e38)


def gaussian(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


_CORPUS = {}


def corpus(n, d):
    """Unit rows with a cluster (dense neighbourhoods for the first queries) and exact duplicates; computed once per shape."""
    if (n, d) not in _CORPUS:
        x = gaussian(n, d, 1000 + d)
        centre = gaussian(1, d, 7)[0]
        x[:600] += 2.0 * centre
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x[300:310] = x[299]
        x[n - 3:] = x[299]
        x.setflags(write=False)
        _CORPUS[(n, d)] = x
    return _CORPUS[(n, d)]


def queries(x, nq, seed):
    q = gaussian(nq, x.shape[1], seed)
    near = min(nq, 6)
    q[:near] = x[np.arange(near) * 50 + 299] * 3.0 + 0.2 * q[:near]     # inside the cluster, not normalised
    return q


def build(native, n, d, x=None):
    idx = native.FlatIndex(d)
    idx.add(corpus(n, d) if x is None else x)
    return idx


def both_routes(idx, q, thr, cap, rowset=None, normalize_q=True, expect_shared=True):
    """(counts, D, I) of the shared route, asserted equal to the per-query route's."""
    idx.set_option("range_shared", 0)
    want = idx.range_search_raw(q, thr, cap, rowset, normalize_q)
    idx.set_option("range_shared", 2)
    before = idx.range_counters()[0]
    got = idx.range_search_raw(q, thr, cap, rowset, normalize_q)
    assert idx.range_counters()[0] - before == (1 if expect_shared else 0)
    assert np.array_equal(got[0], want[0]), (got[0][:10], want[0][:10])
    if cap:
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(got[2], want[2])
    return got


def own_thresholds(idx, q, normalize_q=True, k=200):
    """Per query: its 1st, 10th and 200th best exact score (single-query search), by turns; then one above every score and -inf."""
    thr = np.empty(len(q), np.float32)
    top = []
    for i in range(len(q)):
        D, I = idx.search(q[i:i + 1], k, normalize_q=normalize_q)
        top.append((D[0], I[0]))
        thr[i] = D[0][(0, 9, k - 1)[i % 3]]
    return thr, top


@pytest.mark.parametrize("n,d,nq,normalize_q", [(4_999, 128, 2, True), (20_001, 512, 33, True), (4_999, 1024, 130, False),
                                                (20_001, 128, 300, True), (4_999, 512, 300, False), (4_999, 384, 33, True)])
def test_shared_pass_is_bit_identical(gpu, n, d, nq, normalize_q):
    from minivectordb_amd import _native
    idx = build(_native, n, d)
    q = queries(corpus(n, d), nq, 31)
    thr, top = own_thresholds(idx, q, normalize_q)
    hi = nq - 1
    lo = nq - 2 if nq > 2 else 0
    thr[hi] = np.float32(1e30)            # above every score
    thr[lo] = -np.inf                     # every row: the candidates overflow (fallback) and so does the small cap
    cap = 256
    counts, D, I = both_routes(idx, q, thr, cap, normalize_q=normalize_q)
    assert counts[hi] == 0 and counts[lo] == n
    assert (I[lo] == -1).all() and (D[lo] == -FMAX).all()
    assert idx.range_counters()[1] >= 1
    for i in range(nq):
        if i in (hi, lo):
            continue
        want = (1, 10, 200)[i % 3]
        c = int(counts[i])
        assert c >= want and c <= cap, (i, c)          # (ties at the threshold may add rows)
        Dw, Iw = top[i]
        m = min(c, len(Dw))
        assert np.array_equal(D[i, :m].view(np.uint32), Dw[:m].view(np.uint32)) and np.array_equal(I[i, :m], Iw[:m]), i
        assert (D[i, :c] >= thr[i]).all() and (I[i, c:] == -1).all()
    # one threshold for the whole batch takes the same route
    both_routes(idx, q, float(thr[1 % nq]) if nq > 2 else 0.5, cap, normalize_q=normalize_q)
    # cap == 0: the counts of the full results
    c0 = both_routes(idx, q, thr, 0, normalize_q=normalize_q)[0]
    assert np.array_equal(c0, counts)
    idx.close()


def test_boundaries_ties_and_signed_zero(gpu):
    from minivectordb_amd import _native
    n, d, nq = 4_999, 512, 33
    x = corpus(n, d).copy()
    x[10, :] = -0.0
    x[11, :] = 0.0
    idx = build(_native, n, d, x)
    q = queries(x, nq, 32)
    _, top = own_thresholds(idx, q, normalize_q=False, k=20)
    at = np.array([top[i][0][4] for i in range(nq)], np.float32)          # the 5th best stored score of each query
    counts, D, I = both_routes(idx, q, at, 64, normalize_q=False)
    above = np.nextafter(at, np.float32(np.inf))
    counts_above = both_routes(idx, q, above, 64, normalize_q=False)[0]
    for i in range(nq):
        assert counts[i] == int((top[i][0] >= at[i]).sum()) >= 5 and counts_above[i] == int((top[i][0] > at[i]).sum()) < counts[i], i
        assert np.array_equal(I[i, :counts[i]], top[i][1][:counts[i]])
    # duplicated rows: 299, 300 .. 309 and the last three rows hold the same vector — ties go to the lower row
    dup = np.array([299] + list(range(300, 310)) + [n - 3, n - 2, n - 1])
    qd = np.tile(x[299], (2, 1))
    s = idx.search(qd[:1], 1)[0][0, 0]
    c, Dd, Id = both_routes(idx, qd, np.array([s, s], np.float32), 32, normalize_q=False)
    assert c.tolist() == [len(dup)] * 2 and Id[0, :len(dup)].tolist() == dup.tolist()
    # signed zeros: a zero query scores +-0.0 everywhere; 0.0 and -0.0 as thresholds both select every row
    qz = np.zeros((2, d), np.float32)
    c, _, _ = both_routes(idx, qz, np.array([0.0, -0.0], np.float32), 0, normalize_q=False)
    assert c.tolist() == [n, n]
    # ... and rows of zeros against real queries: score +-0.0, included at 0.0 and at -0.0, excluded just above
    qs = queries(x, 2, 33)
    rs = idx.rowset(np.setdiff1d(np.arange(n), [10, 11]).astype(np.int64), excluded=True)
    assert rs.is_bitmap
    c, _, Iz = both_routes(idx, qs, np.array([0.0, -0.0], np.float32), 8, rowset=rs, normalize_q=False)
    assert c.tolist() == [2, 2] and sorted(Iz[0, :2].tolist()) == [10, 11]
    tiny = np.float32(1e-30)
    assert both_routes(idx, qs, np.array([tiny, tiny], np.float32), 8, rowset=rs, normalize_q=False)[0].tolist() == [0, 0]
    idx.close()


def test_row_sets(gpu):
    from minivectordb_amd import _native
    n, d, nq = 20_001, 128, 33
    idx = build(_native, n, d)
    q = queries(corpus(n, d), nq, 34)
    thr, _ = own_thresholds(idx, q)
    rng = np.random.default_rng(35)
    half = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
    others = np.setdiff1d(np.arange(n), half).astype(np.int64)
    bitmap = idx.rowset(others, excluded=True)                     # a 50 % set in bitmap form
    excluded = idx.rowset(np.arange(290, 320, dtype=np.int64), excluded=True)
    listed = idx.rowset(rng.permutation(n)[:3_000].astype(np.int64))
    assert bitmap.is_bitmap and excluded.is_bitmap and not listed.is_bitmap
    for rs, rows in ((bitmap, half), (excluded, np.setdiff1d(np.arange(n), np.arange(290, 320)))):
        counts, D, I = both_routes(idx, q, thr, 512, rowset=rs)
        for i in range(0, nq, 5):
            c = int(counts[i])
            assert c <= 512 and np.isin(I[i, :c], rows).all()
            Dw, Iw = idx.search_rowset(q[i:i + 1], c + 1, rs, normalize_q=True)
            assert np.array_equal(D[i, :c].view(np.uint32), Dw[0, :c].view(np.uint32)) and np.array_equal(I[i, :c], Iw[0, :c])
            assert Iw[0, c] == -1 or Dw[0, c] < thr[i]
    # a list-form set keeps the per-query route
    both_routes(idx, q, thr, 512, rowset=listed, expect_shared=False)
    idx.close()
    # ... and so does an index that holds a row with a NaN
    x = corpus(n, d).copy()
    x[77, 5] = np.nan
    odd = build(_native, n, d, x)
    counts, _, I = both_routes(odd, q, thr, 512, expect_shared=False)
    assert not (I == 77).any()
    odd.close()


def test_fallbacks(gpu):
    from minivectordb_amd import _native
    n, d, nq = 4_999, 512, 130
    idx = build(_native, n, d)
    q = queries(corpus(n, d), nq, 36)
    thr, _ = own_thresholds(idx, q)
    thr[::3] = np.float32(0.02)                                      # about a third of the corpus each: far more than 64 candidates
    idx.set_option("range_candidates", 64)
    before = idx.range_counters()[1]
    counts, D, I = both_routes(idx, q, thr, 4096)
    assert idx.range_counters()[1] - before >= len(thr[::3])
    assert (counts[::3] > 1000).all() and (counts[::3] <= 4096).all() and (I[::3, 0] >= 0).all()
    idx.set_option("range_candidates", 0)
    before = idx.range_counters()[1]
    q[5] = 0.0                                                       # a zero query scores 0 everywhere
    thr[5] = 0.0
    counts = both_routes(idx, q, thr, 0)[0]
    assert counts[5] == n and idx.range_counters()[1] - before >= 1
    with pytest.raises(ValueError):
        idx.set_option("range_candidates", 63)
    with pytest.raises(ValueError):
        idx.set_option("range_shared", 3)
    idx.close()


def test_launch_counts(gpu):
    from minivectordb_amd import _native
    n, d, nq = 4_999, 512, 130
    idx = build(_native, n, d)
    q = queries(corpus(n, d), nq, 37)
    thr, _ = own_thresholds(idx, q)
    idx.set_option("range_shared", 2)
    idx.range_search_raw(q, thr, 256, normalize_q=True)              # builds the shadow
    fb = idx.range_counters()[1]
    _native.prof_enable(True)
    try:
        for label in ("ip_scan_range", "ip_scan_range_half", "ip_scan_range_rescore", "ip_scan_range_fallback"):
            _native.prof_read(label)
        counts = idx.range_search_raw(q, thr, 256, normalize_q=True)[0]
        scans = _native.prof_read("ip_scan_range")[0]
        passes = _native.prof_read("ip_scan_range_half")[0]
        rescores = _native.prof_read("ip_scan_range_rescore")[0]
        gated, gated_ms = _native.prof_read("ip_scan_range_fallback")
        symbol = _native.prof_symbol("ip_scan_range_half")
    finally:
        _native.prof_enable(False)
    assert idx.range_counters()[1] == fb and (counts <= 256).all()      # no query fell back
    per_pass = _native.half_max_queries(d)                           # queries one pass over the shadow serves at this width
    assert scans == 0 and 1 <= passes <= -(-nq // per_pass) and rescores == 1, (scans, passes, rescores)
    # the structure of a call: one gated launch of the thresholded scan per launch group, whose blocks all return at once here
    # (a scan of 4,999 x 512 for 130 queries would take far longer than a millisecond)
    assert gated == 1 and gated_ms < 1.0, (gated, gated_ms)
    assert symbol.startswith("range_nominate_h16_kernel<"), symbol
    idx.close()


def test_device_entry_and_graph(gpu):
    import torch
    from minivectordb_amd import _native
    n, d, nq, cap, off = 20_001, 512, 33, 300, 1_000_000
    idx = build(_native, n, d)
    idx.set_option("range_shared", 2)
    x = corpus(n, d)
    stream = torch.cuda.Stream()
    qt = torch.zeros((nq, d), dtype=torch.float32, device="cuda")
    tt = torch.zeros(nq, dtype=torch.float32, device="cuda")
    ct = torch.zeros(nq, dtype=torch.int64, device="cuda")
    Dt = torch.zeros((nq, cap), dtype=torch.float32, device="cuda")
    It = torch.zeros((nq, cap), dtype=torch.int64, device="cuda")

    def enqueue():
        idx.range_search_device(qt.data_ptr(), nq, 0.0, cap, ct.data_ptr(), Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream,
                                normalize_q=True, label_offset=off, thresholds_ptr=tt.data_ptr())

    def load(seed):
        q = queries(x, nq, seed)
        thr, _ = own_thresholds(idx, q)
        thr[nq - 1] = -np.inf
        qt.copy_(torch.from_numpy(q))
        tt.copy_(torch.from_numpy(thr))
        torch.cuda.synchronize()
        return q, thr

    def check(q, thr, what):
        idx.set_option("range_shared", 0)
        cw, Dw, Iw = idx.range_search_raw(q, thr, cap, normalize_q=True)
        idx.set_option("range_shared", 2)
        assert np.array_equal(ct.cpu().numpy(), cw), what
        assert cw[nq - 1] == n and (cw[:nq - 1] <= cap).all()
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), Dw.view(np.uint32)), what
        assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + off, -1)), what

    q, thr = load(40)
    calls = idx.range_counters()[0]
    with torch.cuda.stream(stream):
        enqueue()
    stream.synchronize()
    assert idx.range_counters()[0] == calls + 1
    check(q, thr, "eager")
    # a NaN threshold on the device matches nothing
    tn = thr.copy()
    tn[3] = np.nan
    tt.copy_(torch.from_numpy(tn))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        enqueue()
    stream.synchronize()
    assert ct.cpu().numpy()[3] == 0 and (It.cpu().numpy()[3] == -1).all()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    assert idx.range_counters()[0] == calls + 3                      # the captured call took the shared route too
    for r in range(2):
        q, thr = load(41 + r)
        ct.fill_(-9)
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(q, thr, f"replay {r}")
    del g
    idx.close()


def test_host_argument_errors(gpu):
    from minivectordb_amd import _native
    idx = build(_native, 4_999, 128)
    q = queries(corpus(4_999, 128), 4, 44)
    c = np.full(4, -7, np.int64)
    t = np.array([0.1, np.nan, 0.2, 0.3], np.float32)
    rc = _native.lib().mvdb_index_range_search_each(idx._h, _native._ptr(q), 4, _native._ptr(t), 0, None, 0, _native._ptr(c), None, None)
    assert rc != 0 and (c == -7).all()                               # MVDB_ERR_ARG before anything is enqueued
    with pytest.raises(ValueError):
        idx.range_search(q, [0.1, 0.2])
    with pytest.raises(ValueError):
        idx.range_count(q, [0.1, np.nan, 0.2, 0.3])
    l2 = _native.FlatIndex(128, metric=flat.METRIC_L2)
    l2.add(corpus(4_999, 128))
    l2.set_option("range_shared", 2)
    radius = np.array([0.5, 1.5, 1.9, 0.0], np.float32)
    counts, D, I = l2.range_search_raw(q / np.linalg.norm(q, axis=1, keepdims=True), radius, 4_999)
    assert l2.range_counters()[0] == 0                               # L2 keeps the per-query passes
    for i in range(4):
        one = l2.range_search_raw(q[i:i + 1] / np.linalg.norm(q[i]), float(radius[i]), 4_999)
        assert counts[i] == one[0][0] and np.array_equal(D[i].view(np.uint32), one[1][0].view(np.uint32)) and np.array_equal(I[i], one[2][0])
    assert counts[1] < counts[2] and counts[3] == 0
    l2.close()
    idx.close()


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_drop_in_classes_with_one_min_score_per_query(tmp_path, gpu, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    n, d, nq = 20_001, 128, 33
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "r.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=4096)
    x = corpus(n, d)
    db.store_embeddings_batch(list(range(n)), x, [{"tenant": i % 5} for i in range(n)])
    q = queries(x, nq, 45)
    db.find_most_similar(q[0], k=1)                                  # builds the device index
    db.index.set_option("range_shared", 2)
    scores = [float(s) for s in np.linspace(0.05, 0.6, nq)]
    for f in ({}, {"exclude_filter": {"tenant": 2}}):
        before = db.index.range_counters()[0]
        many = db.find_all_similar_batch(q, scores, **f)
        counts = db.count_similar_batch(q, scores, **f)
        assert db.index.range_counters()[0] > before
        assert sum(counts) > nq
        for i in range(nq):
            one = db.find_all_similar(q[i], scores[i], **f)
            assert counts[i] == len(one[0]) == db.count_similar(q[i], scores[i], **f)
            assert list(many[i][0]) == list(one[0]) and list(many[i][2]) == list(one[2])
            assert np.array_equal(np.asarray(many[i][1], np.float32).view(np.uint32), np.asarray(one[1], np.float32).view(np.uint32))
    with pytest.raises(ValueError):
        db.find_all_similar_batch(q, scores[:-1])


def test_against_the_float64_oracle(gpu):
    """Every row at or above t + (d + 8) 2^-24 in float64 is returned, none below t - that (rows of unit norm, unit queries)."""
    from minivectordb_amd import _native
    n, d, nq = 20_001, 512, 33
    x = corpus(n, d)
    idx = build(_native, n, d)
    idx.set_option("range_shared", 2)
    q = queries(x, nq, 46)
    qn = (q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True))
    s64 = qn @ x.astype(np.float64).T
    thr = np.sort(s64, axis=1)[np.arange(nq), -np.array([(3, 40, 400)[i % 3] for i in range(nq)])].astype(np.float32)
    tol = (d + 8) * 2.0 ** -24
    lims, D, I = idx.range_search(q, thr, normalize_q=True)
    assert idx.range_counters()[0] >= 1 and lims[-1] > 40 * (nq // 3)
    for i in range(nq):
        got = set(I[lims[i]:lims[i + 1]].tolist())
        must = set(np.flatnonzero(s64[i] >= float(thr[i]) + tol).tolist())
        may = set(np.flatnonzero(s64[i] >= float(thr[i]) - tol).tolist())
        assert must <= got <= may, (i, len(must), len(got), len(may))
        assert (np.abs(D[lims[i]:lims[i + 1]] - s64[i][I[lims[i]:lims[i + 1]]]) <= tol).all()
    idx.close()


@pytest.mark.parametrize("d", [384, 640, 768, 896])
def test_shadow_widths_batch_search_and_range_against_the_oracle(gpu, monkeypatch, d):
    """The widths of the fp16-shadow kernels that the shapes above leave out, 130 queries over 4,999 rows: one 256-query pass up
    to d = 512, two 128-query passes above; a ragged last tile; fewer tiles (157) than workgroups x ring depth, so every block's
    look-ahead runs past its last tile.  (The certified search of so small a corpus is nominated by its seed launch alone; the
    range pass streams the shadow.)  Search: float64 adjudication of every query and distances within 1e-4 of the fp32 oracle's.
    Range: every row at or above t + (d + 8) 2^-24 in float64 is returned, none below t - that (unit rows, unit queries)."""
    from minivectordb_amd import _native
    monkeypatch.setenv("MVDB_SPLIT_SCAN_MIN_NQ", "24")               # read when the index is created
    n, nq, k = 4_999, 130, 10
    x = flat.synth(n, d, 1234)
    flat.normalize_l2(x)
    q = flat.synth(nq, d, 777)
    flat.normalize_l2(q)
    idx = _native.FlatIndex(d)
    idx.add(x)
    _native.prof_enable(True)
    try:
        _native.prof_read("ip_scan_half_seed")
        D, I = idx.search(q, k)
        assert _native.prof_read("ip_scan_half_seed")[0] >= 1, "the certified pass did not run"
    finally:
        _native.prof_enable(False)
    Do, Io = flat.flat_search(x, q, k)
    for i in range(nq):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], tol=1e-4)
        assert ok, f"query {i}: {msg}"
    np.testing.assert_allclose(D, Do, atol=1e-4, rtol=0)

    idx.set_option("range_shared", 2)
    s64 = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True) @ x.astype(np.float64).T
    thr = np.sort(s64, axis=1)[np.arange(nq), -np.array([(3, 40, 400)[i % 3] for i in range(nq)])].astype(np.float32)
    tol = (d + 8) * 2.0 ** -24
    before = idx.range_counters()[0]
    lims, Dr, Ir = idx.range_search(q, thr, normalize_q=True)
    assert idx.range_counters()[0] > before and lims[-1] > 40 * (nq // 3)
    for i in range(nq):
        got = set(Ir[lims[i]:lims[i + 1]].tolist())
        must = set(np.flatnonzero(s64[i] >= float(thr[i]) + tol).tolist())
        may = set(np.flatnonzero(s64[i] >= float(thr[i]) - tol).tolist())
        assert must <= got <= may, (i, len(must), len(got), len(may))
        assert (np.abs(Dr[lims[i]:lims[i + 1]] - s64[i][Ir[lims[i]:lims[i + 1]]]) <= tol).all()
    idx.close()
