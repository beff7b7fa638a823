"""The single-query int8 prefilter route (option "code8_single_query") against the same index with the
option off: D (as bits) and I equal element for element, and the route really served the calls it claims (the launch recorded
under "ip_scan" is code8_scan_kernel, the code holds every row)."""
import os

import numpy as np
import pytest

from oracle import flat

import bigcheck

pytestmark = pytest.mark.gpu

FAMILIES = {"zero_mean": 0, "positive": flat.SYNTH_POSITIVE, "clustered": flat.SYNTH_CLUSTERED}


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _queries(nq, d, seed=5678):
    q = flat.synth(nq, d, seed)
    flat.normalize_l2(q)
    return q


def _same(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, a[1], b[1])


def _both(native, idx, q, k, normalize_q=False, expect_route=True, what=""):
    """Searches every query of q one per call with the option off, then on; asserts equality; returns the results."""
    idx.set_option("code8_single_query", 0)
    want = [idx.search(qi, k, normalize_q=normalize_q) for qi in q]
    idx.set_option("code8_single_query", 1)
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        got = [idx.search(qi, k, normalize_q=normalize_q) for qi in q]
        sym = native.prof_symbol("ip_scan")
        launches = native.prof_read("ip_scan")[0]
    finally:
        native.prof_enable(False)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"{what} query {i}")
    if expect_route:
        assert sym.startswith("code8_scan_kernel<"), (what, sym)
        assert launches == len(q), (what, launches)
        assert idx.code8_rows == idx.ntotal, what
    else:
        assert sym.startswith("flat_scan_kernel<"), (what, sym)
    return got


@pytest.mark.parametrize("d", [384, 512, 1024])
@pytest.mark.parametrize("n", [499_999, 500_000, 640_000])
def test_dims_sizes_k_and_query_normalisation(native, d, n):
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(6, d)
    for k in (1, 10, 64):
        for normalize_q in (False, True):
            qs = q * np.float32(3.25) if normalize_q else q
            _both(native, idx, qs, k, normalize_q, expect_route=n >= 500_000, what=f"d={d} n={n} k={k} normalize_q={normalize_q}")
    if n < 500_000:
        assert idx.code8_rows == 0
    assert idx.shadow_rows == 0   # the fp16 shadow is not this route's business
    idx.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_families_at_1m_rows(native, family):
    n, d, k = 1_000_000, 512, 10
    flag = FAMILIES[family]
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flag, normalize=True)
    q = flat.synth(32, d, 5678 | flag)
    flat.normalize_l2(q)
    counts = []
    idx.set_option("code8_single_query", 1)
    for qi in q:
        idx.search(qi, k)
        counts.append(idx.code8_counters()[1])
    _both(native, idx, q, k, what=family)
    fallbacks, _, calls = idx.code8_counters()
    print(f"code8 {family} 1M x 512: candidates min/median/max {min(counts)}/{int(np.median(counts))}/{max(counts)}, "
          f"fallbacks {fallbacks} of {calls} calls")
    if family != "clustered":
        assert fallbacks == 0, (family, fallbacks, calls)
    idx.close()


def test_duplicates_and_ties(native):
    n, d, k = 600_000, 512, 10
    rs = np.random.RandomState(5)
    q = _queries(4, d)
    # every row the same: every score ties, the lowest rows win; the candidates overflow and the call falls back
    row = _queries(1, d, seed=77)
    idx = native.FlatIndex(d)
    idx.add(np.repeat(row, n, axis=0))
    got = _both(native, idx, q, k, what="identical rows")
    assert np.array_equal(got[0][1][0], np.arange(k))
    assert idx.code8_counters()[0] >= len(q)
    idx.close()
    # 40 copies of the best row, scattered: they tie exactly and must come back lowest row first
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    x = idx.get_rows(0, n)
    where = np.sort(rs.choice(n, 40, replace=False))
    x[where] = q[0]
    idx.close()
    idx = native.FlatIndex(d)
    idx.add(x)
    for kk in (10, 64):
        got = _both(native, idx, q, kk, what=f"40 copies, k={kk}")
        assert np.array_equal(got[0][1][0][:min(kk, 40)], where[:min(kk, 40)])
    idx.close()


def test_special_values(native):
    n, d, k = 520_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    x = idx.get_rows(0, n)
    idx.close()
    x[7] = 0.0
    x[8] = -0.0
    x[9] = np.float32(1e-42)         # subnormals
    x[10, ::2] = np.float32(1e-40)
    x[11] = np.float32(1e-20)
    x[12, 3] = 50.0                  # one huge element
    q = _queries(5, d)
    queries = [q[0], q[1], np.zeros(d, np.float32), -np.zeros(d, np.float32), np.full(d, 1e-41, np.float32), q[2] * np.float32(1e-20)]
    # finite rows, added raw (the norm bound is measured): the route serves
    idx = native.FlatIndex(d)
    idx.add(x)
    for normalize_q in (False, True):
        _both(native, idx, np.stack(queries), k, normalize_q, what=f"finite specials normalize_q={normalize_q}")
    # queries holding NaN / inf: the call falls back on the device, same bits
    bad_q = []
    for v in (np.nan, np.inf, -np.inf):
        t = q[3].copy()
        t[5] = v
        bad_q.append(t)
    for normalize_q in (False, True):
        _both(native, idx, np.stack(bad_q), k, normalize_q, what=f"non-finite queries normalize_q={normalize_q}")
    idx.close()
    # rows holding NaN / inf, normalised on the device (the norm bound stays 1): such rows are always candidates
    x[20, 1] = np.nan
    x[21, 2] = np.inf
    x[22, 3] = -np.inf
    idx = native.FlatIndex(d)
    idx.add(x, normalize=True)
    _both(native, idx, np.stack(queries[:3] + bad_q[:1]), k, what="non-finite rows, normalised add")
    idx.close()
    # ... added raw: the norm bound is unknown, the exact scan serves as before
    idx = native.FlatIndex(d)
    idx.add(x)
    _both(native, idx, np.stack(queries[:2]), k, expect_route=False, what="non-finite rows, raw add")
    idx.close()


def test_lifecycle_add_remove_rebuild_reset(native):
    n, d, k = 600_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n + 50_002)   # room for every add below: a re-allocation drops the code
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(4, d)
    _both(native, idx, q, k, what="fresh")
    # add: the code follows
    idx.add_synthetic(50_000, 1234, first_row=n, normalize=True)
    assert idx.code8_rows == n + 50_000
    extra = q[:2] * np.float32(0.5)
    idx.add(extra)                       # raw rows of norm 0.5, one equal in direction to a query
    assert idx.code8_rows == idx.ntotal
    _both(native, idx, q, k, what="after add")
    # remove_rows: dropped; the next two eligible queries take the exact scan, the third rebuilds
    idx.remove_rows(np.array([5, 1000, n - 1], np.int64))
    assert idx.code8_rows == 0
    idx.set_option("code8_single_query", 1)
    native.prof_enable(True)
    try:
        for i in range(2):
            idx.search(q[i], k)
            assert native.prof_symbol("ip_scan").startswith("flat_scan_kernel<"), i
            assert idx.code8_rows == 0
        idx.search(q[2], k)
        assert native.prof_symbol("ip_scan").startswith("code8_scan_kernel<")
    finally:
        native.prof_enable(False)
    assert idx.code8_rows == idx.ntotal
    _both(native, idx, q, k, what="after remove_rows and rebuild")
    # reset
    idx.reset()
    assert idx.code8_rows == 0
    idx.add_synthetic(n, 4321, normalize=True)
    _both(native, idx, q, k, what="after reset")
    idx.close()


def test_delete_query_alternation_never_builds(native):
    """One delete, one query, again and again: every delete restarts the wait of two queries, so the code is never rebuilt and
    every query takes the exact scan, as on an index without the route."""
    n, d, k = 600_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(8, d)
    idx.search(q[0], k)
    assert idx.code8_rows == n
    native.prof_enable(True)
    try:
        for i in range(8):
            idx.remove_rows(np.array([17 * i + 3], np.int64))
            assert idx.code8_rows == 0, i
            D, I = idx.search(q[i], k)
            assert native.prof_symbol("ip_scan").startswith("flat_scan_kernel<"), (i, native.prof_symbol("ip_scan"))
            assert idx.code8_rows == 0, i
    finally:
        native.prof_enable(False)
    # left alone, the third query rebuilds
    for i in range(3):
        idx.search(q[i], k)
    assert idx.code8_rows == idx.ntotal
    _both(native, idx, q, k, what="after the alternation")
    idx.close()


def test_forced_fallback_by_capacity(native):
    n, d, k = 600_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(8, d)
    _both(native, idx, q, k, what="default capacity")
    before = idx.code8_counters()[0]
    idx.set_option("code8_capacity", 1)      # k = 10 candidates cannot fit: every call takes the device-gated exact scan
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan_code8_fallback")
        _both(native, idx, q, k, what="capacity 1")
        ran = native.prof_read("ip_scan_code8_fallback")
        assert native.prof_symbol("ip_scan_code8_fallback").endswith(", true>")
    finally:
        native.prof_enable(False)
    assert idx.code8_counters()[0] - before == len(q)
    assert ran[0] == len(q) and ran[1] / ran[0] > 0.05, ran   # the gated scans did run (ms per launch: a full scan)
    idx.set_option("code8_capacity", 32768)
    idx.close()


def test_graph_replay_and_shadow_option_precedence(native):
    import torch
    n, d, k = 600_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(5, d)
    idx.set_option("code8_single_query", 0)
    want = [idx.search(qi, k, normalize_q=True) for qi in q]
    idx.set_option("code8_single_query", 1)
    stream = torch.cuda.Stream()
    qt = torch.zeros(d, dtype=torch.float32, device="cuda")
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream, normalize_q=True, label_offset=1000)

    # captured BEFORE any eager call: nothing may be built inside a capture, the exact scan is recorded
    g0 = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    qt.copy_(torch.from_numpy(q[0]))
    torch.cuda.synchronize()
    idx.search(q[0], k)                 # builds the code; sizes the default workspace only, this stream's workspace is new
    idx.remove_rows(np.array([n - 1], np.int64))   # drops the code again
    idx.add_synthetic(1, 1234, first_row=n - 1, normalize=True)
    assert idx.code8_rows == 0
    with torch.cuda.stream(stream):
        enqueue()                       # an eager exact call on this stream (the code is waiting to be rebuilt): sizes its workspace
    stream.synchronize()
    with torch.cuda.graph(g0, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    assert idx.code8_rows == 0
    g0.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[0][0][0].view(np.uint32))
    assert np.array_equal(It.cpu().numpy(), want[0][1][0] + 1000)
    # one eager call builds the code and sizes the workspace; the capture after it records the prefilter route
    with torch.cuda.stream(stream):
        enqueue()
        enqueue()
    stream.synchronize()
    assert idx.code8_rows == n
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    calls_before = idx.code8_counters()[2]
    for i in range(5):
        qt.copy_(torch.from_numpy(q[i]))
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[i][0][0].view(np.uint32)), i
        assert np.array_equal(It.cpu().numpy(), want[i][1][0] + 1000), i
    assert idx.code8_counters()[2] - calls_before == 5   # every replay ran the prefilter route's launches
    del g, g0
    # shadow_single_query = 1 keeps its own route
    idx.set_option("shadow_single_query", 1)
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan_half")
        D, I = idx.search(q[1], k, normalize_q=True)
        assert native.prof_read("ip_scan_half")[0] >= 1
    finally:
        native.prof_enable(False)
        idx.set_option("shadow_single_query", 0)
    assert np.array_equal(I, want[1][1])
    idx.close()


def test_through_vector_database(native, tmp_path):
    from minivectordb_amd import VectorDatabase
    n, d, k = 500_500, 512, 5
    x = flat.synth(n, d, 1234)
    db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    db.store_embeddings_batch(list(range(n)), list(x), [{"i": i} for i in range(n)])
    q = _queries(3, d)
    db.find_most_similar(q[0], k=k)   # the first search builds the device index
    out = {}
    native.prof_enable(True)
    try:
        for opt in (0, 1):
            db.index.set_option("code8_single_query", opt)
            out[opt] = [db.find_most_similar(qi, k=k) for qi in q]
            sym = native.prof_symbol("ip_scan")
            assert sym.startswith("code8_scan_kernel<" if opt else "flat_scan_kernel<"), (opt, sym)
    finally:
        native.prof_enable(False)
    assert db.index.code8_rows == n
    for a, b in zip(out[0], out[1]):
        assert list(a[0]) == list(b[0])
        assert np.array_equal(np.asarray(a[1], np.float32).view(np.uint32), np.asarray(b[1], np.float32).view(np.uint32))


def test_fullsize_10m_first_1000_bench_queries(native):
    """10M x 512, the first 1,000 queries of the bench stream, one per call: bit-identical to the option-off run and equal to
    the streamed oracle (tests/bigcheck.py, as test_fullsize_gpu.py)."""
    n, d, k, nq = 10_000_000, 512, 10, 1000
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(nq, d)
    (oracle,), cost = bigcheck.oracle_topk_streamed(idx, n, q, k)
    idx.set_option("code8_single_query", 0)
    off = [idx.search(qi, k) for qi in q]
    idx.set_option("code8_single_query", 1)
    counts = []
    on = []
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        for qi in q:
            on.append(idx.search(qi, k))
            counts.append(idx.code8_counters()[1])
        assert native.prof_symbol("ip_scan").startswith("code8_scan_kernel<")
        assert native.prof_read("ip_scan")[0] == nq
    finally:
        native.prof_enable(False)
    assert idx.code8_rows == n
    for i in range(nq):
        _same(on[i], off[i], f"10M query {i}")
    fallbacks, _, calls = idx.code8_counters()
    print(f"code8 zero-mean 10M x 512: candidates min/median/max {min(counts)}/{int(np.median(counts))}/{max(counts)}, "
          f"fallbacks {fallbacks} of {calls} calls")
    D = np.concatenate([o[0] for o in on])
    I = np.concatenate([o[1] for o in on])
    rec = bigcheck.compare(idx, q, D, I, *oracle, "code8 10M x 512, 1,000 single queries")
    bigcheck.report(dict(rec, oracle_cost=cost))
    idx.close()
