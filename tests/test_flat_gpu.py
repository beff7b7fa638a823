"""GPU parity tests of the flat index (libmvdb.so through the C-ABI) against the CPU oracle.

Bar (BASELINE.json north_star): identical top-k ids (id differences only at float64-adjudicated
near-ties) and distances within 1e-4 (fp32) of the float64 score.
"""
import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _corpus(n, d, seed=1234, normalize=True):
    x = flat.synth(n, d, seed)
    if normalize:
        flat.normalize_l2(x)
    return x


def _check(native, x, q, k, D, I, metric=flat.METRIC_IP, rows=None, exact_vs_oracle=True):
    """Every query: float64 adjudication; and (when asked) id-for-id equality with the fp32 oracle
    wherever the oracle itself agrees with float64 (i.e. away from fp32 near-ties)."""
    Do, Io = flat.flat_search(x, q, k, metric=metric, rows=rows)
    mism = 0
    for i in range(q.shape[0]):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], metric=metric, rows=rows, tol=TOL)
        assert ok, f"query {i}: {msg}"
        if not np.array_equal(I[i], Io[i]):
            mism += 1
    if exact_vs_oracle:
        # near-ties are rare on this data: allow none at small n
        assert mism == 0, f"{mism} queries differ from the fp32 oracle in id order"
    np.testing.assert_allclose(D[I >= 0], Do[Io >= 0], atol=TOL, rtol=0)


def test_synth_generator_bit_exact(native):
    for n, d, seed, first in [(1000, 512, 1234, 0), (257, 100, 99, 12345), (64, 3, 7, 1 << 33),
                              (1000, 512, 1234 | flat.SYNTH_POSITIVE, 0), (300, 384, 5678 | flat.SYNTH_POSITIVE, (1 << 33) + 3),
                              (4000, 512, 1234 | flat.SYNTH_CLUSTERED, 0), (513, 100, 77 | flat.SYNTH_CLUSTERED, (1 << 34) + 11)]:
        idx = native.FlatIndex(d)
        idx.add_synthetic(n, seed, first_row=first, normalize=False)
        got = idx.get_rows(0, n)
        want = flat.synth(n, d, seed, first)
        assert got.tobytes() == want.tobytes()
        idx.close()


def test_normalize_matches_oracle(native):
    for n, d in [(1000, 512), (333, 384), (100, 3), (50, 1000)]:
        x = flat.synth(n, d, 42)
        x[n // 2] = 0.0  # zero row must stay zero (faiss: `if nr > 0`)
        want = x.copy()
        flat.normalize_l2(want)
        got = x.copy()
        native.normalize_l2(got)
        np.testing.assert_allclose(got, want, atol=2e-7, rtol=0)
        assert not got[n // 2].any()
        np.testing.assert_allclose(np.linalg.norm(np.delete(got, n // 2, 0).astype(np.float64), axis=1), 1.0,
                                   atol=1e-6)


@pytest.mark.parametrize("n,d,k,nq", [
    (1000, 512, 5, 8),      # BASELINE config 1
    (20000, 384, 10, 4),    # e5-small width
    (5000, 64, 10, 4),      # reference multithread test width
    (8536, 512, 64, 2),     # largest fused k
    (3000, 1024, 10, 2),    # e5-large / bge-m3 width
    (777, 100, 7, 3),       # d % 64 != 0 (masked lanes)
    (500, 3, 4, 3),         # padded rows (d % 4 != 0)
    (500, 2, 3, 3),
    (100, 1, 3, 2),
    (4000, 768, 10, 2),
    (2000, 160, 10, 2),     # G=32, C=5
    (1000, 1100, 5, 2),     # C=5 masked
    (300, 4096, 5, 1),      # max supported d
])
def test_search_matches_oracle(native, n, d, k, nq):
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=5678)
    idx = native.FlatIndex(d)
    idx.add(x)
    D, I = idx.search(q, k)
    _check(native, x, q, k, D, I)
    idx.close()


def test_query_normalisation_fused(native):
    x = _corpus(5000, 512)
    q = flat.synth(4, 512, 5678) * 3.7  # un-normalised queries
    idx = native.FlatIndex(512)
    idx.add(x)
    D, I = idx.search(q, 10, normalize_q=True)
    qn = q.copy()
    flat.normalize_l2(qn)
    _check(native, x, qn, 10, D, I)
    # zero query: normalisation leaves it alone, all scores are 0 -> ties broken by row number
    D0, I0 = idx.search(np.zeros((1, 512), np.float32), 5, normalize_q=True)
    assert I0[0].tolist() == [0, 1, 2, 3, 4] and not D0.any()
    idx.close()


def test_add_normalizes_on_device(native):
    x = flat.synth(4000, 384, 1)
    idx = native.FlatIndex(384)
    idx.add(x[:1000], normalize=True)
    idx.add(x[1000:], normalize=True)  # appended in two pieces
    stored = idx.get_rows(0, 4000)
    want = x.copy()
    flat.normalize_l2(want)
    np.testing.assert_allclose(stored, want, atol=2e-7, rtol=0)
    q = _corpus(3, 384, seed=2)
    D, I = idx.search(q, 10)
    _check(native, stored, q, 10, D, I)
    idx.close()


@pytest.mark.parametrize("k", [65, 100, 825, 999, 5000])
def test_large_k_select_path(native, k):
    n = 8536 if k < 5000 else 6000
    x = _corpus(n, 128)
    q = _corpus(2, 128, seed=5678)
    idx = native.FlatIndex(128)
    idx.add(x)
    D, I = idx.search(q, k)
    keff = min(k, n)
    Do, Io = flat.flat_search(x, q, k)
    assert (I[:, keff:] == -1).all()
    assert (I[:, :keff] >= 0).all()
    # full-length lists: compare as sets + scores, then exact order away from ties
    for i in range(2):
        assert set(I[i, :keff].tolist()) == set(Io[i, :keff].tolist())
        np.testing.assert_allclose(D[i, :keff], Do[i, :keff], atol=TOL, rtol=0)
        assert np.all(np.diff(D[i, :keff]) <= 0)
    idx.close()


def test_k_larger_than_n_pads_like_faiss(native):
    x = _corpus(7, 16)
    idx = native.FlatIndex(16)
    idx.add(x)
    for k in (10, 100):
        D, I = idx.search(x[:1], k)
        assert sorted(I[0, :7].tolist()) == list(range(7))
        assert (I[0, 7:] == -1).all()
        assert np.all(D[0, 7:] == np.float32(-3.4028234663852886e38))
    idx.close()


def test_empty_index(native):
    idx = native.FlatIndex(8)
    D, I = idx.search(np.ones((2, 8), np.float32), 3)
    assert (I == -1).all()
    idx.close()


def test_ties_resolve_to_lower_row(native):
    # colinear rows (the reference tests use [0.5,0.5], [0.1,0.1], [0.7,0.7]): exact score ties
    base = np.array([[0.5, 0.5], [0.1, 0.1], [0.7, 0.7], [0.5, -0.5], [0.2, 0.2]], np.float32)
    x = np.tile(base, (40, 1))
    idx = native.FlatIndex(2)
    idx.add(x, normalize=True)
    D, I = idx.search(np.array([[1.0, 1.0]], np.float32), 10, normalize_q=True)
    stored = idx.get_rows(0, x.shape[0])
    qn = np.array([[1.0, 1.0]], np.float32)
    flat.normalize_l2(qn)
    Do, Io = flat.flat_search(stored, qn, 10)
    assert I[0].tolist() == Io[0].tolist()
    np.testing.assert_allclose(D, Do, atol=1e-6)
    # all-equal corpus, k spanning both selection paths
    ones = np.ones((3000, 8), np.float32)
    idx2 = native.FlatIndex(8)
    idx2.add(ones)
    for k in (1, 10, 64, 65, 300):
        D, I = idx2.search(np.ones((1, 8), np.float32), k)
        assert I[0].tolist() == list(range(k))
    idx.close()
    idx2.close()


def test_subset_search(native):
    n, d = 6000, 256
    x = _corpus(n, d)
    q = _corpus(3, d, seed=5678)
    idx = native.FlatIndex(d)
    idx.add(x)
    rng = np.random.RandomState(0)
    for m, k in [(1, 1), (17, 5), (2500, 10), (2500, 100), (6000, 10)]:
        rows = rng.permutation(n)[:m].astype(np.int64)
        D, I = idx.search_subset(q, k, rows)
        keff = min(k, m)
        assert (I[:, :keff] >= 0).all() and (I[:, :keff] < m).all()
        _check(native, x, q, k, D, I, rows=rows)
    with pytest.raises(ValueError):
        idx.search_subset(q, 3, np.array([n], np.int64))
    idx.close()


def test_l2_metric_extension(native):
    n, d = 4000, 96
    x = flat.synth(n, d, 11)
    q = flat.synth(3, d, 12)
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.add(x)
    for k in (1, 10, 100):
        D, I = idx.search(q, k)
        _check(native, x, q, k, D, I, metric=flat.METRIC_L2)
        assert np.all(np.diff(D, axis=1) >= 0)
    idx.close()


@pytest.mark.parametrize("d,nq,k", [(128, 2, 10), (512, 8, 10), (384, 32, 5), (512, 40, 64), (768, 20, 10), (1024, 5, 3), (100, 4, 7),
                                    (512, 24, 10), (512, 64, 10), (512, 128, 10), (512, 256, 10), (384, 200, 12), (256, 100, 32),
                                    (1024, 70, 10), (640, 130, 16)])   # round 4: the certified passes (14+ queries)
@pytest.mark.parametrize("normalized", [True, False])
def test_l2_batches_share_corpus_passes(native, d, nq, k, normalized):
    """Squared L2 with several queries per call.  Up to 13 queries (and whenever the stored rows' norms differ by more than
    2^-10 — `normalized=False` here): the staged fp32-MFMA pass computes |q|^2 + |x|^2 - 2 q.x (whole rows go through its
    LDS ring, so |x|^2 costs no extra read).  33+ queries: the certified pass of the inner
    product — fp16 nomination by q.x, the nominees re-scored as sum (q - x)^2, the certificate bounding every
    dropped row's distance through min |x|^2 (mvdb.hip: l2_cert_ok) — at the inner product's speed.  One query at a time the
    scan sums (q - x)^2 directly.  All must agree with the float64 adjudication (the expansion cancels: tolerance scales with
    the magnitude of the distances), ties (a planted duplicate row) resolve to the lower row, and a query equal to a stored
    row finds it at distance ~0."""
    n = 30_000
    x = flat.synth(n, d, 21)
    if normalized:
        flat.normalize_l2(x)
    x[17_000] = x[123]
    q = flat.synth(nq, d, 22)
    if normalized:
        flat.normalize_l2(q)
    q[0] = x[123]
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.add(x)
    native.prof_enable(True)
    try:
        _split_launches(native)  # drain
        D, I = idx.search(q, k)
        certified_pass = _split_launches(native) > 0
    finally:
        native.prof_enable(False)
    # the certified pass serves the batches of 33+ queries (30,000 rows: below 100k a smaller batch does not bury its fixed cost),
    # k <= 32, at the widths it has a kernel for: rows of one norm by inner product with the norm-range certificate, rows of
    # any norms by q.x - |x|^2 / 2 with per-row offsets beside the shadow
    expect = nq >= 33 and k <= 32 and d in HALF_DIMS
    assert certified_pass == expect, (certified_pass, expect)
    assert I[0, :2].tolist() == [123, 17_000]
    mag = float(max(1.0, np.abs(D).max()))
    assert abs(D[0, 0]) <= 4e-6 * mag
    assert np.all(np.diff(D, axis=1) >= -4e-6 * mag)
    Do, Io = flat.flat_search(x, q, k, metric=flat.METRIC_L2)
    for i in range(nq):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], metric=flat.METRIC_L2, tol=1e-4 * mag, tie_eps=4e-6 * mag)
        assert ok, f"query {i}: {msg}"
    np.testing.assert_allclose(D, Do, atol=1e-5 * mag, rtol=0)
    for i in (0, nq - 1):                                       # the same query alone: the direct form
        D1, I1 = idx.search(q[i], k)
        np.testing.assert_allclose(D1[0], D[i], atol=1e-5 * mag, rtol=0)
    idx.close()


@pytest.mark.parametrize("staging_bytes", [None, 256, 1792, 100_000])
def test_remove_rows_matches_np_delete(native, monkeypatch, staging_bytes):
    """mvdb_index_remove_rows compacts the tail in place; many scattered rows (the last case here) go chunk by chunk through a
    bounded staging buffer (512 MiB; MVDB_COMPACT_BYTES): one row per chunk (256 B = a 64-float row), 7 rows, 390 rows and the
    whole tail at once.  (Single rows take the one-pass shift: test_remove_a_few_rows_compacts_in_one_pass.)"""
    n, d = 3000, 64
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    if staging_bytes is not None:
        monkeypatch.setenv("MVDB_COMPACT_BYTES", str(staging_bytes))
        idx.reload_env()
    idx.add(x)
    rng = np.random.RandomState(1)
    cur = x
    for dels in ([5], [0], [cur.shape[0] - 3], rng.permutation(2900)[:400].tolist()):
        idx.remove_rows(np.array(dels, np.int64))
        cur = np.delete(cur, dels, 0)
        assert idx.ntotal == cur.shape[0]
        assert idx.get_rows(0, idx.ntotal).tobytes() == cur.tobytes()
    q = _corpus(2, d, seed=3)
    D, I = idx.search(q, 10)
    _check(native, cur, q, 10, D, I)
    with pytest.raises(ValueError):
        idx.remove_rows(np.array([1, 1], np.int64))
    idx.close()


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("n,d", [(3000, 64), (70001, 100), (300_000, 128), (40_000, 512), (9000, 2050)])
def test_remove_a_few_rows_compacts_in_one_pass(native, monkeypatch, n, d, inplace):
    """The reference deletes ONE row per call (vector_database.py:119-131: np.delete on the matrix, index rebuilt).  A single row,
    a run of rows, or up to 8 scattered rows shift the tail in place in ONE pass (shift_rows_kernel: each workgroup walks its
    range upwards, sources beyond its range come from a side copy taken before the launch); more scattered rows, and everything
    under MVDB_COMPACT_INPLACE=0, go through the staging buffer.  Both must leave exactly np.delete's matrix, bit for bit."""
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    if not inplace:
        monkeypatch.setenv("MVDB_COMPACT_INPLACE", "0")
        idx.reload_env()
    idx.add(x)
    rng = np.random.RandomState(n + d)
    cur = x
    cases = [lambda m: [0], lambda m: [1], lambda m: [m - 1], lambda m: [m // 2], lambda m: list(range(10, 17)), lambda m: list(range(0, 3)),
             lambda m: sorted(rng.choice(m // 2, 64, replace=False).tolist()), lambda m: [5, 6, 7, m // 3],
             lambda m: rng.choice(m // 2, 8, replace=False).tolist(), lambda m: rng.choice(m // 2, 9, replace=False).tolist(), lambda m: list(range(100, 400)),
             lambda m: sorted(rng.choice(m // 2, 65, replace=False).tolist()), lambda m: [m - 2, m - 1], lambda m: [3, m - 1]]
    for case in cases:
        dels = case(cur.shape[0])
        idx.remove_rows(np.array(dels, np.int64))
        cur = np.delete(cur, dels, 0)
        assert idx.ntotal == cur.shape[0]
        got = idx.get_rows(0, idx.ntotal)
        if got.tobytes() != cur.tobytes():
            bad = np.flatnonzero((got != cur).any(axis=1))
            raise AssertionError(f"rows differ after deleting {dels[:8]}... ({len(dels)} rows): first bad rows {bad[:10]}, {bad.size} in all")
    q = _corpus(3, d, seed=3)
    D, I = idx.search(q, 10)
    _check(native, cur, q, 10, D, I)
    idx.close()


def test_argument_errors(native):
    with pytest.raises(ValueError):
        native.FlatIndex(0)
    with pytest.raises(ValueError):
        native.FlatIndex(5000)
    idx = native.FlatIndex(4)
    with pytest.raises(ValueError):
        idx.search(np.ones((1, 4), np.float32), 0)
    with pytest.raises(ValueError):
        idx.search(np.ones((1, 5), np.float32), 1)
    with pytest.raises(ValueError):
        idx.get_rows(0, 1)
    idx.close()


def test_concurrent_searches_are_reentrant(native):
    import threading
    x = _corpus(20000, 128)
    q = _corpus(16, 128, seed=9)
    idx = native.FlatIndex(128)
    idx.add(x)
    # reference results from single-query searches (a batched call takes the multi-query MFMA pass,
    # whose fp32 summation order differs in the last bits)
    res = [idx.search(q[i], 10) for i in range(16)]
    D0 = np.concatenate([r[0] for r in res])
    I0 = np.concatenate([r[1] for r in res])
    errs = []

    def worker(i):
        try:
            for _ in range(20):
                D, I = idx.search(q[i:i + 1], 10)
                assert np.array_equal(I[0], I0[i]) and np.array_equal(D[0], D0[i])
        except Exception as e:  # pragma: no cover
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(16)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    idx.close()


def test_config2_1M_x_512(native):
    """BASELINE config 2: 1M x 512 fp32, k = 10 — corpus generated on the device, fetched once for
    the oracle (2 GB)."""
    n, d, k = 1_000_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    x = idx.get_rows(0, n)
    q = _corpus(8, d, seed=5678)
    D, I = idx.search(q, k)
    Do, Io = flat.flat_search(x, q, k, nthreads=flat.max_threads())
    np.testing.assert_allclose(D, Do, atol=TOL, rtol=0)
    for i in range(q.shape[0]):
        if not np.array_equal(I[i], Io[i]):
            ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], tol=TOL)
            assert ok, msg
    # stored rows are what the oracle's generator + normalise produce
    want = flat.synth(4096, d, 1234, 500_000)
    flat.normalize_l2(want)
    np.testing.assert_allclose(x[500_000:504_096], want, atol=2e-7, rtol=0)
    idx.close()


def test_merge_topk_device_matches_numpy(native):
    """The exchange step of the row-partitioned search: merge `world` per-shard lists laid out as one
    all-gather of packed {I, D} blocks (minivectordb_amd/distributed.py) — run here on one GPU."""
    import ctypes
    import torch
    from minivectordb_amd.distributed import PackedTopK
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    for world, nq, k in [(8, 1, 10), (2, 5, 7), (8, 3, 64), (3, 2, 1), (8, 2, 65), (2, 3, 999), (8, 1, 2048)]:  # k > 64: LDS sort
        g = PackedTopK(nq, k, dev, world)
        lists = []
        for l in range(world):
            D, I = g.views(l)
            d = np.sort(rs.rand(nq, k).astype(np.float32), axis=1)[:, ::-1].copy()
            d[:, k // 2:] = np.round(d[:, k // 2:], 1)  # force cross-list score ties
            d = np.sort(d, axis=1)[:, ::-1].copy()
            i = (l * 1000 + np.arange(nq * k).reshape(nq, k)).astype(np.int64)
            if l == world - 1 and k > 2:
                i[:, -1] = -1  # a short last shard
                d[:, -1] = -3.4028234663852886e38
            D.copy_(torch.from_numpy(d))
            I.copy_(torch.from_numpy(i))
            lists.append((d, i))
        Dout = torch.empty((nq, k), dtype=torch.float32, device=dev)
        Iout = torch.empty((nq, k), dtype=torch.int64, device=dev)
        D0, I0 = g.views(0)
        native.check(native.lib().mvdb_merge_topk_device(
            0, world, nq, k, ctypes.c_void_p(D0.data_ptr()), g.stride_D, ctypes.c_void_p(I0.data_ptr()), g.stride_I,
            ctypes.c_void_p(Dout.data_ptr()), ctypes.c_void_p(Iout.data_ptr()), 0,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for qi in range(nq):
            cands = sorted((-float(d[qi, j]), int(i[qi, j])) for d, i in lists for j in range(k) if i[qi, j] >= 0)
            want_i = [c[1] for c in cands[:k]]
            want_d = [-c[0] for c in cands[:k]]
            assert Iout[qi].tolist() == want_i
            assert Dout[qi].tolist() == want_d


def test_sharded_searcher_single_gpu_path(native):
    """world == 1 degenerate path of ShardedSearcher (what bench.py runs at --gpus 1): device-resident
    queries, label offset, no collective."""
    import torch
    from minivectordb_amd.distributed import ShardedSearcher
    dev = torch.device("cuda", 0)
    n, d, k = 30000, 512, 10
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    idx.add(x)
    s = ShardedSearcher(idx, k, rank=0, world=1, label_offset=7_000_000, device=dev)
    q = _corpus(4, d, seed=5678)
    qt = torch.from_numpy(q).to(dev)
    Do, Io = flat.flat_search(x, q, k)
    for nq in (1, 4):
        D, I = s.search_device(qt[:nq])
        torch.cuda.synchronize()
        assert np.array_equal(I.cpu().numpy() - 7_000_000, Io[:nq])
        np.testing.assert_allclose(D.cpu().numpy(), Do[:nq], atol=TOL)
    idx.close()


def test_config3_10M_x_512_properties(native):
    """BASELINE config 3 at full size (20.48 GB resident, generated on the device).  The corpus does
    not cross PCIe; parity is checked through size-independent properties:
      * every returned (id, score): the score equals the float64 dot product of the query with that
        stored row (rows fetched individually) within 1e-4, and the list is sorted;
      * planted needles: rows that are copies of a query are returned first with score ~ 1;
      * union property: top-k of the whole = merge of the top-k of a partition (subset searches);
      * no row of a 200k-row random sample beats the k-th score (float64 check)."""
    n, d, k = 10_000_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n + 8)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _corpus(6, d, seed=5678)
    needles = np.repeat(q[:2], 2, axis=0) * np.float32(2.5)  # un-normalised copies of queries 0 and 1
    idx.add(needles, normalize=True)                          # rows n .. n+3
    D, I = idx.search(q, k)
    assert np.all(np.diff(D, axis=1) <= 0)
    assert I[0, :2].tolist() == [n, n + 1] and I[1, :2].tolist() == [n + 2, n + 3]
    np.testing.assert_allclose(D[:2, :2], 1.0, atol=1e-6)
    rs = np.random.RandomState(5)
    sample = np.sort(rs.choice(n, 200_000, replace=False))
    blocks = [idx.get_rows(int(s0), 1)[0] for s0 in sample[:2000]]  # 2000 individually fetched rows
    xs = np.stack(blocks).astype(np.float64)
    for i in range(q.shape[0]):
        rows = np.stack([idx.get_rows(int(r), 1)[0] for r in I[i]])
        true = rows.astype(np.float64) @ q[i].astype(np.float64)
        np.testing.assert_allclose(D[i], true, atol=TOL, rtol=0)
        assert (xs @ q[i].astype(np.float64)).max() <= D[i, -1] + 1e-6
    # union property on a 3-way partition of the row range
    third = (n + 4) // 3
    parts = [np.arange(a, min(a + third, n + 4), dtype=np.int64) for a in range(0, n + 4, third)]
    cand_d, cand_i = [], []
    for p in parts:
        Dp, Ip = idx.search_subset(q, k, p)
        cand_d.append(Dp)
        cand_i.append(p[Ip])
    cd, ci = np.concatenate(cand_d, 1), np.concatenate(cand_i, 1)
    for i in range(q.shape[0]):
        order = np.lexsort((ci[i], -cd[i]))[:k]
        assert ci[i][order].tolist() == I[i].tolist()
        # the 6-query call takes the multi-query MFMA pass, the subset calls the GEMV kernel: same ids,
        # scores equal up to fp32 summation order
        np.testing.assert_allclose(cd[i][order], D[i], atol=1e-6, rtol=0)
    # and the single-query (GEMV) path returns the same ids as the multi-query pass
    for i in range(q.shape[0]):
        D1, I1 = idx.search(q[i], k)
        assert I1[0].tolist() == I[i].tolist()
        np.testing.assert_allclose(D1[0], D[i], atol=1e-6, rtol=0)
    idx.close()


@pytest.mark.parametrize("n,d,k,nq", [
    (20000, 512, 10, 16), (20000, 512, 10, 17), (9000, 512, 64, 32), (9000, 512, 5, 33), (30000, 384, 10, 40),
    (5000, 64, 10, 2), (7001, 256, 1, 9), (3000, 128, 7, 31), (15, 512, 10, 5), (16, 512, 4, 3), (17, 512, 20, 2),
    (6000, 1024, 10, 16), (6000, 1024, 10, 35), (5000, 768, 64, 9),  # e5-large / bge-m3 widths: one group per pass
])
def test_multi_query_mfma_pass_matches_oracle(native, n, d, k, nq):
    """nq >= 2: one corpus pass serves up to 32 queries on v_mfma_f32_16x16x4_f32 (exact fp32); every query's result must
    equal its own single-query search."""
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=5678)
    idx = native.FlatIndex(d)
    idx.add(x)
    D, I = idx.search(q, k)
    _check(native, x, q, k, D, I)
    # identical to per-query (GEMV kernel) searches up to fp32 summation order
    for i in (0, nq - 1):
        D1, I1 = idx.search(q[i], k)
        assert np.array_equal(I1[0], I[i])
        np.testing.assert_allclose(D1[0], D[i], atol=2e-6)
    # fused normalisation + ties (duplicate rows, duplicate queries)
    q2 = np.concatenate([q[:2] * 3.0, q[:1] * 0.5, np.zeros((1, d), np.float32)])
    D2, I2 = idx.search(q2, k, normalize_q=True)
    assert np.array_equal(I2[0], I2[2]) and np.array_equal(I2[0], I[0])
    assert I2[3].tolist()[:min(k, n)] == list(range(min(k, n)))  # zero query: all scores 0, ties by row
    idx.close()


def test_multi_query_pass_is_deterministic(native):
    """Regression for a scheduling race in the LDS-DMA staged kernel (hipcc hoisted DMA instructions
    into the reads of the buffer they overwrite): repeated 32-query passes must return bit-identical
    results, equal to the per-query searches."""
    n, d, k = 40000, 512, 10
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    idx.add(x)
    for nq in (17, 32):
        q = _corpus(nq, d, seed=4242)
        ref = [idx.search(q[i], k) for i in range(nq)]
        D0, I0 = idx.search(q, k)
        for _ in range(6):
            D, I = idx.search(q, k)
            assert np.array_equal(I, I0) and np.array_equal(D, D0)
        for i in range(nq):
            assert np.array_equal(ref[i][1][0], I0[i])
            np.testing.assert_allclose(ref[i][0][0], D0[i], atol=2e-6, rtol=0)
    idx.close()


@pytest.mark.parametrize("n,d,k,nq", [
    (20000, 512, 10, 64), (9000, 384, 16, 100), (5000, 512, 1, 128), (12345, 256, 10, 129), (300, 64, 5, 200),
    (127, 512, 10, 70), (128, 128, 16, 64), (129, 512, 3, 65), (4000, 512, 17, 64),
])
def test_large_batch_gemm_scan_matches_oracle(native, n, d, k, nq):
    """nq >= 64 and k <= 16: the compute-bound tiled GEMM + in-register top-k gate (k = 17 falls back to the
    32-query passes).  Every query's result must equal its own single-query search."""
    import os
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=777)
    idx = native.FlatIndex(d)
    idx.add(x)
    os.environ["MVDB_DISABLE_SPLIT_SCAN"] = "1"  # this test pins the exact-fp32 tiled kernel (the fallback of the split pass)
    os.environ["MVDB_GEMM_SCAN_MIN_NQ"] = "64"  # also cover half-filled query tiles
    idx.reload_env()  # the library reads its hooks once per index: at creation, and when asked
    try:
        D, I = idx.search(q, k)
        _check(native, x, q, k, D, I)
        del os.environ["MVDB_GEMM_SCAN_MIN_NQ"]
        idx.reload_env()
        Dd, Id = idx.search(q, k)  # default chunking (GEMM launches of up to 128 + 32-query passes for the rest)
        assert np.array_equal(Id, I)
        np.testing.assert_allclose(Dd, D, atol=2e-6)
        D2, I2 = idx.search(q * 2.5, k, normalize_q=True)  # fused normalisation path
        assert np.array_equal(I2, I)
        np.testing.assert_allclose(D2, D, atol=2e-6)
        for i in (0, nq // 2, nq - 1):
            D1, I1 = idx.search(q[i], k)
            assert np.array_equal(I1[0], I[i])
        # determinism across repeats (same path each time)
        for _ in range(3):
            Dr, Ir = idx.search(q, k)
            assert np.array_equal(Ir, Id) and np.array_equal(Dr, Dd)
    finally:
        os.environ.pop("MVDB_GEMM_SCAN_MIN_NQ", None)
        del os.environ["MVDB_DISABLE_SPLIT_SCAN"]
    idx.close()


HALF_DIMS = (128, 256, 384, 512, 640, 768, 896, 1024)   # widths the certified pass (fp16 nomination over the shadow) serves


def _split_launches(native):
    """Chunks that went through the certified pass: each one starts with a seed launch."""
    native.prof_read("ip_scan_half")
    return native.prof_read("ip_scan_half_seed")[0]


@pytest.mark.parametrize("n,d,k,nq", [
    (20000, 512, 10, 64), (9000, 384, 12, 100), (5000, 512, 1, 128), (12345, 256, 10, 129), (300, 64, 5, 200),
    (127, 512, 10, 70), (15, 512, 10, 30), (16, 128, 10, 24), (17, 96, 12, 33), (6000, 1024, 10, 130),
    (30000, 384, 10, 256),
    (300000, 64, 10, 64), (270001, 128, 5, 130), (300000, 64, 10, 24), (70000, 128, 12, 100), (70001, 128, 12, 24), (40003, 256, 3, 129),  # seed + main launch
    (70001, 512, 10, 128), (40003, 512, 12, 50), (150003, 512, 5, 100), (33000, 512, 10, 33),  # seed + the K-split d = 512 kernels: ragged last tile, one and two phases
    (9000, 768, 10, 100), (70001, 1024, 10, 128), (150003, 384, 10, 256), (40003, 512, 10, 200), (100000, 256, 10, 255),  # fp16 pass: every dimension it serves, 128- and 256-query passes
    (60000, 128, 10, 256), (50001, 640, 10, 128), (30000, 896, 10, 70),  # d = 640, 896 (round 3) and 128 (round 6) on the fp16 pass too
    (80000, 512, 16, 128), (150003, 512, 32, 256), (60000, 384, 20, 130), (50001, 640, 16, 100), (40000, 1024, 32, 64),  # k up to 32 (64 nominees)
])
def test_split_precision_batch_pass_matches_oracle(native, monkeypatch, n, d, k, nq):
    """Batches of 24+ queries: where the certified pass has a kernel (HALF_DIMS) ONE fp16 product over the shadow nominates,
    exact fp32 re-scores decide and certify (half_scan.hip); the other widths (64, 96 here — served by the bf16-split
    generation until round 6) take the exact fp32 passes.  Results must equal the oracle's and every query's own
    single-query search."""
    monkeypatch.setenv("MVDB_SPLIT_SCAN_MIN_NQ", "24")  # read when the index is created: also cover sparsely filled query tiles
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=777)
    idx = native.FlatIndex(d)
    idx.add(x)  # raw add: the row-norm bound is measured on the device
    native.prof_enable(True)
    reruns = native.split_rerun_count()
    try:
        _split_launches(native)  # drain
        D, I = idx.search(q, k)
        launches = _split_launches(native)
        if d in HALF_DIMS:
            assert launches >= max(1, nq // 256), "the certified pass did not run"
        else:
            assert launches == 0
    finally:
        native.prof_enable(False)
    _check(native, x, q, k, D, I, exact_vs_oracle=n < 100000)
    if n > 16:
        assert native.split_rerun_count() == reruns, "well-separated scores must certify"
    for i in (0, nq // 2, nq - 1):
        D1, I1 = idx.search(q[i], k)
        assert np.array_equal(I1[0], I[i])
        np.testing.assert_allclose(D1[0], D[i], atol=2e-6, rtol=0)
    D2, I2 = idx.search(q * 2.5, k, normalize_q=True)
    assert np.array_equal(I2, I)
    np.testing.assert_allclose(D2, D, atol=2e-6)
    for _ in range(3):
        Dr, Ir = idx.search(q, k)
        assert np.array_equal(Ir, I) and np.array_equal(Dr, D)
    idx.close()


def test_split_precision_pass_unnormalised_rows_and_queries(native, monkeypatch):
    """Raw rows of very different norms and raw queries: the certification margin scales with |q| * max|row|."""
    n, d, k, nq = 8000, 256, 10, 48
    x = flat.synth(n, d, 99)
    x *= np.linspace(0.01, 30.0, n, dtype=np.float32)[:, None]
    q = flat.synth(nq, d, 100) * np.float32(7.0)
    idx = native.FlatIndex(d)
    idx.add(x)
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search(q, k)
        assert _split_launches(native) == 1
    finally:
        native.prof_enable(False)
    Do, Io = flat.flat_search(x, q, k)
    for i in range(nq):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], tol=1e-4 * 30.0 * float(np.linalg.norm(q[i])))
        assert ok, msg
    assert (I == Io).mean() > 0.99
    np.testing.assert_allclose(D, Do, rtol=1e-5, atol=1e-3)
    idx.close()


def _graded_rows(q, cosines, rs):
    """Unit rows whose score against unit query q is cosines[j] (to fp32 rounding): c q + sqrt(1 - c^2) w, w _|_ q."""
    d = q.shape[0]
    q64 = q.astype(np.float64)
    q64 /= np.linalg.norm(q64)
    out = np.empty((len(cosines), d), np.float32)
    for j, c in enumerate(cosines):
        w = rs.randn(d)
        w -= (w @ q64) * q64
        w /= np.linalg.norm(w)
        out[j] = (c * q64 + np.sqrt(1.0 - c * c) * w).astype(np.float32)
    return out


@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("frac,must_rerun", [(1 / 12, True), (1 / 48, True), (0.9, False)])
def test_split_certificate_at_the_margin(native, d, frac, must_rerun):
    """Rows engineered to sit within +-eps(d) of the k-th score (30 rows graded `frac * eps` apart around 0.9, stored
    contiguously so that ONE block list holds them all): the pass must either certify a correct answer or re-run the
    chunk — never return a wrong id.  With steps of eps / 12 and eps / 48 more than 16 - k rows lie inside the
    margin of the 16 that a block list (or the running list) keeps, so the certificate MUST refuse; with 0.9 eps
    steps the 16th is 5.4 eps below the k-th result and the pass must certify on its own.  eps is the bound of
    the fp16 nomination pass (1.04e-3 at d = 512)."""
    n, k, nq = 20000, 10, 40
    eps = native.half_eps(d)
    assert 3 * 2.0 ** -16 < eps < 2e-3
    spacing = frac * eps
    rs = np.random.RandomState(d + int(frac * 1e4))
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=4242)
    cos = 0.9 - spacing * np.arange(30)
    for qi, base in ((0, 500), (17, 9000), (39, 15000)):
        rows = _graded_rows(q[qi], cos, rs)
        order = rs.permutation(30)            # row numbers must not follow the score order
        x[base:base + 30] = rows[order]
    idx = native.FlatIndex(d)
    idx.add(x)                                # raw add: max|x| measured on the device (1 + 1e-6)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    reran = native.split_rerun_count() - before
    assert (reran >= 1) == must_rerun, (reran, eps)
    x64 = x.astype(np.float64)
    for qi in range(nq):
        t = x64 @ q[qi].astype(np.float64)
        want = np.argsort(-t, kind="stable")[:k]
        if spacing >= 1e-5 or qi not in (0, 17, 39):
            assert I[qi].tolist() == want.tolist(), (qi, I[qi], want)
        else:   # finer steps: fp32 re-scores (1e-7) still order them; float64 adjudicates anything closer
            ok, msg = flat.adjudicate(x, q[qi], k, D[qi], I[qi], tol=TOL)
            assert ok, msg
        np.testing.assert_allclose(D[qi], t[I[qi]], atol=TOL, rtol=0)
    idx.close()


@pytest.mark.parametrize("n,d,nq,k", [(120_000, 256, 8, 10), (120_000, 256, 32, 10), (110_000, 512, 130, 10), (520_000, 256, 2, 5),
                                      (520_000, 256, 40, 32), (40_000, 384, 64, 10), (33_000, 768, 100, 12), (30_001, 1024, 33, 10)])
def test_l2_rows_of_mixed_norms_on_the_shadow_pass(native, n, d, nq, k):
    """L2 over rows whose norms differ by a factor of 30 (the inner product does NOT rank like the distance there): the
    nomination pass over the fp16 shadow subtracts |x|^2 / 2 per row (kept beside the shadow, fetched through the scalar
    cache), re-scores sum (q - x)^2 in fp32 and certifies with d(y) >= |q|^2 - 2 (U + eps).  Queries of small, equal and
    large norm; a duplicated row (exact tie) and a query equal to a stored row.  The certified pass must have run, nearly
    every query must certify, and every result is adjudicated in float64."""
    rs = np.random.RandomState(n % 1000 + d + nq)
    x = flat.synth(n, d, 31)
    flat.normalize_l2(x)
    x *= np.exp(rs.uniform(np.log(0.1), np.log(3.0), size=(n, 1))).astype(np.float32)
    x[n - 7] = x[4321]
    q = flat.synth(nq, d, 32)
    flat.normalize_l2(q)
    q *= np.exp(rs.uniform(np.log(0.05), np.log(4.0), size=(nq, 1))).astype(np.float32)
    q[0] = x[4321]
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.reserve(n + 1000)       # (an add that has to reallocate the matrix drops the shadow instead of extending it)
    idx.add(x)
    before = native.split_rerun_count()
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search(q, k)
        assert _split_launches(native) > 0, "the certified pass did not run"
        assert native.prof_symbol("ip_scan_half").startswith("flat_scan_h16_kernel"), native.prof_symbol("ip_scan_half")
    finally:
        native.prof_enable(False)
    assert idx.shadow_rows == n
    reran = native.split_rerun_count() - before
    assert I[0, :2].tolist() == [4321, n - 7]
    mag = float(max(1.0, np.abs(D).max()))
    assert np.all(np.diff(D, axis=1) >= -4e-6 * mag)
    Do, Io = flat.flat_search(x, q, k, metric=flat.METRIC_L2, nthreads=flat.max_threads())
    for i in range(nq):
        if np.array_equal(I[i], Io[i]) and np.abs(D[i] - Do[i]).max() <= 4e-6 * mag:
            continue
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], metric=flat.METRIC_L2, tol=1e-4 * mag, tie_eps=4e-6 * mag)
        assert ok, (i, msg)
    assert reran <= 1 + nq // 128, reran     # (chunks that held an uncertified query)
    # the same batch again after an append and a delete: the offsets follow the shadow
    extra = flat.synth(100, d, 33)
    flat.normalize_l2(extra)              # (rows beyond the norm bound would change the shadow's scale: rebuilt, not extended)
    idx.add(extra)
    assert idx.shadow_rows == n + 100
    x2 = np.concatenate([x, extra])
    D, I = idx.search(q, k)
    for i in (0, nq - 1):
        ok, msg = flat.adjudicate(x2, q[i], k, D[i], I[i], metric=flat.METRIC_L2, tol=1e-4 * mag, tie_eps=4e-6 * mag)
        assert ok, (i, msg)
    idx.remove_rows(np.array([5, 4321], np.int64))
    x3 = np.delete(x2, [5, 4321], 0)
    D, I = idx.search(q, k)
    assert idx.shadow_rows == n + 98
    for i in (0, nq // 2, nq - 1):
        ok, msg = flat.adjudicate(x3, q[i], k, D[i], I[i], metric=flat.METRIC_L2, tol=1e-4 * mag, tie_eps=4e-6 * mag)
        assert ok, (i, msg)
    idx.close()


@pytest.mark.parametrize("nq", [40, 130])
@pytest.mark.parametrize("frac,must_rerun", [(1 / 48, True), (0.9, False)])
def test_l2_certificate_at_the_margin(native, nq, frac, must_rerun):
    """The L2 metric on the certified pass (fp16 nomination, 64 nominees; 40 queries: one 128-query pass, 130: a 256-query one):
    nomination is by inner product, the certificate bounds a dropped row's DISTANCE through min |x|^2.  30 unit rows graded
    `frac * eps` apart in cosine (2 frac eps apart in squared distance), stored contiguously: steps of eps / 48 MUST be
    refused — and come back exact from the device-gated single-query scan —, steps of 0.9 eps must certify.  One stored
    row is shrunk by 2^-12 so that the norm range measured at add is not degenerate: the certificate then gives up
    (1 - min |x|^2) / 2 = 2.4e-4 of its margin (a dropped row of that norm would be that much nearer than its inner
    product says) and must still certify the 0.9-eps case."""
    n, d, k = 20000, 512, 10
    eps = native.half_eps(d)
    spacing = frac * eps
    rs = np.random.RandomState(int(frac * 1e4) + nq)
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=4242)
    cos = 0.9 - spacing * np.arange(30)
    for qi, base in ((0, 500), (nq // 2, 9000), (nq - 1, 15000)):
        rows = _graded_rows(q[qi], cos, rs)
        x[base:base + 30] = rows[rs.permutation(30)]
    x[3000] *= np.float32(1.0 - 2.0 ** -12)        # the norm range is measured at add: 2^-11 relative in |x|^2
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.add(x)
    before = native.split_rerun_count()
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search(q, k)
        assert _split_launches(native) > 0, "the certified pass did not run"
    finally:
        native.prof_enable(False)
    reran = native.split_rerun_count() - before
    assert (reran >= 1) == must_rerun, (reran, eps)
    x64 = x.astype(np.float64)
    for qi in range(nq):
        d2 = ((x64 - q[qi].astype(np.float64)) ** 2).sum(axis=1)
        want = np.argsort(d2, kind="stable")[:k]
        if spacing >= 1e-5 or qi not in (0, nq // 2, nq - 1):
            assert I[qi].tolist() == want.tolist(), (qi, I[qi], want)
        else:
            ok, msg = flat.adjudicate(x, q[qi], k, D[qi], I[qi], metric=flat.METRIC_L2, tol=TOL, tie_eps=4e-6)
            assert ok, msg
        np.testing.assert_allclose(D[qi], d2[I[qi]], atol=TOL, rtol=0)
    idx.close()


@pytest.mark.parametrize("frac,must_rerun", [(1 / 48, True), (0.9, False)])
def test_l2_offsets_certificate_at_the_margin(native, frac, must_rerun):
    """The certificate of the L2 pass with per-row offsets (rows of mixed norms: largest norm B = 2): 30 UNIT rows graded
    `frac * eps * B` apart in q.x - |x|^2 / 2 (twice that in squared distance), stored contiguously so that one block list
    holds them all.  Steps of eps B / 48: the 16 a block list keeps end 0.125 eps B below the 10th result — the certificate
    (margin eps B |q| + eps_h) MUST refuse and the device-gated exact scan must return the right ids; steps of 0.9 eps B:
    5.4 eps B of room — it must certify on its own.  Either way the ids are exact."""
    n, d, k, nq = 20000, 512, 10, 40
    B = 2.0
    eps = native.half_eps(d) * B
    spacing = frac * eps
    rs = np.random.RandomState(int(frac * 1e4) + 7)
    x = _corpus(n, d)
    x *= np.exp(rs.uniform(np.log(0.5), np.log(1.9), size=(n, 1))).astype(np.float32)   # rows of mixed norms ...
    x[777] *= np.float32(B / np.linalg.norm(x[777].astype(np.float64)))               # ... the largest exactly B
    q = _corpus(nq, d, seed=4242)
    cos = 0.9 - spacing * np.arange(30)
    for qi, base in ((0, 500), (nq // 2, 9000), (nq - 1, 15000)):
        rows = _graded_rows(q[qi], cos, rs)
        x[base:base + 30] = rows[rs.permutation(30)]
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.add(x)
    before = native.split_rerun_count()
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search(q, k)
        assert _split_launches(native) > 0, "the certified pass did not run"
        assert native.prof_symbol("ip_scan_half_seed").startswith("flat_scan_h16_kernel")   # the offsets form: the shadow kernel seeds
    finally:
        native.prof_enable(False)
    reran = native.split_rerun_count() - before
    assert (reran >= 1) == must_rerun, (reran, eps)
    x64 = x.astype(np.float64)
    for qi in range(nq):
        d2 = ((x64 - q[qi].astype(np.float64)) ** 2).sum(axis=1)
        want = np.argsort(d2, kind="stable")[:k]
        if spacing >= 1e-5 or qi not in (0, nq // 2, nq - 1):
            assert I[qi].tolist() == want.tolist(), (qi, I[qi], want)
        else:
            ok, msg = flat.adjudicate(x, q[qi], k, D[qi], I[qi], metric=flat.METRIC_L2, tol=TOL * 4, tie_eps=1.6e-5)
            assert ok, msg
        np.testing.assert_allclose(D[qi], d2[I[qi]], atol=TOL * 4, rtol=0)
    idx.close()


@pytest.mark.parametrize("frac,must_rerun", [(1 / 48, True), (0.9, False)])
def test_fp16_certificate_at_the_margin_k32(native, frac, must_rerun):
    """k = 32 on the fp16 pass (64 nominees re-scored): 80 rows graded `frac * eps` apart, SCATTERED over the corpus (every
    block list holds at most a few).  Steps of eps / 48: the 64th nominee is only 0.67 eps below the 32nd result — the
    certificate must refuse and the exact re-run must return the right ids; steps of 0.9 eps: 29 eps of room — it must
    certify on its own.  Either way the ids are exact."""
    n, d, k, nq = 40000, 512, 32, 40
    assert native.half_max_queries(d) >= nq
    eps = native.half_eps(d)
    spacing = frac * eps
    rs = np.random.RandomState(int(frac * 1e4) + 32)
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=4242)
    cos = 0.9 - spacing * np.arange(80)
    for qi, base in ((0, 100), (17, 133), (39, 171)):
        rows = _graded_rows(q[qi], cos, rs)
        x[base + 490 * rs.permutation(80)] = rows          # one planted row every 490 rows, in random score order
    idx = native.FlatIndex(d)
    idx.add(x)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    reran = native.split_rerun_count() - before
    assert (reran >= 1) == must_rerun, (reran, eps)
    x64 = x.astype(np.float64)
    for qi in range(nq):
        t = x64 @ q[qi].astype(np.float64)
        want = np.argsort(-t, kind="stable")[:k]
        if spacing >= 1e-5 or qi not in (0, 17, 39):
            assert I[qi].tolist() == want.tolist(), (qi, I[qi], want)
        else:
            ok, msg = flat.adjudicate(x, q[qi], k, D[qi], I[qi], tol=TOL)
            assert ok, msg
        np.testing.assert_allclose(D[qi], t[I[qi]], atol=TOL, rtol=0)
    idx.close()


def test_uncertified_queries_are_rerun_one_by_one(native):
    """200 queries, three of them with 40 exact copies of their best row in the corpus: those three fail the certificate
    and ONLY they are re-run on the exact kernels, gathered on the device into one compact batch (the launches of the
    re-run are gated by the device-side count: the host never learns which queries they were).  Every result is exact."""
    n, d, k, nq = 30000, 512, 10, 200
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=77)
    for qi, base in ((3, 1000), (130, 9000), (199, 20000)):
        x[base:base + 40] = q[qi]
    idx = native.FlatIndex(d)
    idx.add(x)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    assert native.split_rerun_count() == before + 1     # one 256-wide pass held all 200 queries
    for qi, base in ((3, 1000), (130, 9000), (199, 20000)):
        assert I[qi].tolist() == list(range(base, base + 10))   # ties resolve to the lowest row numbers
    _check(native, x, q, k, D, I)
    for i in (0, 3, 64, 130, 131, 199):
        D1, I1 = idx.search(q[i], k)
        assert np.array_equal(I1[0], I[i])
        np.testing.assert_allclose(D1[0], D[i], atol=2e-6, rtol=0)
    idx.close()


def test_large_batch_is_cut_into_passes(native):
    """700 queries in one call at d = 384: two 256-query passes, one 128-query pass (60 real queries... 188 left ->
    256-wide), every result equal to the single-query search and to the oracle."""
    n, d, k, nq = 20000, 384, 10, 700
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=5)
    idx = native.FlatIndex(d)
    idx.add(x)
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search(q, k)
        assert _split_launches(native) == 3          # 256 + 256 + 188 queries
    finally:
        native.prof_enable(False)
    _check(native, x, q, k, D, I)
    for i in (0, 255, 256, 511, 512, 699):
        D1, I1 = idx.search(q[i], k)
        assert np.array_equal(I1[0], I[i])
        np.testing.assert_allclose(D1[0], D[i], atol=2e-6, rtol=0)
    idx.close()


def test_fp16_pass_queries_outside_its_range_go_to_the_exact_kernels(native):
    """A zero query (every score ties: nothing can be certified), a query scaled by 1e30 and one scaled by 1e-30 (outside
    the 2^-40 .. 2^40 window the fp16 images are scaled from) ride in a 150-query batch: they are re-run on the exact
    kernels, every other query is served by the fp16 pass, and all results are exact."""
    n, d, k, nq = 30000, 512, 10, 150
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=99)
    q[5] = 0.0
    q[7] *= np.float32(1e30)
    q[9] *= np.float32(1e-30)
    idx = native.FlatIndex(d)
    idx.add(x)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    assert native.split_rerun_count() == before + 1
    assert I[5].tolist() == list(range(k)) and not D[5].any()          # all ties: lowest row numbers, score 0
    x64 = x.astype(np.float64)
    for i in range(nq):
        if i == 5:
            continue
        t = x64 @ q[i].astype(np.float64)
        want = np.argsort(-t, kind="stable")[:k]
        assert I[i].tolist() == want.tolist(), i
        np.testing.assert_allclose(D[i], t[I[i]], rtol=1e-5, atol=1e-4 * float(np.linalg.norm(q[i].astype(np.float64))))
    idx.close()


def test_split_precision_pass_falls_back_when_it_cannot_certify(native, monkeypatch):
    """40 copies of each query's best row: more than 16 - k rows tie with the k-th score, the certificate fails
    and the chunk is re-run on the exact kernels; ties still resolve to the lowest row numbers."""
    n, d, k, nq = 6000, 128, 10, 48
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=31)
    x[100:140] = q[0]          # 40 exact copies of query 0
    x[2000:2011] = x[5]        # a smaller cluster elsewhere
    idx = native.FlatIndex(d)
    idx.add(x)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    assert native.split_rerun_count() == before + 1
    assert I[0].tolist() == list(range(100, 110))
    _check(native, x, q, k, D, I)
    for i in range(nq):
        D1, I1 = idx.search(q[i], k)
        assert np.array_equal(I1[0], I[i])
    # non-finite rows switch the pass off for the index instead of poisoning the margin
    y = _corpus(500, d)
    y[7, 3] = np.inf
    idx2 = native.FlatIndex(d)
    idx2.add(y)
    native.prof_enable(True)
    try:
        _split_launches(native)
        idx2.search(q, k)
        assert _split_launches(native) == 0
    finally:
        native.prof_enable(False)
    idx2.close()
    idx.close()


def test_batch_search_never_syncs_and_is_capturable(native):
    """mvdb_index_search_device reads nothing back from the device: queries a certified batch pass cannot certify are
    compacted, re-run on the exact kernels and scattered by launches that are enabled on the device.  So a 256-query
    search — one of its queries planted on 40 exact duplicates, which MUST be re-run — can be captured into a hipGraph
    (after one eager call has sized the stream's workspace) and replays to the eager call's ids and scores; with other
    queries in the same buffers the replay re-decides on the device which of them to re-run."""
    import torch
    n, d, k, nq = 30000, 512, 10, 256
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=77)
    x[1000:1040] = q[3]            # query 3 cannot be certified
    q2 = _corpus(nq, d, seed=78)
    x[9000:9040] = q2[130]         # in the second query set it is query 130 (and query 3 certifies)
    idx = native.FlatIndex(d)
    idx.add(x)
    dev = torch.device("cuda", 0)
    qt = torch.from_numpy(q).to(dev)
    D = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        before = native.split_rerun_count()
        idx.search_device(qt.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream=stream.cuda_stream)   # eager: sizes the workspace
        stream.synchronize()
        assert native.split_rerun_count() == before + 1
        D0, I0 = D.cpu().numpy().copy(), I.cpu().numpy().copy()
        assert I0[3].tolist() == list(range(1000, 1010))
        _check(native, x, q, k, D0, I0)
        g = torch.cuda.CUDAGraph()
        D.zero_()
        I.zero_()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            idx.search_device(qt.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream=stream.cuda_stream)
        g.replay()
        stream.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(I.cpu().numpy(), I0) and np.array_equal(D.cpu().numpy(), D0)
        # other queries through the SAME graph: which of them is re-run is decided on the device at replay time
        qt.copy_(torch.from_numpy(q2).to(dev))
        g.replay()
        torch.cuda.synchronize()
        D1, I1 = D.cpu().numpy(), I.cpu().numpy()
        assert I1[130].tolist() == list(range(9000, 9010))
        _check(native, x, q2, k, D1, I1)
    idx.close()


def test_fp16_shadow_follows_the_index(native):
    """Batches of 33+ queries at d = 256 / 384 / 512 nominate from an fp16 SHADOW of the rows (flat_scan_h16_kernel: half the
    bytes of the fp32 rows, no conversion).  It is built by the first such search, extended by add, emptied by remove_rows and
    by adds that change the scale (a larger row norm), rebuilt on demand — and every result equals the oracle's and what the same
    index returns with the shadow switched off (half_shadow = 0: the exact fp32-MFMA passes since round 6 — same ids, scores
    within fp32 rounding of the certified pass's re-scores)."""
    import os
    for d in (512, 384, 256):
        n, k, nq = 50000, 10, 130
        x = _corpus(n + 2000, d)
        q = _corpus(nq, d, seed=31)
        idx = native.FlatIndex(d)
        idx.reserve(n + 4000)
        idx.add(x[:30000], normalize=True)
        assert idx.shadow_rows == 0
        D1, I1 = idx.search(q[:8], k)            # fewer than 33 queries: no shadow
        assert idx.shadow_rows == 0
        D, I = idx.search(q, k)
        assert idx.shadow_rows == 30000
        _check(native, x[:30000], q, k, D, I)
        idx.add(x[30000:n], normalize=True)      # fits the reservation: the shadow is extended in place
        assert idx.shadow_rows == n
        D, I = idx.search(q, k)
        _check(native, x[:n], q, k, D, I)
        os.environ["MVDB_DISABLE_HALF_SHADOW"] = "1"
        idx.reload_env()
        try:
            D0, I0 = idx.search(q, k)
        finally:
            del os.environ["MVDB_DISABLE_HALF_SHADOW"]
            idx.reload_env()
        assert np.array_equal(I0, I)
        np.testing.assert_allclose(D0, D, rtol=0, atol=2e-6)
        idx.remove_rows(np.array([5, 40000], np.int64))
        assert idx.shadow_rows == 0
        cur = np.delete(x[:n], [5, 40000], 0)
        D, I = idx.search(q, k)
        assert idx.shadow_rows == n - 2
        _check(native, cur, q, k, D, I)
        idx.add(x[n:n + 2000] * np.float32(3.0))   # raw rows of norm 3: the scale of the fp16 image changes -> rebuilt
        assert idx.shadow_rows == 0
        cur = np.concatenate([cur, x[n:n + 2000] * np.float32(3.0)])
        D, I = idx.search(q, k)
        assert idx.shadow_rows == cur.shape[0]
        _check(native, cur, q, k, D, I)
        idx.close()


def test_captured_search_survives_a_larger_eager_call_on_its_stream(native):
    """A captured search names its stream's workspace buffers.  A later, LARGER eager call on the same stream must not free
    them (it allocates new ones and parks the old): replaying the earlier graph still answers correctly."""
    import torch
    n, d, k = 40000, 512, 10
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    idx.add(x)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    q_small = _corpus(8, d, seed=5)
    q_big = _corpus(700, d, seed=6)
    qt = torch.from_numpy(q_small).to(dev)
    D = torch.empty((8, k), dtype=torch.float32, device=dev)
    I = torch.empty((8, k), dtype=torch.int64, device=dev)
    with torch.cuda.stream(stream):
        idx.search_device(qt.data_ptr(), 8, k, D.data_ptr(), I.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        D0, I0 = D.cpu().numpy().copy(), I.cpu().numpy().copy()
        _check(native, x, q_small, k, D0, I0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            idx.search_device(qt.data_ptr(), 8, k, D.data_ptr(), I.data_ptr(), stream=stream.cuda_stream)
        # far larger shapes on the same stream: every workspace buffer of the 8-query call is outgrown
        qb = torch.from_numpy(q_big).to(dev)
        Db = torch.empty((700, 64), dtype=torch.float32, device=dev)
        Ib = torch.empty((700, 64), dtype=torch.int64, device=dev)
        idx.search_device(qb.data_ptr(), 700, 64, Db.data_ptr(), Ib.data_ptr(), stream=stream.cuda_stream)
        idx.search_device(qb.data_ptr(), 300, 200, Db.data_ptr(), Ib.data_ptr(), stream=stream.cuda_stream)  # k > 64: the score matrix
        stream.synchronize()
        junk = [torch.full((1 << 22,), 7, dtype=torch.int64, device=dev) for _ in range(8)]   # reuse whatever WAS freed
        for _ in range(3):
            D.zero_()
            I.zero_()
            g.replay()
            stream.synchronize()
            assert np.array_equal(I.cpu().numpy(), I0) and np.array_equal(D.cpu().numpy(), D0)
        del junk
    idx.close()


def test_add_does_not_synchronise_the_device(native):
    """Mutators wait for the searches of THEIR index only and work on the index's own stream: with ~0.3 s of unrelated work
    queued on another stream (an encoder forward in production), a store into an index returns — rows searchable — while
    that stream is still busy; and a search already enqueued on the index being grown is waited for."""
    import time
    import torch
    dev = torch.device("cuda", 0)
    d = 256
    idx = native.FlatIndex(d)
    x = _corpus(20000, d)
    idx.reserve(40000)   # (outgrowing the allocation frees the old matrix: hipFree is a device-wide wait, amortised by the
                         #  geometric growth; the steady-state add below must not wait for anybody else's work)
    idx.add(x[:10000], normalize=True)
    busy = torch.cuda.Stream(dev)
    a = torch.randn((8192, 8192), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(busy):
        for _ in range(40):
            a = (a @ a).clamp_(-1, 1)
    t_enq = time.perf_counter() - t0
    idx.add(x[10000:], normalize=True)          # upload + normalise on the index's own stream
    D, I = idx.search(x[15000], 3)
    still_busy = not busy.query()
    t_add = time.perf_counter() - t0 - t_enq
    busy.synchronize()
    t_all = time.perf_counter() - t0
    assert I[0, 0] == 15000
    assert still_busy, f"the add waited for an unrelated stream ({t_add * 1e3:.1f} ms of {t_all * 1e3:.1f} ms)"
    # a search in flight on a caller stream IS waited for: its results are those of the pre-add matrix
    s = torch.cuda.Stream(dev)
    qt = torch.from_numpy(_corpus(4, d, seed=3)).to(dev)
    Dd = torch.empty((4, 5), dtype=torch.float32, device=dev)
    Id = torch.empty((4, 5), dtype=torch.int64, device=dev)
    with torch.cuda.stream(s):
        idx.search_device(qt.data_ptr(), 4, 5, Dd.data_ptr(), Id.data_ptr(), stream=s.cuda_stream)
    idx.add(qt.cpu().numpy() * 3.0, normalize=True)   # rows 20000..20003 = the queries themselves
    s.synchronize()
    assert (Id.cpu().numpy() < 20000).all()
    D2, I2 = idx.search(qt.cpu().numpy(), 1)
    assert I2[:, 0].tolist() == [20000, 20001, 20002, 20003]
    idx.close()


@pytest.mark.parametrize("n,d,nq", [(300_000, 512, 96), (1_000_000, 384, 256), (200_000, 1024, 80), (250_000, 768, 40)])
def test_refused_queries_rerun_from_an_admission_floor_with_identical_results(native, monkeypatch, n, d, nq):
    """A refused query's exact re-run starts its lists from the k-th exact score of the nominees (less a rounding margin) instead
    of -inf (half_certify_kernel -> gather_failed_kernel -> flat_scan_mfma2_gated_kernel).  On a clustered corpus — every batch
    holds refused queries — the results are bit for bit those of the re-run without floors (MVDB_DISABLE_RERUN_FLOOR=1: same
    kernel, same arithmetic).  And the RESCUE pass in front of the re-run (default: the refused queries once more over the
    shadow, every row above the floor kept and re-scored in fp32) answers them itself: the exact passes are skipped, the float64
    adjudication accepts every result, and ids differ from the exact re-run's only inside near-ties."""
    k = 10
    q = flat.synth(nq, d, 5678 | flat.SYNTH_CLUSTERED)
    flat.normalize_l2(q)
    got = {}
    for mode in ("rescue", "floor", "plain"):
        monkeypatch.delenv("MVDB_DISABLE_RERUN_FLOOR", raising=False)
        monkeypatch.delenv("MVDB_DISABLE_RESCUE", raising=False)
        if mode == "floor":
            monkeypatch.setenv("MVDB_DISABLE_RESCUE", "1")
        if mode == "plain":
            monkeypatch.setenv("MVDB_DISABLE_RERUN_FLOOR", "1")
        idx = native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234 | flat.SYNTH_CLUSTERED, normalize=True)
        idx.search(q[:nq], k)  # (builds the shadow and sizes the workspace)
        native.prof_enable(True)
        try:
            for f in ("ip_scan_rescue", "ip_scan_rerun"):
                native.prof_read(f)
            before = native.split_rerun_count()
            D, I = idx.search(q, k)
            assert native.split_rerun_count() > before, "the clustered corpus must refuse some certificates"
            rescue, rerun = native.prof_read("ip_scan_rescue"), native.prof_read("ip_scan_rerun")
        finally:
            native.prof_enable(False)
        if mode == "rescue":
            assert rescue[0] >= 1 and rescue[1] > 0.02, rescue           # the rescue launches ran ...
            assert rerun[1] < 0.05 * max(1, rerun[0]), rerun              # ... and every exact pass returned at its gate
        else:
            assert rescue[0] == 0, rescue
            assert rerun[0] == 1 and rerun[1] > 0.05, rerun               # ONE launch walks the exact passes of the compact batch
        if mode != "plain":
            stored = idx.get_rows(0, n)
            for i in range(0, nq, 3 if mode == "rescue" else 5):
                ok, msg = flat.adjudicate(stored, q[i], k, D[i], I[i], tol=1e-4, tie_eps=2e-6)
                assert ok, (mode, i, msg)
        got[mode] = (D.copy(), I.copy())
        idx.close()
    assert np.array_equal(got["floor"][1], got["plain"][1])
    assert np.array_equal(got["floor"][0].view(np.uint32), got["plain"][0].view(np.uint32))
    # the rescue's scores are the certification kernel's fp32 sums, the re-run's the matrix cores': the same rows but for swaps of
    # rows within rounding of each other
    same = (got["rescue"][1] == got["floor"][1]).mean()
    assert same > 0.9, same
    np.testing.assert_allclose(np.sort(got["rescue"][0], axis=1), np.sort(got["floor"][0], axis=1), rtol=0, atol=2e-6)


def test_rescue_pass_hands_an_overflowing_neighbourhood_to_the_exact_pass(native):
    """60,000 rows within 1e-4 of one direction: for a query along it the rescue pass's 32-deep per-block lists fill (~230 rows
    per block inside the band), the query's `need` word is raised and its exact fp32 pass runs; the other refused queries of the
    batch are answered by the rescue pass.  Every result stands the float64 adjudication."""
    n, d, k, nq = 200_000, 512, 10, 96
    rs = np.random.RandomState(5)
    x = _corpus(n, d)
    v = rs.standard_normal(d).astype(np.float32)
    v /= np.linalg.norm(v)
    x[20_000:80_000] = v + 1e-4 * rs.standard_normal((60_000, d)).astype(np.float32)
    flat.normalize_l2(x)
    q = _corpus(nq, d, seed=41)
    q[3] = v + 1e-3 * rs.standard_normal(d).astype(np.float32)
    q[64] = -v                                   # the same neighbourhood at the bottom of the ranking: certifies
    flat.normalize_l2(q)
    idx = native.FlatIndex(d)
    idx.add(x)
    idx.search(q, k)                             # shadow, workspaces
    native.prof_enable(True)
    try:
        for f in ("ip_scan_rescue", "ip_scan_rerun"):
            native.prof_read(f)
        before = native.split_rerun_count()
        D, I = idx.search(q, k)
        assert native.split_rerun_count() == before + 1
        rescue, rerun = native.prof_read("ip_scan_rescue"), native.prof_read("ip_scan_rerun")
    finally:
        native.prof_enable(False)
    assert rescue[0] == 1 and rescue[1] > 0.02, rescue       # the rescue launch ran ...
    assert rerun[0] == 1 and rerun[1] > 0.03, rerun          # ... and so did the exact pass of the overflowing query
    assert set(I[3].tolist()) <= set(range(20_000, 80_000))
    for i in range(nq):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], I[i], tol=1e-4, tie_eps=2e-6)
        assert ok, (i, msg)
    idx.close()


def test_single_query_shadow_route_suspends_itself_on_a_clustered_corpus(native):
    """The opt-in single-query route costs more than the exact scan when its certificate is refused.  On a clustered corpus (1M
    rows: every query's 10th and 64th best within 1e-3) every call is refused; the library notices within a window of 32 calls
    (a device counter mirrored into host-mapped memory, no synchronisation) and sends the next 512 single queries to the exact
    scan.  Results are the exact scan's in every phase."""
    n, d, k = 1_000_000, 256, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flat.SYNTH_CLUSTERED, normalize=True)
    q = flat.synth(200, d, 5678 | flat.SYNTH_CLUSTERED)
    flat.normalize_l2(q)
    stored = idx.get_rows(0, n)
    lib = native.lib()
    assert lib.mvdb_index_single_route_suspensions(idx.handle) == 0
    idx.set_option("shadow_single_query", 1)
    before = native.split_rerun_count()
    for i in range(200):
        D, I = idx.search(q[i], k)
        # (the exact kernels behind the two routes sum in different orders: rows within 2e-6 of each other may swap, which the
        #  float64 adjudication accepts — and nothing else)
        ok, msg = flat.adjudicate(stored, q[i], k, D[0], I[0], tol=1e-4, tie_eps=2e-6)
        assert ok, (i, msg)
    reruns = native.split_rerun_count() - before
    assert lib.mvdb_index_single_route_suspensions(idx.handle) == 1
    assert 16 <= reruns <= 96, reruns          # the first window (plus what was in flight) paid the nomination pass, the rest did not
    idx.close()
    # a friendly corpus never suspends
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = flat.synth(100, d, 5678)
    flat.normalize_l2(q)
    idx.set_option("shadow_single_query", 1)
    for i in range(100):
        idx.search(q[i], k)
    assert lib.mvdb_index_single_route_suspensions(idx.handle) == 0
    idx.close()


def test_a_corpus_of_duplicates_does_not_stall_the_batch_passes(native):
    """Every row the same vector: every score ties with the k-th best.  The batch passes gate their list inserts on the
    (score, row) KEY since round 5 — with the score-only gate every row paid a wave-cooperative insert attempt the key order
    then refused (64 queries over 1M identical rows: 21.8 ms instead of 0.33).  Results: the k lowest row numbers, as faiss'
    strict-greater heap returns them; cost: within a loose factor of the same batch over distinct rows."""
    import time
    n, d, k = 600_000, 256, 10
    base = _corpus(n, d)
    q = _corpus(64, d, seed=9)

    def timed(idx, nq):
        idx.search(q[:nq], k)
        t0 = time.perf_counter()
        for _ in range(5):
            D, I = idx.search(q[:nq], k)
        return (time.perf_counter() - t0) / 5, D, I

    idx = native.FlatIndex(d)
    idx.add(base)
    t_plain = {nq: timed(idx, nq)[0] for nq in (8, 64)}
    idx.close()
    dup = np.repeat(q[:1], n, axis=0)
    idx = native.FlatIndex(d)
    idx.add(dup)
    for nq in (8, 64):
        t, D, I = timed(idx, nq)
        assert (I == np.arange(k)[None, :]).all(), (nq, I[:2])
        want = (q[:nq] @ q[0]).astype(np.float32)
        np.testing.assert_allclose(D, np.repeat(want[:, None], k, axis=1), atol=1e-5, rtol=0)
        assert t < 15 * t_plain[nq] + 2e-3, f"{nq} queries over duplicates: {t * 1e3:.2f} ms against {t_plain[nq] * 1e3:.2f} ms over distinct rows"
    idx.close()


def test_a_destroyed_caller_stream_does_not_wedge_the_index(native):
    """Round-4 advisor finding: mutators wait on every stream that ever searched the index; a caller that destroyed such a
    stream made every later add / remove_rows / reset / reserve fail.  The dead handle is forgotten (hipStreamDestroy has
    completed its work), anything else falls back to a device-wide wait."""
    import ctypes
    import torch
    dev = torch.device("cuda", 0)
    hip = ctypes.CDLL(None)   # the process's one HIP runtime (torch's, bound RTLD_GLOBAL)
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    d = 128
    idx = native.FlatIndex(d)
    x = _corpus(5000, d)
    idx.add(x[:4000], normalize=True)
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    qt = torch.from_numpy(_corpus(2, d, seed=3)).to(dev)
    Dd = torch.empty((2, 5), dtype=torch.float32, device=dev)
    Id = torch.empty((2, 5), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    idx.search_device(qt.data_ptr(), 2, 5, Dd.data_ptr(), Id.data_ptr(), stream=s.value)
    assert hip.hipStreamSynchronize(s) == 0
    want = Id.cpu().numpy().copy()
    assert hip.hipStreamDestroy(s) == 0
    idx.add(x[4000:], normalize=True)            # waited on the dead stream before the fix: every mutator failed from here on
    idx.remove_rows(np.arange(4000, 4500, dtype=np.int64))
    idx.reserve(20000)
    D, I = idx.search(qt.cpu().numpy(), 5)
    assert I.shape == (2, 5) and idx.ntotal == 4500
    Do, Io = flat.flat_search(idx.get_rows(0, 4500), qt.cpu().numpy(), 5)
    assert np.array_equal(I, Io) and (want < 4000).all()
    idx.close()


def test_single_queries_over_the_shadow_when_asked_for(native, tmp_path):
    """mvdb_index_set_option("shadow_single_query", 1) — and VectorDatabase(fast_single_query=True) — send ONE query per call through the
    certified nomination pass over the fp16 shadow too (>= 500,000 rows at d = 256 / 384 / 512): same ids as the exact scan and as
    the oracle, fp32 re-scored distances; a query with 40 exact copies of its best row cannot be certified and comes back from the
    exact re-run.  Off (the default) the single-query scan is the exact fp32 kernel and no shadow is built."""
    n, d, k = 520_000, 256, 10
    x = _corpus(n, d)
    q = _corpus(24, d, seed=77)
    x[1000:1040] = q[3]
    idx = native.FlatIndex(d)
    idx.add(x)
    exact = [idx.search(q[i], k) for i in range(24)]
    assert idx.shadow_rows == 0
    idx.set_option("shadow_single_query", 1)
    before = native.split_rerun_count()
    native.prof_enable(True)
    try:
        _split_launches(native)
        fast = [idx.search(q[i], k) for i in range(24)]
        assert _split_launches(native) >= 24, "the certified pass did not serve the single queries"
    finally:
        native.prof_enable(False)
    assert idx.shadow_rows == n
    assert native.split_rerun_count() - before >= 1          # the query with 40 tied rows
    for i in range(24):
        assert np.array_equal(fast[i][1], exact[i][1]), i
        np.testing.assert_allclose(fast[i][0], exact[i][0], atol=2e-6, rtol=0)
    D = np.concatenate([f[0] for f in fast])
    I = np.concatenate([f[1] for f in fast])
    _check(native, x, q, k, D, I)
    idx.set_option("shadow_single_query", 0)
    with pytest.raises(ValueError):
        idx.set_option("no_such_option", 1)
    idx.close()
    # the drop-in class: same answers with and without the switch
    from minivectordb_amd import VectorDatabase
    fastdb = VectorDatabase(storage_file=str(tmp_path / "fast.pkl"), fast_single_query=True)
    plain = VectorDatabase(storage_file=str(tmp_path / "plain.pkl"))
    ids = list(range(n))
    for db in (fastdb, plain):
        db.store_embeddings_batch(ids, x)
    for i in (0, 3, 23):
        a = fastdb.find_most_similar(q[i], k=k)
        b = plain.find_most_similar(q[i], k=k)
        assert list(a[0]) == list(b[0])
        np.testing.assert_allclose(a[1], b[1], atol=2e-6, rtol=0)
    assert fastdb.index.shadow_rows == n and plain.index.shadow_rows == 0


def test_delete_does_not_synchronise_the_device(native):
    """remove_rows on an index that holds an fp16 shadow: the shadow is emptied, not freed (hipFree waits for the whole device),
    the compaction runs on the index's own stream through the staging buffer the index keeps from its first delete on — so with
    unrelated work queued on another stream a delete returns, rows renumbered and searchable, while that stream is still busy."""
    import time
    import torch
    dev = torch.device("cuda", 0)
    d, n = 256, 120_000
    x = _corpus(n, d)
    idx = native.FlatIndex(d)
    idx.add(x, normalize=True)
    q = _corpus(40, d, seed=9)
    idx.search(q, 5)                                   # builds the shadow
    assert idx.shadow_rows == n
    idx.remove_rows(np.array([n - 1], np.int64))       # first delete: allocates the staging buffer (kept)
    cur = x[:n - 1]
    idx.search(q, 5)
    assert idx.shadow_rows == n - 1
    busy = torch.cuda.Stream(dev)
    a = torch.randn((8192, 8192), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(busy):
        for _ in range(40):
            a = (a @ a).clamp_(-1, 1)
    t_enq = time.perf_counter() - t0
    idx.remove_rows(np.array([7, 50_000], np.int64))
    D1, I1 = idx.search(x[60_000], 3)
    still_busy = not busy.query()
    t_del = time.perf_counter() - t0 - t_enq
    busy.synchronize()
    assert I1[0, 0] == 60_000 - 2 and idx.ntotal == n - 3
    assert still_busy, f"the delete waited for an unrelated stream ({t_del * 1e3:.1f} ms)"
    assert idx.shadow_rows == 0                        # emptied; the next batch rebuilds it in the same allocation
    cur = np.delete(cur, [7, 50_000], 0)
    D, I = idx.search(q, 5)
    assert idx.shadow_rows == n - 3
    _check(native, cur, q, 5, D, I)
    idx.close()


# ---- bitmap-selected search and resident row sets (reference: the per-query sub-index, vector_database.py:508-523) --------
@pytest.mark.parametrize("d,metric", [(512, flat.METRIC_IP), (100, flat.METRIC_IP), (384, flat.METRIC_L2)])
@pytest.mark.parametrize("frac", [0.01, 0.5, 0.99])
def test_masked_search_equals_the_subset_search_of_the_ascending_list(native, d, metric, frac):
    """mvdb_index_search_masked == mvdb_index_search_subset on the ascending list of the mask's set rows: same scores, and
    with labels = positions the same labels (the oracle's flat_search(rows=...)); labels = rows gives rows[position].  Exact
    ties (planted duplicates) resolve to the lower row in both."""
    n, k, nq = 50_000, 10, 3
    x = _corpus(n, d, normalize=metric == flat.METRIC_IP)
    q = _corpus(nq, d, seed=9, normalize=metric == flat.METRIC_IP)
    x[40_001] = x[300]       # exact duplicates: equal scores for every query
    x[777] = x[300]
    rs = np.random.RandomState(int(frac * 100) + d)
    rows = np.sort(rs.choice(n, int(n * frac), replace=False)).astype(np.int64)
    rows = np.unique(np.concatenate([rows, [300, 777, 40_001]]))
    q[0] = x[300]            # query 0's best rows ARE the three duplicates
    idx = native.FlatIndex(d, metric=metric)
    idx.add(x)
    mask = native.pack_row_mask(n, rows=rows)
    Dp, Ip = idx.search_masked(q, k, mask, labels="positions")
    Do, Io = flat.flat_search(x, q, k, metric=metric, rows=rows)
    Ds, Is = idx.search_subset(q, k, rows)
    assert np.array_equal(Ip, Is)
    np.testing.assert_allclose(Dp, Ds, atol=2e-6, rtol=0)    # (several queries + bitmap: the fp32-MFMA pass; the list: the GEMV scan)
    D1, I1 = idx.search_masked(q[1], k, mask, labels="positions")
    D2, I2 = idx.search_subset(q[1], k, rows)
    assert np.array_equal(I1, I2)
    np.testing.assert_allclose(D1, D2, atol=0, rtol=0)       # one query: the same kernel arithmetic, row for row
    _check(native, x, q, k, Dp, Ip, metric=metric, rows=rows)
    Dr, Ir = idx.search_masked(q, k, mask, labels="rows")
    assert np.array_equal(Ir, rows[Ip]) and np.array_equal(Dr, Dp)
    assert Ir[0, :3].tolist() == [300, 777, 40_001]           # ties: ascending row
    idx.close()


@pytest.mark.parametrize("d,nq,k", [(512, 8, 10), (512, 40, 10), (384, 256, 10), (512, 300, 32), (768, 130, 10), (128, 40, 10),
                                    (100, 40, 10)])
@pytest.mark.parametrize("frac", [0.5, 0.97])
def test_masked_batches_match_oracle(native, d, nq, k, frac):
    """A bitmap and a BATCH of queries: 33+ queries go through the fp16 nomination pass (the bit is looked at where a row is
    about to be nominated), fewer — and widths without that pass (d = 128) — through the staged fp32-MFMA pass, d = 100
    through the one-query scan; the best rows of several queries sit OUTSIDE the selection and must not come back.
    Ids equal the oracle's on the selected rows."""
    n = 60_000
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=31)
    rs = np.random.RandomState(d + nq)
    rows = np.sort(rs.choice(n, int(n * frac), replace=False)).astype(np.int64)
    sel = np.zeros(n, bool)
    sel[rows] = True
    out = np.flatnonzero(~sel)
    for j, qi in enumerate(range(0, nq, max(1, nq // 7))):      # a perfect match per probed query, outside the selection
        x[out[11 * j + 3]] = q[qi]
    idx = native.FlatIndex(d)
    idx.add(x)
    mask = native.pack_row_mask(n, rows=rows)
    D, I = idx.search_masked(q, k, mask, labels="rows")
    assert sel[I].all()
    _check(native, x, q, k, D, np.searchsorted(rows, I), rows=rows)
    Dp, Ip = idx.search_masked(q, k, mask, labels="positions")
    assert np.array_equal(rows[Ip], I) and np.array_equal(Dp, D)
    idx.close()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("d,nq,k", [(512, 40, 10), (256, 130, 10), (384, 64, 32)])
def test_l2_batches_under_a_bitmap(native, d, nq, k, mixed):
    """The L2 metric, a bitmap and a batch (round 4): through the fp16 nomination pass — rows of one norm by inner product
    with the norm-range certificate, rows of mixed norms by q.x - |x|^2 / 2 with per-row offsets —, the gate looks the bit up,
    uncertified queries are re-run by the single-query scan under the same bitmap.  Perfect matches OUTSIDE the selection
    must not come back; two queries have 30 exact copies of their nearest row inside it (their certificate must fail)."""
    n = 60_000
    rs = np.random.RandomState(d + nq + mixed)
    x = _corpus(n, d)
    if mixed:
        x *= np.exp(rs.uniform(np.log(0.2), np.log(2.5), size=(n, 1))).astype(np.float32)
    q = _corpus(nq, d, seed=41)
    rows = np.sort(rs.choice(n, int(n * 0.6), replace=False)).astype(np.int64)
    sel = np.zeros(n, bool)
    sel[rows] = True
    out = np.flatnonzero(~sel)
    for j, qi in enumerate(range(0, nq, max(1, nq // 5))):
        x[out[13 * j + 1]] = q[qi]                              # distance 0, not selected
    for qi, base in ((1, 2000), (nq - 2, 30_000)):
        sel[base:base + 30] = True
        x[base:base + 30] = q[qi] * np.float32(0.999)
    rows = np.flatnonzero(sel).astype(np.int64)
    idx = native.FlatIndex(d, metric=native.METRIC_L2)
    idx.add(x)
    mask = native.pack_row_mask(n, rows=rows)
    before = native.split_rerun_count()
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search_masked(q, k, mask, labels="rows")
        assert _split_launches(native) > 0, "the certified pass did not run"
        # the exact re-run under the bitmap is enabled per query ON THE DEVICE (round-4 advisor finding: the masked form had no
        # gated instantiation, so every query of the batch paid a full masked scan behind the certified pass)
        sym = native.prof_symbol("ip_scan")
        assert sym.startswith("flat_scan_kernel<") and sym.endswith(", true>"), sym
    finally:
        native.prof_enable(False)
    assert native.split_rerun_count() - before >= 1
    assert sel[I].all()
    mag = float(max(1.0, np.abs(D).max()))
    pos = np.searchsorted(rows, I)
    for i in range(nq):
        ok, msg = flat.adjudicate(x, q[i], k, D[i], pos[i], metric=flat.METRIC_L2, rows=rows, tol=1e-4 * mag, tie_eps=4e-6 * mag)
        assert ok, (i, msg)
    Dp, Ip = idx.search_masked(q, k, mask, labels="positions")
    assert np.array_equal(rows[Ip], I) and np.array_equal(Dp, D)
    idx.close()


def test_masked_batch_reruns_uncertified_queries_under_the_mask(native):
    """200 queries under a bitmap keeping 70 % of the rows; three of them have 40 exact copies of their best row INSIDE the
    selection (their certificates must fail: the exact re-run — the gated fp32-MFMA pass, with the bitmap — answers them)
    and 40 more copies OUTSIDE it (never returned)."""
    n, d, k, nq = 40_000, 512, 10, 200
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=78)
    sel = np.ones(n, bool)
    sel[np.random.RandomState(5).choice(n, int(0.3 * n), replace=False)] = False
    for qi, base in ((3, 1000), (130, 9000), (199, 20000)):
        sel[base:base + 40] = True
        x[base:base + 40] = q[qi]
        sel[base + 5000:base + 5040] = False
        x[base + 5000:base + 5040] = q[qi]
    rows = np.flatnonzero(sel).astype(np.int64)
    idx = native.FlatIndex(d)
    idx.add(x)
    mask = native.pack_row_mask(n, rows=rows)
    before = native.split_rerun_count()
    D, I = idx.search_masked(q, k, mask, labels="rows")
    assert native.split_rerun_count() == before + 1
    assert sel[I].all()
    for qi, base in ((3, 1000), (130, 9000), (199, 20000)):
        assert I[qi].tolist() == list(range(base, base + 10))   # ties resolve to the lowest row numbers
    _check(native, x, q, k, D, np.searchsorted(rows, I), rows=rows)
    rs_ = idx.rowset(np.flatnonzero(~sel).astype(np.int64), excluded=True)   # the same through a resident (bitmap) row set
    assert rs_.is_bitmap
    Dr, Ir = idx.search_rowset(q, k, rs_)
    assert np.array_equal(Ir, I)
    np.testing.assert_allclose(Dr, D, atol=2e-6, rtol=0)
    rs_.close()
    idx.close()


def test_masked_search_edge_cases(native):
    """k larger than the number of selected rows (tail -1), k > 64 (scores + radix select path), an empty mask, a mask with
    bits set beyond ntotal, several queries."""
    n, d = 20_000, 256
    x = _corpus(n, d)
    q = _corpus(2, d, seed=4)
    idx = native.FlatIndex(d)
    idx.add(x)
    rows = np.array([5, 17, 19_999], dtype=np.int64)
    mask = native.pack_row_mask(n, rows=rows)
    mask[-1] |= np.uint64(0xFFFF) << np.uint64(48)            # garbage beyond row n - 1 must be ignored
    D, I = idx.search_masked(q, 8, mask)
    t = x[rows].astype(np.float64) @ q.astype(np.float64).T
    for i in range(2):
        want = rows[np.argsort(-t[:, i], kind="stable")]
        assert I[i, :3].tolist() == want.tolist() and (I[i, 3:] == -1).all()
        assert (D[i, 3:] == np.float32(-3.4028234663852886e38)).all()
    D0, I0 = idx.search_masked(q, 5, np.zeros_like(mask))
    assert (I0 == -1).all()
    rs = np.random.RandomState(1)
    many = np.sort(rs.choice(n, 9000, replace=False)).astype(np.int64)
    mk = native.pack_row_mask(n, rows=many)
    for k in (100, 1000):                                      # the scores + select path, restricted by the bitmap
        Dk, Ik = idx.search_masked(q, k, mk)
        Do, Io = flat.flat_search(x, q, k, rows=many)
        assert np.array_equal(Ik, many[Io])
        np.testing.assert_allclose(Dk, Do, atol=2e-6, rtol=0)
    Dm, Im = idx.search_masked(q, 9500, mk)                    # more than the mask selects
    assert (Im[:, :9000] >= 0).all() and (Im[:, 9000:] == -1).all()
    idx.close()


@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2])
def test_batches_under_a_resident_row_list_share_corpus_passes(native, metric):
    """A sorted row LIST kept resident (a filter keeping 30 % of the rows stays a list: one gathered scan per query costs
    0.3 passes) also carries its bitmap twin: a BATCH of 40 queries under it is searched on shared corpus passes (round 4) —
    same row labels, ties to the lower row as in the list —, a single query and an UNSORTED list keep the gathered scan."""
    n, d, k, nq = 200_000, 256, 10, 40
    x = _corpus(n, d)
    q = _corpus(nq, d, seed=12)
    rs = np.random.RandomState(4)
    rows = np.sort(rs.choice(n, int(0.3 * n), replace=False)).astype(np.int64)
    x[rows[100]] = x[rows[5000]]                                 # an exact tie inside the selection
    q[3] = x[rows[100]]
    idx = native.FlatIndex(d, metric=native.METRIC_L2 if metric == flat.METRIC_L2 else native.METRIC_IP)
    idx.add(x)
    s = idx.rowset(rows)
    assert not s.is_bitmap and len(s) == len(rows)
    native.prof_enable(True)
    try:
        _split_launches(native)
        D, I = idx.search_rowset(q, k, s)
        assert _split_launches(native) > 0, "the batch did not share corpus passes"
        D1, I1 = idx.search_rowset(q[3], k, s)                  # one query: the gathered scan
        assert _split_launches(native) == 0
    finally:
        native.prof_enable(False)
    sel = np.zeros(n, bool)
    sel[rows] = True
    assert sel[I].all()
    assert I[3, :2].tolist() == sorted([int(rows[100]), int(rows[5000])])
    assert np.array_equal(I1[0], I[3])
    np.testing.assert_allclose(D1[0], D[3], atol=4e-6, rtol=0)
    _check(native, x, q, k, D, np.searchsorted(rows, I), rows=rows, metric=metric)
    shuffled = rows[rs.permutation(len(rows))]
    s2 = idx.rowset(shuffled)
    native.prof_enable(True)
    try:
        _split_launches(native)
        D2, I2 = idx.search_rowset(q[:4], k, s2)
        assert _split_launches(native) == 0                     # caller's order decides ties: no bitmap twin
    finally:
        native.prof_enable(False)
    for i in (0, 1, 2):
        assert np.array_equal(I2[i], I[i])
    s.close()
    s2.close()
    idx.close()


def test_resident_row_sets(native):
    """mvdb_rowset: a filter's rows made resident once.  An unsorted list stays a list (ties by list position, as the
    reference's sub-index); a sorted list that keeps 90 % of the rows, and every 'all but these' set, become bitmaps;
    results are ROW NUMBERS and equal the subset search; appends keep a set valid (new rows are not part of it), a removal
    makes it stale (ValueError)."""
    n, d, k = 30_000, 512, 10
    x = _corpus(n, d)
    q = _corpus(2, d, seed=2)
    x[123] = x[29_000]                                          # a tie between rows 123 and 29,000
    q[0] = x[123]
    idx = native.FlatIndex(d)
    idx.add(x)
    rs = np.random.RandomState(3)
    perm = rs.permutation(n)[:5000].astype(np.int64)
    perm = np.concatenate([[29_000, 123], perm[(perm != 123) & (perm != 29_000)]])   # 29,000 is listed BEFORE 123
    s1 = idx.rowset(perm)
    assert not s1.is_bitmap and len(s1) == len(perm)
    D1, I1 = idx.search_rowset(q, k, s1)
    Ds, Is = idx.search_subset(q, k, perm)
    assert np.array_equal(I1, perm[Is]) and np.array_equal(D1, Ds)
    assert I1[0, :2].tolist() == [29_000, 123]                   # list order decides the tie
    dense = np.sort(rs.choice(n, 28_000, replace=False)).astype(np.int64)
    dense = np.unique(np.concatenate([dense, [123, 29_000]]))
    s2 = idx.rowset(dense)
    assert s2.is_bitmap and len(s2) == len(dense)
    D2, I2 = idx.search_rowset(q, k, s2)
    Dd, Id = idx.search_subset(q, k, dense)
    assert np.array_equal(I2, dense[Id])                       # (two queries + bitmap: the fp32-MFMA pass; the list: the GEMV scan)
    np.testing.assert_allclose(D2, Dd, atol=2e-6, rtol=0)
    assert I2[0, :2].tolist() == [123, 29_000]                   # ascending rows
    excl = np.array([123, 7, 7, 15_000], dtype=np.int64)          # a row listed twice is removed once
    s3 = idx.rowset(excl, excluded=True)
    assert s3.is_bitmap and len(s3) == n - 3
    D3, I3 = idx.search_rowset(q, k, s3)
    keep = np.setdiff1d(np.arange(n), excl)
    De, Ie = idx.search_subset(q, k, keep)
    assert np.array_equal(I3, keep[Ie])
    np.testing.assert_allclose(D3, De, atol=2e-6, rtol=0)
    assert 123 not in I3[0] and I3[0, 0] == 29_000
    idx.add(_corpus(10, d, seed=8))                               # appended rows: the sets still answer, without them
    D3b, I3b = idx.search_rowset(q, k, s3)
    assert np.array_equal(I3b, I3) and np.array_equal(D3b, D3)
    assert np.array_equal(idx.search_rowset(q, k, s1)[1], I1)
    idx.remove_rows(np.array([5], dtype=np.int64))                # rows renumbered: stale
    for s in (s1, s2, s3):
        with pytest.raises(ValueError, match="another state"):
            idx.search_rowset(q, k, s)
        s.close()
    with pytest.raises(ValueError, match="out of range"):
        idx.rowset(np.array([idx.ntotal], dtype=np.int64))
    idx.close()


def test_drop_in_exclude_filter_runs_as_a_resident_bitmap(native, tmp_path):
    """VectorDatabase.find_most_similar with an exclude-filter over everything: the reference subtracts from an O(N) set and
    gathers ~N rows into a throw-away index per query (vector_database.py:354-386, :508-523); here the excluded rows go
    up once, the search is one full-rate pass under a bitmap, and the next query under the same filter uploads nothing."""
    from minivectordb_amd import VectorDatabase
    from minivectordb_amd import _dbcore
    n, d = 6000, 64
    x = _corpus(n, d)
    db = VectorDatabase(storage_file=str(tmp_path / "excl.pkl"))
    db.store_embeddings_batch(list(range(n)), list(x), [{"tag": "odd" if i % 7 == 3 else "even", "i": i} for i in range(n)])
    made = []
    orig = native.FlatIndex.rowset

    def spy(self, rows, excluded=False):
        made.append((len(rows), excluded))
        return orig(self, rows, excluded)

    native.FlatIndex.rowset = spy
    try:
        ids, dist, meta = db.find_most_similar(x[3], exclude_filter={"tag": "odd"}, k=5)
        ids2, _, _ = db.find_most_similar(x[11], exclude_filter={"tag": "odd"}, k=5)
    finally:
        native.FlatIndex.rowset = orig
    assert made == [(len(range(3, n, 7)), True)]                  # one resident set, built from the EXCLUDED rows, reused
    assert all(m["tag"] == "even" for m in meta) and 3 not in ids and ids2[0] == 11
    kept = np.array([i for i in range(n) if i % 7 != 3])
    Do, Io = flat.flat_search(db.embeddings, x[3:4] / np.linalg.norm(x[3]), 5, rows=kept)
    assert list(ids) == kept[Io[0]].tolist()
    db.store_embedding("new", x[3], {"tag": "even"})              # a write drops the resident sets
    ids3, _, _ = db.find_most_similar(x[3], exclude_filter={"tag": "odd"}, k=2)
    assert "new" in ids3


@pytest.mark.parametrize("disable_rescue", [False, True])
def test_a_call_of_thousands_of_queries_keeps_its_workspace_bounded_and_its_results(native, monkeypatch, disable_rescue):
    """search_core answers a call 1,024 queries at a time and walks the exact re-run passes of refused queries eight per launch
    over ONE list buffer (round-5 advisor: the re-run lists were reserved for every query of the call — 195 KB per query, 4 GB
    at 16k queries next to a 20 GB corpus).  On a clustered corpus (refusals in every chunk) a 2,600-query call returns what
    the same queries return 256 per call, and stands the float64 adjudication."""
    n, d, k, nq = 300_000, 512, 10, 2600
    if disable_rescue:
        monkeypatch.setenv("MVDB_DISABLE_RESCUE", "1")   # every refused query takes an exact pass: 32 per pass, 8 passes per launch
    q = flat.synth(nq, d, 5678 | flat.SYNTH_CLUSTERED)
    flat.normalize_l2(q)
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flat.SYNTH_CLUSTERED, normalize=True)
    before = native.split_rerun_count()
    D, I = idx.search(q, k)
    assert native.split_rerun_count() > before
    parts = [idx.search(q[a:a + 256], k) for a in range(0, nq, 256)]
    Dp, Ip = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert (I == Ip).mean() > 0.98
    np.testing.assert_allclose(np.sort(D, axis=1), np.sort(Dp, axis=1), rtol=0, atol=2e-6)
    stored = idx.get_rows(0, n)
    for i in list(range(0, nq, 41)) + [1023, 1024, 2047, 2048, nq - 1]:
        ok, msg = flat.adjudicate(stored, q[i], k, D[i], I[i], tol=1e-4, tie_eps=2e-6)
        assert ok, (i, msg)
    idx.close()


@pytest.mark.parametrize("d,metric,mixed_norms", [(640, "ip", False), (896, "ip", False), (512, "l2", False), (384, "l2", True), (640, "l2", False)])
def test_rescue_tier_at_the_wide_dimensions_and_for_the_l2_metric(native, monkeypatch, d, metric, mixed_norms):
    """Round 6 closes two holes of the rescue tier (round 5: inner product, d = 256 .. 512 and 768 / 1024 only).  d = 640 / 896 now
    have the gated exact fp32-MFMA pass behind them, so a rescue launch has somewhere to send a full list.  L2: a refused
    query's floor is stated in the units of the nomination keys — q.x >= (|q|^2 + min|x|^2 - r) / 2 for rows of one norm,
    q.x - |x|^2 / 2 >= (|q|^2 - r) / 2 with per-row offsets, r = the k-th exact distance of its nominees — and the queries the
    rescue pass answers skip their exact single-query scan (one `need` word per query).  Clustered corpus: every batch holds
    refused queries; results stand the float64 adjudication, the rescue launches ran, and the exact tier did (almost) nothing."""
    n, k, nq = 300_000, 10, 96
    l2 = metric == "l2"
    q = flat.synth(nq, d, 5678 | flat.SYNTH_CLUSTERED)
    flat.normalize_l2(q)
    idx = native.FlatIndex(d, metric=native.METRIC_L2 if l2 else native.METRIC_IP)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flat.SYNTH_CLUSTERED, normalize=True)
    stored = idx.get_rows(0, n)
    if mixed_norms:   # rows of TWO norms (beyond the norm-range certificate: the offsets form of the L2 pass); the near-duplicates
        #               of a class stay near-duplicates, so certificates are still refused
        scale = np.where(np.arange(n) % 2 == 0, 1.0, 1.002).astype(np.float32)[:, None]   # (|x|^2 spread 4e-3 > 2^-10)
        stored = (stored * scale).astype(np.float32)
        idx.close()
        idx = native.FlatIndex(d, metric=native.METRIC_L2)
        idx.reserve(n)
        idx.add(stored)
    idx.search(q, k)   # shadow, workspaces
    got = {}
    for mode in ("rescue", "exact"):
        if mode == "exact":
            monkeypatch.setenv("MVDB_DISABLE_RESCUE", "1")
            idx.reload_env()
        native.prof_enable(True)
        try:
            for f in ("ip_scan_rescue", "ip_scan_rerun", "ip_scan"):
                native.prof_read(f)
            before = native.split_rerun_count()
            D, I = idx.search(q, k)
            assert native.split_rerun_count() > before, "the clustered corpus must refuse some certificates"
            rescue, rerun, single = native.prof_read("ip_scan_rescue"), native.prof_read("ip_scan_rerun"), native.prof_read("ip_scan")
        finally:
            native.prof_enable(False)
        exact_ms = single[1] if l2 else rerun[1]      # the exact tier: gated single-query scans (L2) / gated fp32-MFMA passes
        if mode == "rescue":
            assert rescue[0] >= 1 and rescue[1] > 0.02, rescue
            t_rescue_mode = exact_ms
        else:
            assert rescue[0] == 0, rescue
            assert exact_ms > 4 * max(t_rescue_mode, 0.01), (exact_ms, t_rescue_mode)   # what the rescue pass saved
        mag = float(max(1.0, np.abs(D).max()))
        for i in range(0, nq, 3):
            ok, msg = flat.adjudicate(stored, q[i], k, D[i], I[i], metric=flat.METRIC_L2 if l2 else flat.METRIC_IP,
                                      tol=1e-4 * mag, tie_eps=4e-6 * mag)
            assert ok, (mode, i, msg)
        got[mode] = (D.copy(), I.copy())
    monkeypatch.delenv("MVDB_DISABLE_RESCUE")
    idx.reload_env()
    assert (got["rescue"][1] == got["exact"][1]).mean() > 0.9
    np.testing.assert_allclose(np.sort(got["rescue"][0], axis=1), np.sort(got["exact"][0], axis=1), rtol=0, atol=4e-6 * mag)
    idx.close()


@pytest.mark.parametrize("n,d,k,nq,masked", [(400_000, 256, 10, 256, False), (300_000, 512, 16, 200, False), (400_000, 384, 10, 130, True),
                                             (1_100_000, 128, 10, 256, False), (250_000, 512, 10, 640, False)])
def test_rescue_launches_skip_tiles_no_refused_query_flagged(native, monkeypatch, n, d, k, nq, masked):
    """Round 6: the certified pass's main launches raise, per query, the bit of every 32-row tile that comes within
    (2.25 eps + 2 margin) |q| of the threshold the scanning wave holds at that moment — a lower bound of the rescue pass's admission
    floor, should the query be refused (launch_half_pass: the derivation).  The rescue launch then walks only the tiles some refused
    query of its batch flagged (+ the seed's tiles) instead of the whole shadow.  Results must be the same BITS as with every tile
    scanned (MVDB_DISABLE_TILE_SKIP=1) — the rescue lists hold every row above the floor either way — and stand the float64
    adjudication; on the clustered corpus some certificates are refused and the launches are handed a fraction of the tiles.
    (The flags are kept from ~400k rows on — MVDB_TILE_FLAG_MIN_TILES=1 brings smaller corpora in — and only while the index has been
    refusing certificates: the first call of a fresh index scans every tile, a corpus that certifies everything never pays.)"""
    monkeypatch.setenv("MVDB_TILE_FLAG_MIN_TILES", "1")
    q = flat.synth(nq, d, 5678 | flat.SYNTH_CLUSTERED)
    flat.normalize_l2(q)
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flat.SYNTH_CLUSTERED, normalize=True)
    stored = idx.get_rows(0, n)
    mask = None
    if masked:
        rng = np.random.RandomState(3)
        keep = rng.rand(n) < 0.6
        mask = native.pack_row_mask(n, rows=np.flatnonzero(keep))
    def run():
        return idx.search_masked(q, k, mask, labels="positions") if masked else idx.search(q, k)
    l0, t0 = native.rescue_tile_stats()
    run()   # shadow, workspaces — and the first refusals this index sees: no flags were kept yet, the launches scan every tile
    l1, t1 = native.rescue_tile_stats()
    assert t1 > t0 and l1 - l0 == t1 - t0, "a fresh index keeps no tile flags before it has refused a certificate"
    got = {}
    for mode in ("skip", "all"):
        if mode == "all":
            monkeypatch.setenv("MVDB_DISABLE_TILE_SKIP", "1")
            idx.reload_env()
        l0, t0 = native.rescue_tile_stats()
        before = native.split_rerun_count()
        D, I = run()
        assert native.split_rerun_count() > before, "the clustered corpus must refuse some certificates"
        l1, t1 = native.rescue_tile_stats()
        assert t1 > t0, "no rescue launch ran"
        if mode == "skip":
            assert (l1 - l0) < 0.9 * (t1 - t0), (l1 - l0, t1 - t0)
            print(f"rescue launches were handed {l1 - l0} of {t1 - t0} tiles")
        else:
            assert l1 - l0 == t1 - t0
        got[mode] = (D.copy(), I.copy())
    monkeypatch.delenv("MVDB_DISABLE_TILE_SKIP")
    idx.reload_env()
    assert got["skip"][0].tobytes() == got["all"][0].tobytes() and got["skip"][1].tobytes() == got["all"][1].tobytes()
    D, I = got["skip"]
    src = stored if not masked else stored[keep]
    for i in range(0, nq, 5):
        ok, msg = flat.adjudicate(src, q[i], k, D[i], I[i], tol=1e-4, tie_eps=4e-6)
        assert ok, (i, msg)
    idx.close()


def test_freeing_an_index_returns_its_device_memory(native, monkeypatch):
    """Every buffer a search workspace holds is freed with its index.  One cycle: a fresh index of 400,000 x 256 normalised rows
    answers 1,024 queries (k = 10) — one whole tile of search_core's queries through the certified pass, tile flags kept
    (MVDB_TILE_FLAGS=1, MVDB_TILE_FLAG_MIN_TILES=1) and the rescue pass set up — and is closed.  The call asks for, among others,
        tflags  1,024 queries x ceil(ceil(400,000 / 32) / 32) = 1,024 x 391 words of 4 bytes          = 1,601,536 bytes
        tlist   ceil(1,024 / 128) = 8 rescue launches x 12,500 tiles x 4 bytes                        =   400,000 bytes
        qfloor  (2 x 1,024 + 128) floats, need (1,024 + 128) / 32 + 8 + 8 words                       — a few KB,
    the four buffers a hand-kept release list once forgot: at least 2.0 MB lost per cycle (the allocator's slack and granularity
    only add to it), 32 MB over 16 cycles.  Bound: the free device memory drops by less than 16 MB — half of that — over 16 cycles.
    The card may be shared, so three rounds are measured and the smallest drop counts: a leak shows in every round, a
    neighbour's allocation only in the round it lands in."""
    import torch
    monkeypatch.setenv("MVDB_TILE_FLAGS", "1")
    monkeypatch.setenv("MVDB_TILE_FLAG_MIN_TILES", "1")
    n, d, nq, k = 400_000, 256, 1024, 10
    q = flat.synth(nq, d, 5678)
    flat.normalize_l2(q)

    def cycle():
        idx = native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234, normalize=True)
        D, I = idx.search(q, k)
        idx.close()
        return I

    I = cycle()   # warm-up: the runtime's one-time allocations, the process-wide re-run counter
    assert (I >= 0).all()
    drops = []
    for _ in range(3):
        before = torch.cuda.mem_get_info(0)[0]
        for _ in range(16):
            cycle()
        drops.append(before - torch.cuda.mem_get_info(0)[0])
    print("free device memory lost over 16 create / search / free cycles, per round:", drops)
    assert min(drops) < 16e6, drops
