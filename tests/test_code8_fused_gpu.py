"""The two fused launches of the single-query int8 route: code8_seed_kernel (the floor from the codes,
block lists merged by the last block to arrive) and code8_rescore_kernel (fallback decision, exact scores of the unsorted
candidates keyed by ROW, merge and (D, I) in one launch).  The reference is always the same index with
`code8_single_query` = 0: D is compared as bits, I element for element."""
import os

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

N = 500_001
SEED_ROWS = 131072   # rows of the floor's sample: (i * n) // SEED_ROWS


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _queries(nq, d, seed=5678):
    q = flat.synth(nq, d, seed)
    flat.normalize_l2(q)
    return q


def _warm(idx, q, k=10):
    """The exact scan answers the first eligible queries after a change; the third builds the code."""
    idx.set_option("code8_single_query", 1)
    for _ in range(4):
        idx.search(q, k)
        if idx.code8_rows == idx.ntotal:
            break
    assert idx.code8_rows == idx.ntotal


def _both(idx, q, k, normalize_q=False, what=""):
    """One query with the option off, then on: equal bits; the route answered (its call counter advanced).  Returns
    (D, I, candidates of the call, fallbacks the call added)."""
    idx.set_option("code8_single_query", 0)
    want = idx.search(q, k, normalize_q=normalize_q)
    idx.set_option("code8_single_query", 1)
    fb0, _, calls0 = idx.code8_counters()
    got = idx.search(q, k, normalize_q=normalize_q)
    fb1, count, calls1 = idx.code8_counters()
    assert calls1 - calls0 == 1, (what, calls0, calls1)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    return got[0].reshape(-1), got[1].reshape(-1), count, fb1 - fb0


@pytest.fixture(scope="module")
def base(native):
    """500,001 x 512 zero-mean rows, the code built; x: the stored rows on the host (tests that plant rows put them back)."""
    d = 512
    idx = native.FlatIndex(d)
    idx.reserve(N)
    idx.add_synthetic(N, 1234, normalize=True)
    q = _queries(4, d)
    _warm(idx, q[0])
    x = idx.get_rows(0, N)
    yield idx, x, q
    idx.close()


def test_capacity_edges_taken_from_the_device(base):
    idx, _, q = base
    k = 10
    try:
        _, _, c, fb = _both(idx, q[1], k, what="default capacity")
        assert fb == 0 and k <= c <= 32768, (c, fb)
        idx.set_option("code8_capacity", c)
        _, _, c2, fb = _both(idx, q[1], k, what="capacity = count")
        assert c2 == c and fb == 0, (c, c2, fb)
        idx.set_option("code8_capacity", c - 1)
        _, _, c3, fb = _both(idx, q[1], k, what="capacity = count - 1")
        assert c3 == c and fb == 1, (c, c3, fb)
    finally:
        idx.set_option("code8_capacity", 32768)
    _, _, _, fb = _both(idx, q[1], k, what="capacity restored")
    assert fb == 0


@pytest.mark.parametrize("k", [10, 64])
def test_ties_across_blocks_from_unsorted_candidates(base, k):
    idx, x, q = base
    rs = np.random.RandomState(31 + k)
    where = np.sort(rs.choice(N, 300, replace=False)).astype(np.int64)
    try:
        # 300 exact copies of the best row there can be (the query itself), scattered over the whole index
        idx.set_rows(where, np.repeat(q[0][None, :], 300, axis=0))
        D, I, c, fb = _both(idx, q[0], k, what=f"300 copies of the best row, k={k}")
        assert fb == 0 and c >= 300, (c, fb)
        assert np.array_equal(I, where[:k]), (I, where[:k])
        assert np.all(D.view(np.uint32) == D.view(np.uint32)[0])
        idx.set_rows(where, x[where])
        # 300 copies of the row that holds the k-th place: places 1 .. k-1 stay, the k-th goes to the lowest row of the tie
        D0, I0, _, _ = _both(idx, q[0], k, what=f"no copies, k={k}")
        kth = int(I0[k - 1])
        spots = where[~np.isin(where, I0)]   # (a spot that holds one of the k results stays as it is)
        idx.set_rows(spots, np.repeat(x[kth][None, :], len(spots), axis=0))
        D, I, c, fb = _both(idx, q[0], k, what=f"copies of the k-th row, k={k}")
        assert fb == 0, (c, fb)
        assert np.array_equal(I[:k - 1], I0[:k - 1]) and I[k - 1] == min(kth, int(spots[0])), (I, I0, spots[:3])
        assert np.array_equal(D.view(np.uint32), D0.view(np.uint32))
    finally:
        idx.set_rows(where, x[where])


@pytest.mark.parametrize("k", [64, 1])
def test_few_candidates(base, k):
    """64 planted rows (1 - j 2^-10) q, all of them rows of the floor's sample: they score 1 .. 0.938 against ~0.25 for the
    best synthetic row and a margin of ~0.01, so at k = 64 the floor sits just under the worst of them and exactly the 64
    pass (count == k, the least the route serves without a fallback); at k = 1 the floor sits one margin under the best, and
    between 1 and 64 of them pass."""
    idx, x, q = base
    rs = np.random.RandomState(77)
    rows = np.sort((rs.choice(SEED_ROWS, 64, replace=False).astype(np.int64) * N) // SEED_ROWS)
    assert len(np.unique(rows)) == 64
    planted = np.stack([np.float32(1.0 - j * 2.0 ** -10) * q[2] for j in range(64)]).astype(np.float32)
    try:
        idx.set_rows(rows, planted)
        D, I, c, fb = _both(idx, q[2], k, what=f"64 planted rows, k={k}")
        print(f"few candidates k={k}: count {c}")
        assert fb == 0, (c, fb)
        assert np.array_equal(I, rows[:k])
        if k == 64:
            assert c == 64, c
        else:
            assert 1 <= c <= 64, c
    finally:
        idx.set_rows(rows, x[rows])


@pytest.mark.parametrize("rows_per_block", [0, 2])
def test_thousands_of_candidates_run_the_many_block_merge(base, rows_per_block):
    """3,000 exact copies of the query tie at the top, so every one of them is a candidate: at least 3,000 per call.  With the
    default 32 candidates per block that is 94+ active blocks, whose 6,000+ keys at k = 64 take the long steps of the last
    block's merge; with 2 per block (tuning hook) the 1,024-block grid is short of the count, so the active blocks are
    clamped to the grid and every wave walks several batches."""
    idx, x, q = base
    rs = np.random.RandomState(4242)
    where = np.sort(rs.choice(N, 3000, replace=False)).astype(np.int64)
    old = os.environ.get("MVDB_CODE8_RESCORE_ROWS")
    try:
        if rows_per_block:
            os.environ["MVDB_CODE8_RESCORE_ROWS"] = str(rows_per_block)
            idx.reload_env()
        idx.set_rows(where, np.repeat(q[3][None, :], len(where), axis=0))
        for k in (10, 64):
            D, I, c, fb = _both(idx, q[3], k, what=f"3,000 copies, k={k}, rows per block {rows_per_block}")
            assert fb == 0 and 3000 <= c <= 32768, (c, fb)
            assert np.array_equal(I, where[:k]), (I, where[:k])
    finally:
        if old is None:
            os.environ.pop("MVDB_CODE8_RESCORE_ROWS", None)
        else:
            os.environ["MVDB_CODE8_RESCORE_ROWS"] = old
        idx.reload_env()
        idx.set_rows(where, x[where])


def test_large_count_many_queries_back_to_back(native):
    n, d, k = 500_000, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flat.SYNTH_POSITIVE, normalize=True)
    q = flat.synth(16, d, 5678 | flat.SYNTH_POSITIVE)
    flat.normalize_l2(q)
    _warm(idx, q[0])
    idx.set_option("code8_capacity", 65536)
    idx.set_option("code8_single_query", 0)
    want = [idx.search(qi, k) for qi in q]
    idx.set_option("code8_single_query", 1)
    fb0, _, calls0 = idx.code8_counters()
    got, counts = [], []
    # back to back on one index: a list left by the call before must not reach this one's merge (a few hundred candidates
    # per call here; the merge of thousands is test_thousands_of_candidates_run_the_many_block_merge's)
    for qi in q:
        got.append(idx.search(qi, k))
        counts.append(idx.code8_counters()[1])
    fb1, _, calls1 = idx.code8_counters()
    print(f"positive 500k x 512, capacity 65536: candidates {counts}, fallbacks {fb1 - fb0} of {calls1 - calls0}")
    assert calls1 - calls0 == len(q) and min(counts) >= k
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0].view(np.uint32), w[0].view(np.uint32)), (i, g[0], w[0])
        assert np.array_equal(g[1], w[1]), (i, g[1], w[1])
    idx.close()


@pytest.mark.parametrize("d", [384, 1024])
def test_other_shapes(native, d):
    idx = native.FlatIndex(d)
    idx.reserve(N)
    idx.add_synthetic(N, 1234, normalize=True)
    q = _queries(3, d)
    _warm(idx, q[0])
    fb0 = idx.code8_counters()[0]
    for k in (1, 10, 64):
        for normalize_q in (False, True):
            for qi in q:
                qs = qi * np.float32(3.25) if normalize_q else qi
                _both(idx, qs, k, normalize_q, what=f"d={d} k={k} normalize_q={normalize_q}")
    assert idx.code8_counters()[0] == fb0
    idx.close()


def test_non_finite_rows(native):
    n, d, k = 500_007, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = _queries(2, d)
    _warm(idx, q[0])
    # a NaN row through the device normalisation (the norm bound stays known): residual bound +inf, a candidate of every
    # query, a NaN lower bound or -inf in the seed launch, never a result
    idx.set_rows(np.asarray([n - 3], np.int64), np.full((1, d), np.nan, np.float32), normalize=True)
    _warm(idx, q[0])
    for kk in (1, k, 64):
        D, I, c, fb = _both(idx, q[0], kk, what=f"NaN row, k={kk}")
        assert fb == 0 and (n - 3) not in I, (c, fb, I)
    # a row that scores +inf: 1e10 q against the query 1e29 q (raw: the measured norm bound becomes 1e10, the margin of every
    # row with it — the call may fall back; either way the result is the reference's, +inf first)
    idx.set_rows(np.asarray([12345], np.int64), (np.float32(1e10) * q[1])[None, :])
    _warm(idx, q[0])
    big = (np.float32(1e29) * q[1]).astype(np.float32)
    for kk in (1, k):
        D, I, c, fb = _both(idx, big, kk, what=f"+inf-scoring row, k={kk}")
        assert I[0] == 12345 and np.isposinf(D[0]), (D, I)
        assert (n - 3) not in I
    idx.close()


def test_graph_capture_and_replays(base):
    import torch
    idx, _, q = base
    d, k = 512, 10
    idx.set_option("code8_single_query", 0)
    want = [idx.search(qi, k, normalize_q=True) for qi in q]
    idx.set_option("code8_single_query", 1)
    stream = torch.cuda.Stream()
    qt = torch.zeros(d, dtype=torch.float32, device="cuda")
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream, normalize_q=True, label_offset=7)

    qt.copy_(torch.from_numpy(q[0]))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):   # eager calls size this stream's workspace: nothing is allocated inside a capture
        enqueue()
        enqueue()
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    calls0 = idx.code8_counters()[2]
    for i in range(5):
        j = i % len(q)
        qt.copy_(torch.from_numpy(q[j]))
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[j][0][0].view(np.uint32)), i
        assert np.array_equal(It.cpu().numpy(), want[j][1][0] + 7), i
    assert idx.code8_counters()[2] - calls0 == 5
    del g
