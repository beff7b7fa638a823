"""The stored copy of the floor's sample and the fused floor launch of the single-query int8 route.

The index keeps the codes and (a, r) of the rows (i * n) // 131072 a second time and code8_seed_kernel streams that copy; the
copy has to follow every write to the code (set_rows, add, a rebuild after a delete).  A stale copy shows as a wrong floor:
more candidates than the planted rows, a fallback, or a wrong result.  The reference is always the same index with
`code8_single_query` = 0: D is compared as bits, I element for element."""
import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

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


def _make(native, n, d, extra=0):
    idx = native.FlatIndex(d)
    idx.reserve(n + extra)
    idx.add_synthetic(n, 1234, normalize=True)
    return idx


def _sample_rows(n, seed, count=64):
    rs = np.random.RandomState(seed)
    rows = np.sort((rs.choice(SEED_ROWS, count, replace=False).astype(np.int64) * n) // SEED_ROWS)
    assert len(np.unique(rows)) == count
    return rows


def _planted(q, count=64):
    """(1 - j 2^-10) q: scores 1 .. 0.938 against ~0.25 for the best synthetic row (test_code8_fused_gpu.test_few_candidates)."""
    return np.stack([np.float32(1.0 - j * 2.0 ** -10) * q for j in range(count)]).astype(np.float32)


def _get(idx, rows):
    return np.concatenate([idx.get_rows(int(r), 1) for r in rows])


def _planted_check(idx, q, seed, what):
    """64 planted rows at sample positions of the index's CURRENT n: at k = 64 exactly they pass."""
    rows = _sample_rows(idx.ntotal, seed)
    idx.set_rows(rows, _planted(q))
    D, I, c, fb = _both(idx, q, 64, what=what)
    print(f"{what}: count {c}")
    assert fb == 0, (what, c, fb)
    assert np.array_equal(I, rows), (what, I, rows)
    assert c == 64, (what, c)


@pytest.fixture(scope="module")
def base(native):
    """500,000 x 512 zero-mean rows (the fewest the route serves: the sample's stride is 3.8 rows), the code built."""
    idx = _make(native, 500_000, 512)
    q = _queries(4, 512)
    _warm(idx, q[0])
    yield idx, q
    idx.close()


def test_copy_follows_set_rows_under_graph_replay(base):
    import torch
    idx, q = base
    n, d, k = idx.ntotal, 512, 64
    rows = _sample_rows(n, 77)
    old = _get(idx, rows)
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(q[2]).cuda()
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    def reference():
        idx.set_option("code8_single_query", 0)
        want = idx.search(q[2], k)
        idx.set_option("code8_single_query", 1)
        return want[0][0], want[1][0]

    def replay(g, what):
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        calls0 = idx.code8_counters()[2]
        g.replay()
        torch.cuda.synchronize()
        fb, count, calls = idx.code8_counters()
        assert calls - calls0 == 1, what
        wd, wi = reference()
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), wd.view(np.uint32)), what
        assert np.array_equal(It.cpu().numpy(), wi), what
        return fb, count

    idx.set_option("code8_single_query", 1)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):   # eager calls size this stream's workspace: nothing is allocated inside a capture
        enqueue()
        enqueue()
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    try:
        fb0, _ = replay(g, "before planting")
        idx.set_rows(rows, _planted(q[2]))
        fb1, count = replay(g, "planted")
        print(f"graph replay over planted sample rows: count {count}")
        assert np.array_equal(It.cpu().numpy(), rows)
        assert count == 64 and fb1 == fb0, (count, fb0, fb1)
        idx.set_rows(rows, old)
        fb2, _ = replay(g, "rows put back")
        assert fb2 == fb0
    finally:
        idx.set_rows(rows, old)
        del g


def test_copy_follows_add(native):
    idx = _make(native, 500_000, 512, extra=200)
    q = _queries(2, 512)
    _warm(idx, q[0])
    idx.add_synthetic(101, 4321, normalize=True)   # n and every sample position change
    assert idx.ntotal == 500_101 and idx.code8_rows == idx.ntotal
    _planted_check(idx, q[1], 78, "after add")
    idx.close()


def test_copy_follows_a_rebuild(native):
    idx = _make(native, 500_001, 512)
    q = _queries(2, 512)
    _warm(idx, q[0])
    idx.remove_rows(np.asarray([5], np.int64))
    assert idx.code8_rows != idx.ntotal
    _warm(idx, q[0])
    assert idx.ntotal == 500_000
    _planted_check(idx, q[1], 79, "after a rebuild")
    idx.close()


@pytest.mark.parametrize("d", [384, 1024])
def test_other_widths(native, d):
    idx = _make(native, 500_001, d)
    q = _queries(4, d)
    _warm(idx, q[0])
    fb0 = idx.code8_counters()[0]
    for k in (1, 10, 64):
        for normalize_q in (False, True):
            for qi in q[:3]:
                qs = qi * np.float32(3.25) if normalize_q else qi
                _both(idx, qs, k, normalize_q, what=f"d={d} k={k} normalize_q={normalize_q}")
    assert idx.code8_counters()[0] == fb0
    _planted_check(idx, q[3], 80 + d, f"planted, d={d}")
    idx.close()


@pytest.mark.parametrize("slot", [0, SEED_ROWS - 1])
def test_non_finite_row_at_a_sample_position(base, slot):
    """r = +inf in the stored copy: a NaN or -inf lower bound that never enters a list.  Slot 131071 is the tail of the last batch."""
    idx, q = base
    n = idx.ntotal
    row = np.asarray([(slot * n) // SEED_ROWS], np.int64)
    old = _get(idx, row)
    try:
        idx.set_rows(row, np.full((1, 512), np.nan, np.float32), normalize=True)
        assert idx.code8_rows == n
        for k in (1, 10, 64):
            D, I, c, fb = _both(idx, q[1], k, what=f"NaN row at slot {slot}, k={k}")
            assert fb == 0 and int(row[0]) not in I, (slot, k, c, fb, I)
    finally:
        idx.set_rows(row, old)
    _both(idx, q[1], 10, what="row put back")


def test_counter_and_tickets_from_call_to_call(base):
    idx, q = base
    try:
        idx.set_option("code8_capacity", 1)
        _, _, _, fb = _both(idx, q[0], 10, what="forced fallback")
        assert fb == 1
        idx.set_option("code8_capacity", 32768)
        _, _, c, fb = _both(idx, q[1], 1, what="k=1 behind a fallback")
        assert fb == 0 and c >= 1, (c, fb)
        _, _, c, fb = _both(idx, q[2], 64, what="k=64")
        assert fb == 0 and c >= 64, (c, fb)
        idx.set_option("code8_capacity", 1)
        _, _, _, fb = _both(idx, q[3], 10, what="forced fallback again")
        assert fb == 1
    finally:
        idx.set_option("code8_capacity", 32768)
    _both(idx, np.zeros(512, np.float32), 10, what="zero query")
    bad = q[0].copy()
    bad[17] = np.inf
    _, _, _, fb = _both(idx, bad, 10, what="query with an infinite element")
    assert fb == 1
    _, _, c, fb = _both(idx, q[0], 10, what="behind the non-finite query")
    assert fb == 0 and c >= 10, (c, fb)


@pytest.mark.parametrize("normalize_q", [False, True])
def test_forced_fallback_merge_with_label_offset(base, normalize_q):
    import torch
    idx, q = base
    qs = q[1] * np.float32(3.25) if normalize_q else q[1]
    qt = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    try:
        for k in (1, 10, 64):
            idx.set_option("code8_single_query", 0)
            want = idx.search(qs, k, normalize_q=normalize_q)
            idx.set_option("code8_single_query", 1)
            idx.set_option("code8_capacity", 1)
            Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
            It = torch.zeros(k, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            fb0, _, calls0 = idx.code8_counters()
            idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), normalize_q=normalize_q, label_offset=7)
            torch.cuda.synchronize()
            fb1, _, calls1 = idx.code8_counters()
            assert calls1 - calls0 == 1 and fb1 - fb0 == 1, (k, fb0, fb1, calls0, calls1)
            assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[0][0].view(np.uint32)), k
            assert np.array_equal(It.cpu().numpy(), want[1][0] + 7), k
    finally:
        idx.set_option("code8_capacity", 32768)
