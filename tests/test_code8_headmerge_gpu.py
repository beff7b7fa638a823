"""The block lists of the single-query int8 route, merged at the head of the next launch.

code8_seed_kernel ends with one sorted k-list per block and every block of code8_scan_kernel derives the floor from them;
code8_rescore_kernel ends with one list per active block and code8_finish_kernel, the route's last launch, merges the lists
of THIS call — the re-score's, or the gated exact scan's where the call fell back — into (D, I).  A wrong floor shows as a
candidate count that moves with the seed grid, a fallback or a wrong result; a stale or missing list as wrong bits.

Every index has 500,001 - 600,000 rows, the fewest the route serves.  The reference is always the same index with
`code8_single_query` = 0 (the exact scan): D is compared as uint32 bits, I as int64."""
import contextlib
import os

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

N = 500_001
SEED_ROWS = 131072   # slots of the floor's sample: slot i is row (i * n) // SEED_ROWS
FAMILIES = {"zero_mean": 0, "positive": flat.SYNTH_POSITIVE, "clustered": flat.SYNTH_CLUSTERED}
HOOKS = ("MVDB_CODE8_SEED_BLOCKS", "MVDB_CODE8_SEED_THREADS", "MVDB_CODE8_RESCORE_ROWS")


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _queries(nq, d, flag=0):
    q = flat.synth(nq, d, 5678 | flag)
    flat.normalize_l2(q)
    return q


def _index(native, d, n, flag=0):
    """n rows of a family, the code built (the exact scan answers the first eligible queries; the third builds the code)."""
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flag, normalize=True)
    q = _queries(1, d, flag)[0]
    idx.set_option("code8_single_query", 1)
    for _ in range(4):
        idx.search(q, 10)
        if idx.code8_rows == idx.ntotal:
            break
    assert idx.code8_rows == idx.ntotal
    return idx


def _exact(idx, q, k, normalize_q=False):
    idx.set_option("code8_single_query", 0)
    try:
        return idx.search(q, k, normalize_q=normalize_q)
    finally:
        idx.set_option("code8_single_query", 1)


def _same(got, want, what):
    g0, w0 = np.ascontiguousarray(got[0]).reshape(-1), np.ascontiguousarray(want[0]).reshape(-1)
    g1, w1 = np.asarray(got[1]).reshape(-1), np.asarray(want[1]).reshape(-1)
    assert g1.dtype == np.int64 and w1.dtype == np.int64, (what, g1.dtype, w1.dtype)
    assert np.array_equal(g0.view(np.uint32), w0.view(np.uint32)), (what, g0, w0)
    assert np.array_equal(g1, w1), (what, g1, w1)


def _route(idx, q, k, want=None, normalize_q=False, what=""):
    """One call of the route against the exact scan's (D, I).  Returns (D, I, candidates of the call, fallbacks it added)."""
    if want is None:
        want = _exact(idx, q, k, normalize_q)
    fb0, _, calls0 = idx.code8_counters()
    got = idx.search(q, k, normalize_q=normalize_q)
    fb1, count, calls1 = idx.code8_counters()
    assert calls1 - calls0 == 1, (what, calls0, calls1)
    _same(got, want, what)
    return got[0].reshape(-1), got[1].reshape(-1), int(count), fb1 - fb0


@contextlib.contextmanager
def _hooks(idx, **values):
    """The tuning hooks of the route (0 / unset: the defaults), read again by reload_env; put back on the way out."""
    old = {name: os.environ.get(name) for name in HOOKS}
    try:
        for name in HOOKS:
            v = values.get(name[len("MVDB_CODE8_"):].lower(), 0)
            if v:
                os.environ[name] = str(v)
            else:
                os.environ.pop(name, None)
        idx.reload_env()
        yield
    finally:
        for name, v in old.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
        idx.reload_env()


@pytest.fixture(scope="module")
def zero_mean(native):
    idx = _index(native, 512, N)
    yield idx, _queries(6, 512)
    idx.close()


@pytest.fixture(scope="module")
def positive(native):
    idx = _index(native, 512, N, flat.SYNTH_POSITIVE)
    yield idx, _queries(6, 512, flat.SYNTH_POSITIVE)
    idx.close()


@pytest.fixture(scope="module")
def clustered(native):
    idx = _index(native, 512, N, flat.SYNTH_CLUSTERED)
    yield idx, _queries(6, 512, flat.SYNTH_CLUSTERED)
    idx.close()


def _sample_row(slot, n):
    return (slot * n) // SEED_ROWS


# ---- A: the floor, merged by the prefilter's blocks from the seed launch's lists ----------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 64])
def test_a1_floor_from_any_number_of_lists(zero_mean, k):
    """The floor is the k-th best lower bound of the SAMPLE, however the seed's grid split it into lists: with 1, 7 and the
    default number of blocks, of 256 and 1,024 threads, a query has the candidates it has at the default grid."""
    idx, q = zero_mean
    want = [_exact(idx, qi, k) for qi in q[:3]]
    default = []
    for qi, w in zip(q[:3], want):
        _, _, c, fb = _route(idx, qi, k, w, what=f"default grid, k={k}")
        assert fb == 0 and c >= k, (k, c, fb)
        default.append(c)
    for blocks in (1, 7, 0):
        for threads in (256, 1024):
            with _hooks(idx, seed_blocks=blocks, seed_threads=threads):
                for i, (qi, w) in enumerate(zip(q[:3], want)):
                    what = f"seed grid {blocks or 'default'} x {threads}, k={k}, query {i}"
                    _, _, c, fb = _route(idx, qi, k, w, what=what)
                    print(f"{what}: candidates {c} (default grid {default[i]})")
                    assert fb == 0, (what, c, fb)
                    assert c == default[i], (what, c, default[i])


@pytest.mark.parametrize("k", [1, 10, 64])
def test_a2_ties_at_the_floor_across_lists(zero_mean, k):
    """The same row at 2 k sample positions of 2 k different seed blocks (a wave takes batches of 8 slots, a block of 512
    threads 8 batches: slot 64 i opens block i's first batch, i < the grid of one block per CU): 2 k equal lower bounds, told
    apart by their slot alone, in 2 k lists.  The query is that row: it scores highest, the ties are the exact scan's, by row."""
    idx, q = zero_mean
    n = idx.ntotal
    slots = 64 * np.arange(2 * k, dtype=np.int64)
    rows = np.asarray([_sample_row(int(s), n) for s in slots], np.int64)
    assert len(np.unique(rows)) == 2 * k
    old = np.concatenate([idx.get_rows(int(r), 1) for r in rows])
    try:
        idx.set_rows(rows, np.repeat(q[4][None, :], len(rows), axis=0))
        D, I, c, fb = _route(idx, q[4], k, what=f"2k tied rows, k={k}")
        print(f"ties across {2 * k} lists, k={k}: candidates {c}")
        assert fb == 0 and c >= 2 * k, (k, c, fb)
        assert np.array_equal(I, rows[:k]), (I, rows[:k])
        assert len(np.unique(D.view(np.uint32))) == 1, D
    finally:
        idx.set_rows(rows, old)
    _route(idx, q[4], k, what="rows put back")


def test_a3_fewer_than_k_lower_bounds(zero_mean):
    idx, q = zero_mean
    bad = q[0].copy()
    bad[17] = np.inf
    for what, qi in (("zero query", np.zeros(512, np.float32)), ("query with an infinite element", bad)):
        for k in (1, 10):
            _, _, c, fb = _route(idx, qi, k, what=f"{what}, k={k}")
            assert fb == 1, (what, k, c, fb)
    _, _, c, fb = _route(idx, q[0], 10, what="behind the calls that fell back")
    assert fb == 0 and c >= 10, (c, fb)


@pytest.mark.parametrize("family", ["zero_mean", "positive"])
@pytest.mark.parametrize("d", [384, 512, 1024])
def test_a4_all_three_widths(native, d, family):
    flag = FAMILIES[family]
    idx = _index(native, d, N, flag)
    try:
        q = _queries(3, d, flag)
        for normalize_q in (False, True):
            for i, qi in enumerate(q):
                qs = qi * np.float32(3.25) if normalize_q else qi
                what = f"{family} d={d} normalize_q={normalize_q} query {i}"
                _, _, c, fb = _route(idx, qs, 10, normalize_q=normalize_q, what=what)
                assert fb == 0 and c >= 10, (what, c, fb)
    finally:
        idx.close()


# ---- B: (D, I), merged by the last launch from the lists of this call ------------------------------------------------------------------
def _planted_single(idx, q):
    """q itself at one sample position: at k = 1 its lower bound is the floor, and next to nothing else reaches it."""
    row = np.asarray([_sample_row(70001, idx.ntotal)], np.int64)
    old = idx.get_rows(int(row[0]), 1)
    idx.set_rows(row, q[None, :])
    return row, old


@pytest.mark.parametrize("rows_per_block", [0, 16, 64])
def test_b1_active_lists_from_one_to_many(clustered, positive, rows_per_block):
    """A few active blocks (the clustered family at k = 1: the candidates are one cluster, about 120 rows), exactly one (a
    planted copy of the query: at most 16 candidates, one block at every setting), dozens (all-positive queries: hundreds
    of candidates)."""
    cidx, cq = clustered
    pidx, pq = positive
    with _hooks(cidx, rescore_rows=rows_per_block):
        for i, qi in enumerate(cq[:3]):
            _, _, c, fb = _route(cidx, qi, 1, what=f"clustered k=1 query {i}, rows per block {rows_per_block}")
            print(f"clustered k=1 query {i}, rows per block {rows_per_block or 32}: candidates {c}, fallbacks {fb}")
        row, old = _planted_single(pidx, pq[5])
        try:
            D, I, c, fb = _route(pidx, pq[5], 1, what=f"planted copy k=1, rows per block {rows_per_block}")
            print(f"planted copy k=1, rows per block {rows_per_block or 32}: candidates {c}")
            assert fb == 0 and 1 <= c <= 16 and I[0] == row[0], (c, fb, I)
        finally:
            pidx.set_rows(row, old)
        for k in (10, 64):
            for i, qi in enumerate(pq[:3]):
                what = f"positive k={k} query {i}, rows per block {rows_per_block}"
                _, _, c, fb = _route(pidx, qi, k, what=what)
                print(f"{what}: candidates {c}")
                # (the corpus is a narrow cone: hundreds of rows reach the floor — at least 4 active blocks of 64, 16 of 16)
                assert fb == 0 and c >= 4 * 64, (what, c, fb)


def test_b2_no_stale_list_is_merged(positive):
    """One index, one stream: a call with dozens of active blocks, directly behind it the call with the fewest candidates (one
    list), a forced fallback (the exact scan's lists go through the same buffer), the small call again."""
    idx, q = positive
    k = 10
    big = q[0]
    small = q[5]
    want_big = _exact(idx, big, k)
    row, old = _planted_single(idx, small)
    try:
        want_small = _exact(idx, small, 1)
        want_small_k = _exact(idx, small, k)
        for rnd in range(2):
            _, _, cb, fb = _route(idx, big, k, want_big, what=f"round {rnd}: many active blocks")
            assert fb == 0 and cb >= 8 * 32, (cb, fb)
            _, _, cs, fb = _route(idx, small, 1, want_small, what=f"round {rnd}: one list behind many")
            assert fb == 0 and cs <= 16, (cs, fb)
            try:
                idx.set_option("code8_capacity", 1)
                _, _, _, fb = _route(idx, big, k, want_big, what=f"round {rnd}: forced fallback")
                assert fb == 1
            finally:
                idx.set_option("code8_capacity", 32768)
            _, _, cs, fb = _route(idx, small, 1, want_small, what=f"round {rnd}: one list behind the fallback's lists")
            assert fb == 0 and cs <= 16, (cs, fb)
            _, _, _, fb = _route(idx, small, k, want_small_k, what=f"round {rnd}: k=10 behind k=1")
            assert fb == 0
            print(f"round {rnd}: candidates {cb} then {cs}")
    finally:
        idx.set_rows(row, old)


@pytest.mark.parametrize("normalize_q", [False, True])
def test_b3_fallback_through_the_last_launch(zero_mean, normalize_q):
    import torch
    idx, q = zero_mean
    qs = q[1] * np.float32(3.25) if normalize_q else q[1]
    qt = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    try:
        for k in (1, 10, 64):
            want = _exact(idx, qs, k, normalize_q)
            idx.set_option("code8_capacity", 1)
            Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
            It = torch.zeros(k, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            fb0, _, calls0 = idx.code8_counters()
            idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), normalize_q=normalize_q, label_offset=7)
            torch.cuda.synchronize()
            fb1, _, calls1 = idx.code8_counters()
            assert calls1 - calls0 == 1 and fb1 - fb0 == 1, (k, fb0, fb1, calls0, calls1)
            _same((Dt.cpu().numpy(), It.cpu().numpy()), (want[0][0], want[1][0] + 7), f"forced fallback k={k}")
            idx.set_option("code8_capacity", 32768)
    finally:
        idx.set_option("code8_capacity", 32768)


def test_b4_graph_replay(zero_mean):
    import torch
    idx, q = zero_mean
    k = 10
    want = [_exact(idx, qi, k) for qi in q[:5]]
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(q[0]).cuda()
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    with torch.cuda.stream(stream):   # eager calls on this stream size its workspace: nothing is allocated inside a capture
        enqueue()
        enqueue()
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    torch.cuda.synchronize()
    fb0, _, calls0 = idx.code8_counters()
    for i in range(5):
        qt.copy_(torch.from_numpy(q[i]))
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same((Dt.cpu().numpy(), It.cpu().numpy()), (want[i][0][0], want[i][1][0]), f"replay {i}")
    fb1, _, calls1 = idx.code8_counters()
    assert calls1 - calls0 == 5 and fb1 == fb0, (calls0, calls1, fb0, fb1)
    del g
