"""The library's launch timers (include/mvdb.h, profiling hooks): a bracket of one kernel hands its stop event to the launch,
the four brackets of the single-query int8 route share their boundaries, the events come from a pool, and a captured stream
gets plain launches.

What is checked is the host logic — counts per label, durations that are the kernel's and no longer than the wall time around
the call, pairs that survive `prof_enable(False)`, the two rules that bound unread pairs (off -> on returns them to the pool; a
label holds at most `PROF_LABEL_CAP`), and that a capture records and counts nothing — so the shapes are the smallest that
take each route: 20,000 x 128 for the exact scan, 500,001 x 384 for the int8 route (its smallest eligible size)."""
import time

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

CODE8_LABELS = ("ip_scan_code8_seed", "ip_scan", "ip_scan_code8_rescore", "ip_scan_code8_fallback")


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    _native.prof_enable(False)
    return _native


def _queries(nq, d):
    q = flat.synth(nq, d, 5678)
    flat.normalize_l2(q)
    return q


@pytest.fixture(scope="module")
def small(native):
    """20,000 x 128: single queries take the exact scan."""
    idx = native.FlatIndex(128)
    idx.add_synthetic(20_000, 1234, normalize=True)
    q = _queries(4, 128)
    idx.search(q[0], 10)   # (sizes the workspace)
    yield idx, q
    idx.close()


def _wall_ms(torch, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def test_exact_scan_one_launch_its_own_duration(native, small):
    import torch
    idx, q = small
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        _, wall = _wall_ms(torch, lambda: idx.search(q[0], 10))
        sym = native.prof_symbol("ip_scan")
        first = native.prof_read("ip_scan")
        second = native.prof_read("ip_scan")
    finally:
        native.prof_enable(False)
    print(f"exact scan 20,000 x 128: ip_scan {first}, wall {wall:.4f} ms, symbol {sym}")
    assert first[0] == 1, first
    assert 0.0 < first[1] < wall, (first, wall)
    assert sym.startswith("flat_scan_kernel<"), sym
    assert second == (0, 0.0), second


def test_pairs_stay_readable_after_profiling_is_turned_off(native, small):
    idx, q = small
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        for i in range(3):
            idx.search(q[i], 10)
    finally:
        native.prof_enable(False)
    idx.search(q[3], 10)   # (off: not bracketed)
    launches, ms = native.prof_read("ip_scan")
    assert launches == 3 and ms > 0.0, (launches, ms)
    assert native.prof_read("ip_scan") == (0, 0.0)


def test_int8_route_four_labels_per_call(native):
    import torch
    n, d, k, nq = 500_001, 384, 10, 8
    idx = native.FlatIndex(d)
    try:
        idx.reserve(n)
        idx.add_synthetic(n, 1234, normalize=True)
        q = _queries(nq, d)
        idx.set_option("code8_single_query", 0)
        exact = [idx.search(qi, k) for qi in q]
        idx.set_option("code8_single_query", 1)
        for _ in range(3):   # the exact scan answers the first eligible queries; the third call builds the code
            idx.search(q[0], k)
        assert idx.code8_rows == n
        off = [idx.search(qi, k) for qi in q]
        native.prof_enable(True)
        try:
            for label in CODE8_LABELS:
                native.prof_read(label)
            on, wall = _wall_ms(torch, lambda: [idx.search(qi, k) for qi in q])
            read = {label: native.prof_read(label) for label in CODE8_LABELS}
            sym = native.prof_symbol("ip_scan")
        finally:
            native.prof_enable(False)
    finally:
        idx.close()
    print(f"int8 route 500,001 x 384, 8 calls: {read}, wall {wall:.4f} ms")
    assert sym.startswith("code8_scan_kernel<"), sym
    for label in CODE8_LABELS:
        assert read[label][0] == nq, (label, read)
    total = sum(ms for _, ms in read.values())
    assert 0.0 < total < wall, (read, wall)
    for i in range(nq):
        for other, what in ((off, "profiling off"), (exact, "the exact scan")):
            assert np.array_equal(on[i][0].view(np.uint32), other[i][0].view(np.uint32)), (i, what)
            assert np.array_equal(on[i][1], other[i][1]), (i, what)


def _device_call(torch, idx, q, k):
    qt = torch.from_numpy(q).cuda()
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    return qt, lambda: idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream)


def test_unread_pairs_go_back_to_the_pool_when_profiling_is_turned_on(native, small):
    """Rule 1 of include/mvdb.h.  2,000 bracketed calls (one bracket each: the exact scan) in four on-periods of 500, the label
    never read: each off -> on returns the period before it to the pool, so at most 500 pairs are ever held at one time and the
    pool ends with 2 x 500 events — or with what it held before this test, if earlier tests left more pairs unread at once."""
    import torch
    idx, q = small
    _, call = _device_call(torch, idx, q[0], 10)
    before = native.prof_live_events()
    for _ in range(4):
        native.prof_enable(True)
        try:
            for _ in range(500):
                call()
        finally:
            native.prof_enable(False)
    torch.cuda.synchronize()
    after = native.prof_live_events()
    print(f"pool events before {before}, after 4 x 500 unread brackets {after}")
    assert after <= max(before, 2 * 500), (before, after)
    launches, ms = native.prof_read("ip_scan")   # the last period is still there to be read
    assert launches == 500 and ms > 0.0, (launches, ms)
    assert native.prof_live_events() == after


def test_a_label_holds_no_more_unread_pairs_than_its_cap(native, small):
    """Rule 2: past PROF_LABEL_CAP unread pairs a label's launches run untimed and uncounted, and a read makes room again."""
    import torch
    idx, q = small
    cap = native.PROF_LABEL_CAP
    _, call = _device_call(torch, idx, q[0], 10)
    before = native.prof_live_events()
    native.prof_enable(False)
    native.prof_enable(True)   # (off -> on: nothing of this label is held)
    try:
        for _ in range(cap + 100):
            call()
        torch.cuda.synchronize()
        after = native.prof_live_events()
        full = native.prof_read("ip_scan")
        call()
        one = native.prof_read("ip_scan")
    finally:
        native.prof_enable(False)
    assert full[0] == cap, (full, cap)
    assert one[0] == 1, one
    assert after <= max(before, 2 * cap), (before, after)
    assert native.prof_live_events() == after


def test_a_captured_search_is_not_counted(native, small):
    import torch
    idx, q = small
    k = 10
    want = [idx.search(qi, k) for qi in q[:2]]
    stream = torch.cuda.Stream()
    qt = torch.zeros(128, dtype=torch.float32, device="cuda")
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    qt.copy_(torch.from_numpy(q[0]))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):   # eager calls size this stream's workspace: nothing is allocated inside a capture
        enqueue()
        enqueue()
    stream.synchronize()
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue()
        for j in range(2):
            qt.copy_(torch.from_numpy(q[j]))
            Dt.zero_()
            It.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[j][0][0].view(np.uint32)), j
            assert np.array_equal(It.cpu().numpy(), want[j][1][0]), j
        counted = native.prof_read("ip_scan")
        with torch.cuda.stream(stream):   # the same stream, eager again: counted again
            enqueue()
        stream.synchronize()
        eager = native.prof_read("ip_scan")
    finally:
        native.prof_enable(False)
    del g
    assert counted == (0, 0.0), counted
    assert eager[0] == 1 and eager[1] > 0.0, eager
