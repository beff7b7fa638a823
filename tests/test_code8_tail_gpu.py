"""The int8 prefilter's batch loop at the end of the index and at its batch-to-wave assignment.

`code8_scan_kernel` runs full batches of rows in a loop without a row test and the one partial batch behind them apart; a
re-scheduled loop can lose or repeat exactly those rows.  The route only serves n >= 500,000, so the sizes are the smallest
that run the kernel at all and are no multiple of any rows-per-batch it may use (2 … 16).  Rows that must come out on top
are planted where a wrong tail or a wrong assignment loses them: the last 9 rows, row 0 and the first row of the last
64-row block hold (1 - j 2^-10) q for distinct j (scores 1 - j / 1024 against ~0.25 for the best synthetic row).  The
reference is the same index with the option off: D as bits and I must be equal."""
import numpy as np
import pytest

from oracle import flat

DIMS = (384, 512, 1024)
SIZES = (500_001, 500_007, 500_033)


def _planted(n):
    """Planted rows in planted-score order (best first); at n = 500,033 the last block starts at the last row: 10 rows."""
    rows = list(range(n - 1, n - 10, -1)) + [0, ((n - 1) // 64) * 64]
    return list(dict.fromkeys(rows))


def _query(d):
    q = flat.synth(1, d, 5678)
    flat.normalize_l2(q)
    return q[0]


def _plant(q, rows):
    return np.stack([np.float32(1.0 - j * 2.0 ** -10) * q for j in range(len(rows))]).astype(np.float32)


@pytest.mark.parametrize("d", DIMS)
def test_planted_rows_top_the_exact_scan_on_the_cpu(d):
    """The premise of the GPU cases, on the oracle at n = 5,000: the fp32 scan alone ranks the planted rows first."""
    n = 5_000
    x = flat.synth(n, d, 1234)
    flat.normalize_l2(x)
    q = _query(d)
    rows = _planted(n)
    x[rows] = _plant(q, rows)
    D, I = flat.flat_search(x, q[None, :], len(rows))
    assert I[0].tolist() == rows, (I[0], rows)
    assert D[0][-1] > 0.98 and np.all(np.diff(D[0]) < 0)


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


@pytest.fixture(scope="module")
def planted_index(native):
    """One planted index at a time, shared by the k cases of a (d, n)."""
    held = {}

    def get(d, n):
        if held.get("key") != (d, n):
            if "idx" in held:
                held.pop("idx").close()
            idx = native.FlatIndex(d)
            idx.reserve(n)
            idx.add_synthetic(n, 1234, normalize=True)
            rows = _planted(n)
            q = _query(d)
            idx.set_rows(np.asarray(rows, dtype=np.int64), _plant(q, rows))
            held.update(key=(d, n), idx=idx, rows=rows, q=q)
        return held["idx"], held["rows"], held["q"]

    yield get
    if "idx" in held:
        held.pop("idx").close()


def _off_then_on(native, idx, q, k, what):
    idx.set_option("code8_single_query", 0)
    want = idx.search(q, k)
    idx.set_option("code8_single_query", 1)
    for _ in range(3):   # the exact scan answers the first eligible queries after a change; the third builds the code
        idx.search(q, k)
    fallbacks = idx.code8_counters()[0]
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        got = idx.search(q, k)
        sym = native.prof_symbol("ip_scan")
        launches = native.prof_read("ip_scan")[0]
    finally:
        native.prof_enable(False)
    assert sym.startswith("code8_scan_kernel<"), (what, sym)
    assert launches == 1, (what, launches)
    assert idx.code8_rows == idx.ntotal, what
    assert idx.code8_counters()[0] == fallbacks, (what, idx.code8_counters())
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", DIMS)
def test_planted_tail_rows(native, planted_index, d, n, k):
    idx, rows, q = planted_index(d, n)
    D, I = _off_then_on(native, idx, q, k, f"d={d} n={n} k={k}")
    if k <= 11:
        m = min(k, len(rows))
        assert I.reshape(-1)[:m].tolist() == rows[:m], (d, n, k, I, rows)
    else:
        assert I.reshape(-1)[:len(rows)].tolist() == rows, (d, n, k, I, rows)


@pytest.mark.gpu
def test_planted_tail_rows_with_a_nan_last_row(native):
    n, d, k = 500_007, 512, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    rows = _planted(n)
    q = _query(d)
    x = _plant(q, rows)
    assert rows[0] == n - 1
    idx.set_rows(np.asarray(rows[1:], dtype=np.int64), x[1:])
    # the NaN row goes in through the device normalisation: the index' norm bound stays known, so the route keeps serving
    # and the row (residual bound +inf) is a candidate of every query
    idx.set_rows(np.asarray(rows[:1], dtype=np.int64), np.full((1, d), np.nan, np.float32), normalize=True)
    D, I = _off_then_on(native, idx, q, k, "NaN last row")
    assert I.reshape(-1).tolist() == rows[1:k + 1], (I, rows)   # the NaN row never enters; the next ten planted rows do
    idx.close()
