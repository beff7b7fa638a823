"""The exact scans' launch table on the device: which kernel instantiation every (width, row selection, call kind) launches.

Scores do not depend on the rows a wave keeps in flight (U), and the range and grouped suites compare the library with its own
top-k path: a wrong U, or the streaming U for gathered rows, costs bandwidth and fails none of them.  This file pins the table.
For one width per (G, C) shape in its full form and one in its lane-masked form where one exists, both metrics, it runs a
single-query search, a search under an unsorted row list and under a bitmap-form set, a range search under no set / a list / a
bitmap and a grouped search of eight queries under list sets — and, inner product at the widths of the fp16 shadow, a 40-query
range search on the shared pass — with profiling on, and asserts

  1. the results: top-k lists against the float64 oracle (oracle.flat.adjudicate, tol = 1e-4 mag, tie_eps = 4e-6 mag), range
     results through the bit-identity check of tests/test_range_gpu.py;
  2. the symbol recorded under the launch's label (ip_scan, ip_scan_range, ip_scan_range_rescore, grouped_scan) against
     tests/golden/launch_symbols.json.

The fixture is written by `record()` below (PYTHONPATH=. python tests/test_launch_table_gpu.py) and was recorded ONCE, against a build of the
commit BEFORE the launchers were rewritten around one shape table: it states what the hand-written tables launched.  Re-record it
only with a change that means to launch other kernels, from a build without that change's launch code.

2,051 rows: no multiple of any block step, several blocks at every shape.  60,000 rows at d = 64: the grid's bound of CUs x
resident blocks is the active one."""
import json
import os
import sys

import numpy as np
import pytest

import test_range_gpu as range_suite
from oracle import flat

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_symbols.json")

# (d, the (G, C) shape, lane-masked): choose_shape of mvdb.hip, restated for the reader — the fixture is what is asserted
WIDTHS = [64, 30,        # 16 x 1
          128, 100,      # 32 x 1
          256, 200,      # 64 x 1
          384,           # 32 x 3 (full only)
          512, 500,      # 64 x 2
          768, 640,      # 64 x 3
          1024, 896,     # 64 x 4
          1280, 1100,    # 64 x 5
          1536,          # 64 x 6
          1792,          # 64 x 7
          2048,          # 64 x 8
          4096, 2304]    # 64 x 16
SHADOW_WIDTHS = [128, 256, 384, 512, 640, 768, 896, 1024]
N = 2_051
CASES = [(d, N) for d in WIDTHS] + [(64, 60_000)]
METRICS = {"ip": flat.METRIC_IP, "l2": flat.METRIC_L2}
K = 10
NQ_RANGE = 3
NQ_GROUPED = 8
NQ_SHARED = 40

_DATA = {}


def data(d, n):
    """Unit rows and raw Gaussian queries, computed once per shape and shared (read-only) by both metrics."""
    if (d, n) not in _DATA:
        rng = np.random.default_rng(7000 + d + n)
        x = rng.standard_normal((n, d)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q = rng.standard_normal((NQ_SHARED, d)).astype(np.float32)
        q[:4] += 3.0 * x[[5, n // 2, n - 1, 17]]          # queries with near neighbours
        unsorted = rng.permutation(rng.choice(n, n * 13 // 15, replace=False)).astype(np.int64)   # 87 % of the rows: a list
        excluded = np.sort(rng.choice(n, 100, replace=False)).astype(np.int64)                     # ... a bitmap
        lists = [rng.permutation(rng.choice(n, m, replace=False)).astype(np.int64)
                 for m in (1, K - 1, K, 300, 700, n // 2, 1_000, 77)]
        for a in (x, q, unsorted, excluded, *lists):
            a.setflags(write=False)
        _DATA[(d, n)] = (x, q, unsorted, excluded, lists)
    return _DATA[(d, n)]


def adjudicated(x, q1, D, I, metric, rows, what):
    """One top-k list against the float64 oracle; rows: the list the labels are row numbers of (None: every row)."""
    mag = float(max(1.0, np.abs(D[I >= 0]).max())) if (I >= 0).any() else 1.0
    k = len(D)
    if rows is not None:
        at = {int(r): p for p, r in enumerate(rows)}
        I = np.array([at[int(r)] if r >= 0 else -1 for r in I], np.int64)
    ok, msg = flat.adjudicate(x, q1, k, D, I, metric=metric, rows=rows, tol=1e-4 * mag, tie_eps=4e-6 * mag)
    assert ok, f"{what}: {msg}"


def launched(native, label, call):
    """call() with the label's launch counter drained before: (its result, the symbol its launch recorded)."""
    native.prof_read(label)
    out = call()
    assert native.prof_read(label)[0] >= 1, f"nothing was launched under {label}"
    return out, native.prof_symbol(label)


def run_cases(native, d, n, metric):
    """Every case of one (width, rows, metric): results asserted, {case: symbol} returned."""
    x, q, unsorted, excluded, lists = data(d, n)
    ip = metric == flat.METRIC_IP
    symbols = {}
    idx = native.FlatIndex(d, metric=metric)
    idx.add(x)
    native.prof_enable(True)
    try:
        list_set, bitmap_set = idx.rowset(unsorted), idx.rowset(excluded, excluded=True)
        assert not list_set.is_bitmap and bitmap_set.is_bitmap
        kept = np.setdiff1d(np.arange(n, dtype=np.int64), excluded)
        sets = [("none", None, None, np.arange(n, dtype=np.int64)), ("list", list_set, unsorted, unsorted), ("bitmap", bitmap_set, kept, kept)]
        what = f"d={d} n={n} metric={metric}"
        # top-k of a single query: every row, the row list, the bitmap
        for name, rs, rows, _ in sets:
            call = (lambda: idx.search(q[:1], K)) if rs is None else (lambda: idx.search_rowset(q[:1], K, rs))
            (D, I), symbols[f"search/{name}"] = launched(native, "ip_scan", call)
            adjudicated(x, q[0], D[0], I[0], metric, rows, f"{what} search/{name}")
        # range: each query's 20th best score of the set as its threshold
        for name, rs, _, tie_order in sets:
            thr = np.array([range_suite.reference(idx, q[i], rs, 64, metric, False)[0][19] for i in range(NQ_RANGE)], np.float32)
            (lims, D, I), symbols[f"range/{name}"] = launched(native, "ip_scan_range", lambda: idx.range_search(q[:NQ_RANGE], thr, rowset=rs))
            for i in range(NQ_RANGE):
                assert lims[i + 1] - lims[i] >= 20, (what, name, i)
                range_suite.check_query(idx, x, q[i], rs, tie_order, thr[i], D[lims[i]:lims[i + 1]], I[lims[i]:lims[i + 1]], metric, False,
                                        f"{what} range/{name} query {i}")
        # grouped: eight queries, each under a list of its own
        group = [idx.rowset(rows) for rows in lists]
        assert not any(rs.is_bitmap for rs in group)
        (D, I), symbols["grouped/list"] = launched(native, "grouped_scan", lambda: idx.search_grouped(q[:NQ_GROUPED], K, group))
        for i in range(NQ_GROUPED):
            adjudicated(x, q[i], D[i], I[i], metric, lists[i], f"{what} grouped query {i}")
        # the shared pass of a range batch: nomination over the fp16 shadow, exact re-score of the candidates
        if ip and n == N and d in SHADOW_WIDTHS:
            idx.set_option("range_shared", 2)
            thr = np.array([range_suite.reference(idx, q[i], None, 64, metric, False)[0][19] for i in range(NQ_SHARED)], np.float32)
            before = idx.range_counters()[0]
            (lims, D, I), symbols["range_shared/none"] = launched(native, "ip_scan_range_rescore", lambda: idx.range_search(q, thr))
            assert idx.range_counters()[0] == before + 1
            for i in range(NQ_SHARED):
                range_suite.check_query(idx, x, q[i], None, sets[0][3], thr[i], D[lims[i]:lims[i + 1]], I[lims[i]:lims[i + 1]], metric, False,
                                        f"{what} range_shared query {i}")
        for rs in [list_set, bitmap_set] + group:
            rs.close()
    finally:
        native.prof_enable(False)
        idx.close()
    return symbols


def case_id(d, n, metric_name):
    return f"d{d}-n{n}-{metric_name}"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("metric_name", list(METRICS))
@pytest.mark.parametrize("d,n", CASES)
def test_results_and_launched_kernels(gpu, golden, d, n, metric_name):
    from minivectordb_amd import _native
    want = golden[case_id(d, n, metric_name)]
    got = run_cases(_native, d, n, METRICS[metric_name])
    assert got == want, {c: (got.get(c), want.get(c)) for c in sorted(set(got) | set(want)) if got.get(c) != want.get(c)}


def test_fixture_covers_the_table(golden):
    """Every (G, C) of the table, its three rows-in-flight policies and the re-score are in the fixture (read by eye against the
    hand-written tables when it was recorded; these four are the ones named there)."""
    assert len(golden) == 2 * len(CASES)
    assert golden["d512-n2051-ip"]["search/none"] == "flat_scan_kernel<64, 2, 2, 0, 0, true, 0, false, false>"
    assert golden["d512-n2051-ip"]["search/list"] == "flat_scan_kernel<64, 2, 4, 0, 0, true, 1, false, false>"
    assert golden["d640-n2051-ip"]["grouped/list"] == "grouped_scan_kernel<64, 3, 4, 0, true>"
    assert golden["d1024-n2051-ip"]["range_shared/none"] == "range_rescore_kernel<64, 4, 2, false>"
    assert sum("range_shared/none" in v for v in golden.values()) == len(SHADOW_WIDTHS)


def record(path=GOLDEN):
    """Write the fixture from the library that is loaded (see the module docstring for which build that must be)."""
    from minivectordb_amd import _native
    out = {}
    for d, n in CASES:
        for metric_name, metric in METRICS.items():
            out[case_id(d, n, metric_name)] = run_cases(_native, d, n, metric)
            print(case_id(d, n, metric_name), out[case_id(d, n, metric_name)], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record(*sys.argv[1:2])
