"""mvdb_index_search_grouped on the device: every query under its own resident row set, one gathered launch.

The core claim is BIT IDENTITY: row i of search_grouped equals — D.view(uint32) and I element for element — what a loop of
search_rowset(q[i:i+1], k, sets[i]) / search(q[i:i+1], k) returns on the same index, for every (G, C) shape choose_shape
returns, both metrics, with and without the fused query normalisation, and for data holding NaN, +-inf, -0.0 and exact
duplicate rows.  The independent oracle (oracle.flat) is compared through tests/bigcheck.compare with its own tolerances.
Indexes are shared across the cases of one width to keep the file's wall time down."""
import threading
import time

import numpy as np
import pytest

import bigcheck
from oracle import flat

pytestmark = pytest.mark.gpu

DIMS = [16, 30, 64, 100, 256, 384, 512, 640, 1024, 1280, 1536, 1792, 2048, 2304]
NQ = 96


def rows_of(d):
    return 50_000 if d < 1280 else 20_000


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


def make_sets(idx, n, k, seed):
    """[(name, RowSet | None, rows the set selects in tie order | None)] — the cases of the issue."""
    rng = np.random.default_rng(seed)
    tail = np.arange(n - 5, n)

    def pick(m, special=False):
        rows = rng.choice(n, m, replace=False)
        if special:
            rows = np.union1d(np.union1d(rows, SPECIAL_ROWS), tail)
        return np.sort(rows).astype(np.int64)

    big = min(30_000, 3 * n // 5)
    unsorted = rng.permutation(pick(2_000, special=True))
    repeated = pick(500)
    repeated = np.concatenate([repeated, repeated[17:18], repeated[:3]])
    dense = np.setdiff1d(np.arange(n), rng.choice(n, n // 20, replace=False)).astype(np.int64)   # 95 % of the rows, sorted
    excluded = pick(100)
    cases = [
        ("empty", np.empty(0, np.int64)),
        ("one row", pick(1)),
        ("k - 1 rows", pick(k - 1)),
        ("k rows", pick(k)),
        ("300 rows", pick(300, special=True)),
        ("5,000 rows", pick(5_000, special=True)),
        (f"{big} rows", pick(big, special=True)),
        ("unsorted", unsorted),
        ("repeated row", repeated),
    ]
    out = [(name, idx.rowset(rows), rows) for name, rows in cases]
    assert not any(rs.is_bitmap for _, rs, _ in out)
    out.append(("NULL", None, None))
    rs = idx.rowset(excluded, excluded=True)
    assert rs.is_bitmap
    out.append(("excluded bitmap", rs, np.setdiff1d(np.arange(n), excluded)))
    rs = idx.rowset(dense)
    assert rs.is_bitmap, "a sorted list of >= 90 % of the rows is stored as a bitmap"
    out.append(("dense bitmap", rs, dense))
    return out


def loop_of_single_calls(idx, q, k, sets, normalize_q):
    D = np.empty((q.shape[0], k), np.float32)
    I = np.empty((q.shape[0], k), np.int64)
    for i, rs in enumerate(sets):
        if rs is None:
            D[i:i + 1], I[i:i + 1] = idx.search(q[i:i + 1], k, normalize_q=normalize_q)
        else:
            D[i:i + 1], I[i:i + 1] = idx.search_rowset(q[i:i + 1], k, rs, normalize_q=normalize_q)
    return D, I


def assert_bit_identical(got, want, what):
    (D, I), (Dw, Iw) = got, want
    same_i = I == Iw
    same_d = D.view(np.uint32) == Dw.view(np.uint32)
    if not (same_i.all() and same_d.all()):
        bad = np.argwhere(~(same_i & same_d))
        i, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} elements differ; first at query {i} slot {j}: grouped "
                             f"({D[i, j]!r}, {I[i, j]}) loop ({Dw[i, j]!r}, {Iw[i, j]})")


@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2], ids=["ip", "l2"])
@pytest.mark.parametrize("d", DIMS)
def test_grouped_is_bit_identical_to_the_loop_of_single_calls(gpu, d, metric):
    from minivectordb_amd import _native
    n = rows_of(d)
    x = gaussian(n, d, 1000 + d)
    q = gaussian(NQ, d, 2000 + d)
    spike(x, q)
    idx = _native.FlatIndex(d, metric=metric)
    idx.add(x)
    try:
        for k in (1, 10, 64):
            cases = make_sets(idx, n, k, 3000 + d + k)
            sets = [cases[i % len(cases)][1] for i in range(NQ)]   # every set is named by eight queries
            for normalize_q in (False, True):
                want = loop_of_single_calls(idx, q, k, sets, normalize_q)
                got = idx.search_grouped(q, k, sets, normalize_q=normalize_q)
                assert_bit_identical(got, want, f"d={d} metric={metric} k={k} normalize_q={normalize_q}")
                # what the cases are there for: padding, ties lowest position first
                D, I = got
                for i in range(NQ):
                    name, _, rows = cases[i % len(cases)]
                    m = n if rows is None else len(rows)
                    if i not in (3, 4):   # (a NaN / inf query scores NaN against most rows: fewer results, same as the loop)
                        assert (I[i] >= 0).sum() <= min(k, m), (name, i)
                    if m == 0:
                        assert (I[i] == -1).all()
            for _, rs, _ in cases:
                if rs is not None:
                    rs.close()
    finally:
        idx.close()


def test_ties_come_back_lowest_position_first(gpu):
    from minivectordb_amd import _native
    d, n = 512, 4096
    x = np.tile(gaussian(1, d, 5), (n, 1))
    idx = _native.FlatIndex(d)
    idx.add(x)
    rows = np.array([900, 17, 3000, 17, 5, 2222], np.int64)
    rs = idx.rowset(rows)
    D, I = idx.search_grouped(np.tile(x[:1], (3, 1)), 4, [rs, None, rs])
    assert I[0].tolist() == [900, 17, 3000, 17] and I[2].tolist() == I[0].tolist()
    assert I[1].tolist() == [0, 1, 2, 3]
    idx.close()


def oracle_single(x, q, k, rows, metric):
    """oracle.flat for ONE query under a row list (labels: row numbers) or over every row."""
    if rows is None:
        return flat.flat_search(x, q, k, metric=metric)
    if len(rows) == 0:
        return (np.full((1, k), -3.4028234663852886e38 if metric == flat.METRIC_IP else 3.4028234663852886e38, np.float32),
                np.full((1, k), -1, np.int64))
    D, P = flat.flat_search(x, q, k, metric=metric, rows=np.ascontiguousarray(rows))
    return D, np.where(P >= 0, rows[np.maximum(P, 0)], -1)


@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2], ids=["ip", "l2"])
@pytest.mark.parametrize("d", [100, 512])
def test_grouped_against_the_independent_oracle(gpu, d, metric):
    """The same sets against oracle.flat, adjudicated by bigcheck.compare (TOL, TIE_EPS); k = 100 takes the large-k route
    (scores + radix select per query) and is held to both comparisons too.  Rows and queries are scaled to unit length, as
    the database classes store them: bigcheck's TOL is an ABSOLUTE 1e-4, calibrated for scores of order 1 — the squared
    distance of two raw Gaussian vectors at d = 512 is ~1000, where ONE fp32 ulp is already 6e-5.
    Of the special values of the bit-identity test, the exact duplicate rows (sixteen copies of one row, three queries equal
    to it: ties, lowest position first — asserted against the list order as well as through the oracle), the all -0.0 row
    and the -0.0 query elements go through the oracle here.  NaN and +-inf cannot: `compare` takes |D - Do| (inf - inf and
    NaN fail its bound by construction) and the oracle's C sort has no defined order for NaN scores; those stay covered by
    the comparison with the single-query kernel, whose own handling of them the existing suite holds against the oracle's
    conventions."""
    from minivectordb_amd import _native
    n = 50_000
    x = gaussian(n, d, 4000 + d)
    q = gaussian(NQ, d, 5000 + d)
    flat.normalize_l2(x)
    flat.normalize_l2(q)
    x[10, :] = -0.0
    x[100:110] = x[99]
    x[n - 5:] = x[99]
    twins = np.concatenate([np.arange(99, 110), np.arange(n - 5, n)])   # sixteen identical rows, all in the `special` sets
    q[4] = q[5] = q[7] = x[99]                                           # cases 4, 5 (sorted lists) and 7 (the unsorted list)
    q[6, ::2] = -0.0
    idx = _native.FlatIndex(d, metric=metric)
    idx.add(x)
    ks = (1, 10, 64, 100) if d == 512 else (1, 10, 64)
    for k in ks:
        cases = make_sets(idx, n, k, 6000 + d + k)
        sets = [cases[i % len(cases)][1] for i in range(NQ)]
        D, I = idx.search_grouped(q, k, sets)
        if k == 100:
            assert_bit_identical((D, I), loop_of_single_calls(idx, q, k, sets, False), f"d={d} metric={metric} k=100")
        Do = np.empty_like(D)
        Io = np.empty_like(I)
        for i in range(NQ):
            Do[i:i + 1], Io[i:i + 1] = oracle_single(x, q[i:i + 1], k, cases[i % len(cases)][2], metric)
        stats = bigcheck.compare(idx, q, D, I, Do, Io, f"grouped d={d} metric={metric} k={k}", metric=metric)
        print("[grouped vs oracle]", stats)
        for i in (4, 5, 7):   # the sixteen twins tie at the top: they come back in the order of their positions in the list
            rows = cases[i][2]
            in_list_order = rows[np.isin(rows, twins)]
            assert len(in_list_order) == 16
            assert I[i][:min(k, 16)].tolist() == in_list_order[:min(k, 16)].tolist(), (k, i)
            assert I[i][:min(k, 16)].tolist() == Io[i][:min(k, 16)].tolist(), (k, i)
    idx.close()


def test_skewed_batch_at_one_million_rows(gpu):
    """1M x 512, 256 queries, 31 sets of 1,000 rows and one of 600,000: bit identity with the loop, and the oracle for 32 of the
    queries (the eight under the large set among them)."""
    from minivectordb_amd import _native
    n, d, k, nq = 1_000_000, 512, 10, 256
    idx = _native.FlatIndex(d)
    idx.add_synthetic(n, 77)
    q = flat.synth(nq, d, 78)
    flat.normalize_l2(q)
    rng = np.random.default_rng(79)
    lists = [np.sort(rng.choice(n, 1_000, replace=False)).astype(np.int64) for _ in range(31)]
    lists.append(np.sort(rng.choice(n, 600_000, replace=False)).astype(np.int64))
    rowsets = [idx.rowset(r) for r in lists]
    assert not any(rs.is_bitmap for rs in rowsets)
    sets = [rowsets[i % 32] for i in range(nq)]
    got = idx.search_grouped(q, k, sets)
    assert_bit_identical(got, loop_of_single_calls(idx, q, k, sets, False), "skew")
    for s in (31, 0, 1, 2):
        members = [i for i in range(nq) if i % 32 == s]
        keep = np.zeros(n, np.uint8)
        keep[lists[s]] = 1
        (want,), _ = bigcheck.oracle_topk_streamed(idx, n, q[members], k, keeps=(keep,))
        stats = bigcheck.compare(idx, q[members], got[0][members], got[1][members], want[0], want[1], f"skew, set {s}")
        print("[grouped vs oracle]", stats)
    idx.close()


def test_errors_leave_the_outputs_untouched(gpu):
    from minivectordb_amd import _native
    d, n = 64, 5_000
    x = gaussian(n, d, 11)
    q = gaussian(4, d, 12)
    idx, other = _native.FlatIndex(d), _native.FlatIndex(d)
    idx.add(x)
    other.add(x)
    good = idx.rowset(np.arange(0, 1000, 3))
    stale = idx.rowset(np.arange(10, 500))
    idx.remove_rows([4999])
    other.remove_rows([4999])
    fresh = idx.rowset(np.arange(0, 1000, 3))
    # a set of another index: same device, same rows, same row count, same removal history — ONLY the owner differs
    foreign = other.rowset(np.arange(0, 1000, 3))
    assert other.ntotal == idx.ntotal and len(foreign) == len(fresh) and not foreign.is_bitmap
    foreign_bitmap = other.rowset(np.arange(5), excluded=True)

    def sentinel():
        return np.full((4, 5), 123.0, np.float32), np.full((4, 5), -77, np.int64)

    for sets, k in (([fresh, stale, fresh, None], 5), ([fresh, fresh, fresh, good], 5), ([fresh, foreign, None, fresh], 5),
                    ([fresh, None, foreign_bitmap, fresh], 5), ([fresh, None, None, fresh], 0)):
        D, I = sentinel()
        with pytest.raises(ValueError):
            idx.search_grouped(q, k, sets, out=(D, I)) if k else _raw_grouped(_native, idx, q, 0, sets, D, I)
        assert (D == 123.0).all() and (I == -77).all()
    for rs in (foreign, foreign_bitmap, stale):                  # the single-set entry point refuses them too
        D, I = sentinel()
        with pytest.raises(ValueError):
            _native.check(_native.lib().mvdb_index_search_rowset(idx._h, _native._ptr(q), 4, 5, 0, rs._h, _native._ptr(D),
                                                                 _native._ptr(I)))
        assert (D == 123.0).all() and (I == -77).all()
    Do, Io = other.search_rowset(q, 5, foreign)                  # ... and each set still serves its own index
    Dn, In = idx.search_rowset(q, 5, fresh)
    assert np.array_equal(Io, In) and np.array_equal(Do.view(np.uint32), Dn.view(np.uint32))
    with pytest.raises(ValueError):
        idx.search_grouped(q, 5, [fresh, fresh, fresh])          # sets shorter than nq (Python wrapper)
    D, I = idx.search_grouped(q, 5, [fresh, None, fresh, None], out=sentinel())
    assert (I >= 0).all()
    idx.close()
    other.close()


def test_the_shadow_single_query_option_does_not_apply(gpu):
    """With the index option shadow_single_query switched on, a single find goes through the certified fp16 route; the
    grouped entry point keeps every query — NULL and bitmap entries and the k > 64 route included — on the exact scan: its
    result is bit for bit what it was before the option was set."""
    from minivectordb_amd import _native
    d, n, nq = 512, 600_000, 12
    idx = _native.FlatIndex(d)
    idx.add_synthetic(n, 91)
    q = flat.synth(nq, d, 92)
    rng = np.random.default_rng(93)
    listed = idx.rowset(np.sort(rng.choice(n, 4_000, replace=False)))
    bitmap = idx.rowset(np.arange(0, n, 50), excluded=True)
    assert bitmap.is_bitmap and not listed.is_bitmap
    sets = [(listed, None, bitmap)[i % 3] for i in range(nq)]
    before = {k: idx.search_grouped(q, k, sets, normalize_q=True) for k in (10, 100)}
    for k, want in before.items():
        assert_bit_identical(want, loop_of_single_calls(idx, q, k, sets, True), f"option off, k={k}")
    idx.set_option("shadow_single_query", 1)
    idx.search(q[:1], 10, normalize_q=True)          # a single query now builds and uses the shadow
    assert idx.shadow_rows == n
    for k, want in before.items():
        assert_bit_identical(idx.search_grouped(q, k, sets, normalize_q=True), want, f"option on, k={k}")
    idx.close()


def _raw_grouped(_native, idx, q, k, sets, D, I):
    """k = 0 through the C-ABI itself (the wrapper would fail on the shape of `out` first)."""
    table = idx._rowset_table(sets, q.shape[0])
    _native.check(_native.lib().mvdb_index_search_grouped(idx._h, _native._ptr(q), q.shape[0], k, 0, table, _native._ptr(D),
                                                          _native._ptr(I)))


def test_device_entry_stream_graph_and_label_offset(gpu):
    import torch
    from minivectordb_amd import _native
    d, n, nq, k, off = 512, 60_000, 24, 10, 5_000_000
    x = gaussian(n, d, 21)
    idx = _native.FlatIndex(d)
    idx.add(x)
    rng = np.random.default_rng(22)
    rowsets = [idx.rowset(np.sort(rng.choice(n, m, replace=False))) for m in (3, 700, 20_000)]
    rowsets.append(idx.rowset(np.empty(0, np.int64)))
    rowsets.append(idx.rowset(np.arange(5), excluded=True))
    sets = [(rowsets + [None])[i % 6] for i in range(nq)]
    stream = torch.cuda.Stream()
    qt = torch.zeros((nq, d), dtype=torch.float32, device="cuda")
    Dt = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    It = torch.zeros((nq, k), dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_grouped_device(qt.data_ptr(), nq, k, sets, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream,
                                  normalize_q=True, label_offset=off)

    def check(q, what):
        Dw, Iw = idx.search_grouped(q, k, sets, normalize_q=True)
        D, I = Dt.cpu().numpy(), It.cpu().numpy()
        assert np.array_equal(D.view(np.uint32), Dw.view(np.uint32)), what
        assert np.array_equal(I, np.where(Iw >= 0, Iw + off, -1)), what
        assert (I[3] == -1).all() and (I[0][:3] >= off).all() and (I[0][3:] == -1).all()   # the empty set; three rows, k = 10

    q0 = gaussian(nq, d, 23)
    qt.copy_(torch.from_numpy(q0))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        enqueue()
    stream.synchronize()
    check(q0, "eager, caller stream")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    for r in range(3):
        qr = gaussian(nq, d, 30 + r)
        qt.copy_(torch.from_numpy(qr))
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(qr, f"replay {r}")
        if r == 0:   # a larger eager call on the same stream in between: the graph's table and buffers must survive it
            q2 = torch.from_numpy(gaussian(64, d, 40)).cuda()
            D2 = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
            I2 = torch.zeros((64, 64), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                idx.search_grouped_device(q2.data_ptr(), 64, 64, [rowsets[2]] * 64, D2.data_ptr(), I2.data_ptr(),
                                          stream=stream.cuda_stream)
            stream.synchronize()
            Dw, Iw = idx.search_grouped(q2.cpu().numpy(), 64, [rowsets[2]] * 64)
            assert np.array_equal(I2.cpu().numpy(), Iw) and np.array_equal(D2.cpu().numpy().view(np.uint32), Dw.view(np.uint32))
    idx.close()


def _each_filters(i):
    return [{"metadata_filter": {"tenant": i % 50}}, None, {"exclude_filter": {"lang": "de"}},
            {"or_filters": [{"tenant": 3}, {"tenant": 4}]}, {"metadata_filter": {"tenant": (i * 7) % 50, "lang": "en"}}][i % 5]


def _check_each_against_single_calls(db, q, k, grouped_exact):
    filters = [_each_filters(i) for i in range(q.shape[0])]
    many = db.find_most_similar_each(q, filters, k=k)
    assert len(many) == q.shape[0]
    for i, f in enumerate(filters):
        one = db.find_most_similar(q[i], k=k, **(f or {}))
        assert list(many[i][0]) == list(one[0]), (i, f)
        assert list(many[i][2]) == list(one[2]), (i, f)
        got, want = np.asarray(many[i][1], np.float32), np.asarray(one[1], np.float32)
        if grouped_exact and i % 5 in (0, 3, 4):   # list-form sets: the grouped launch, bit for bit
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, f)
        else:                                       # groups that share a batch pass: the existing batch contract
            np.testing.assert_allclose(got, want, atol=1e-6, rtol=0)


def _each_metadata(n):
    return [{"tenant": i % 50, "lang": ("en", "de", "fr")[i % 3]} for i in range(n)]


def test_find_most_similar_each_flat(tmp_path, gpu):
    from minivectordb_amd import VectorDatabase
    n, d = 200_000, 128
    db = VectorDatabase(storage_file=str(tmp_path / "e.pkl"))
    db.store_embeddings_batch(list(range(n)), flat.synth(n, d, 51), _each_metadata(n))
    _check_each_against_single_calls(db, flat.synth(100, d, 52), 10, grouped_exact=True)


def test_find_most_similar_each_sharded(tmp_path, gpu):
    from minivectordb_amd import ShardedVectorDatabase
    n, d = 200_000, 128
    db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=4096)
    db.store_embeddings_batch(list(range(n)), flat.synth(n, d, 53), _each_metadata(n))
    _check_each_against_single_calls(db, flat.synth(100, d, 54), 10, grouped_exact=True)


def test_find_most_similar_each_int8_takes_the_per_filter_route(tmp_path, gpu):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    n, d = 20_000, 128
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=4096)
    db.store_embeddings_batch(list(range(n)), flat.synth(n, d, 55), _each_metadata(n))
    _check_each_against_single_calls(db, flat.synth(100, d, 56), 10, grouped_exact=False)
    assert not hasattr(db.index, "search_grouped")


def test_threads_each_while_storing_and_deleting(tmp_path, gpu):
    """Four threads call find_most_similar_each while a fifth stores and deletes (tests/test_threads_gpu.py's manner): no
    exception beyond the ValueError / IndexError a search racing a delete may raise there, every id returned existed."""
    from minivectordb_amd import VectorDatabase
    d, base, extra = 64, 4_000, 600
    x = flat.synth(base + extra, d, 61)
    db = VectorDatabase(storage_file=str(tmp_path / "t.pkl"))
    db.store_embeddings_batch(list(range(base)), x[:base], [{"tenant": i % 20} for i in range(base)])
    errs, stop, served = [], threading.Event(), [0, 0, 0, 0]

    def searcher(s):
        try:
            q = flat.synth(32, d, 700 + s)
            filters = [None if i % 8 == 7 else {"metadata_filter": {"tenant": (i + s) % 20}} for i in range(32)]
            while not stop.is_set():
                try:
                    out = db.find_most_similar_each(q, filters, k=5)
                except (ValueError, IndexError):
                    continue
                assert len(out) == 32
                served[s] += 1
                for ids, dist, meta in out:
                    assert len(ids) == len(dist) == len(meta) <= 5
                    assert all(0 <= u < base + extra for u in ids)
        except Exception as e:  # pragma: no cover
            errs.append(("s", e))

    def writer():
        try:
            for i in range(extra):
                uid = base + i
                db.store_embedding(uid, x[uid], {"tenant": uid % 20})
                if i % 3 == 0:
                    db.delete_embedding(i)
                    # a delete renumbers rows and outdates every set a running call holds; paced so that a call (twenty filters,
                    # twenty row sets, one launch) fits between two of them — the stores in between are not paced
                    time.sleep(0.03)
        except Exception as e:  # pragma: no cover
            errs.append(("w", e))
        finally:
            stop.set()

    ts = [threading.Thread(target=searcher, args=(s,)) for s in range(4)] + [threading.Thread(target=writer)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert all(c > 0 for c in served), f"calls answered per searcher while the writer ran: {served}"
    q = flat.synth(20, d, 800)
    out = db.find_most_similar_each(q, [{"metadata_filter": {"tenant": t}} for t in range(20)], k=5)
    for t, (ids, dist, meta) in enumerate(out):
        assert len(ids) == 5 and all(m["tenant"] == t for m in meta)
        assert list(ids) == list(db.find_most_similar(q[t], k=5, metadata_filter={"tenant": t})[0])
