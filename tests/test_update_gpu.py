"""set_rows / update_embedding on the device (include/mvdb.h: mvdb_index_set_rows, mvdb_cos8_set_rows).

The claim is INDISTINGUISHABILITY: index A = add(x) then set_rows(rows, y) answers every search bit for bit as index B =
add(x') with x' the final matrix — D.view(uint32) and I, element for element — and keeps its derived stores (fp16 shadow, L2
offsets, int8 code) and its resident row sets while doing so."""
import threading

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu

IP, L2 = 0, 1


@pytest.fixture(scope="module")
def native(gpu):
    from conftest import assert_product_native
    assert_product_native()
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def same(a, b, what=""):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), (what, a[1], b[1])


def same_range(a, b, what=""):
    """(counts, D, I) of two range calls: the counts, and the first count entries of every row that fitted the capacity."""
    assert np.array_equal(a[0], b[0]), (what, a[0], b[0])
    cap = a[1].shape[1]
    for i, c in enumerate(a[0]):
        if c <= cap:
            assert np.array_equal(a[1][i, :c].view(np.uint32), b[1][i, :c].view(np.uint32)), (what, i)
            assert np.array_equal(a[2][i, :c], b[2][i, :c]), (what, i)


def unit(x):
    x = np.array(x, dtype=np.float32)
    flat.normalize_l2(x)
    return x


def scattered(n, m, seed):
    """m distinct rows of [0, n), unsorted; row n - 1 first, row 0 second (from m = 2 on)."""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.arange(1, n - 1))
    return np.concatenate([[n - 1, 0], rest])[:m].astype(np.int64)


# ---- 1. rows and the exact scan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [10, 64, 100, 128, 384, 512, 640, 1024])
def test_rows_and_exact_scan_equal_a_rebuild(native, d):
    import torch
    n = 4999
    x = flat.synth(n, d, 1)
    q = flat.synth(1, d, 2)
    for metric in (IP, L2):
        for normalize in (0, 1):
            for m in (1, 7, 300, n):
                rows = scattered(n, m, m)
                y = flat.synth(m, d, 100 + m) * np.float32(1.5)
                stay = np.setdiff1d(np.arange(n), rows)
                nonfinite = d == 64 and m == 7 and not normalize
                if m >= 7:
                    y[2] = 0.0                                  # a zero row: normalisation leaves it alone
                    y[3, ::2] = -0.0                            # -0.0 elements
                    y[3, 1::2] = 0.25
                    if stay.size:
                        y[4] = x[stay[0]]                       # a duplicate of a stored row that stays: a tie, lower row first
                    if nonfinite:
                        y[5, 1] = np.nan
                        y[6, 0] = np.inf
                final = x.copy()
                final[rows] = y
                A = native.FlatIndex(d, metric=metric)
                A.add(x, normalize=bool(normalize))
                A.set_rows(rows, y, normalize=bool(normalize))
                A2 = native.FlatIndex(d, metric=metric)
                A2.add(x, normalize=bool(normalize))
                yt = torch.from_numpy(y).cuda()
                torch.cuda.synchronize()
                A2.set_rows_device(rows, yt.data_ptr(), m, normalize=bool(normalize))
                B = native.FlatIndex(d, metric=metric)
                B.add(final, normalize=bool(normalize))
                what = f"d={d} metric={metric} normalize={normalize} m={m}"
                assert A.ntotal == A2.ntotal == B.ntotal == n
                want = B.get_rows(0, n)
                assert A.get_rows(0, n).tobytes() == want.tobytes(), what
                assert A2.get_rows(0, n).tobytes() == want.tobytes(), what + " (device entry)"
                if m >= 7 and stay.size:
                    probe = unit(x[stay[0]:stay[0] + 1]) if metric == IP else x[stay[0]:stay[0] + 1]
                    if not nonfinite:
                        lo, hi = sorted((int(stay[0]), int(rows[4])))
                        got = A.search(probe, 2, normalize_q=bool(normalize))
                        if normalize or metric == L2:
                            assert list(got[1][0]) == [lo, hi], (what, got)
                for k in (1, 10, 100):
                    for qq in (q, unit(final[rows[0]:rows[0] + 1] + np.float32(0.01))):
                        same(A.search(qq, k, normalize_q=True), B.search(qq, k, normalize_q=True), f"{what} k={k}")
                        same(A2.search(qq, k, normalize_q=True), B.search(qq, k, normalize_q=True), f"{what} k={k} device")
                for ix in (A, A2, B):
                    ix.close()


# ---- shared construction of tests 2, 3, 5 -------------------------------------------------------------------------------------
def planted_update(native, x, q, m, metric=IP, normalize=True, seed=7, exclude=()):
    """A = add(x), the first batch run (builds the derived stores), then rows / new rows with the planting of the issue: the
    best row of query 0 becomes -q0, some other row becomes q0.  Returns (A, rows, y, best, other, first batch result)."""
    n, d = x.shape
    A = native.FlatIndex(d, metric=metric)
    A.add(x, normalize=normalize)
    first = A.search(q, 10, normalize_q=True)
    best = int(first[1][0, 0])
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(n), np.concatenate([[best], np.asarray(exclude, dtype=np.int64)]))
    rows = np.concatenate([[best], rng.choice(pool, m - 1, replace=False)]).astype(np.int64)
    other = int(rows[1])
    y = flat.synth(m, d, 1000 + seed)
    return A, rows, y, best, other, first


@pytest.mark.parametrize("d", [512, 1024])
def test_shadow_kept_not_rebuilt(native, d):
    n, nq = 20_001, 40
    x = unit(flat.synth(n, d, 11))
    q = unit(flat.synth(nq, d, 12))
    A, rows, y, best, other, _ = planted_update(native, x, q, 64)
    y = unit(y)
    y[0], y[1] = -q[0], q[0]
    assert A.shadow_rows == n
    A.set_rows(rows, y, normalize=True)
    assert A.shadow_rows == n                                   # kept, not dropped
    final = x.copy()
    final[rows] = y
    B = native.FlatIndex(d)
    B.add(final, normalize=True)
    got, want = A.search(q, 10, normalize_q=True), B.search(q, 10, normalize_q=True)
    assert B.shadow_rows == n
    same(got, want, "batch over the shadow")
    assert got[1][0, 0] == other and best not in got[1][0]
    mask = native.pack_row_mask(n, excluded=np.arange(0, n, 3))
    same(A.search_masked(q, 10, mask, normalize_q=True), B.search_masked(q, 10, mask, normalize_q=True), "masked")
    # one threshold per query: just below its 20th best score (a batch pass re-scores in fp32 in another order than the range
    # kernels sum: the last bit of a score may differ, 1e-6 is far above that and far below the gap to the 21st)
    thr = np.ascontiguousarray(B.search(q, 20, normalize_q=True)[0][:, -1] - np.float32(1e-6))
    for ix in (A, B):
        ix.set_option("range_shared", 2)
    before = A.range_counters()[0]
    ga, gb = A.range_search_raw(q, thr, 64, normalize_q=True), B.range_search_raw(q, thr, 64, normalize_q=True)
    assert A.range_counters()[0] - before == 1                  # the shared route ran
    assert (ga[0] >= 20).all() and (ga[0] <= 64).any()
    same_range(ga, gb, "range_search_each, shared pass")
    assert A.shadow_rows == n
    A.close()
    B.close()


def test_scale_step_invalidates_the_shadow(native):
    """Raw rows of norm ~6.5 (bound in [4, 8)); one new row of four times that moves row_norm_bound across a power of two, so
    the shadow's scale: the shadow is emptied as add would empty it, the next batch converts in place."""
    n, d, nq = 20_001, 512, 40
    x = flat.synth(n, d, 21)
    q = flat.synth(nq, d, 22)
    A = native.FlatIndex(d)
    A.add(x)
    A.search(q, 10)
    assert A.shadow_rows == n
    rows = np.array([n - 1, 17, 4000], dtype=np.int64)
    y = flat.synth(3, d, 23)
    y[1] *= np.float32(4.0)
    A.set_rows(rows, y)
    assert A.shadow_rows == 0
    batch = A.search(q, 10)
    assert A.shadow_rows == n
    for i in range(nq):
        one = A.search(q[i:i + 1], 10)
        assert np.array_equal(batch[1][i], one[1][0]), i
        assert np.allclose(batch[0][i], one[0][0], rtol=1e-5, atol=1e-5), i
    final = x.copy()
    final[rows] = y
    B = native.FlatIndex(d)
    B.add(final)
    same(A.search(q[:1], 10), B.search(q[:1], 10), "exact scan")
    A.close()
    B.close()


# ---- 3. L2 with offsets -------------------------------------------------------------------------------------------------------
def test_l2_offsets_kept(native):
    n, d, nq = 20_001, 512, 40
    rng = np.random.default_rng(31)
    x = flat.synth(n, d, 31) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    q = flat.synth(nq, d, 32)
    norms = (x.astype(np.float64) ** 2).sum(1)
    keep_out = [int(norms.argmax()), int(norms.argmin())]
    A = native.FlatIndex(d, metric=L2)
    A.add(x)
    A.search(q, 10)
    assert A.shadow_rows == n
    pool = np.setdiff1d(np.arange(n), keep_out)
    rows = rng.choice(pool, 64, replace=False).astype(np.int64)
    y = flat.synth(64, d, 33)                                    # scale 1: inside the range of norms of x
    final = x.copy()
    final[rows] = y
    fn = (final.astype(np.float64) ** 2).sum(1)
    # the precondition: A (bounds widened only) and B see the same norm2_lo / norm2_hi, so the same routes
    assert int(fn.argmax()) == keep_out[0] and int(fn.argmin()) == keep_out[1]
    assert fn.max() == norms.max() and fn.min() == norms.min()
    A.set_rows(rows, y)
    assert A.shadow_rows == n
    B = native.FlatIndex(d, metric=L2)
    B.add(final)
    same(A.search(q, 10), B.search(q, 10), "L2 batch")
    same(A.search(q[:1], 10), B.search(q[:1], 10), "L2 single")
    A.close()
    B.close()


# ---- 4. int8 code kept --------------------------------------------------------------------------------------------------------
def test_code8_kept(native):
    n, d, k = 500_000, 384, 10
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, normalize=True)
    q = unit(flat.synth(4, d, 5678))
    idx.set_option("code8_single_query", 1)
    for qi in q:
        idx.search(qi, k)
    assert idx.code8_rows == n
    best = int(idx.search(q[0], k)[1][0, 0])
    rng = np.random.default_rng(41)
    rows = np.concatenate([[best], rng.choice(np.setdiff1d(np.arange(n), [best]), 99, replace=False)]).astype(np.int64)
    y = unit(flat.synth(100, d, 42))
    y[0], y[1] = -q[0], q[0]
    idx.set_rows(rows, y, normalize=True)
    assert idx.code8_rows == n                                  # kept: no rebuild, no wait
    fallbacks, _, calls = idx.code8_counters()
    got = idx.search(q[0], k)
    fallbacks2, _, calls2 = idx.code8_counters()
    assert calls2 - calls == 1 and fallbacks2 - fallbacks == 0  # served by the prefilter
    assert got[1][0, 0] == rows[1] and best not in got[1][0]
    served = [idx.search(qi, k) for qi in q]
    idx.set_option("code8_single_query", 0)
    for qi, g in zip(q, served):
        same(g, idx.search(qi, k), "prefilter against the exact scan")
    idx.close()


# ---- 5. row sets survive ------------------------------------------------------------------------------------------------------
def test_row_sets_and_graphs_survive(native):
    import torch
    n, d, nq, k = 20_001, 512, 40, 10
    x = unit(flat.synth(n, d, 51))
    q = unit(flat.synth(nq, d, 52))
    A, rows, y, best, other, _ = planted_update(native, x, q, 64)
    y = unit(y)
    y[0], y[1] = -q[0], q[0]
    rng = np.random.default_rng(53)
    lists = {
        "sorted": np.sort(np.concatenate([[best, other], rng.choice(n, 700, replace=False)])),
        "unsorted": np.concatenate([[other, best], rng.permutation(n)[:300]]),
        "bitmap": np.setdiff1d(np.arange(n), np.arange(7, n, 50)),
    }
    lists = {name: np.unique(v) if name != "unsorted" else v[np.sort(np.unique(v, return_index=True)[1])] for name, v in lists.items()}
    gone = np.arange(5, n, 1000)

    def build(ix):
        sets = {name: ix.rowset(v) for name, v in lists.items()}
        sets["excluded"] = ix.rowset(gone, excluded=True)
        return sets

    sa = build(A)
    assert sa["bitmap"].is_bitmap and not sa["unsorted"].is_bitmap
    # a device call captured BEFORE the update
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(q).cuda()
    Dt = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    It = torch.zeros((nq, k), dtype=torch.int64, device="cuda")

    def enqueue():
        A.search_rowset_device(qt.data_ptr(), nq, k, sa["sorted"], Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        enqueue()
    stream.synchronize()
    old = (Dt.cpu().numpy().copy(), It.cpu().numpy().copy())
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    torch.cuda.synchronize()

    A.set_rows(rows, y, normalize=True)
    final = x.copy()
    final[rows] = y
    B = native.FlatIndex(d)
    B.add(final, normalize=True)
    B.search(q, k)                                               # B's shadow, as A has one
    sb = build(B)
    Dt.zero_()
    It.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = B.search_rowset(q, k, sb["sorted"])
    same((Dt.cpu().numpy(), It.cpu().numpy()), want, "graph captured before the update")
    assert not np.array_equal(old[1], want[1])                   # (the update is visible in this result)
    for name in sa:
        for qq in (q[:1], q):
            same(A.search_rowset(qq, k, sa[name]), B.search_rowset(qq, k, sb[name]), f"search_rowset {name} nq={len(qq)}")
        ca, cb = A.range_search_raw(q, 0.12, 256, sa[name]), B.range_search_raw(q, 0.12, 256, sb[name])
        assert ca[0].sum() > 0, name
        same_range(ca, cb, f"range_search {name}")
    order = ["sorted", "unsorted", "bitmap", "excluded", None]
    ga = A.search_grouped(q, k, [sa[order[i % 5]] if order[i % 5] else None for i in range(nq)])
    gb = B.search_grouped(q, k, [sb[order[i % 5]] if order[i % 5] else None for i in range(nq)])
    same(ga, gb, "search_grouped")
    assert ga[1][0, 0] == other
    A.close()
    B.close()


# ---- 6. errors leave no trace -------------------------------------------------------------------------------------------------
def test_errors_leave_no_trace(native):
    import ctypes
    n, d = 20_001, 512
    x = unit(flat.synth(n, d, 61))
    idx = native.FlatIndex(d)
    idx.add(x, normalize=True)
    idx.search(unit(flat.synth(40, d, 62)), 10)
    rows_before, shadow = idx.get_rows(0, n), idx.shadow_rows
    assert shadow == n
    y = unit(flat.synth(3, d, 63))
    lib = native.lib()
    for bad in ([1, 2, n], [1, -1, 2], [5, 9, 5]):
        with pytest.raises(ValueError) as err:
            idx.set_rows(bad, y)
        assert str(err.value)
        ptr = ctypes.c_void_p(0)
        r = np.array(bad, dtype=np.int64)
        assert lib.mvdb_index_set_rows_device(idx.handle, r.ctypes.data_as(ctypes.c_void_p), ptr, 3, 0) == native.ERR_ARG
    r = np.array([1, 2, 3], dtype=np.int64)
    rp = r.ctypes.data_as(ctypes.c_void_p)
    assert lib.mvdb_index_set_rows(idx.handle, rp, None, 3, 1) == native.ERR_ARG and native.last_error()
    assert lib.mvdb_index_set_rows(idx.handle, None, y.ctypes.data_as(ctypes.c_void_p), 3, 1) == native.ERR_ARG
    assert lib.mvdb_index_set_rows_device(idx.handle, rp, None, 3, 1) == native.ERR_ARG
    assert lib.mvdb_index_set_rows(idx.handle, None, None, 0, 1) == 0
    assert lib.mvdb_index_set_rows_device(idx.handle, None, None, 0, 0) == 0
    idx.set_rows(np.empty(0, np.int64), np.empty((0, d), np.float32))
    with pytest.raises(ValueError):
        idx.set_rows([1, 2], y)                                  # shapes disagree
    with pytest.raises(ValueError):
        idx.set_rows([1, 2, 3], np.zeros((3, d + 1), np.float32))
    assert idx.get_rows(0, n).tobytes() == rows_before.tobytes()
    assert idx.shadow_rows == shadow and idx.code8_rows == 0 and idx.ntotal == n
    idx.close()


# ---- 7. the int8 cosine index -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 512, 1100])
def test_cos8_equals_a_rebuild(native, d):
    import ctypes
    import torch
    n, k = 4999, 10
    x = flat.synth(n, d, 71)
    q = flat.synth(40, d, 72)
    rows = scattered(n, 300, 73)
    y = flat.synth(300, d, 74) * np.float32(3.0)
    y[2] = 0.0
    y[4] = x[1]
    y[5], y[6] = q[0], -q[0]
    final = x.copy()
    final[rows] = y
    A, A2, B = (native.Cos8Index(d) for _ in range(3))
    for ix in (A, A2):
        ix.add(x)
    B.add(final)
    lists = [np.unique(np.concatenate([rows[:20], np.arange(100, 900)])), np.setdiff1d(np.arange(n), np.arange(3, n, 40))]
    sa = [A.rowset(lists[0]), A.rowset(lists[1]), A.rowset(np.arange(0, n, 9), excluded=True)]
    A.set_rows(rows, y)
    yt = torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    A2.set_rows_device(rows, yt.data_ptr(), 300)
    sb = [B.rowset(lists[0]), B.rowset(lists[1]), B.rowset(np.arange(0, n, 9), excluded=True)]
    want = B.get_codes(0, n)
    for ix in (A, A2):
        got = ix.get_codes(0, n)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for nq in (1, 5, 40):
        same(A.search(q[:nq], k), B.search(q[:nq], k), f"cos8 nq={nq}")
        for a, b in zip(sa, sb):
            same(A.search_rowset(q[:nq], k, a), B.search_rowset(q[:nq], k, b), f"cos8 rowset nq={nq}")
    assert A.search(q[:1], 1)[1][0, 0] == rows[5]
    lib = native.lib()
    for bad in ([1, 2, n], [1, -1, 2], [5, 9, 5]):
        with pytest.raises(ValueError) as err:
            A.set_rows(bad, y[:3])
        assert str(err.value)
    r = np.array([1, 2, 3], dtype=np.int64)
    assert lib.mvdb_cos8_set_rows(A.handle, r.ctypes.data_as(ctypes.c_void_p), None, 3) == native.ERR_ARG
    assert lib.mvdb_cos8_set_rows_device(A.handle, None, ctypes.c_void_p(yt.data_ptr()), 3) == native.ERR_ARG
    assert lib.mvdb_cos8_set_rows(A.handle, None, None, 0) == 0
    got = A.get_codes(0, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for ix in (A, A2, B):
        ix.close()


# ---- 8. threads ---------------------------------------------------------------------------------------------------------------
def test_searches_see_the_old_or_the_new_state(native):
    """Four threads search while a fifth flips two planted rows back and forth: a result is the old state's or the new
    state's, never a mix (in a mix the query would find both planted rows, or neither)."""
    n, d, k = 20_001, 512, 2
    x = unit(flat.synth(n, d, 81))
    q = unit(flat.synth(1, d, 82))
    a, b = 100, 15_000
    idx = native.FlatIndex(d)
    idx.add(x, normalize=True)
    states = [np.stack([q[0], -q[0]]), np.stack([-q[0], q[0]])]   # (row a, row b): the query's copy sits in a, or in b
    rows = np.array([a, b], dtype=np.int64)
    idx.set_rows(rows, states[0])
    answers = []
    for s in (0, 1):
        idx.set_rows(rows, states[s])
        D, I = idx.search(q, k)
        answers.append((D.tobytes(), I.tobytes()))
        assert I[0, 0] == (a, b)[s]
    labels = [a[1] for a in answers]
    stop, errors, seen = threading.Event(), [], [set() for _ in range(4)]

    def searcher(slot):
        try:
            while not stop.is_set():
                if slot % 2 == 0:
                    D, I = idx.search(q, k)
                    got = (D.tobytes(), I.tobytes())
                    assert got in answers, (slot, D, I)
                    seen[slot].add(answers.index(got))
                else:   # a batch (the passes over the fp16 shadow re-score in another order: the rows decide)
                    D, I = idx.search(np.repeat(q, 40, 0), k)
                    for i in range(40):
                        assert I[i:i + 1].tobytes() in labels, (slot, i, D[i], I[i])
                        seen[slot].add(labels.index(I[i:i + 1].tobytes()))
        except BaseException as e:   # noqa: B036
            errors.append(e)
            stop.set()

    threads = [threading.Thread(target=searcher, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    try:
        for flip in range(200):
            idx.set_rows(rows, states[flip % 2])
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors[0]
    assert all(seen)
    idx.close()


# ---- 9. the database classes --------------------------------------------------------------------------------------------------
def make_db(kind, where):
    from minivectordb_amd import ShardedVectorDatabase, ShardedVectorDatabaseUsearch, VectorDatabase
    where.mkdir(parents=True, exist_ok=True)
    if kind == "flat":
        return VectorDatabase(storage_file=str(where / "db.pkl"))
    if kind == "sharded":
        return ShardedVectorDatabase(storage_dir=str(where / "shards"), shard_size=500)
    return ShardedVectorDatabaseUsearch(storage_dir=str(where / "shards"), shard_size=500)


def shard_bytes(where):
    folder = where / "shards"
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


@pytest.mark.parametrize("kind", ["flat", "sharded", "usearch"])
def test_database_classes(native, tmp_path, kind):
    n, d = 2000, 128
    x = flat.synth(n, d, 91)
    q = flat.synth(24, d, 92)
    meta = [{"tenant": i % 20, "lang": "en" if i % 3 else "de"} for i in range(n)]

    def fresh(where):
        db = make_db(kind, where)
        db.store_embeddings_batch(list(range(n)), x, [dict(m) for m in meta])
        return db

    def ids_of(result):
        return list(result[0])

    db, early = fresh(tmp_path / "a"), fresh(tmp_path / "e")
    # a pending row (before the first query) and a flushed row behave alike
    early.update_embedding(700, embedding=q[0])
    db.find_most_similar(q[0], k=1)
    db.update_embedding(700, embedding=q[0])
    ra, rb = early.find_most_similar(q[0], k=5), db.find_most_similar(q[0], k=5)
    assert ids_of(ra) == ids_of(rb) and ids_of(rb)[0] == 700 and list(ra[1]) == list(rb[1])
    want = unit(q[:1])[0] if kind == "flat" else q[0]            # the shard files keep the raw row
    tol = 1e-6 if kind == "flat" else 0.0                        # (device normalisation against the oracle's)
    np.testing.assert_allclose(db.get_vector(700), want, atol=tol, rtol=0)
    if kind != "flat":
        assert np.array_equal(early.get_vector(700), want)
    else:
        assert np.array_equal(early.get_vector(700), db.get_vector(700))   # add's normalisation and set_rows' agree bit for bit
    # metadata only: the id moves between filter results
    f3, f4 = {"metadata_filter": {"tenant": 3}}, {"metadata_filter": {"tenant": 4}}
    assert 3 in ids_of(db.find_most_similar(x[3], k=3, **f3))
    db.update_embedding(3, metadata_dict={"tenant": 4, "lang": "en"})
    assert 3 not in ids_of(db.find_most_similar(x[3], k=3, **f3))
    assert ids_of(db.find_most_similar(x[3], k=3, **f4))[0] == 3
    # embedding only, after a filtered query: no new row set
    made = []
    real_rowset = db.index.rowset
    db.index.rowset = lambda *a, **kw: (made.append(1), real_rowset(*a, **kw))[1]
    db.find_most_similar(q[1], k=3, **f4)
    made_before = len(made)
    db.update_embedding(3, embedding=q[1])
    got = db.find_most_similar(q[1], k=3, **f4)
    assert ids_of(got)[0] == 3 and len(made) == made_before
    # 20 tenants after an embedding-only update: each equals the loop of single calls
    tenants = [{"metadata_filter": {"tenant": t}} for t in range(20)]
    db.find_most_similar_each(q[:20], tenants, k=5)
    made_before = len(made)
    db.update_embedding(25, embedding=q[5])                     # tenant 5
    each = db.find_most_similar_each(q[:20], tenants, k=5)
    assert len(made) == made_before
    for i, t in enumerate(tenants):
        one = db.find_most_similar(q[i], k=5, **t)
        assert ids_of(each[i]) == ids_of(one) and list(each[i][1]) == list(one[1]), i
    assert ids_of(each[5])[0] == 25
    # a batch of 300 equals 300 single updates
    twin = fresh(tmp_path / "t")
    twin.find_most_similar(q[0], k=1)
    for uid, v, m in ((700, q[0], None), (3, q[1], {"tenant": 4, "lang": "en"}), (25, q[5], None)):
        twin.update_embedding(uid, v, m)
    ids = list(range(1000, 1300))
    y = flat.synth(300, d, 93)
    metas = [{"tenant": (i * 7) % 20, "lang": "fr"} for i in ids]
    before = shard_bytes(tmp_path / "a") if kind != "flat" else None
    db.update_embeddings_batch(ids, y, metas)
    for uid, v, m in zip(ids, y, metas):
        twin.update_embedding(uid, v, m)
    for kw in ({}, {"metadata_filter": {"lang": "fr"}}, {"exclude_filter": {"lang": "fr"}}, f4):
        for qq in (q[2], y[10], y[299]):
            ra, rb = db.find_most_similar(qq, k=8, **kw), twin.find_most_similar(qq, k=8, **kw)
            assert ids_of(ra) == ids_of(rb) and list(ra[1]) == list(rb[1]) and list(ra[2]) == list(rb[2])
    if kind != "flat":
        after = shard_bytes(tmp_path / "a")
        assert sorted(name for name in before if before[name] != after[name]) == ["shard_2.pkl"]   # ids 1000 .. 1299
    # the ValueErrors change nothing
    snapshot = [db.find_most_similar(q[2], k=8, **kw) for kw in ({}, f4)]
    for kw in (dict(unique_ids=[1, 2]), dict(unique_ids=[1, 99999], embeddings=y[:2]), dict(unique_ids=[1, 1], embeddings=y[:2]),
               dict(unique_ids=[1, 2], embeddings=np.zeros((2, d + 1), np.float32)), dict(unique_ids=[1, 2], embeddings=y[:3]),
               dict(unique_ids=[1, 2], metadata_dicts=[{}])):
        with pytest.raises(ValueError):
            db.update_embeddings_batch(**kw)
    with pytest.raises(ValueError):
        db.store_embedding(1, y[0])                              # as before
    again = [db.find_most_similar(q[2], k=8, **kw) for kw in ({}, f4)]
    for ra, rb in zip(snapshot, again):
        assert ids_of(ra) == ids_of(rb) and list(ra[1]) == list(rb[1])
    # persist / reopen shows the new state
    if kind == "flat":
        db.persist_to_disk()
    reopened = make_db(kind, tmp_path / "a")
    assert ids_of(reopened.find_most_similar(q[5], k=1, **tenants[5]))[0] == 25
    assert ids_of(reopened.find_most_similar(y[10], k=1, metadata_filter={"lang": "fr"}))[0] == 1010
    assert 3 not in ids_of(reopened.find_most_similar(x[3], k=5, **f3))
    np.testing.assert_allclose(reopened.get_vector(1010), unit(y[10:11])[0] if kind == "flat" else y[10], atol=1e-6, rtol=0)
