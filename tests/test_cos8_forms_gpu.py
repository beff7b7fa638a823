"""Every form of the int8 cosine scan on the device against the exact CPU oracle (tests/cos8_oracle.py), through the C-ABI
classes Cos8Index / Cos8RowSet: all 96 instantiations of cos8_scan_kernel and both of cos8_mfma_kernel (the table in
tests/cos8_cases.py; tests/test_cos8_cpu.py proves that the table reaches them), the quantiser's edges as stored rows and as
queries, row sets older than the index and at their size edges, the device entry point with a label offset, tie groups
of more than a thousand rows, corpora that keep the estimate gate open or shut, graph replay after the workspace grew, and
the store's growth and removal edges.  Every comparison is bit-exact on I and on D.view(uint32).

Measured on one MI355X: the 169 tests of this file take 23 s; the rest of the -m gpu suite (411 tests) takes 457 s."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cos8_cases as C  # noqa: E402
import cos8_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def check_equal(D, I, Do, Io, what):
    assert D.shape == Do.shape and I.shape == Io.shape, (what, D.shape, Do.shape)
    assert np.array_equal(I, Io), (what, np.argwhere(I != Io)[:5], I[:2], Io[:2])
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), (what, np.argwhere(D != Do)[:5], D[:2], Do[:2])


def missing(nq, k):
    return np.full((nq, k), O.FLT_MAX, np.float32), np.full((nq, k), -1, np.int64)


def osearch(codes, a2, q, k, rows=None):
    """O.search, and the contract's answer for an empty selection (the oracle's top-k needs one row at least)."""
    q = np.atleast_2d(q)
    if (rows is not None and len(rows) == 0) or codes.shape[0] == 0:
        return missing(q.shape[0], k)
    return O.search(codes, a2, q, k, rows=rows)


def search(idx, q, k, rs=None):
    return idx.search(q, k) if rs is None else idx.search_rowset(q, k, rs)


def check_batch_and_singles(idx, codes, a2, q, k, rs, rows, what):
    D, I = search(idx, q, k, rs)
    check_equal(D, I, *osearch(codes, a2, q, k, rows), what)
    nq = q.shape[0]
    for i in sorted({0, nq // 2, nq - 1}):     # batch row i == a single call under the same filter, bit for bit
        D1, I1 = search(idx, q[i], k, rs)
        check_equal(D1[0], I1[0], D[i], I[i], (what, "single", i))
    return D, I


def dev_search(idx, q, k, stream, rs=None, label_offset=0):
    """The device entry points on a side stream; returns host copies of D and I."""
    import torch
    nq = q.shape[0]
    qt = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    Dt = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    It = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        if rs is None:
            idx.search_device(qt.data_ptr(), nq, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream,
                              label_offset=label_offset)
        else:
            idx.search_rowset_device(qt.data_ptr(), nq, k, rs, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream,
                                     label_offset=label_offset)
    stream.synchronize()
    return Dt.cpu().numpy(), It.cpu().numpy()


def labelled(Io, offset):
    return np.where(Io >= 0, Io + offset, -1)


# ---- 1. the form table ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stores():
    """One index per (n, d) of the table, shared by its cases (searches do not change an index)."""
    made = {}
    yield made
    for idx, _, _, _ in made.values():
        idx.close()


def _store(stores, n, d):
    from minivectordb_amd import _native
    if (n, d) not in stores:
        x = C.corpus(n, d)
        idx = _native.Cos8Index(d)
        idx.add(x)
        codes, a2 = idx.get_codes(0, n)
        oc, oa = O.quantize(x)
        assert np.array_equal(codes, oc) and np.array_equal(a2, oa)
        stores[(n, d)] = (idx, codes, a2, x[:2].copy())
    return stores[(n, d)]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_form(gpu, stores, case):
    n, d, nq, k, kind = case
    idx, codes, a2, head = _store(stores, n, d)
    q = C.queries(head, nq)
    rows, excluded, keep = C.filter_rows(n, kind)
    rs = None
    if kind != "none":
        rs = idx.rowset(rows, excluded=excluded)
        assert rs.is_bitmap == C.rowset_is_bitmap(n, len(rows), excluded) == (C.FILTER_FORM[kind] == 2)
        assert len(rs) == len(keep)
    D, I = check_batch_and_singles(idx, codes, a2, q, k, rs, keep, case)
    if kind == "none":
        assert I[0, 0] == 1 and D[0, 0] == 0.0      # q[0] is stored row 1; its copies follow in row order
    if rs is not None:
        rs.close()


# ---- 2. quantiser edges on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 17, 64, 1000, 4096])
def test_special_rows_bytes(gpu, d):
    import torch
    from minivectordb_amd import _native
    x = C.special_rows(d, np.random.default_rng(d))
    m = x.shape[0]
    with np.errstate(all="ignore"):
        oc, oa = O.quantize(x)
    assert (oc[7] == 127).all() and oa[7] == 127 * 127 * d               # 3e37 * 127f overflows: every code clamps
    assert (oc[8] == -int(127 / np.sqrt(d))).all()                       # subnormals count: a flushing build gives zeros
    for i in C.SPECIAL_ZERO_ROWS:
        assert not oc[i].any()
    idx = _native.Cos8Index(d)
    idx.add(x)
    xt = torch.from_numpy(x).cuda()
    idx.add_device(xt.data_ptr(), m)
    torch.cuda.synchronize()
    assert idx.ntotal == 2 * m
    for row0, what in ((0, "add"), (m, "add_device")):
        codes, a2 = idx.get_codes(row0, m)
        bad = np.nonzero((codes != oc).any(axis=1) | (a2 != oa))[0]
        assert bad.size == 0, (what, d, bad, codes[bad[:1]], oc[bad[:1]])
    idx.close()


@pytest.mark.parametrize("d", [48, 1040])
def test_special_queries(gpu, d):
    """The quantiser's edge rows as QUERIES at nq = 1, 5 and 25: b2 == 0 (zero, -0.0, NaN, inf), ab == 0 and a2 above
    127^2 on every search route (single scan, batch scan, matrix cores at d = 48, scores at k = 100)."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(d)
    x = rng.standard_normal((300, d)).astype(np.float32)
    x[7] = 0.0
    x[200] = 0.0
    x[9] = np.eye(1, d, 0)[0]          # against the one-hot queries: ab == 0 with a2, b2 > 0 for most rows
    x[10] = 3e37
    q = C.special_rows(d, rng)
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, 300)
    assert list(np.nonzero(a2 == 0)[0]) == [7, 200] and a2[10] == 127 * 127 * d
    with np.errstate(all="ignore"):
        qb2 = O.quantize(q)[1]
    zero_q = [i for i in range(q.shape[0]) if qb2[i] == 0]
    assert set(C.SPECIAL_ZERO_ROWS) <= set(zero_q)
    others = [r for r in range(300) if r not in (7, 200)]
    for k in (1, 10, 64, 100):
        with np.errstate(all="ignore"):
            Do, Io = O.search(codes, a2, q, k)
        for i in zero_q:               # zero rows first at distance 0 in row order, then distance 1 in row order
            assert list(Io[i]) == ([7, 200] + others)[:k]
            assert list(Do[i]) == ([0.0, 0.0] + [1.0] * 298)[:k]
        D, I = idx.search(q, k)
        check_equal(D, I, Do, Io, ("special queries", d, k))
        for i0 in range(0, q.shape[0], 5):
            D5, I5 = idx.search(q[i0:i0 + 5], k)
            check_equal(D5, I5, Do[i0:i0 + 5], Io[i0:i0 + 5], ("special queries by 5", d, k, i0))
        for i in range(q.shape[0]):
            D1, I1 = idx.search(q[i], k)
            check_equal(D1, I1, Do[i:i + 1], Io[i:i + 1], ("special query alone", d, k, i))
    rs = idx.rowset([7, 9, 10, 250], excluded=True)
    keep = np.setdiff1d(np.arange(300), [7, 9, 10, 250])
    for k in (10, 100):
        with np.errstate(all="ignore"):
            Do, Io = O.search(codes, a2, q, k, rows=keep)
        check_equal(*idx.search_rowset(q, k, rs), Do, Io, ("special queries, excluded", d, k))
        check_equal(*idx.search_rowset(q[:5], k, rs), Do[:5], Io[:5], ("special queries by 5, excluded", d, k))
        check_equal(*idx.search_rowset(q[18], k, rs), Do[18:19], Io[18:19], ("NaN query alone, excluded", d, k))
    idx.close()


def test_arguments_refused(gpu):
    from minivectordb_amd import _native
    for d in (0, -1, C.MAX_D + 1):
        with pytest.raises(ValueError):
            _native.Cos8Index(d)
    idx = _native.Cos8Index(C.MAX_D)
    assert idx.d == C.MAX_D and idx.ntotal == 0
    idx.close()
    x = np.random.default_rng(0).standard_normal((100, 8)).astype(np.float32)
    idx, other = _native.Cos8Index(8), _native.Cos8Index(8)
    idx.add(x)
    other.add(x)
    for k in (0, -3, C.MAX_K + 1):
        with pytest.raises(ValueError):
            idx.search(x[:2], k)
    rs_other = other.rowset([1, 2, 3])
    with pytest.raises(ValueError):
        idx.search_rowset(x[:2], 5, rs_other)
    for bad in ([-1], [100], [3, 3]):
        with pytest.raises(ValueError):
            idx.rowset(bad)
    codes, a2 = idx.get_codes(0, 100)
    check_equal(*idx.search(x[:2], 5), *O.search(codes, a2, x[:2], 5), "after refused calls")
    rs_other.close()
    idx.close()
    other.close()


# ---- 3. row sets and the device entry point -------------------------------------------------------------------------
@pytest.mark.parametrize("n_base", [64 * 40 - 1, 64 * 40, 64 * 40 + 1])
def test_rowset_older_than_index(gpu, n_base):
    """include/mvdb.h: "rows appended later are not part of it" — also when they are exact copies of the best hits."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(n_base)
    d = 96
    x = rng.standard_normal((n_base, d)).astype(np.float32)
    q = rng.standard_normal((33, d)).astype(np.float32)
    q[1] = x[n_base - 1]
    idx = _native.Cos8Index(d)
    idx.add(x)
    base_codes, base_a2 = idx.get_codes(0, n_base)
    few = np.union1d(rng.choice(n_base, 200, replace=False), [0, n_base - 1])
    half = np.union1d(rng.choice(n_base, n_base // 2, replace=False), [n_base - 1])
    gone = rng.choice(n_base - 1, 40, replace=False)          # the last row stays selected
    sets = {"list": (idx.rowset(few), few), "bitmap": (idx.rowset(half), half),
            "excluded": (idx.rowset(gone, excluded=True), np.setdiff1d(np.arange(n_base), gone)),
            "exclude nothing": (idx.rowset([], excluded=True), np.arange(n_base))}
    assert not sets["list"][0].is_bitmap and sets["bitmap"][0].is_bitmap and sets["excluded"][0].is_bitmap
    best = np.unique(np.concatenate([O.search(base_codes, base_a2, q, 3, rows=rows)[1].ravel()
                                     for _, rows in sets.values()]))
    later = np.concatenate([x[best], rng.standard_normal((700, d)).astype(np.float32), x[best[:5]]])
    idx.add(later)                                            # crosses the capacity of the first allocation: the store moves
    n = idx.ntotal
    codes, a2 = idx.get_codes(0, n)
    assert np.array_equal(codes[:n_base], base_codes) and n == n_base + later.shape[0]
    D, I = idx.search(q, 10)
    check_equal(D, I, *O.search(codes, a2, q, 10), "plain search sees the new rows")
    assert (I >= n_base).any()
    for name, (rs, rows) in sets.items():
        assert len(rs) == len(rows)
        for k in (10, 100):
            for nq in (1, 5, 33):
                Dr, Ir = idx.search_rowset(q[:nq], k, rs)
                check_equal(Dr, Ir, *O.search(base_codes, base_a2, q[:nq], k, rows=rows), (name, n_base, k, nq))
                assert Ir.max() < n_base
        rs.close()
    idx.close()


def test_rowset_edges(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(5)
    n, d = 1003, 40
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[n - 1] = x[0]
    q = rng.standard_normal((33, d)).astype(np.float32)
    q[0] = x[0]
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    every = np.arange(n)

    def run(rs, rows, what, ks=(1, 10, 64, 100), nqs=(1, 5, 33)):
        assert len(rs) == len(rows)
        for k in ks:
            for nq in nqs:
                check_equal(*idx.search_rowset(q[:nq], k, rs), *osearch(codes, a2, q[:nq], k, rows), (what, k, nq))
        rs.close()

    empty = idx.rowset(np.zeros(0, np.int64))
    assert len(empty) == 0 and not empty.is_bitmap
    for k in (10, 100):
        for nq in (1, 5, 33):
            D, I = idx.search_rowset(q[:nq], k, empty)
            assert (I == -1).all() and (D.view(np.uint32) == O.FLT_MAX.view(np.uint32)).all()
    empty.close()
    nothing_out = idx.rowset(np.zeros(0, np.int64), excluded=True)
    assert nothing_out.is_bitmap and len(nothing_out) == n
    for k in (10, 100):
        for nq in (1, 5, 33):
            check_equal(*idx.search_rowset(q[:nq], k, nothing_out), *idx.search(q[:nq], k), ("exclude nothing", k, nq))
    run(nothing_out, every, "exclude nothing")
    for one in (0, 517, n - 1):
        run(idx.rowset(np.delete(every, one), excluded=True), [one], ("all but one", one), ks=(1, 10, 100))
    run(idx.rowset([0, n - 1]), [0, n - 1], "both ends, list")
    run(idx.rowset([n - 1, 0, 64, 63, 960]), [0, 63, 64, 960, n - 1], "unsorted list")
    run(idx.rowset([0, n - 1], excluded=True), every[1:-1], "both ends excluded")
    # the list-or-bitmap switch at m * 8 >= n: the answers do not depend on the side
    for m in (n // 8 - 1, n // 8, -(-n // 8)):
        rows = np.union1d(rng.choice(np.arange(1, n - 1), m - 2, replace=False), [0, n - 1])
        rs = idx.rowset(rows)
        assert len(rows) == m and rs.is_bitmap == (m * 8 >= n) == C.rowset_is_bitmap(n, m, False)
        run(rs, rows, ("switch", m))
    assert not C.rowset_is_bitmap(n, n // 8 - 1, False) and C.rowset_is_bitmap(n, -(-n // 8), False)
    # k larger than the set: padding in fused mode (k <= 64) and after the radix select (k > 64)
    run(idx.rowset([3, 4, 5, 900, 1002]), [3, 4, 5, 900, 1002], "k above a list", ks=(10, 64, 65, 300))
    run(idx.rowset(np.delete(every, [3, 4, 5, 900, 1002]), excluded=True), [3, 4, 5, 900, 1002], "k above a bitmap",
        ks=(10, 64, 65, 300))
    wide = np.arange(0, n, 5)                                  # an included bitmap of 201 rows
    rs = idx.rowset(wide)
    assert rs.is_bitmap
    run(rs, wide, "k above an included bitmap", ks=(64, 250, 2000))
    D, I = idx.search(q[:5], 2000)                             # and k above the whole index
    check_equal(D, I, *O.search(codes, a2, q[:5], 2000), "k above the index")
    assert (I[:, n:] == -1).all() and (I[:, :n] >= 0).all()
    idx.close()


def test_rowset_device_entry_with_label_offset(gpu):
    import torch
    from minivectordb_amd import _native
    rng = np.random.default_rng(17)
    n, d = 9001, 200
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((33, d)).astype(np.float32)
    q[0] = x[n - 1]
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    few = np.union1d(rng.choice(n, 150, replace=False), [0, n - 1])
    half = np.union1d(rng.choice(n, n // 2, replace=False), [n - 1])
    tiny = np.array([n - 1, 5, 77])
    rs_few, rs_half, rs_tiny = idx.rowset(few), idx.rowset(half), idx.rowset(tiny)
    assert not rs_few.is_bitmap and rs_half.is_bitmap and not rs_tiny.is_bitmap
    stream = torch.cuda.Stream()
    off = 1000
    for rs, rows, nq, k, what in ((rs_few, few, 33, 10, "list"), (rs_few, few, 33, 100, "list, position mapping"),
                                  (rs_few, few, 1, 100, "list, one query"), (rs_half, half, 33, 10, "bitmap, matrix cores"),
                                  (rs_half, half, 3, 10, "bitmap, batch scan"), (rs_half, half, 3, 100, "bitmap, scores"),
                                  (rs_tiny, np.sort(tiny), 5, 10, "padding"), (rs_tiny, np.sort(tiny), 5, 100, "padding, mapped")):
        D, I = dev_search(idx, q[:nq], k, stream, rs=rs, label_offset=off)
        Do, Io = O.search(codes, a2, q[:nq], k, rows=rows)
        check_equal(D, I, Do, labelled(Io, off), what)
        if what.startswith("padding"):
            assert (I[:, 3:] == -1).all() and (I[:, :3] >= off).all()
    D, I = dev_search(idx, q, 100, stream, label_offset=off)
    Do, Io = O.search(codes, a2, q, 100)
    check_equal(D, I, Do, labelled(Io, off), "plain, scores, offset")
    for rs in (rs_few, rs_half, rs_tiny):
        rs.close()
    idx.close()


def test_after_reset(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(23)
    d = 72
    x = rng.standard_normal((3000, d)).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x)
    rs_list, rs_map = idx.rowset([1, 2, 3]), idx.rowset([1, 2, 3], excluded=True)
    idx.reset()
    assert idx.ntotal == 0
    for rs in (rs_list, rs_map):
        with pytest.raises(ValueError):
            idx.search_rowset(x[:3], 5, rs)
    for nq, k in ((1, 5), (5, 5), (33, 5), (5, 100)):
        D, I = idx.search(x[:nq], k)
        check_equal(D, I, *missing(nq, k), ("empty after reset", nq, k))
    with pytest.raises(ValueError):
        idx.get_codes(0, 1)
    idx.add(x[1000:1700])
    codes, a2 = idx.get_codes(0, 700)
    oc, oa = O.quantize(x[1000:1700])
    assert idx.ntotal == 700 and np.array_equal(codes, oc) and np.array_equal(a2, oa)
    D, I = idx.search(x[1000:1033], 5)
    check_equal(D, I, *O.search(codes, a2, x[1000:1033], 5), "after reset and add")
    assert (I[:, 0] == np.arange(33)).all()
    for rs in (rs_list, rs_map):                               # still refused: the rows were renumbered
        with pytest.raises(ValueError):
            idx.search_rowset(x[:3], 5, rs)
        rs.close()
    rs = idx.rowset([0, 699])
    check_equal(*idx.search_rowset(x[1000:1005], 5, rs), *O.search(codes, a2, x[1000:1005], 5, rows=[0, 699]), "new set")
    rs.close()
    idx.close()


# ---- 4. tie-heavy and gate-hostile corpora --------------------------------------------------------------------------
def oracle_distances(codes, a2, q):
    """O.distance over every row, eight queries at a time (the fp64 temporaries of a million rows are large)."""
    qc, qb2 = O.quantize(q)
    return np.concatenate([O.distance(O.dots(qc[i:i + 8], codes), a2, qb2[i:i + 8]) for i in range(0, q.shape[0], 8)])


@pytest.mark.parametrize("n,d", [(1_000_000, 2), (1_000_000, 3), (200_000, 4)])
def test_tie_heavy(gpu, n, d):
    """A corpus with a few thousand distinct codes: every k-th place falls inside a tie group of hundreds or thousands of
    rows, and "ties to the lower row" must hold across lanes, waves, blocks and the merge."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(n + d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((32, d)).astype(np.float32)
    q[0] = x[n - 1]
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    dist = oracle_distances(codes, a2, q)
    if d == 2:
        tenth = np.partition(dist[1], 9)[9]
        assert (dist[1] == tenth).sum() > 500                  # the premise: the 10th place lies in a large tie group
    first = np.unique(O.topk_from_distances(dist, 3)[1])       # the best hits leave, and a thousand other rows
    gone = np.union1d(first, rng.choice(n, 1000, replace=False))
    keep = np.setdiff1d(np.arange(n), gone)
    rs = idx.rowset(gone, excluded=True)
    dist_keep = dist[:, keep]
    for k in (1, 10, 64, 100):
        Do, Io = O.topk_from_distances(dist, k)
        Dx, Ix = O.topk_from_distances(dist_keep, k, keep)
        for nq in (1, 5, 32):
            check_equal(*idx.search(q[:nq], k), Do[:nq], Io[:nq], ("ties", n, d, k, nq))
            check_equal(*idx.search_rowset(q[:nq], k, rs), Dx[:nq], Ix[:nq], ("ties, excluded", n, d, k, nq))
    rs.close()
    idx.close()


@pytest.mark.parametrize("order", ["falling", "rising"])
def test_gate_hostile(gpu, order):
    """Rows q0 + s_r * noise.  s_r falling with the row number: every row beats the list so far, so the fp32 estimate gate
    stays open and the exact distance and the insert run for every row.  Rising: the gate closes after the first rows."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(41)
    n, d = 50_000, 512
    q0 = rng.standard_normal(d).astype(np.float32)
    s = np.linspace(2.0, 0.02, n) if order == "falling" else np.linspace(0.02, 2.0, n)
    x = (q0[None, :] + s[:, None].astype(np.float32) * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    q = (q0[None, :] + np.float32(0.05) * rng.standard_normal((40, d)).astype(np.float32)).astype(np.float32)
    q[0] = q0
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    gone = np.arange(0, n, 7)
    rs = idx.rowset(gone, excluded=True)
    keep = np.setdiff1d(np.arange(n), gone)
    for k in (10, 64):
        Do, Io = O.search(codes, a2, q, k)
        Dx, Ix = O.search(codes, a2, q, k, rows=keep)
        if order == "falling":
            assert Io[0].min() > n - 2000
        for nq in (1, 5, 40):
            check_equal(*idx.search(q[:nq], k), Do[:nq], Io[:nq], (order, k, nq))
            check_equal(*idx.search_rowset(q[:nq], k, rs), Dx[:nq], Ix[:nq], (order, "excluded", k, nq))
    rs.close()
    idx.close()


# ---- 5. lifecycle ---------------------------------------------------------------------------------------------------
def test_graph_replay_after_workspace_growth(gpu):
    """A captured search keeps the workspace buffers it was captured with: a later eager call on the same stream that needs
    larger ones must not free them under the graph."""
    import torch
    from minivectordb_amd import _native
    rng = np.random.default_rng(31)
    n, d = 20001, 128
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((64, d)).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    few = np.union1d(rng.choice(n, 400, replace=False), [0, n - 1])
    rs = idx.rowset(few)
    stream = torch.cuda.Stream()
    off = 1000

    def buffers(nq, k):
        return (torch.from_numpy(q[:nq].copy()).cuda(), torch.zeros((nq, k), dtype=torch.float32, device="cuda"),
                torch.zeros((nq, k), dtype=torch.int64, device="cuda"))

    def enqueue(qt, Dt, It, nq, k, rowset):
        if rowset is None:
            idx.search_device(qt.data_ptr(), nq, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream, label_offset=off)
        else:
            idx.search_rowset_device(qt.data_ptr(), nq, k, rowset, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream,
                                     label_offset=off)

    def eager(bufs, nq, k, rowset, rows, what):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue(*bufs, nq, k, rowset)
        stream.synchronize()
        Do, Io = O.search(codes, a2, q[:nq], k, rows=rows)
        check_equal(bufs[1].cpu().numpy(), bufs[2].cpu().numpy(), Do, labelled(Io, off), what)
        return Do, labelled(Io, off)

    def capture(bufs, nq, k, rowset):
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue(*bufs, nq, k, rowset)
        return g

    def replay(g, bufs, want, what):
        bufs[1].zero_()
        bufs[2].zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_equal(bufs[1].cpu().numpy(), bufs[2].cpu().numpy(), *want, what)

    small = buffers(4, 10)
    want_small = eager(small, 4, 10, None, None, "eager 4 x 10")
    g1 = capture(small, 4, 10, None)
    replay(g1, small, want_small, "first replay")
    big = buffers(64, 64)                                       # larger query codes and candidate lists
    eager(big, 64, 64, None, None, "eager 64 x 64")
    wide = buffers(9, 100)                                      # the score matrix and the select's keys appear
    eager(wide, 9, 100, None, None, "eager 9 x 100")
    replay(g1, small, want_small, "replay after the workspace grew")
    listed = buffers(5, 100)
    want_listed = eager(listed, 5, 100, rs, few, "eager row set 5 x 100")
    g2 = capture(listed, 5, 100, rs)
    replay(g2, listed, want_listed, "row set replay")
    bigger = buffers(64, 100)
    eager(bigger, 64, 100, None, None, "eager 64 x 100")
    replay(g2, listed, want_listed, "row set replay after the workspace grew")
    replay(g1, small, want_small, "first graph, third replay")
    del g1, g2
    torch.cuda.synchronize()
    rs.close()
    idx.close()


def test_growth_through_small_adds(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(37)
    d = 24
    sizes = [1, 1022, 1, 2, 511, 1537, 1, 1, 1535, 2305, 1]    # across the first 1024 rows and each 1.5 x step after it
    x = rng.standard_normal((sum(sizes), d)).astype(np.float32)
    oc, oa = O.quantize(x)
    idx = _native.Cos8Index(d)
    at = 0
    for m in sizes:
        idx.add(x[at:at + m])
        at += m
        assert idx.ntotal == at
        codes, a2 = idx.get_codes(0, at)
        assert np.array_equal(codes, oc[:at]) and np.array_equal(a2, oa[:at]), (m, at)
    check_equal(*idx.search(x[:9], 10), *O.search(oc, oa, x[:9], 10), "after many adds")
    idx.close()


def test_three_upload_chunks_at_the_widest_row(gpu):
    """mvdb_cos8_add uploads 64 MiB at a time: 4,096 rows of d = 4096, so 9,000 rows go up in three pieces."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(43)
    n, d = 9000, 4096
    x = rng.standard_normal((n, d), dtype=np.float32)
    x[4096] = x[4095]
    x[8192] = x[0]
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    oc, oa = O.quantize(x)
    bad = np.nonzero((codes != oc).any(axis=1) | (a2 != oa))[0]
    assert bad.size == 0, bad[:10]
    q = np.stack([x[0], x[4095], x[8999], x[4097], x[8191]])
    for k in (10, 100):
        check_equal(*idx.search(q, k), *O.search(codes, a2, q, k), ("three chunks", k))
    idx.close()


def test_remove_rows_edges(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(47)
    n, d = 2050, 56
    x = rng.standard_normal((n, d)).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)

    def same(keep, what):
        assert idx.ntotal == len(keep), what
        if len(keep):
            c, a = idx.get_codes(0, len(keep))
            assert np.array_equal(c, codes[keep]) and np.array_equal(a, a2[keep]), what
            for nq, k in ((1, 10), (5, 10), (33, 10), (5, 100)):
                check_equal(*idx.search(x[:nq], k), *O.search(codes[keep], a2[keep], x[:nq], k), (what, nq, k))

    keep = np.arange(n)
    for bad in ([5, 5], [n], [-1], [0, n - 1, n], [7, 3, 7]):   # refused whole: nothing moves
        with pytest.raises(ValueError):
            idx.remove_rows(bad)
        same(keep, ("refused", bad))
    idx.remove_rows([n - 1])
    keep = keep[:-1]
    same(keep, "last row")
    idx.remove_rows([0])
    keep = keep[1:]
    same(keep, "row 0")
    with pytest.raises(ValueError):
        idx.remove_rows([len(keep)])
    same(keep, "refused after removals")
    idx.remove_rows(np.arange(idx.ntotal)[::-1])                # every row, listed backwards
    assert idx.ntotal == 0
    for nq, k in ((1, 10), (5, 10), (33, 10), (5, 100)):
        check_equal(*idx.search(x[:nq], k), *missing(nq, k), ("empty", nq, k))
    with pytest.raises(ValueError):
        idx.remove_rows([0])
    idx.add(x[100:164])
    c, a = idx.get_codes(0, 64)
    assert np.array_equal(c, codes[100:164]) and np.array_equal(a, a2[100:164])
    D, I = idx.search(x[100:133], 5)
    check_equal(D, I, *O.search(c, a, x[100:133], 5), "add after removing every row")
    assert (I[:, 0] == np.arange(33)).all()
    idx.close()
