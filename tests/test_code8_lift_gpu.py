"""The bit plane of the int8 code and the lift of the prefilter's front form ("The bit plane")
against the same index without the plane, at the smallest size the route serves.

With the plane of bit 2 the front form of `code8_scan_kernel` stages (row, T5, a, r) for the rows its stage 0 cannot reject
and lifts their T6 = T5 + 4 Q . b2 from d / 8 bytes of that plane (its loads behind the stream's), where it used to gather
their 3 d / 4 bytes of the 6-bit plane and their (a, r) entry.  The same rows reach stage 1 with the same T6 and (a, r): the
stage-0 survivors, the refined rows, the candidates and (D, I) of every query are what they are with option
"code8_bit_plane" = 0 in the same build.  What can go wrong is what these cases plant: families whose stage fills never,
sometimes and all the time (1), rows where the staging's indexing can go wrong (2), every writer of the plane (3), the two
options that free a plane each (4), a captured stream (5).  The front form is pinned on ("code8_front_plane" = 2): the
all-positive family would otherwise suspend it, and d = 1024 does not stream the plane by default."""
import numpy as np
import pytest

from oracle import flat

import test_code8_planes_gpu as PG

DIMS = PG.DIMS
FAMILIES = PG.FAMILIES
N = 500_001   # the route's smallest eligible size plus one: the partial batch is taken


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _exact(idx, qs, k):
    idx.set_option("code8_single_query", 0)
    want = [idx.search(q, k) for q in qs]
    idx.set_option("code8_single_query", 1)
    return want


def _warm(idx, q, k=10):
    for _ in range(3):   # (the exact scan answers the first eligible queries after a change; the third builds the code)
        idx.search(q, k)
    assert idx.code8_rows == idx.ntotal


def _routed(native, idx, qs, k, want, plane, what):
    """The queries through the front form: bit-equal to `want`, the plane held or not as asked, no fallback; returns per
    query (stage-0 survivors, rows refined, candidates)."""
    assert idx.code8_bit_plane_held() == plane and idx.code8_front_counters()[3], what
    fallbacks = idx.code8_counters()[0]
    out = []
    native.prof_enable(True)
    try:
        for q, w in zip(qs, want):
            s0, c0 = idx.code8_front_counters()[:2]
            r0 = idx.code8_refined()
            D, I = idx.search(q, k)
            sym = native.prof_symbol("ip_scan")
            assert sym.startswith("code8_scan_kernel<") and sym.count(",") == 4, (what, sym)   # (the front form, five arguments)
            s1, c1 = idx.code8_front_counters()[:2]
            assert c1 - c0 == 1, what
            assert np.array_equal(D.view(np.uint32), w[0].view(np.uint32)), (what, D, w[0])
            assert np.array_equal(I, w[1]), (what, I, w[1])
            out.append((s1 - s0, idx.code8_refined() - r0, int(idx.code8_counters()[1])))
    finally:
        native.prof_enable(False)
    assert idx.code8_counters()[0] == fallbacks, what
    return out


def _bits_match_code(native, idx, rows, what):
    for r in rows:
        high, low, _ = idx.code8_read_row(int(r), front=False)
        c = native.code8_unpack(high, low)
        assert np.array_equal(idx.code8_read_bit2(int(r)), native.code8_bit2_pack(c)), (what, r)


# ---- 1. the three families, with the plane and without it ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_families_with_and_without_the_plane(native, family, d):
    """(the all-positive family keeps a third to two thirds of the rows at stage 0 — more per batch than one lift takes away
    at d = 384 and 1024, about as many at d = 512: waves fill their 64 slots with a lift in flight; test_planted_survivors
    makes one wave do so for certain)"""
    flag = FAMILIES[family]
    idx = PG._index(native, d, N, flag)
    qs = list(PG._query(d, flag, nq=8))
    idx.set_option("code8_front_plane", 2)
    want = {k: _exact(idx, qs, k) for k in (1, 10, 64)}
    got = {}
    for plane in (1, 0):
        idx.set_option("code8_bit_plane", plane)
        _warm(idx, qs[0])
        got[plane] = {k: _routed(native, idx, qs, k, want[k], bool(plane), f"{family} d={d} plane={plane} k={k}") for k in (1, 10, 64)}
    print(f"code8 lift {family} d={d}: (survivors, refined, candidates) at k = 10: {got[1][10]}")
    assert got[1] == got[0], (family, d, got)
    assert all(s >= r for per_k in got[1].values() for (s, r, c) in per_k)
    idx.close()


# ---- 2. planted survivors ------------------------------------------------------------------------------------------------------------
def _planted(native, d, n):
    """Rows where the staging's indexing can go wrong: row 0, the last row of a tile of the front plane and the first of the
    next, 80 consecutive rows of ONE wave's batches starting a quarter into a batch (the wave's 64 slots fill in the middle
    of a batch, with a lift in flight), the last rows (the partial batch where there is one) and row n - 1."""
    rb, waves = native.code8_front_geometry(d, n)
    tile = {384: 4, 512: 16, 1024: 2}[d]
    edge = [0, 1000 * tile - 1, 1000 * tile, n - 3, n - 2, n - 1]
    w, skip = 7, rb // 4
    dense = [(w + j * waves) * rb + i for j in range(80 // rb + 2) for i in range(rb)][skip:skip + 80]
    assert len(dense) == 80 and max(dense) < n // rb * rb and not set(dense) & set(edge)
    if n % rb >= 3:
        assert min(edge[3:]) >= n // rb * rb
    return edge, dense


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_planted_survivors(native, d):
    k = 64
    edge, dense = _planted(native, d, N)
    q = PG._query(d)
    # scaled copies of the query: the edge rows on top, the dense rows behind them, all far above the synthetic rows
    x = np.stack([np.float32(1.0 - j * 2.0 ** -12) * q for j in range(len(edge))] +
                 [np.float32(0.9 - j * 2.0 ** -12) * q for j in range(len(dense))]).astype(np.float32)
    idx = PG._index(native, d, N)
    idx.set_option("code8_front_plane", 2)
    idx.set_rows(np.asarray(edge + dense, dtype=np.int64), x)
    _warm(idx, q)
    want = _exact(idx, [q], k)
    with_plane = _routed(native, idx, [q], k, want, True, f"planted d={d}")
    first = want[0][1].reshape(-1).tolist()
    assert first[:len(edge)] == edge and set(first) <= set(edge + dense), (d, first)
    _bits_match_code(native, idx, edge + dense, f"planted d={d}")
    # the 86 planted rows are more than one call returns: the ones that came back are zeroed, the others must come back now
    idx.set_rows(np.asarray(first, dtype=np.int64), np.zeros((len(first), d), np.float32))
    want2 = _exact(idx, [q], k)
    _routed(native, idx, [q], k, want2, True, f"planted d={d}, second call")
    rest = [r for r in edge + dense if r not in set(first)]
    second = want2[0][1].reshape(-1).tolist()
    assert second[:len(rest)] == rest, (d, second, rest)
    _bits_match_code(native, idx, first[:8] + rest[:8], f"planted d={d}, zeroed")
    # and without the plane, on the first state again: the same counts
    idx.set_rows(np.asarray(edge + dense, dtype=np.int64), x)
    again = _routed(native, idx, [q], k, want, True, f"planted d={d}, again")
    idx.set_option("code8_bit_plane", 0)
    without = _routed(native, idx, [q], k, want, False, f"planted d={d}, no plane")
    assert with_plane == again == without, (d, with_plane, again, without)
    assert with_plane[0][0] >= len(edge) + len(dense)
    idx.close()


# ---- 3. every writer of the plane ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_writers(native, d):
    n, k = N, 10
    idx = PG._index(native, d, n, spare=64)
    idx.set_option("code8_front_plane", 2)
    q = PG._query(d)
    rs = np.random.default_rng(d)
    copies = np.stack([np.float32(1.0 - j * 2.0 ** -10) * q for j in range(8)]).astype(np.float32)

    def check(what, top, extra=(), warm=False):
        if warm:
            _warm(idx, q)
        want = _exact(idx, [q], k)
        _routed(native, idx, [q], k, want, True, what)
        assert want[0][1].reshape(-1)[:len(top)].tolist() == list(top), (what, want[0][1], top)
        m = idx.ntotal
        probe = [0, 1, 15, 16, 17, m - 1, m - 2, m - 3] + rs.integers(0, m, 12).tolist() + list(top) + list(extra)
        _bits_match_code(native, idx, probe, what)

    check("fresh", [], warm=True)
    # add into reserved space: 37 rows, planted ones among them
    extra = flat.synth(37, d, 99)
    flat.normalize_l2(extra)
    extra[0], extra[36] = copies[0], copies[1]
    idx.add(extra)
    assert idx.code8_rows == idx.ntotal == n + 37 and idx.code8_bit_plane_held()
    check("add 37", [n, n + 36], extra=range(n, n + 37))
    # set_rows over planted rows (the list form of the build), a row of the floor's sample among them
    slot_row = (33_333 * (n + 37)) // PG.SEED
    idx.set_rows(np.array([n, 5, slot_row, n + 36], np.int64), copies[2:6])
    check("set_rows", [n, 5, slot_row, n + 36], extra=[n, 5, slot_row, n + 36])
    # remove_rows empties the code; the third query rebuilds it, the plane with it
    idx.remove_rows(np.array([3, n + 36], np.int64))
    assert idx.code8_rows == 0
    check("remove_rows", [n - 1, 4, slot_row - 1], warm=True)
    # a reserve that reallocates: the code is dropped with the matrix' allocation, the plane with the code
    idx.reserve(idx.ntotal + 100_000)
    assert idx.code8_rows == 0 and not idx.code8_bit_plane_held()
    check("reserve", [n - 1, 4, slot_row - 1], warm=True)
    idx.close()


# ---- 4. the options --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_options(native):
    import torch
    n, d, k = N, 512, 10
    idx = PG._index(native, d, n)
    idx.set_option("code8_front_plane", 2)
    qs = list(PG._query(d, nq=4))
    want = _exact(idx, qs, k)
    _warm(idx, qs[0])
    _routed(native, idx, qs, k, want, True, "options: fresh")

    def freed_by(option, value):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        idx.set_option(option, value)
        return torch.cuda.mem_get_info(0)[0] - free0

    # code8_bit_plane = 0 frees the plane alone: d / 8 bytes per row of the capacity; the front form gathers again
    freed = freed_by("code8_bit_plane", 0)
    assert n * d // 8 - (2 << 20) <= freed <= n * d // 8 + (2 << 20), freed
    assert not idx.code8_bit_plane_held() and idx.code8_front_counters()[3] and idx.code8_rows == n
    _routed(native, idx, qs, k, want, False, "options: no bit plane")
    # = 1 again: the code is rebuilt with the plane by the next eligible query
    idx.set_option("code8_bit_plane", 1)
    assert idx.code8_rows == 0
    _warm(idx, qs[0])
    _routed(native, idx, qs, k, want, True, "options: bit plane again")
    # code8_front_plane = 0 still frees the front plane only (whole tiles of 5 d / 8 bytes per row); the bit plane stays
    freed = freed_by("code8_front_plane", 0)
    plane = (n + 15) // 16 * 16 * (5 * d // 8)
    assert plane - (2 << 20) <= freed <= plane + (2 << 20), (freed, plane)
    assert idx.code8_bit_plane_held() and not idx.code8_front_counters()[3] and idx.code8_rows == n
    for q, w in zip(qs, want):
        D, I = idx.search(q, k)
        assert np.array_equal(D.view(np.uint32), w[0].view(np.uint32)) and np.array_equal(I, w[1])
    _bits_match_code(native, idx, [0, 1, n - 1], "options: no front plane")
    # the front plane again: a code without it is dropped, the next eligible query builds all planes
    idx.set_option("code8_front_plane", 2)
    assert idx.code8_rows == 0 and not idx.code8_bit_plane_held()
    _warm(idx, qs[0])
    _routed(native, idx, qs, k, want, True, "options: both again")
    _bits_match_code(native, idx, [0, 1, n - 1], "options: both again")
    with pytest.raises(Exception):
        idx.set_option("code8_bit_plane", 2)
    idx.close()


# ---- 5. a captured stream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_with_the_lift(native):
    import torch
    n, d, k = N, 512, 10
    idx = PG._index(native, d, n)
    qs = list(PG._query(d, nq=4))
    want = _exact(idx, qs, k)
    idx.set_option("code8_front_plane", 2)
    stream = torch.cuda.Stream()
    qt = torch.zeros(d, dtype=torch.float32, device="cuda")
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    # eager calls build the code with its planes and size the workspace; the capture records the front form with the lift
    qt.copy_(torch.from_numpy(qs[0]))
    with torch.cuda.stream(stream):
        for _ in range(4):
            enqueue()
    stream.synchronize()
    assert idx.code8_rows == n and idx.code8_front_counters()[3] and idx.code8_bit_plane_held()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    before = idx.code8_front_counters()[1]
    for i in range(4):
        qt.copy_(torch.from_numpy(qs[i]))
        Dt.zero_()
        It.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[i][0][0].view(np.uint32)), i
        assert np.array_equal(It.cpu().numpy(), want[i][1][0]), i
    assert idx.code8_front_counters()[1] - before == 4   # every replay ran the front form
    del g
    idx.close()
