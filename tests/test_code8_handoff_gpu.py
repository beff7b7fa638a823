"""The survivor wave of the int8 prefilter's front form ("The survivor wave") against the same launch
without it, at the smallest size the route serves.

With `MVDB_CODE8_HANDOFF=2` the quad front form with the lift runs five waves per block: four stream the front plane and
hand the rows stage 0 cannot reject to a ring in LDS, the fifth takes them from there through the lift, stage 1, the
refinement and the appends.  A batch whose reservation the ring refuses goes the parent's way, inline on the streaming
wave.  Whichever wave takes a row, it meets the same arithmetic with the same (T5, a, r): per call the stage-0 survivors,
the refined rows, the candidates, the fallback counter and the bits of (D, I) are what `MVDB_CODE8_HANDOFF=1` — the parent's
instantiation — gives in the same build.  What can go wrong is what these cases plant: rings that are never, sometimes and
nearly always full (1), bursts longer than a small ring and the partial batch (2), a floor that rejects nothing (3), a
captured stream (4), two streams in one index (5).  The label of the launch keeps its five arguments in both forms, so the
cells are told apart by the hook alone.  The front form is pinned on ("code8_front_plane" = 2): the all-positive family would
otherwise suspend it."""
import contextlib
import os

import numpy as np
import pytest

import test_code8_planes_gpu as PG

FAMILIES = PG.FAMILIES
N, D = 500_001, 512   # the route's smallest eligible size plus one: the partial batch is taken, every wave has batches
HOOKS = ("MVDB_CODE8_HANDOFF", "MVDB_CODE8_RING")
OFF = (1, 0)
CELLS = (OFF, (2, 0), (2, 64), (2, 4096))   # (hand-off hook, ring entries; 0: the default ring)


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


@contextlib.contextmanager
def _cell(idx, handoff, ring):
    old = {name: os.environ.get(name) for name in HOOKS}
    try:
        for name, v in zip(HOOKS, (handoff, ring)):
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


def _exact(idx, qs, k):
    idx.set_option("code8_single_query", 0)
    want = [idx.search(q, k) for q in qs]
    idx.set_option("code8_single_query", 1)
    return want


def _warm(idx, q, k=10):
    for _ in range(3):   # (the exact scan answers the first eligible queries after a change; the third builds the code)
        idx.search(q, k)
    assert idx.code8_rows == idx.ntotal and idx.code8_bit_plane_held() and idx.code8_front_counters()[3]


def _routed(native, idx, qs, k, want, what):
    """The queries through the front form with the lift: bit-equal to `want`; returns per query (stage-0 survivors, rows
    refined, candidates, fallbacks added)."""
    out = []
    native.prof_enable(True)
    try:
        for q, w in zip(qs, want):
            s0, c0 = idx.code8_front_counters()[:2]
            r0 = idx.code8_refined()
            f0 = idx.code8_counters()[0]
            Dg, Ig = idx.search(q, k)
            sym = native.prof_symbol("ip_scan")
            assert sym.startswith("code8_scan_kernel<") and sym.count(",") == 4, (what, sym)   # (the front form, five arguments)
            s1, c1 = idx.code8_front_counters()[:2]
            assert c1 - c0 == 1, what
            assert np.array_equal(Dg.view(np.uint32), w[0].view(np.uint32)), (what, Dg, w[0])
            assert np.array_equal(Ig, w[1]), (what, Ig, w[1])
            out.append((s1 - s0, idx.code8_refined() - r0, int(idx.code8_counters()[1]), idx.code8_counters()[0] - f0))
    finally:
        native.prof_enable(False)
    return out


def _open(native, flag=0):
    idx = PG._index(native, D, N, flag)
    idx.set_option("code8_front_plane", 2)
    return idx


@pytest.fixture(scope="module")
def families(native):
    """One index per family with its eight queries and their exact results per k (computed once, never changed)."""
    held = {}

    def get(family):
        if family not in held:
            flag = FAMILIES[family]
            idx = _open(native, flag)
            qs = list(PG._query(D, flag, nq=8))
            want = {k: _exact(idx, qs, k) for k in (1, 10, 64)}
            _warm(idx, qs[0])
            held[family] = (idx, qs, want)
        return held[family]

    yield get
    for idx, _, _ in held.values():
        idx.close()


# ---- 1. the forms agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_forms_agree(native, families, family, k):
    """(the all-positive family keeps a third to two thirds of the rows at stage 0: at ring 64 most reservations are refused
    and the streaming waves drain inline beside the fifth wave; the clustered family hands over next to nothing)"""
    idx, qs, want = families(family)
    got = {}
    for cell in CELLS:
        with _cell(idx, *cell):
            got[cell] = _routed(native, idx, qs, k, want[k], f"{family} k={k} handoff={cell[0]} ring={cell[1]}")
    print(f"code8 hand-off {family} k={k}: (survivors, refined, candidates, fallbacks) {got[OFF]}")
    for cell in CELLS[1:]:
        assert got[cell] == got[OFF], (family, k, cell, got[cell], got[OFF])
    assert all(s >= r for (s, r, c, f) in got[OFF])


# ---- 2. bursts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bursts(native):
    """2,048 consecutive survivors from a row that is no multiple of 32 — 64 whole batches and two split ones, more than a
    ring of 64 holds and more than its wave takes away meanwhile — and row n - 1 in the partial batch."""
    k, first, burst = 64, 100_013, 2048
    assert first % 32 and N % 32
    q = PG._query(D)
    rows = [N - 1] + list(range(first, first + burst))
    # scaled copies of the query 2^-20 apart: the last scores 0.998 of the first, far inside the margin of stage 0 (the residual
    # bound of such a row alone is several thousandths), so every one of them survives it whatever the sample makes the floor
    x = np.stack([np.float32(1.0 - j * 2.0 ** -20) * q for j in range(len(rows))]).astype(np.float32)
    idx = _open(native)
    idx.set_rows(np.asarray(rows, dtype=np.int64), x)
    _warm(idx, q)
    want = _exact(idx, [q], k)
    assert set(want[0][1].reshape(-1).tolist()) <= set(rows)   # planted rows only; _routed holds the route to the exact scan's order
    got = {}
    for cell in (OFF, (2, 64), (2, 0)):
        with _cell(idx, *cell):
            got[cell] = _routed(native, idx, [q], k, want, f"bursts handoff={cell[0]} ring={cell[1]}")
    assert got[(2, 64)] == got[OFF] and got[(2, 0)] == got[OFF], got
    assert got[OFF][0][0] >= len(rows) and got[OFF][0][3] == 0, got
    idx.close()


# ---- 3. everything passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ring", [64, 0])
def test_everything_passes(native, families, ring):
    """The zero query: its floor rejects nothing, every row survives both stages on whichever wave meets it, the candidates
    overflow and the call falls back once."""
    idx, qs, want = families("zero_mean")
    zero = np.zeros(D, np.float32)
    want_zero = _exact(idx, [zero], 10)
    with _cell(idx, *OFF):
        off = _routed(native, idx, [zero], 10, want_zero, "zero query, off")
    with _cell(idx, 2, ring):
        on = _routed(native, idx, [zero], 10, want_zero, f"zero query, ring={ring}")
        after = _routed(native, idx, qs[:1], 10, want[10][:1], f"the query behind the zero query, ring={ring}")
    assert on == off and on[0][0] == N and on[0][1] == N and on[0][2] == N and on[0][3] == 1, (on, off)
    assert after[0][3] == 0, after


# ---- 4. a captured stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_with_the_survivor_wave(native, families):
    import torch
    k = 10
    idx, qs, want = families("zero_mean")
    stream = torch.cuda.Stream()
    qt = torch.zeros(D, dtype=torch.float32, device="cuda")
    Dt = torch.zeros(k, dtype=torch.float32, device="cuda")
    It = torch.zeros(k, dtype=torch.int64, device="cuda")

    def enqueue():
        idx.search_device(qt.data_ptr(), 1, k, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream)

    with _cell(idx, 2, 0):
        # eager calls size this stream's workspace; the capture records the hand-off form
        qt.copy_(torch.from_numpy(qs[0]))
        with torch.cuda.stream(stream):
            for _ in range(2):
                enqueue()
        stream.synchronize()
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
        assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[k][i][0][0].view(np.uint32)), i
        assert np.array_equal(It.cpu().numpy(), want[k][i][1][0]), i
    assert idx.code8_front_counters()[1] - before == 4   # every replay ran the front form
    del g


# ---- 5. two streams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_streams(native, families):
    import torch
    k, calls = 10, 8
    idx, qs, want = families("zero_mean")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    qd = torch.from_numpy(np.stack(qs)).to("cuda")
    Dt = torch.zeros((2, calls, k), dtype=torch.float32, device="cuda")
    It = torch.zeros((2, calls, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with _cell(idx, 2, 0):
        for i in range(calls):
            for s, stream in enumerate(streams):
                j = (i + 3 * s) % len(qs)
                idx.search_device(qd[j].data_ptr(), 1, k, Dt[s, i].data_ptr(), It[s, i].data_ptr(), stream=stream.cuda_stream)
        for stream in streams:
            stream.synchronize()
    Dh, Ih = Dt.cpu().numpy(), It.cpu().numpy()
    for i in range(calls):
        for s in range(2):
            j = (i + 3 * s) % len(qs)
            assert np.array_equal(Dh[s, i].view(np.uint32), want[k][j][0][0].view(np.uint32)), (s, i)
            assert np.array_equal(Ih[s, i], want[k][j][1][0]), (s, i)
