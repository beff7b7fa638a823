"""The front plane of the int8 code and the front form of the prefilter against the same index with
the route off and with the other form of the kernel, at the smallest sizes the route serves.

The front form of `code8_scan_kernel` streams the plane of the top 5 bits of every code, stages the rows its stage 0 cannot
reject, gathers their chunks of the 6-bit plane and hands them to the two stages of the other form.  Which form ran may change
the time, never the candidates or the results.  Option "code8_front_plane": 1 the library decides (a window over the share
of staged rows), 2 always the front form, 3 the plane kept and never streamed, 0 no plane.  What can go wrong is what these
cases plant: rows that differ only in the bit the front plane lacks and the 6-bit plane has (2), a wave whose stage fills
several times and ends exactly full (3), every writer of the plane (4), the switch (5), a captured stream (6)."""
import json

import numpy as np
import pytest

from oracle import flat

import test_code8_planes_gpu as PG

DIMS = PG.DIMS
FAMILIES = PG.FAMILIES
SEED = PG.SEED


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _sizes(native, d):
    """The smallest size the route serves plus one (the partial batch is taken), and one row short of one batch more."""
    rb, _ = native.code8_front_geometry(d, 500_001)
    return (500_001, 500_000 + rb - 1)


def _exact(idx, qs, k):
    idx.set_option("code8_single_query", 0)
    want = [idx.search(q, k) for q in qs]
    idx.set_option("code8_single_query", 1)
    return want


def _routed(native, idx, qs, k, want, form, what, warm=3):
    """The queries through the route with the given value of code8_front_plane: bit-equal to `want`, the form asserted,
    no fallback; returns the candidate counts."""
    idx.set_option("code8_front_plane", form)
    for _ in range(warm):   # (the exact scan answers the first eligible queries after a change; the third builds the code)
        idx.search(qs[0], k)
    fallbacks = idx.code8_counters()[0]
    counts = []
    native.prof_enable(True)
    try:
        for q, w in zip(qs, want):
            native.prof_read("ip_scan")
            D, I = idx.search(q, k)
            sym = native.prof_symbol("ip_scan")
            assert sym.startswith("code8_scan_kernel<"), (what, sym)
            assert (sym.count(",") == 4) == (form in (1, 2)), (what, form, sym)   # (the front form names its two arguments more)
            assert native.prof_read("ip_scan")[0] == 1, what
            assert np.array_equal(D.view(np.uint32), w[0].view(np.uint32)), (what, form, D, w[0])
            assert np.array_equal(I, w[1]), (what, form, I, w[1])
            counts.append(int(idx.code8_counters()[1]))
    finally:
        native.prof_enable(False)
    assert idx.code8_rows == idx.ntotal, what
    assert idx.code8_front_counters()[3] == (form != 0), what
    assert idx.code8_counters()[0] == fallbacks, what
    return counts


# ---- 1. results and candidates in every form -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_results_and_candidate_counts_in_every_form(native, family, d):
    with open(PG.GOLDEN) as f:
        golden = json.load(f)[f"{family}/{d}"]
    flag, k = FAMILIES[family], 10
    for n in _sizes(native, d):
        idx = PG._index(native, d, n, flag)
        qs = list(PG._query(d, flag, nq=8))
        want = _exact(idx, qs, k)
        counts = {form: _routed(native, idx, qs, k, want, form, f"{family} d={d} n={n} form={form}") for form in (2, 3, 0)}
        print(f"code8 front {family} d={d} n={n}: candidates {counts[2]}, stage-0 survivors so far {idx.code8_front_counters()[0]}")
        assert counts[2] == counts[3] == counts[0], (family, d, n, counts)
        if n == 500_001:
            assert counts[2] == golden, (family, d, counts[2], golden)
        idx.close()


# ---- 2. rows that differ only in the bit the front plane lacks ---------------------------------------------------------------------
def _bit2_variants(q, m):
    """m rows a * c_j whose codes agree with the codes of q except in bit 2 (c & 4) of a random half of the elements: the front
    plane of all of them is the same, the 6-bit plane tells them apart."""
    d = q.shape[0]
    top = int(np.argmax(np.abs(q)))
    a = np.float32(np.abs(q[top]) / np.float32(127))
    c = np.clip(np.rint(q / a), -127, 127).astype(np.int64)
    rows = []
    for j in range(m):
        flip = np.random.default_rng(300 + j).integers(0, 2, d) * 4
        cj = (c & ~4) | flip
        cj = np.where(cj == -128, -124, cj)                   # (-128 is no code)
        cj[top] = c[top]                                      # the scale stays
        rows.append((cj * np.float64(a)).astype(np.float32))
    rows = np.stack(rows)
    back = np.clip(np.rint(rows / (np.abs(rows).max(axis=1, keepdims=True) / np.float32(127))), -127, 127).astype(np.int64)
    keep = np.ones(d, bool)
    keep[top] = False
    assert ((back & ~7)[:, keep] == (c & ~7)[keep]).all() and len({r.tobytes() for r in (back & 4)}) == m
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_rows_that_differ_only_in_the_bit_the_front_plane_lacks(native, d):
    """Planted as test_code8_planes_gpu plants its low-plane variants: with 12 of them in the floor's sample the floor of
    k = 1 and k = 10 is a planted row's lower bound, and bit 2 carries up to 4 / 127 of a planted row's score — more than the
    margin.  Every planted row is kept or dropped as the predicate on the full code says: the candidates equal the other
    form's, the results the exact scan's."""
    for n in _sizes(native, d):
        idx = PG._index(native, d, n)
        q = PG._query(d)
        rows = PG._planted_rows(n)
        idx.set_rows(np.asarray(rows, dtype=np.int64), _bit2_variants(q, len(rows)))
        for k in (1, 10, 64):
            want = _exact(idx, [q], k)
            counts = {form: _routed(native, idx, [q], k, want, form, f"bit 2 d={d} n={n} k={k}", warm=3 if k == 1 and form == 2 else 0)
                      for form in (2, 3)}
            assert counts[2] == counts[3], (d, n, k, counts)
            m = min(k, len(rows))
            assert set(want[0][1].reshape(-1)[:m].tolist()) <= set(rows), (d, n, k)
        idx.close()


# ---- 3. a wave whose stage fills several times ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_dense_survival(native, d):
    """Wave w of the front form takes the batches w, w + waves, ... (mvdb_code8_front_geometry).  All rows of its first batches
    are near-copies of the query, a whole number of stages of 64 (four, or as many as the wave has batches for at this n):
    stage 0 keeps them all and the wave's stage fills that often.  Then the planted rows that are no rows of the floor's sample
    are zeroed (a zero row is rejected by the front plane; the sample, and so the floor, stays): the count of stage-0 survivors
    of a call drops by exactly their number — planted + background, the background being the call that lacks them."""
    n, k = 500_001, 64
    rb, waves = native.code8_front_geometry(d, n)
    w = 5
    nb = min(4 * 64 // rb, (n // rb - 1 - w) // waves + 1)
    nb -= nb % (64 // rb)
    assert (w + (nb - 1) * waves + 1) * rb <= n and nb * rb >= 2 * 64, (rb, waves, nb)
    rows = [(w + j * waves) * rb + i for j in range(nb) for i in range(rb)]
    assert len(rows) % 64 == 0
    q = PG._query(d)
    x = np.stack([np.float32(1.0 - j * 2.0 ** -17) * q for j in range(len(rows))]).astype(np.float32)
    idx = PG._index(native, d, n)
    idx.set_rows(np.asarray(rows, dtype=np.int64), x)
    want = _exact(idx, [q], k)
    _routed(native, idx, [q], k, want, 2, f"dense d={d}")
    assert set(want[0][1].reshape(-1).tolist()) <= set(rows)

    def survivors_of_a_call():
        before = idx.code8_front_counters()
        idx.search(q, k)
        after = idx.code8_front_counters()
        assert after[1] - before[1] == 1
        return after[0] - before[0]

    full = survivors_of_a_call()
    sample = {(s * n) // SEED for s in range(SEED)}
    gone = [r for r in rows if r not in sample]
    assert len(gone) >= 64
    idx.set_rows(np.asarray(gone, dtype=np.int64), np.zeros((len(gone), d), np.float32))
    background = survivors_of_a_call()
    print(f"dense d={d}: rows per batch {rb}, waves {waves}, planted {len(rows)}, zeroed {len(gone)}, survivors {full} -> {background}")
    assert full - background == len(gone), (full, background, len(gone))
    idx.close()


# ---- 4. every writer of the plane ------------------------------------------------------------------------------------------------------
def _plane_matches_code(native, idx, rows, what):
    for r in rows:
        high, low, image = idx.code8_read_row(int(r))
        c = native.code8_unpack(high, low)
        h5 = native.code8_front_unpack(image)
        assert np.array_equal(h5, (c.view(np.uint8) & 0xF8).view(np.int8)), (what, r)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_writers(native, d):
    n, k = _sizes(native, d)[1], 10
    idx = PG._index(native, d, n, spare=64)
    q = PG._query(d)
    rs = np.random.default_rng(d)

    def check(what, extra=(), warm=0):
        want = _exact(idx, [q], k)
        _routed(native, idx, [q], k, want, 2, what, warm=warm)
        m = idx.ntotal
        probe = [0, 1, 2, 3, 4, 5, 6, 7, m - 1, m - 2, m - 3, m - 4, m - 5] + rs.integers(0, m, 16).tolist() + list(extra)
        _plane_matches_code(native, idx, probe, what)
        return want

    check("fresh", warm=3)
    variants = _bit2_variants(q, 4)
    slot_row = (33_333 * n) // SEED
    idx.set_rows(np.array([n - 1, n - 2, slot_row], np.int64), variants[:3])
    want = check("set_rows", extra=[slot_row])
    assert set(want[0][1].reshape(-1)[:3].tolist()) == {n - 1, n - 2, slot_row}
    # add into reserved space: the plane is tiles of whole rows by capacity, nothing moves
    extra = flat.synth(37, d, 99)
    flat.normalize_l2(extra)
    extra[5] = variants[3]
    idx.add(extra)
    assert idx.code8_rows == idx.ntotal == n + 37 and idx.code8_front_counters()[3]
    want = check("add 37", extra=range(n, n + 37))
    assert n + 5 in want[0][1].reshape(-1)[:4].tolist()
    # add that grows the matrix: the code is dropped with it, the third query builds code and plane again
    more = flat.synth(100, d, 77)
    flat.normalize_l2(more)
    idx.add(more)
    assert idx.code8_rows == 0 and not idx.code8_front_counters()[3]
    check("add that grows", extra=range(n + 37, n + 137), warm=3)
    # remove_rows empties the code; the third query rebuilds it
    idx.remove_rows(np.array([3, n - 1], np.int64))
    assert idx.code8_rows == 0
    check("remove_rows", warm=3)
    # reset + re-add
    idx.reset()
    idx.add_synthetic(n, 4321, normalize=True)
    check("reset + re-add", warm=3)
    idx.close()


@pytest.mark.gpu
def test_update_embedding_writes_the_front_plane(native, tmp_path):
    from minivectordb_amd import VectorDatabase
    n, d, k = 500_017, 512, 5
    x = flat.synth(n, d, 1234)
    db = VectorDatabase(storage_file=str(tmp_path / "db.pkl"))
    db.store_embeddings_batch(list(range(n)), x)
    q = PG._query(d)
    for _ in range(4):
        db.find_most_similar(q, k=k)   # the first search builds the device index, the third eligible one the code
    assert db.index.code8_rows == n and db.index.code8_front_counters()[3]
    new = _bit2_variants(q, 2)
    db.update_embedding(n - 1, new[0])
    db.update_embedding(12_345, new[1])
    _plane_matches_code(native, db.index, [n - 1, 12_345, 0, n - 2], "update_embedding")
    db.index.set_option("code8_front_plane", 2)
    got = db.find_most_similar(q, k=k)
    db.index.set_option("code8_single_query", 0)
    want = db.find_most_similar(q, k=k)
    assert list(got[0]) == list(want[0]) and set(list(got[0])[:2]) == {n - 1, 12_345}
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32))


# ---- 5. the switch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_switch(native):
    import torch
    n, d, k = 500_001, 512, 10
    for family, suspends in (("positive", True), ("zero_mean", False)):
        flag = FAMILIES[family]
        idx = PG._index(native, d, n, flag)
        qs = list(PG._query(d, flag, nq=8))
        want = _exact(idx, qs, k)
        idx.set_option("code8_front_plane", 1)
        for _ in range(3):
            idx.search(qs[0], k)
        assert idx.code8_front_counters()[3]
        forms = set()
        native.prof_enable(True)
        try:
            for i in range(64):
                D, I = idx.search(qs[i % 8], k)
                forms.add(native.prof_symbol("ip_scan").count(",") == 4)
                assert np.array_equal(D.view(np.uint32), want[i % 8][0].view(np.uint32)) and np.array_equal(I, want[i % 8][1]), (family, i)
        finally:
            native.prof_enable(False)
        survivors, calls, suspensions, held = idx.code8_front_counters()
        print(f"switch {family}: front calls {calls}, survivors per front call {survivors / max(calls, 1):.0f} of {n}, suspensions {suspensions}")
        if suspends:
            assert suspensions == 1 and forms == {True, False} and calls < 64, (family, suspensions, forms, calls)
        else:
            assert suspensions == 0 and forms == {True} and calls >= 64, (family, suspensions, forms, calls)
        # option 0 returns the plane's bytes (whole tiles of 5 d / 8 bytes per row of the capacity)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        idx.set_option("code8_front_plane", 0)
        freed = torch.cuda.mem_get_info(0)[0] - free0
        plane = (n + 3) // 4 * 4 * (5 * d // 8)
        assert not idx.code8_front_counters()[3] and idx.code8_rows == n
        assert plane - (2 << 20) <= freed <= plane + (2 << 20), (freed, plane)
        D, I = idx.search(qs[0], k)
        assert np.array_equal(D.view(np.uint32), want[0][0].view(np.uint32)) and np.array_equal(I, want[0][1])
        idx.close()


# ---- 6. a captured stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay(native):
    import torch
    n, d, k = 500_001, 512, 10
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

    def replay_all(g, what):
        for i in range(4):
            qt.copy_(torch.from_numpy(qs[i]))
            Dt.zero_()
            It.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(Dt.cpu().numpy().view(np.uint32), want[i][0][0].view(np.uint32)), (what, i)
            assert np.array_equal(It.cpu().numpy(), want[i][1][0]), (what, i)

    # cold: this stream's workspace has never served the route and the index holds no code — nothing is allocated or built
    # inside the capture, the exact scan is recorded
    qt.copy_(torch.from_numpy(qs[0]))
    with torch.cuda.stream(stream):
        idx.set_option("code8_single_query", 0)
        enqueue()                       # (sizes the exact scan's workspace of this stream)
        idx.set_option("code8_single_query", 1)
    stream.synchronize()
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=stream, capture_error_mode="thread_local"):   # (an allocation in here ends the capture with an error)
        enqueue()
    assert idx.code8_rows == 0 and not idx.code8_front_counters()[3]
    replay_all(g0, "cold")
    # warm: eager calls build code and plane and size the workspace; the capture records the front form
    with torch.cuda.stream(stream):
        for _ in range(4):
            enqueue()
    stream.synchronize()
    assert idx.code8_rows == n and idx.code8_front_counters()[3]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        enqueue()
    before = idx.code8_front_counters()[1]
    replay_all(g, "warm")
    assert idx.code8_front_counters()[1] - before == 4   # every replay ran the front form
    del g, g0
    idx.close()
