"""The quad layout of the front plane and the quad form of the prefilter's stage 0 ("The front plane:
a lane quad per row") at d = 512, at the smallest sizes the route serves.

At d = 512 a lane quad holds a row, lane t of it the codes [128 t, 128 t + 128): four chunks, unpacked by the unchanged chunk
function and summed into one (hi, lo) pair against 128 dimensions of the query's planes.  What can go wrong is a code that
meets the wrong query element (1), the partial batch and the head batch (1, 2), a stage 0 that passes other rows than the
parent's (3: T5 is an exact integer, so the survivors per call are the parent's, recorded from a build of the parent commit),
and a writer that puts a part of a row where the scan does not read it (4)."""
import json
import os

import numpy as np
import pytest

from oracle import flat

import test_code8_front_gpu as FG
import test_code8_planes_gpu as PG

D, K = 512, 10
N = 500_001
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "code8_front_survivors.json")


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


# ---- 1. every code position meets its query element ------------------------------------------------------------------------------
def _planted_positions(n, rb, waves):
    """One stored row per dimension j.  The rows cycle through the 16 positions of a tile (not in step with j: a code's place
    in its chunk and its row's place in the tile vary independently); j < 128 lie in the head batches of their waves (batch
    b < waves is wave b's first), the others behind every head batch, the last in the partial tile at the index's end."""
    rows = []
    for j in range(D):
        g = (5 * j + j // 16) % 16
        tile = 7 * j if j < 128 else 5000 + 51 * j
        rows.append(16 * tile + g)
    rows[D - 1] = n - 1
    assert len(set(rows)) == D and max(rows) < n
    assert {r % 16 for r in rows} == set(range(16))
    assert all(r // rb < waves for r in rows[:128]) and all(r // rb >= waves for r in rows[128:])
    assert (n - 1) // 16 * 16 + 16 > n   # (the last row's tile is partial)
    return rows


@pytest.mark.gpu
def test_every_code_position_meets_its_query_element(native):
    rb, waves = native.code8_front_geometry(D, N)
    rows = _planted_positions(N, rb, waves)
    idx = PG._index(native, D, N)
    bg = flat.synth(D, D, 4242)
    flat.normalize_l2(bg)
    x = (np.float32(0.9) * np.eye(D, dtype=np.float32) + np.float32(0.1) * bg).astype(np.float32)
    flat.normalize_l2(x)
    idx.set_rows(np.asarray(rows, dtype=np.int64), x)
    qs = list(np.eye(D, dtype=np.float32))
    want = FG._exact(idx, qs, K)
    FG._routed(native, idx, qs, K, want, 2, "one planted row per dimension")   # (bit-equal, the front form, no fallback)
    for j in range(D):
        assert int(want[j][1].reshape(-1)[0]) == rows[j], (j, rows[j], want[j][1])
    idx.close()


# ---- 2. the sizes around the partial batch ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sizes_around_the_partial_batch(native):
    rb, _ = native.code8_front_geometry(D, N)
    assert rb in (16, 32, 64)   # (16 rows per tile, 1, 2 or 4 tiles per batch: a whole number of batches fills a stage of 64)
    for n in (N, 500_000 + rb - 1):
        idx = PG._index(native, D, n)
        qs = list(PG._query(D, nq=8))
        want = FG._exact(idx, qs, K)
        counts = {form: FG._routed(native, idx, qs, K, want, form, f"n={n} form={form}") for form in (2, 3, 0)}
        assert counts[2] == counts[3] == counts[0], (n, counts)
        idx.set_option("code8_front_plane", 2)
        native.prof_enable(True)
        try:
            idx.search(qs[0], K)
            sym = native.prof_symbol("ip_scan")
        finally:
            native.prof_enable(False)
        args = sym[sym.index("<") + 1:sym.index(">")].split(",")
        assert len(args) == 5 and args[3].strip() == "4" and int(args[4]) * 16 == rb, sym   # GF = 4: a lane quad per row
        idx.close()


# ---- 3. stage 0 is the parent's ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(PG.FAMILIES))
def test_stage_zero_survivors_are_the_parents(native, family):
    """benchmarks/code8_front_survivors.py, restated: the golden file was written by it from a build of the commit before
    this layout.  A count that differs means the layout or the unpacking is wrong, whatever (D, I) say."""
    with open(GOLDEN) as f:
        golden = json.load(f)[f"{family}/{D}"]
    flag = PG.FAMILIES[family]
    idx = PG._index(native, D, N, flag)
    qs = list(PG._query(D, flag, nq=8))
    idx.set_option("code8_front_plane", 2)
    for _ in range(3):
        idx.search(qs[0], K)
    got = []
    for q in qs:
        before = idx.code8_front_counters()
        idx.search(q, K)
        after = idx.code8_front_counters()
        assert after[1] - before[1] == 1
        got.append(int(after[0] - before[0]))
    print(f"stage-0 survivors {family}: {got}")
    assert got == golden, (family, got, golden)
    idx.close()


# ---- 4. the writers ----------------------------------------------------------------------------------------------------------------
def _image(idx, r):
    return idx.code8_read_row(int(r))[2].copy()


def _matches_code(native, idx, rows, what):
    for r in rows:
        high, low, image = idx.code8_read_row(int(r))
        c = native.code8_unpack(high, low)
        assert np.array_equal(native.code8_front_unpack(image), (c.view(np.uint8) & 0xF8).view(np.int8)), (what, r)


@pytest.mark.gpu
def test_writers_put_every_part_where_the_offsets_say(native):
    n = N
    idx = PG._index(native, D, n, spare=64)
    q = PG._query(D)
    idx.set_option("code8_front_plane", 2)
    for _ in range(3):
        idx.search(q, K)
    assert idx.code8_rows == n and idx.code8_front_counters()[3]
    written = [0, 15, 16, n - 1]
    neighbours = [1, 2, 14, 17, 31, 32, n - 2, n - 3, n - 17]
    _matches_code(native, idx, written + neighbours, "fresh")
    before = {r: _image(idx, r) for r in neighbours}
    old = {r: _image(idx, r) for r in written}
    new = flat.synth(len(written), D, 31337)
    flat.normalize_l2(new)
    idx.set_rows(np.asarray(written, dtype=np.int64), new)
    _matches_code(native, idx, written + neighbours, "set_rows")
    for r in neighbours:
        assert np.array_equal(_image(idx, r), before[r]), ("set_rows moved a neighbour", r)
    # the written rows hold the new rows' codes
    for r, image in old.items():
        assert not np.array_equal(_image(idx, r), image), ("set_rows left a written row's image", r)
    # add into reserved space: nothing moves, the new rows' parts go to their own tiles
    before.update({r: _image(idx, r) for r in written})
    extra = flat.synth(37, D, 99)
    flat.normalize_l2(extra)
    idx.add(extra)
    assert idx.code8_rows == idx.ntotal == n + 37 and idx.code8_front_counters()[3]
    _matches_code(native, idx, list(range(n - 3, n + 37)) + written + neighbours, "add 37")
    for r, image in before.items():
        assert np.array_equal(_image(idx, r), image), ("add moved a stored row", r)
    want = FG._exact(idx, [q], K)
    FG._routed(native, idx, [q], K, want, 2, "after the writers", warm=0)
    idx.close()
