"""Where the device keeps the front plane of the int8 code ("The front plane: a lane quad per row"),
on the CPU, through the diagnostic export mvdb_code8_front_offset: the functions every reader and writer of the plane uses.

At d = 512 the plane is stored in tiles of 16 rows, 16 x 320 bytes = five contiguous 1-KiB slabs.  Lane t of the quad of
row g owns the chunks 4 t .. 4 t + 3: in slab s = 0 .. 3 it holds the 16-byte part of chunk 4 t + s at (4 g + t) * 16, in slab
4 the four 4-byte parts of its chunks as one 16-byte unit at the same place.  At d = 384 and d = 1024 the layout is the one
the plane has always had: tiles of R = 4 (2) rows, the 16-byte parts of the tile's rows — row g at g * d / 2, chunk t at
16 t — and behind them the 4-byte parts, row g at g * d / 8, chunk t at 4 t."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

CAPACITIES = [1, 15, 16, 17, 1000]


def _offsets(d, rows):
    wide = np.empty((rows, d // 32), np.int64)
    narrow = np.empty((rows, d // 32), np.int64)
    for r in range(rows):
        for t in range(d // 32):
            wide[r, t], narrow[r, t] = native.code8_front_offset(d, r, t)
    return wide, narrow


@pytest.mark.parametrize("cap", CAPACITIES)
def test_quad_layout_at_512(cap):
    d, R, stride = 512, 16, 320
    plane = (cap + R - 1) // R * R * stride               # code8_front_bytes: whole tiles of the capacity
    wide, narrow = _offsets(d, cap)
    assert (wide % 16 == 0).all() and (narrow % 4 == 0).all()
    assert wide.min() >= 0 and narrow.min() >= 0 and (wide + 16).max() <= plane and (narrow + 4).max() <= plane
    # no two parts share a byte
    used = np.zeros(plane, np.int32)
    for w in wide.reshape(-1):
        used[w:w + 16] += 1
    for m in narrow.reshape(-1):
        used[m:m + 4] += 1
    assert used.max() == 1
    assert len(set(wide.reshape(-1).tolist())) == wide.size and len(set(narrow.reshape(-1).tolist())) == narrow.size
    # the parts of a full tile fill its 5 KiB exactly; the rows of the last tile past the capacity are the only holes
    full = cap // R
    assert (used[:full * R * stride] == 1).all()
    assert int(used.sum()) == cap * stride
    # the formula: slab s of the tile, the lane's unit at (4 g + t) * 16
    for r in range(cap):
        tile, g = r // R * R * stride, r % R
        for c in range(d // 32):
            t, s = c // 4, c % 4
            assert wide[r, c] == tile + s * 1024 + (4 * g + t) * 16, (r, c)
            assert narrow[r, c] == tile + 4096 + (4 * g + t) * 16 + 4 * s, (r, c)
    # what one wave-instruction of the scan reads — lane (g, t) 16 bytes at slab + lane * 16 — is one contiguous KiB
    if cap >= R:
        for s in range(4):
            lanes = np.array([wide[g, 4 * t + s] for g in range(R) for t in range(4)])
            assert np.array_equal(lanes, s * 1024 + 16 * np.arange(64))
        lanes = np.array([narrow[g, 4 * t] for g in range(R) for t in range(4)])
        assert np.array_equal(lanes, 4096 + 16 * np.arange(64))


@pytest.mark.parametrize("d,R", [(384, 4), (1024, 2)])
@pytest.mark.parametrize("cap", CAPACITIES)
def test_other_widths_keep_their_layout(d, R, cap):
    stride = 5 * d // 8
    plane = (cap + R - 1) // R * R * stride
    wide, narrow = _offsets(d, cap)
    for r in range(cap):
        tile, g = r // R * R * stride, r % R
        for t in range(d // 32):
            assert wide[r, t] == tile + g * (d // 2) + 16 * t, (r, t)
            assert narrow[r, t] == tile + R * (d // 2) + g * (d // 8) + 4 * t, (r, t)
    assert (wide % 16 == 0).all() and (narrow % 4 == 0).all()
    assert (wide + 16).max() <= plane and (narrow + 4).max() <= plane
    spans = sorted([(int(w), 16) for w in wide.reshape(-1)] + [(int(m), 4) for m in narrow.reshape(-1)])
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))


def test_offset_refuses_what_is_no_chunk():
    for d, row, chunk in ((500, 0, 0), (512, -1, 0), (512, 0, 16), (512, 0, -1), (2080, 0, 0)):
        with pytest.raises(Exception):
            native.code8_front_offset(d, row, chunk)
