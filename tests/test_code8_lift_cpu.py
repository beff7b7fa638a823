"""The bit plane of the int8 code and the lift of the front form ("The bit plane"), on the CPU.

The front plane holds H5 = c & ~7 of every code, stage 1 of the prefilter wants T6 = Q . (c & ~3).  With b2 = (c >> 2) & 1:
c & ~3 = H5 + 4 b2 in two's complement, so T6 = T5 + 4 Q . b2 — the rows the front plane cannot reject read d / 8 bytes of
the plane of bit 2 where they used to read their 3 d / 4 bytes of the 6-bit plane.  Here: the plane's row image through the
exports (bit i of dword s is bit 2 of code 32 s + i), the identity for every int8 value with the int32 argument, and the
kernel's nibble spread restated."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

DIMS = (32, 384, 512, 1024, 2048)


def _codes(d, seed):
    c = np.random.default_rng(seed).integers(-128, 128, d).astype(np.int8)
    c[:4] = (-128, 127, -4, 4)
    return c


@pytest.mark.parametrize("d", DIMS)
def test_pack_unpack_round_trip(d):
    for seed in range(4):
        c = _codes(d, seed)
        bits = native.code8_bit2_pack(c)
        assert bits.dtype == np.uint8 and bits.shape == (d // 8,)
        b2 = (c.astype(np.int64) >> 2) & 1
        # the layout: bit i of dword s of the row is bit 2 of code 32 s + i (dwords are little-endian)
        words = bits.view("<u4")
        for s in range(d // 32):
            want = sum(int(b2[32 * s + i]) << i for i in range(32))
            assert int(words[s]) == want, (d, seed, s)
        back = native.code8_bit2_unpack(bits)
        assert back.dtype == np.int8 and np.array_equal(back.astype(np.int64), b2)
    for c in (np.full(d, -128, np.int8), np.full(d, 127, np.int8), np.zeros(d, np.int8), np.full(d, 4, np.int8), np.full(d, -5, np.int8)):
        assert np.array_equal(native.code8_bit2_unpack(native.code8_bit2_pack(c)).astype(np.int64), (c.astype(np.int64) >> 2) & 1)


def test_pack_refuses_what_is_no_row():
    for d in (0, 16, 500, 2080):
        with pytest.raises(Exception):
            native.code8_bit2_pack(np.zeros(d, np.int8))


def _qmax(d):
    return 32512 if d <= 512 else 16256   # code8_qmax


@pytest.mark.parametrize("d", (384, 512, 1024))
def test_the_identity_for_every_code_value(d):
    """T6 = T5 + 4 Q . b2, exactly, in int32: every one of the 256 code values (-128 and 127 among them) at every position
    class, against queries at +qmax, -qmax, zero, mixed signs at the extremes and random ones."""
    qmax = _qmax(d)
    rs = np.random.default_rng(d)
    values = np.arange(-128, 128, dtype=np.int64)
    assert values[0] == -128 and values[-1] == 127
    rows = [np.full(d, v, np.int64) for v in values]                           # a row of one value: the extreme of every sum
    rows += [np.roll(np.resize(values, d), s) for s in (0, 1, 7, 31)]           # every value in one row
    rows += [rs.integers(-128, 128, d) for _ in range(8)]
    queries = [np.full(d, qmax, np.int64), np.full(d, -qmax, np.int64), np.zeros(d, np.int64),
               np.where(np.arange(d) % 2 == 0, qmax, -qmax).astype(np.int64)]
    queries += [rs.integers(-qmax, qmax + 1, d) for _ in range(4)]
    lim = 2 ** 31
    for c in rows:
        h5, h6 = c & ~7, c & ~3
        b2 = (c >> 2) & 1
        assert np.array_equal(h6, h5 + 4 * b2)
        # every factor of the lifted sum lies in an int8: H5 + 4 in [-128, 127]
        assert h5.min() >= -128 and (h5 + 4).max() <= 127 and h6.min() >= -128 and h6.max() <= 127
        for Q in queries:
            lo = ((Q + 128) & 255) - 128
            hi = (Q - lo) >> 8
            assert np.array_equal(hi * 256 + lo, Q) and hi.min() >= -128 and hi.max() <= 127
            t5 = int((Q * h5).sum())
            t6 = int((Q * h6).sum())
            # what the lane sums: one (hi, lo) pair of dot products with bytes of 0 / 1
            lhi, llo = int((hi * b2).sum()), int((lo * b2).sum())
            lift = 256 * lhi + llo
            assert lift == int((Q * b2).sum())
            assert t6 == t5 + 4 * lift
            for v in (t5, t6, lhi, llo, lift, 4 * lift, 256 * lhi):
                assert -lim <= v < lim, (d, v)


def _spread(w, j):
    """code8_bit2_spread: nibble j of a dword of the plane -> four bytes of 0 / 1 (uint32 arithmetic)."""
    return ((((w >> (4 * j)) & 0xF) * 0x00204081) & 0xFFFFFFFF) & 0x01010101


def test_the_nibble_spread():
    # all 16 nibbles: bit b of the nibble lands at bit 8 b, nothing else is set, the product fits 32 bits without a carry
    for x in range(16):
        p = x * 0x00204081
        assert p < 2 ** 32
        s = p & 0x01010101
        assert [(s >> (8 * b)) & 0xFF for b in range(4)] == [(x >> b) & 1 for b in range(4)]
    # against the export: the bytes the spread yields for dword s, nibble j are the plane's bits of codes 32 s + 4 j .. + 3
    d = 512
    c = _codes(d, 11)
    words = native.code8_bit2_pack(c).view("<u4")
    b2 = native.code8_bit2_unpack(native.code8_bit2_pack(c)).astype(np.int64)
    for s in range(d // 32):
        for j in range(8):
            v = _spread(int(words[s]), j)
            assert [(v >> (8 * b)) & 0xFF for b in range(4)] == b2[32 * s + 4 * j:32 * s + 4 * j + 4].tolist()
