"""The two planes of the int8 code and the prefilter's first stage, on the CPU.

The codes of a row are stored as a plane of the top 6 bits of every code and a plane of the low 2 bits.  The prefilter
streams the first plane alone: with H = c & ~3 it has T6 = Q . H, and the row's integer sum T = Q . c lies in
[T6 - 3 N, T6 + 3 P] (P: the sum of the positive Q_j, N: of the magnitudes of the negative ones).  Its first stage must
pass every row the predicate passes at the true T, at the bit level and for every floor: the bound it forms must be at or
above the predicate's, or NaN.  Both are restated here in numpy float32 — with the margin's two fused multiply-adds and
without (the products rounded first), and with the final sum s + m fused into the product that forms s and without — over
pairs drawn as test_code8_bound_cpu draws them, plus the edges.  The pack / unpack functions are the library's own
(mvdb_code8_pack / mvdb_code8_unpack: the functions the device code packs 16-code chunks with)."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

import test_code8_bound_cpu as B

f32 = np.float32
FLT_MAX = f32(3.402823466e+38)
INT_MIN = -2 ** 31


# ---- pack / unpack --------------------------------------------------------------------------------------------------------------
def _roundtrip(codes):
    high, low = native.code8_pack(codes)
    d = codes.shape[0]
    assert high.shape == (3 * d // 4,) and low.shape == (d // 4,)
    back = native.code8_unpack(high, low)
    assert np.array_equal(back, codes), (codes[:16], back[:16])
    # the layout: `& 0xFC` of the first three dwords of a chunk's 12 bytes is c & ~3 of codes 0 .. 11; the low bits of the
    # three dwords hold bits 7:6, 5:4, 3:2 of codes 12 .. 15; the low plane holds c & 3 at bit pairs 0, 2, 4, 6
    c = codes.view(np.uint8).reshape(-1, 4, 4)          # chunk, dword, byte
    h = high.reshape(-1, 3, 4)
    assert np.array_equal(h & 0xFC, c[:, :3] & 0xFC)
    top = ((h[:, 0] & 3) << 6) | ((h[:, 1] & 3) << 4) | ((h[:, 2] & 3) << 2)
    assert np.array_equal(top, c[:, 3] & 0xFC)
    lo = low.reshape(-1, 4)
    for i in range(4):
        assert np.array_equal((lo >> (2 * i)) & 3, c[:, i] & 3)
    # as signed bytes the high part is c rounded down to a multiple of 4: c = H + (c & 3)
    H = (codes.view(np.uint8) & 0xFC).view(np.int8).astype(np.int64)
    assert np.array_equal(H + (codes.view(np.uint8) & 3), codes.astype(np.int64))
    return H


@pytest.mark.parametrize("d", [384, 512, 1024])
def test_pack_unpack_round_trips(d):
    rs = np.random.default_rng(d)
    for _ in range(8):
        _roundtrip(rs.integers(-127, 128, d).astype(np.int8))
    H = _roundtrip(np.full(d, 127, np.int8))
    assert (H == 124).all()
    H = _roundtrip(np.full(d, -127, np.int8))
    assert (H == -128).all()                       # -127 masks to -128 (+ 1 in the low plane)
    _roundtrip(np.where(np.arange(d) % 2 == 0, 127, -127).astype(np.int8))
    _roundtrip((rs.integers(-31, 32, d) * 4).astype(np.int8))          # low bits all 0
    _roundtrip((rs.integers(-32, 31, d) * 4 + 3).astype(np.int8))      # low bits all 3
    _roundtrip(np.zeros(d, np.int8))


def test_pack_refuses_a_width_that_is_no_multiple_of_16():
    with pytest.raises(Exception):
        native.code8_pack(np.zeros(24, np.int8))


# ---- the two predicates -----------------------------------------------------------------------------------------------------------
def _fma(a, b, c, fused):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    if fused:
        return B.fma32(a, b, c)
    return ((a * b).astype(f32) + c).astype(f32)


def _bounds(T, T6, P3, N3, qstep, a, r, alpha, beta, fused_m, fused_ub):
    """(the predicate's bound at T, the first stage's bound from T6): code8_scan_kernel's epilogue and stage1, in fp32."""
    with np.errstate(all="ignore"):
        def s_of(t):
            tq = (t.astype(f32) * qstep).astype(f32)
            return tq, (tq * a).astype(f32)

        def margin(w):
            m = _fma(f32(alpha), r, f32(beta), fused_m)
            return _fma((w + m).astype(f32), f32(2.4e-7), m, fused_m)

        def total(tq, s, m):
            return B.fma32(tq, a, m) if fused_ub else (s + m).astype(f32)

        tq, s = s_of(T)
        ub = total(tq, s, margin(np.abs(s)))
        up = T6 + P3
        lo = np.maximum(T6, INT_MIN + N3) - N3
        assert up.max(initial=0) < 2 ** 31 and lo.min(initial=0) >= INT_MIN     # the kernel's int32 arithmetic
        tqu, su = s_of(up)
        _, sl = s_of(lo)
        w = np.where(np.isnan(sl), np.abs(su), np.where(np.isnan(su), np.abs(sl), np.maximum(np.abs(su), np.abs(sl))))   # fmaxf
        ub1 = total(tqu, su, margin(w.astype(f32)))
    return ub, ub1


FLOORS = [-FLT_MAX, f32(-1e30), f32(-1.0), f32(-1e-3), f32(-1e-45), f32(0.0), f32(1e-45), f32(1e-3), f32(0.25), f32(1.0)]


def _check(c, a, r, Q, qstep, alpha, beta, what):
    """Every (row, query) pair, every form of the arithmetic; returns the number of pairs."""
    c = np.asarray(c, np.int64)
    Q = np.asarray(Q, np.int64)
    H = (c.astype(np.int8).view(np.uint8) & 0xFC).view(np.int8).astype(np.int64)
    T, T6 = c @ Q, H @ Q
    P3, N3 = 3 * int(Q[Q > 0].sum()), 3 * int(-Q[Q < 0].sum())
    assert np.abs(T).max(initial=0) < 2 ** 31 and np.abs(T6).max(initial=0) < 2 ** 31, what
    assert ((T6 - N3 <= T) & (T <= T6 + P3)).all(), what
    a, r = np.asarray(a, f32), np.asarray(r, f32)
    for fused_m in (True, False):
        for fused_ub in (False, True):
            ub, ub1 = _bounds(T, T6, P3, N3, f32(qstep), a, r, alpha, beta, fused_m, fused_ub)
            nan0, nan1 = np.isnan(ub), np.isnan(ub1)
            # for every floor: !(ub < floor) implies !(ub1 < floor)
            ok = nan1 | (~nan0 & (ub1 >= ub)) | (nan0 & (ub1 == np.inf))
            assert ok.all(), (what, fused_m, fused_ub, int((~ok).sum()), ub[~ok][:3], ub1[~ok][:3], T[~ok][:3], T6[~ok][:3])
            # and at the floors themselves, the values of the bound among them (the ties)
            with np.errstate(all="ignore"):
                finite = ub[np.isfinite(ub)]
                floors = FLOORS + [f for f in np.quantile(finite, [0.0, 0.5, 0.99, 1.0]).astype(f32)] if finite.size else FLOORS
                for fl in floors:
                    keep, keep1 = ~(ub < fl), ~(ub1 < fl)
                    assert not (keep & ~keep1).any(), (what, fused_m, fused_ub, float(fl))
    return c.shape[0]


def _coded_pairs(x, queries, d, normalize_q, what):
    x = np.ascontiguousarray(x, f32)
    bound = f32(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1).max()) * 1.00001)
    c, a, r = B.code_rows(x, d)
    pairs = 0
    for qi, q in enumerate(queries):
        q = np.ascontiguousarray(q, f32)
        Q, qstep, qn, qtiny = B.code_query(q, d, normalize_q)
        alpha, beta = native.code8_margin(d, qn, qstep, bound)
        if qtiny:
            alpha = float(f32(qn * f32(1.00001)))
            beta = float(f32(B.fma32(np.array(qn * f32(1.00001)), np.array(bound), np.array(f32(1e-30))) * f32(1.00001)))
        pairs += _check(c, a, r, Q, qstep, alpha, beta, (what, qi, normalize_q))
    return pairs


@pytest.mark.parametrize("d,n", [(512, 3072), (384, 1024), (1024, 1024)])
def test_stage_one_passes_what_the_predicate_passes(d, n):
    rs = np.random.default_rng(2000 + d)
    total = 0
    for name, x in B.families(d, n, rs).items():
        qs = [rs.standard_normal(d), np.abs(rs.standard_normal(d)), -np.abs(rs.standard_normal(d)), x[0].copy(), -x[1] * 3.0,
              rs.standard_normal(d) * 1e-3]
        for normalize_q in (1, 0):
            total += _coded_pairs(x, qs, d, normalize_q, name)
    assert total >= (100_000 if d == 512 else 30_000), total


@pytest.mark.parametrize("d", [384, 512, 1024])
def test_stage_one_at_the_ends_of_the_integer_range(d):
    """Q at +-qmax in every element against all-(+127) and all-(-127) rows (and mixtures): T, T6 + 3 P and the saturated
    T6 - 3 N stay inside an int32 (asserted in _bounds and _check)."""
    qmax = 32512 if d <= 512 else 16256
    rows = np.stack([np.full(d, 127), np.full(d, -127), np.where(np.arange(d) % 2 == 0, 127, -127), np.full(d, 124), np.full(d, -128 + 1),
                     np.zeros(d, np.int64)]).astype(np.int64)
    a = np.array([1.0 / 127, 1e-3, 1.0, 3e30, 1e-30, 0.0], f32)
    r = np.array([1e-3, 0.0, np.inf, 1.0, 1e-30, np.inf], f32)
    for Q in (np.full(d, qmax), np.full(d, -qmax), np.where(np.arange(d) % 2 == 0, qmax, -qmax), np.where(np.arange(d) % 2 == 0, -qmax, qmax)):
        for qstep in (f32(1.0 / qmax), f32(1e-8), f32(1e30)):
            for alpha, beta in ((1.0, 1e-5), (0.0, 0.0), (1e-3, 1e-30)):
                _check(rows, a, r, Q, qstep, alpha, beta, ("range", d, float(qstep), alpha))


def test_stage_one_near_zero_scores_and_degenerate_queries():
    d = 512
    rs = np.random.default_rng(11)
    # scores within a few ulps of zero, of both signs: T in [-4, 4] from rows of a few small codes against a sparse query
    c = np.zeros((4096, d), np.int64)
    c[np.arange(4096), rs.integers(0, d, 4096)] = rs.integers(-3, 4, 4096)
    c[np.arange(4096), rs.integers(0, d, 4096)] = rs.integers(-3, 4, 4096)
    Q = np.zeros(d, np.int64)
    Q[rs.integers(0, d, 64)] = rs.integers(-2, 3, 64)
    for scale in (1e-38, 1e-30, 1e-10, 1.0):
        a = (np.abs(rs.standard_normal(4096)) * scale).astype(f32)
        r = (a * f32(3.0)).astype(f32)
        for qstep in (f32(1e-45), f32(1e-38), f32(1e-20), f32(3e-5)):
            for alpha, beta in ((1.0, 1e-30), (1.0, 0.0), (0.0, 0.0)):
                _check(c, a, r, Q, qstep, alpha, beta, ("near zero", scale, float(qstep)))
    # dense queries of one sign against small codes
    cs = rs.integers(-3, 4, (2048, d)).astype(np.int64)
    for Q in (np.abs(rs.integers(-5, 6, d)), -np.abs(rs.integers(-5, 6, d))):
        _check(cs, np.full(2048, 1e-3, f32), np.full(2048, 1e-3, f32), Q, f32(1e-4), 1.0, 1e-7, "one sign")
    # the zero query (coded as zero: qstep = 0) against rows of unbounded residual: 0 * inf, NaN on both sides — passes
    x = B.normalized(rs.standard_normal((64, d)))
    cc, a, r = B.code_rows(x, d)
    r[::2] = np.inf
    for alpha in (0.0, 1.0):
        ub, ub1 = _bounds(cc @ np.zeros(d, np.int64), np.zeros(64, np.int64), 0, 0, f32(0), a, r, alpha, 1e-30, True, False)
        assert (np.isnan(ub) == np.isnan(ub1)).all()
        _check(cc, a, r, np.zeros(d, np.int64), f32(0), alpha, 1e-30, "zero query")
    for normalize_q in (1, 0):
        _coded_pairs(x, [np.zeros(d), np.full(d, 1e-30), np.eye(d)[5], -np.eye(d)[7] * 1e6], d, normalize_q, "degenerate")
