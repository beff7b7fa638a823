"""The front plane of the int8 code and stage 0 of the prefilter, on the CPU.

Beside the two planes the code keeps a plane of the top 5 bits of every code, H5 = c & ~7.  The prefilter's front form
streams that plane alone: it has T5 = Q . H5, and the row's integer sum T = Q . c lies in [T5 - 7 N, T5 + 7 P].  Stage 0
must pass every row the predicate passes at the true T, at the bit level and for every floor: its bound must be at or above
the predicate's, or NaN.  Both are test_code8_planes_cpu's numpy float32 restatements (the arithmetic of stage 0 is stage
1's with 7 for 3), in all four forms — the margin fused and unfused, the final sum fused and unfused — over pairs drawn as
that file draws them, plus the edges.  The pack / unpack functions are the library's own (mvdb_code8_front_pack /
mvdb_code8_front_unpack: the functions the device code packs 32-code chunks with)."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

import test_code8_bound_cpu as B
import test_code8_planes_cpu as P

f32 = np.float32
INT_MIN = -2 ** 31


# ---- pack / unpack --------------------------------------------------------------------------------------------------------------
def _roundtrip(codes):
    image = native.code8_front_pack(codes)
    d = codes.shape[0]
    assert image.shape == (5 * d // 8,)
    H5 = native.code8_front_unpack(image)
    want = (codes.view(np.uint8) & 0xF8).view(np.int8)
    assert np.array_equal(H5, want), (codes[:32], H5[:32])
    # the layout: the 16-byte parts of the d / 32 chunks, then their 4-byte parts; `& 0xF8` of a chunk's five dwords is
    # c & ~7 of its codes 0 .. 19, the low 3 bits of those bytes hold the top bits of the codes 20 .. 31
    c = codes.view(np.uint8).reshape(-1, 8, 4)          # chunk, dword, byte
    f = np.concatenate([image[:d // 2].reshape(-1, 4, 4), image[d // 2:].reshape(-1, 1, 4)], axis=1)   # chunk, dword, byte
    assert np.array_equal(f & 0xF8, c[:, :5] & 0xF8)
    assert np.array_equal(((f[:, 0] & 7) << 5) | ((f[:, 1] & 3) << 3), c[:, 5] & 0xF8)
    assert np.array_equal(((f[:, 2] & 7) << 5) | ((f[:, 3] & 3) << 3), c[:, 6] & 0xF8)
    assert np.array_equal(((f[:, 4] & 7) << 5) | ((f[:, 1] & 4) << 2) | ((f[:, 3] & 4) << 1), c[:, 7] & 0xF8)
    # as signed bytes the front part is c rounded down to a multiple of 8: c = H5 + (c & 7)
    assert np.array_equal(H5.astype(np.int64) + (codes.view(np.uint8) & 7), codes.astype(np.int64))
    return H5.astype(np.int64)


@pytest.mark.parametrize("d", [384, 512, 1024])
def test_front_pack_unpack_round_trips(d):
    rs = np.random.default_rng(d)
    for _ in range(8):
        _roundtrip(rs.integers(-127, 128, d).astype(np.int8))
    assert (_roundtrip(np.full(d, 127, np.int8)) == 120).all()
    assert (_roundtrip(np.full(d, -127, np.int8)) == -128).all()       # -127 masks to -128 (+ 1 in the missing bits)
    _roundtrip(np.where(np.arange(d) % 2 == 0, 127, -127).astype(np.int8))
    _roundtrip((rs.integers(-15, 16, d) * 8).astype(np.int8))          # missing bits all 0
    _roundtrip((rs.integers(-16, 15, d) * 8 + 7).astype(np.int8))      # missing bits all 7
    _roundtrip(np.zeros(d, np.int8))
    # every chunk position on its own: one code set, the others zero
    for j in range(32):
        c = np.zeros(d, np.int8)
        c[j::32] = -8 - j
        _roundtrip(c)


@pytest.mark.parametrize("d", [16, 48, 500, 2080])
def test_front_pack_refuses_a_width_the_chunks_cannot_serve(d):
    with pytest.raises(Exception):
        native.code8_front_pack(np.zeros(d, np.int8))
    with pytest.raises(Exception):
        native.code8_front_unpack(np.zeros(5 * d // 8, np.uint8))


# ---- stage 0 against the predicate ------------------------------------------------------------------------------------------------
def _check(c, a, r, Q, qstep, alpha, beta, what):
    """Every (row, query) pair, every form of the arithmetic; returns the number of pairs."""
    c = np.asarray(c, np.int64)
    Q = np.asarray(Q, np.int64)
    H5 = (c.astype(np.int8).view(np.uint8) & 0xF8).view(np.int8).astype(np.int64)
    T, T5 = c @ Q, H5 @ Q
    Psum, Nsum = int(Q[Q > 0].sum()), int(-Q[Q < 0].sum())
    P7, N7 = 7 * Psum, 7 * Nsum
    assert np.abs(T).max(initial=0) < 2 ** 31 and np.abs(T5).max(initial=0) < 2 ** 31, what
    assert ((T5 - N7 <= T) & (T <= T5 + P7)).all(), what
    assert P7 < 2 ** 31 and N7 < 2 ** 31, what
    a, r = np.asarray(a, f32), np.asarray(r, f32)
    for fused_m in (True, False):
        for fused_ub in (False, True):
            # (P._bounds asserts that T5 + 7 P and the saturated T5 - 7 N fit an int32)
            ub, ub0 = P._bounds(T, T5, P7, N7, f32(qstep), a, r, alpha, beta, fused_m, fused_ub)
            nan, nan0 = np.isnan(ub), np.isnan(ub0)
            ok = nan0 | (~nan & (ub0 >= ub)) | (nan & (ub0 == np.inf))
            assert ok.all(), (what, fused_m, fused_ub, int((~ok).sum()), ub[~ok][:3], ub0[~ok][:3], T[~ok][:3], T5[~ok][:3])
            with np.errstate(all="ignore"):
                finite = ub[np.isfinite(ub)]
                floors = P.FLOORS + [f for f in np.quantile(finite, [0.0, 0.5, 0.99, 1.0]).astype(f32)] if finite.size else P.FLOORS
                for fl in floors:
                    keep, keep0 = ~(ub < fl), ~(ub0 < fl)
                    assert not (keep & ~keep0).any(), (what, fused_m, fused_ub, float(fl))
            # stage 0 is at or above stage 1 as well: a row stage 1 keeps was handed to it
            _, ub1 = P._bounds(T, (c.astype(np.int8).view(np.uint8) & 0xFC).view(np.int8).astype(np.int64) @ Q, 3 * Psum, 3 * Nsum, f32(qstep), a, r,
                               alpha, beta, fused_m, fused_ub)
            nan1 = np.isnan(ub1)
            assert (nan0 | (~nan1 & (ub0 >= ub1)) | (nan1 & (ub0 == np.inf))).all(), (what, fused_m, fused_ub)
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
def test_stage_zero_passes_what_the_predicate_passes(d, n):
    rs = np.random.default_rng(3000 + d)
    total = 0
    for name, x in B.families(d, n, rs).items():
        qs = [rs.standard_normal(d), np.abs(rs.standard_normal(d)), -np.abs(rs.standard_normal(d)), x[0].copy(), -x[1] * 3.0,
              rs.standard_normal(d) * 1e-3]
        for normalize_q in (1, 0):
            total += _coded_pairs(x, qs, d, normalize_q, name)
    assert total >= (100_000 if d == 512 else 30_000), total


@pytest.mark.parametrize("d", [384, 512, 1024])
def test_stage_zero_at_the_ends_of_the_integer_range(d):
    """Q at +-qmax in every element against all-(+127) and all-(-127) rows (and mixtures): T, T5 + 7 P and the saturated
    T5 - 7 N stay inside an int32 (asserted in P._bounds and _check)."""
    qmax = 32512 if d <= 512 else 16256
    rows = np.stack([np.full(d, 127), np.full(d, -127), np.where(np.arange(d) % 2 == 0, 127, -127), np.full(d, 120), np.full(d, -128 + 1),
                     np.zeros(d, np.int64)]).astype(np.int64)
    a = np.array([1.0 / 127, 1e-3, 1.0, 3e30, 1e-30, 0.0], f32)
    r = np.array([1e-3, 0.0, np.inf, 1.0, 1e-30, np.inf], f32)
    for Q in (np.full(d, qmax), np.full(d, -qmax), np.where(np.arange(d) % 2 == 0, qmax, -qmax), np.where(np.arange(d) % 2 == 0, -qmax, qmax)):
        H5 = (rows.astype(np.int8).view(np.uint8) & 0xF8).view(np.int8).astype(np.int64)
        up = H5 @ Q + 7 * int(Q[Q > 0].sum())
        assert up.max() < 2 ** 31 and (H5 @ Q).min() >= INT_MIN, (d, up.max())
        for qstep in (f32(1.0 / qmax), f32(1e-8), f32(1e30)):
            for alpha, beta in ((1.0, 1e-5), (0.0, 0.0), (1e-3, 1e-30)):
                _check(rows, a, r, Q, qstep, alpha, beta, ("range", d, float(qstep), alpha))


def test_stage_zero_near_zero_scores_and_degenerate_queries():
    d = 512
    rs = np.random.default_rng(12)
    # scores within a few ulps of zero, of both signs: rows of a few small codes against a sparse query
    c = np.zeros((4096, d), np.int64)
    c[np.arange(4096), rs.integers(0, d, 4096)] = rs.integers(-7, 8, 4096)
    c[np.arange(4096), rs.integers(0, d, 4096)] = rs.integers(-7, 8, 4096)
    Q = np.zeros(d, np.int64)
    Q[rs.integers(0, d, 64)] = rs.integers(-2, 3, 64)
    for scale in (1e-38, 1e-30, 1e-10, 1.0):
        a = (np.abs(rs.standard_normal(4096)) * scale).astype(f32)
        r = (a * f32(3.0)).astype(f32)
        for qstep in (f32(1e-45), f32(1e-38), f32(1e-20), f32(3e-5)):
            for alpha, beta in ((1.0, 1e-30), (1.0, 0.0), (0.0, 0.0)):
                _check(c, a, r, Q, qstep, alpha, beta, ("near zero", scale, float(qstep)))
    # dense queries of one sign against small codes
    cs = rs.integers(-7, 8, (2048, d)).astype(np.int64)
    for Q in (np.abs(rs.integers(-5, 6, d)), -np.abs(rs.integers(-5, 6, d))):
        _check(cs, np.full(2048, 1e-3, f32), np.full(2048, 1e-3, f32), Q, f32(1e-4), 1.0, 1e-7, "one sign")
    # the zero query (coded as zero: qstep = 0) against rows of unbounded residual, r = +inf: 0 * inf, NaN on both sides — passes
    x = B.normalized(rs.standard_normal((64, d)))
    cc, a, r = B.code_rows(x, d)
    r[::2] = np.inf
    for alpha in (0.0, 1.0):
        ub, ub0 = P._bounds(cc @ np.zeros(d, np.int64), np.zeros(64, np.int64), 0, 0, f32(0), a, r, alpha, 1e-30, True, False)
        assert (np.isnan(ub) == np.isnan(ub0)).all()
        _check(cc, a, r, np.zeros(d, np.int64), f32(0), alpha, 1e-30, "zero query")
    for normalize_q in (1, 0):
        _coded_pairs(x, [np.zeros(d), np.full(d, 1e-30), np.eye(d)[5], -np.eye(d)[7] * 1e6], d, normalize_q, "degenerate")
