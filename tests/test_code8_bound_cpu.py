"""The int8 prefilter's bound, restated in numpy: for every (query, row) pair the fp32 score the exact
kernel computes lies inside [s~ - m, s~ + m], where s~ is the coded score and m = alpha r + beta is the margin the library
exports (mvdb_code8_margin).  No allowance: every pair must hold.  The quantiser, the query rounding and the exact kernel's
summation order (lane-strided fma chains, then the xor butterfly) are restated here in fp32 arithmetic."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

f32 = np.float32
TINY = f32(1e-15)


def shape_of(d):
    return {384: (32, 3), 512: (64, 2), 1024: (64, 4)}[d]


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def exact_scores(x, q, d, normalize_q):
    """flat_scan_kernel's arithmetic: lane t of G takes 16-byte chunks t, t + G, ...; C x 4 fma in chunk order; butterfly."""
    G, C = shape_of(d)
    qv = q.reshape(C, G, 4).copy()
    if normalize_q:
        nr = np.zeros(G, f32)
        for c in range(C):
            nr = nr + ((qv[c, :, 0] * qv[c, :, 0] + qv[c, :, 1] * qv[c, :, 1]) + qv[c, :, 2] * qv[c, :, 2]) + qv[c, :, 3] * qv[c, :, 3]
        m = G // 2
        while m >= 1:
            nr = nr + nr[np.arange(G) ^ m]
            m //= 2
        if nr[0] > 0:
            qv = qv * (f32(1.0) / np.sqrt(nr[0], dtype=f32))
    xv = x.reshape(x.shape[0], C, G, 4)
    acc = np.zeros((x.shape[0], G), f32)
    for c in range(C):
        for j in range(4):
            acc = fma32(xv[:, c, :, j], np.broadcast_to(qv[c, :, j], acc.shape), acc)
    m = G // 2
    while m >= 1:
        acc = acc + acc[:, np.arange(G) ^ m]
        m //= 2
    return acc[:, 0]


def code_rows(x, d):
    """code8_build_kernel: (codes, a, r)."""
    mx = np.abs(x).max(axis=1)
    tiny = mx < TINY
    a = np.where(tiny, f32(0), mx / f32(127)).astype(f32)
    safe = np.where(a > 0, a, f32(1))[:, None]
    c = np.clip(np.rint(x / safe), -127, 127).astype(f32)
    c[tiny] = 0
    e = fma32(-np.broadcast_to(a[:, None], x.shape), c, x)
    r2 = np.zeros(x.shape[0], f32)
    for j in range(d):
        r2 = fma32(e[:, j], e[:, j], r2)
    r = np.sqrt(r2 + f32(d) * f32(2e-38), dtype=f32) * f32(1.001)
    r_tiny = fma32(mx, np.full_like(mx, np.sqrt(f32(d)) * f32(1.01)), np.full_like(mx, f32(1e-44)))
    r = np.where(tiny, r_tiny, r).astype(f32)
    return c.astype(np.int64), a, r


def code_query(q, d, normalize_q):
    """code8_query_kernel: (Q, qstep, qn)."""
    nr = f32(0)
    for j in range(d):
        nr = f32(np.float64(q[j]) * np.float64(q[j]) + np.float64(nr))
    inorm = f32(1.0) / np.sqrt(nr, dtype=f32) if (normalize_q and nr > 0) else f32(1.0)
    qh = (q * inorm).astype(f32)
    mx = np.abs(qh).max()
    qn = f32(np.sqrt((qh.astype(np.float64) ** 2).sum()) * (1.0 + 1e-6))
    qmax = 32512 if d <= 512 else 16256
    if mx < TINY:
        return np.zeros(d, np.int64), f32(0), qn, True
    qstep = f32(mx / f32(qmax))
    Q = np.clip(np.rint((qh / qstep).astype(f32)), -qmax, qmax).astype(np.int64)
    return Q, qstep, qn, False


def check_pairs(x, queries, d, normalize_q, bound=None):
    """Returns the number of pairs checked; asserts the bound on every one."""
    x = np.ascontiguousarray(x, f32)
    if bound is None:
        bound = f32(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1).max()) * 1.00001)
    c, a, r = code_rows(x, d)
    # the residual bound really bounds the residual
    true_r = np.sqrt(((x.astype(np.float64) - a.astype(np.float64)[:, None] * c) ** 2).sum(axis=1))
    assert (true_r <= r.astype(np.float64)).all()
    pairs = 0
    for q in queries:
        q = np.ascontiguousarray(q, f32)
        exact = exact_scores(x, q, d, normalize_q).astype(np.float64)
        Q, qstep, qn, qtiny = code_query(q, d, normalize_q)
        alpha, beta = native.code8_margin(d, qn, qstep, bound)
        if qtiny:
            alpha = float(f32(qn * f32(1.00001)))
            beta = float(f32(fma32(np.array(qn * f32(1.00001)), np.array(bound), np.array(f32(1e-30))) * f32(1.00001)))
        T = c @ Q
        assert np.abs(T).max() < 2 ** 31
        s = ((T.astype(f32) * qstep).astype(f32) * a).astype(f32)
        m = fma32(np.full_like(r, f32(alpha)), r, np.full_like(r, f32(beta)))
        m = fma32(np.abs(s) + m, np.full_like(m, f32(2.4e-7)), m)
        ub, lb = (s + m).astype(np.float64), (s - m).astype(np.float64)   # as the kernel forms them: in fp32
        bad = ~((exact <= ub) & (exact >= lb))
        assert not bad.any(), (int(bad.sum()), exact[bad][:3], s[bad][:3], m[bad][:3])
        pairs += x.shape[0]
    return pairs


def normalized(x):
    x = np.ascontiguousarray(x, f32)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    return (x / np.where(n > 0, n, 1)).astype(f32)


def families(d, n, rs):
    out = {}
    out["random"] = normalized(rs.standard_normal((n, d)))
    out["positive"] = normalized(rs.random((n, d)) + 0.05)
    centres = normalized(rs.standard_normal((16, d)))
    out["clustered"] = normalized(centres[rs.integers(0, 16, n)] + 0.05 * rs.standard_normal((n, d)) / np.sqrt(d))
    # adversarial for the quantiser: one huge element (everything else rounds to code 0 and is all residual)
    huge = (0.01 * rs.standard_normal((n, d))).astype(f32)
    huge[np.arange(n), rs.integers(0, d, n)] = 1000.0
    out["huge_element"] = huge
    # every element half a step from its code, signs alternating: the largest residual a row can have
    step = f32(1.0 / 127.0)
    codes = rs.integers(-126, 126, (n, d)).astype(f32)
    alt = (codes + 0.4999 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)) * step
    alt[:, 0] = 1.0   # pins the scale: a = 1 / 127
    out["half_step"] = alt.astype(f32)
    out["raw_scales"] = (rs.standard_normal((n, d)) * np.exp(rs.uniform(-20, 20, (n, 1)))).astype(f32)
    out["tiny_and_zero"] = (rs.standard_normal((n, d)) * np.where(np.arange(n)[:, None] % 3 == 0, 0.0, 1e-20)).astype(f32)
    return out


@pytest.mark.parametrize("d,n", [(512, 3072), (384, 1024), (1024, 1024)])
def test_bound_holds_on_every_pair(d, n):
    rs = np.random.default_rng(1000 + d)
    total = 0
    for name, x in families(d, n, rs).items():
        qs = [rs.standard_normal(d), np.abs(rs.standard_normal(d)), x[0].copy(), x[1] * 3.0, rs.standard_normal(d) * 1e-3]
        # a query aligned with a row's coding residual: the worst direction for q . (x - a c)
        c, a, _ = code_rows(np.ascontiguousarray(x[:4], f32), d)
        res = x[2].astype(np.float64) - float(a[2]) * c[2]
        if np.abs(res).max() > 0:
            qs.append(res / np.abs(res).max())
        for normalize_q in (1, 0):
            total += check_pairs(x, qs, d, normalize_q)
    assert total >= (100_000 if d == 512 else 30_000), total


def test_degenerate_queries():
    d, n = 512, 512
    rs = np.random.default_rng(7)
    x = normalized(rs.standard_normal((n, d)))
    qs = [np.zeros(d), np.full(d, 1e-30), np.eye(d)[5], -np.eye(d)[7] * 1e6]
    for normalize_q in (1, 0):
        assert check_pairs(x, qs, d, normalize_q, bound=f32(1.000004)) == n * len(qs)


def test_margin_is_no_wider_than_half_a_step_per_element():
    """Rounding to the nearest code leaves at most half a step a = max|x| / 127 per element, so r <= a sqrt(d) / 2 (+ the
    0.1 % the build rounds up by); beside it the margin holds the query-rounding term, max|q| sqrt(d) / (2 * 32512), and the
    fp32 terms, (gam + eta + kap) ~ (3 d + 60) 2^-24, times the norms (both 1 here)."""
    d = 512
    rs = np.random.default_rng(3)
    x = normalized(rs.standard_normal((2048, d)))
    _, a, r = code_rows(x, d)
    q = normalized(rs.standard_normal((1, d)))[0]
    _, qstep, qn, _ = code_query(q, d, 1)
    alpha, beta = native.code8_margin(d, qn, qstep, 1.000004)
    small = 1.01 * (np.abs(q).max() * np.sqrt(d) / (2 * 32512) + (3 * d + 60) * 2.0 ** -24)
    assert beta <= small and alpha <= 1.0 + small
    m = alpha * r.astype(np.float64) + beta
    assert (m <= 1.002 * a.astype(np.float64) * np.sqrt(d) / 2 + small).all()
