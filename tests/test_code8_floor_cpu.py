"""The floor of the int8 prefilter from the codes alone (code8_seed_kernel), restated in numpy.

The floor is the k-th best LOWER bound lb = s~ - m (formed in fp32, as test_code8_bound_cpu.check_pairs forms it) over a
sample of rows, NaN lower bounds ignored, -FLT_MAX when fewer than k are left.  Two things must hold, with no allowance:
the floor lies at or below the k-th best exact score over ALL rows, and every row whose exact score reaches that k-th best
survives the prefilter's predicate not(ub < floor)."""
import numpy as np
import pytest

from minivectordb_amd import _native as native

from test_code8_bound_cpu import code_query, code_rows, exact_scores, families, fma32

f32 = np.float32
FLT_MAX = f32(3.402823466e+38)


def bounds(x, q, d, normalize_q, bound):
    """(lb, ub) of every row, in fp32 as the kernels form them (check_pairs' arithmetic)."""
    c, a, r = code_rows(x, d)
    Q, qstep, qn, qtiny = code_query(q, d, normalize_q)
    alpha, beta = native.code8_margin(d, qn, qstep, bound)
    if qtiny:
        alpha = float(f32(qn * f32(1.00001)))
        beta = float(f32(fma32(np.array(qn * f32(1.00001)), np.array(bound), np.array(f32(1e-30))) * f32(1.00001)))
    T = c @ Q
    assert np.abs(T).max() < 2 ** 31
    s = ((T.astype(f32) * qstep).astype(f32) * a).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = fma32(np.full_like(r, f32(alpha)), r, np.full_like(r, f32(beta)))
        m = fma32(np.abs(s) + m, np.full_like(m, f32(2.4e-7)), m)
        return (s - m).astype(f32), (s + m).astype(f32)


def floor_of(lb, k):
    """code8_seed_kernel's selection: NaN never enters a list; fewer than k keys, or a k-th of -inf, give -FLT_MAX."""
    lb = lb[~np.isnan(lb)]
    if lb.size < k:
        return -FLT_MAX
    return max(np.sort(lb)[::-1][k - 1], -FLT_MAX)


def check_floor(x, q, d, normalize_q, ks, step=8):
    x = np.ascontiguousarray(x, f32)
    q = np.ascontiguousarray(q, f32)
    bound = f32(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1).max()) * 1.00001)
    exact = exact_scores(x, q, d, normalize_q)
    lb, ub = bounds(x, q, d, normalize_q, bound)
    sample = lb[::step]
    for k in ks:
        floor = floor_of(sample, k)
        kth = np.sort(exact)[::-1][k - 1]
        assert floor <= kth, (k, floor, kth)
        top = exact >= kth
        assert top.sum() >= k
        assert not (ub[top] < floor).any(), (k, floor, ub[top].min())


@pytest.mark.parametrize("d,n", [(512, 3072), (384, 1024), (1024, 1024)])
def test_floor_from_the_codes_keeps_the_top_k(d, n):
    rs = np.random.default_rng(2000 + d)
    for name, x in families(d, n, rs).items():
        qs = [rs.standard_normal(d), np.abs(rs.standard_normal(d)), x[0].copy(), x[1] * 3.0]
        for normalize_q in (1, 0):
            for q in qs:
                check_floor(x, q, d, normalize_q, (1, 10, 64))


def test_fewer_than_k_finite_lower_bounds_give_no_floor():
    d, n, k = 512, 256, 10
    rs = np.random.default_rng(11)
    x = (rs.standard_normal((n, d)) / np.sqrt(d)).astype(f32)
    q = rs.standard_normal(d).astype(f32)
    lb, ub = bounds(x, q, d, 1, f32(2.0))
    # rows with a non-finite element carry r = +inf (code8_build_kernel): their margin is +inf, their lower bound -inf — or
    # NaN against a query coded as zero; only 7 rows of the sample keep a finite lower bound
    sample = lb[::8].copy()
    assert sample.size == 32
    sample[7:20] = -np.inf
    sample[20:] = np.nan
    assert floor_of(sample, k) == -FLT_MAX
    assert floor_of(sample[:7], k) == -FLT_MAX
    assert floor_of(sample, 7) == np.sort(lb[::8][:7])[0]
    # with no floor everything passes the predicate: the call overflows and falls back
    assert not (ub < floor_of(sample, k)).any()
