"""The bound of the wide certified pass (half_wide_scan.hip: half_wide_eps, exported as mvdb_half_wide_eps; d = 1536 .. 4096):
the formula restated and pinned, and an emulation of flat_scan_h16_wide_kernel's accumulation — NK chains of d / NK products,
one per wave, then NK - 1 ordered fp32 additions — held against it on the case families of test_split_bound.py."""
import numpy as np
import pytest

from test_split_bound import _fp16_image, _fp32_chain, _half_cases, _pow2_scale

PARTS = {1536: 4, 2048: 4, 3072: 8, 4096: 8}   # NK: the waves that share a query group's K


def half_wide_eps(d):
    u11, u23, u24 = 2.0 ** -11, 2.0 ** -23, 2.0 ** -24
    e_op = 2 * u11 + u11 * u11
    e_uf = np.sqrt(float(d)) * 2.0 ** -27 * (1 + u11) + d * 2.0 ** -56
    n = d // PARTS[d] + PARTS[d] - 1.0
    e_acc = n * u23 / (1 - n * u23) * (1 + u11) ** 2
    depth = ((d + 3) // 4 + 63) // 64 * 4 + 6
    e_re = depth * u24 / (1 - depth * u24)
    return (e_op + e_uf + e_acc + e_re) * (1 + 4e-6) + 4 * u24


@pytest.mark.parametrize("d", sorted(PARTS))
def test_library_half_wide_eps_is_the_documented_formula(d):
    from minivectordb_amd import _native
    assert _native.half_wide_eps(d) == pytest.approx(half_wide_eps(d), rel=1e-12)
    assert _native.half_wide_queries(d) == (64 if d <= 2048 else 32)
    assert _native.half_wide_eps(d // 2 + 16) == 0.0 and _native.half_wide_queries(1024) == 0


@pytest.mark.parametrize("d", [1536, 4096])
@pytest.mark.parametrize("mode", ["rne", "trunc"])
@pytest.mark.parametrize("flush", [False, True])
def test_half_wide_eps_covers_emulated_nomination(d, mode, flush):
    nk, ks = PARTS[d], 32
    ksp = ks // nk
    # wave p holds the 16-k blocks [p ksp, (p + 1) ksp) of every stage of ks blocks: its chain walks them stage by stage
    blocks = np.arange(d // 16).reshape(-1, nk, ksp)                       # [stage][part][block of the part]
    cols = [(blocks[:, p, :].reshape(-1, 1) * 16 + np.arange(16)).ravel() for p in range(nk)]
    eps, worst = half_wide_eps(d), 0.0
    for name, q, x in _half_cases(d):
        bound = np.float32(np.linalg.norm(x.astype(np.float64), axis=-1).max() * (1 + 4e-6))
        sx = _pow2_scale(bound)
        sq = np.array([_pow2_scale(np.abs(r).max()) if np.abs(r).max() > 0 else 1.0 for r in q])
        qh = np.stack([_fp16_image(q[i], sq[i], flush) for i in range(q.shape[0])])
        prod = qh * _fp16_image(x, sx, flush)
        partial = np.stack([_fp32_chain(prod[:, c], mode) for c in cols], axis=-1).astype(np.float64)
        approx = _fp32_chain(partial, mode).astype(np.float64) / (sq * sx)   # ascending part order (the leading 0 + p0 is exact)
        t = np.sum(q.astype(np.float64) * x.astype(np.float64), axis=-1)
        scale = np.linalg.norm(q.astype(np.float64), axis=-1) * float(bound)
        resc = _fp32_chain(q.astype(np.float64) * x.astype(np.float64), "rne").astype(np.float64)
        err = (np.abs(approx - t) + np.abs(resc - t)) / scale
        assert np.all(err <= eps), (name, mode, flush, float(err.max()), eps)
        worst = max(worst, float(err.max()))
    assert 0 < worst < eps
