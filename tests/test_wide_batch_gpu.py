"""The certified batch pass at d = 1536 / 2048 / 3072 / 4096 (index option "wide_shadow", half_wide_scan.hip; DESIGN.md section
4.3h) against the CPU oracle under bigcheck.compare.  Every index runs with "wide_shadow_blocks" = 8: a workgroup of
flat_scan_h16_wide_kernel walks a dozen 32-row tiles, its ring wraps many times, and the last tile is ragged."""
import numpy as np
import pytest

from oracle import flat

import bigcheck

pytestmark = pytest.mark.gpu

N = 32 * 96 + 5
LABEL = "ip_scan_half_wide"
_cache = {}


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    return _native


def _tie_eps(d):
    """bigcheck's 2e-6, or — where it is larger — the worst case of the fp32 re-score that ranks the results: the depth term of
    half_wide_eps (4 ceil(d / 256) + 6 roundings of 2^-24) times |q| max|x| = 1 for unit queries and rows."""
    depth = ((d + 3) // 4 + 63) // 64 * 4 + 6
    return max(bigcheck.TIE_EPS, depth * 2.0 ** -24 / (1 - depth * 2.0 ** -24))


def _rows(family, d):
    rs = np.random.RandomState(d + len(family))
    if family == "gaussian":
        return rs.randn(N, d).astype(np.float32)
    if family == "positive":
        return (rs.rand(N, d) + 0.5).astype(np.float32)
    return np.repeat(rs.randn(39, d).astype(np.float32), 80, axis=0)   # "copies": 3120 rows, every distinct row 80 times


def _case(native, family, d):
    """One index per (family, d) with 257 unit queries and the oracle's top 16 of each, computed once and left unchanged."""
    if (family, d) not in _cache:
        idx = native.FlatIndex(d, device=0)
        idx.set_option("wide_shadow_blocks", 8)
        idx.add(_rows(family, d), normalize=True)
        q = np.random.RandomState(7 * d).randn(257, d).astype(np.float32)
        flat.normalize_l2(q)
        Do, Io = flat.flat_search(idx.get_rows(0, idx.ntotal), q, 16, nthreads=8)
        _cache[(family, d)] = (idx, q, Do, Io)
    return _cache[(family, d)]


def _search(native, idx, q, k, option, call=None):
    """(D, I, launches under LABEL) of one call with "wide_shadow" = option"""
    idx.set_option("wide_shadow", option)
    native.prof_enable(True)
    try:
        native.prof_read(LABEL)
        D, I = call() if call else idx.search(q, k)
        return D, I, native.prof_read(LABEL)[0]
    finally:
        native.prof_enable(False)


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("nq", [33, 64, 100, 257])
@pytest.mark.parametrize("d", [1536, 2048, 3072, 4096])
def test_wide_batch_matches_oracle(native, d, nq, k):
    idx, q, Do, Io = _case(native, "gaussian", d)
    assert _search(native, idx, q[:nq], k, 0)[2] == 0
    before = native.split_rerun_count()
    D, I, launches = _search(native, idx, q[:nq], k, 1)
    assert launches > 0
    if k == 1:   # the best of 3077 unit Gaussian rows scores ~3.4 / sqrt(d), the best row any list drops ~2.3 / sqrt(d): a gap of
        # 0.017 at d = 4096 against a band of 1e-3 — every certificate holds, so the answers are the wide kernel's nominees
        assert native.split_rerun_count() == before
    bigcheck.compare(idx, q[:nq], D, I, Do[:nq, :k], Io[:nq, :k], f"wide d={d} nq={nq} k={k}", tie_eps=_tie_eps(d))


@pytest.mark.parametrize("family", ["positive", "copies"])
@pytest.mark.parametrize("d", [1536, 4096])
def test_wide_batch_families(native, d, family):
    idx, q, Do, Io = _case(native, family, d)
    before = native.split_rerun_count()
    D, I, launches = _search(native, idx, q[:100], 10, 1)
    assert launches > 0
    if family == "copies":   # the 64 nominees of every query tie: every certificate is refused, the gated exact re-run answers
        assert native.split_rerun_count() > before
    bigcheck.compare(idx, q[:100], D, I, Do[:100, :10], Io[:100, :10], f"wide {family} d={d}", tie_eps=_tie_eps(d))


@pytest.mark.parametrize("d", [1536, 4096])
def test_wide_batch_after_mutations(native, d):
    idx = native.FlatIndex(d, device=0)
    idx.set_option("wide_shadow_blocks", 8)
    idx.add(_rows("gaussian", d), normalize=True)
    q = _case(native, "gaussian", d)[1][:64]
    assert _search(native, idx, q, 10, 1)[2] > 0   # (the shadow exists before the rows change)
    idx.set_rows(np.array([0, 31, 1000, N - 1]), q[:4].copy())   # four queries become rows: their best hits move
    idx.remove_rows(np.array([5, 2000]))
    D, I, launches = _search(native, idx, q, 10, 1)
    assert launches > 0 and I[0, 0] == 0 and idx.ntotal == N - 2
    Do, Io = flat.flat_search(idx.get_rows(0, idx.ntotal), q, 10, nthreads=8)
    bigcheck.compare(idx, q, D, I, Do, Io, f"wide mutated d={d}", tie_eps=_tie_eps(d))
    idx.close()


def test_wide_out_of_scope_calls_are_served_as_before(native):
    d = 1536
    idx, q, _, _ = _case(native, "gaussian", d)
    q = q[:64]
    words = native.pack_row_mask(idx.ntotal, rows=np.arange(0, idx.ntotal, 3))
    l2 = native.FlatIndex(d, metric=native.METRIC_L2, device=0)
    l2.add(idx.get_rows(0, 2000))
    for what, index, call in (("masked", idx, lambda: idx.search_masked(q, 10, words)), ("k = 32", idx, lambda: idx.search(q, 32)),
                              ("L2", l2, lambda: l2.search(q, 10))):
        D0, I0, _ = _search(native, index, q, 10, 0, call)
        D1, I1, launches = _search(native, index, q, 10, 1, call)
        assert launches == 0, what
        assert np.array_equal(D0, D1) and np.array_equal(I0, I1), what
    l2.close()
