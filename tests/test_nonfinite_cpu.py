"""The fixtures and the reference of the non-finite tests (tests/nonfinite_cases.py), checked without a GPU: the reference agrees
with the oracle, the fp32 oracle agrees with float64 on every fixture (so id-for-id equality may be asked of the device), no
finite score can overflow, and the normalisation cases of the contract hold."""
import numpy as np
import pytest

from oracle import flat
from tests import nonfinite_cases as nf

DIMS = (128, 100, 3, 64, 80, 256, 768)    # every width tests/test_nonfinite_gpu.py searches
FIXTURES = [(n, d) for d in DIMS for n in (nf.N_BIG, nf.N_SMALL)]
METRICS = (flat.METRIC_IP, flat.METRIC_L2)


def _selections(n):
    return (("all", None), ("list", nf.row_list(n)))


def test_fixtures_hold_every_special_row_and_query():
    for n, d in FIXTURES:
        x = nf.corpus(n, d)
        kinds = set(nf.special_positions(n).values())
        assert kinds == {"nan", "nan_last", "pinf", "pinf0", "ninf", "mixed", "negzero", "zero", "dup"} - ({"pinf0"} if n < 256 else set())
        assert np.isnan(x[0]).any() and np.isnan(x[n - 1]).any() and np.isinf(x[n - 2]).any()
        dups = [r for r, kd in nf.special_positions(n).items() if kd == "dup"]
        assert len(dups) == 2 and all(np.array_equal(x[r], x[nf.DUP_SOURCE]) for r in dups)
        assert np.abs(x[np.isfinite(x)]).max() <= 1.0
        q = nf.query_set(x)
        assert np.isnan(q[1]).sum() == 1 and q[2, nf.COL_INF] == np.inf and q[3, nf.COL_INF] == -np.inf
        assert not q[4].any() and np.signbit(q[5, 0::2]).all() and not q[5, 0::2].any() and q[6, nf.COL_INF] == 0.0
        assert np.array_equal(q[7], x[nf.DUP_SOURCE])
        for nq in (1, 3, 5, 8, 20, 40, 130):
            qb, kb = nf.batch(x, nq)
            assert qb.shape == (nq, d) and len(kb) == nq
            if nq >= 11:
                assert sorted(k for k in kb if k != "plain") == sorted(nf.QUERY_KINDS[i] for i in nf.SPECIAL_QUERIES)
        keep = nf.keep_mask(n)
        plan = nf.special_positions(n)
        assert any(keep[r] for r in plan) and not all(keep[r] for r in plan) and keep[n - 1] and not keep[0]
        assert set(plan) <= set(nf.row_list(n).tolist())


@pytest.mark.parametrize("n,d", FIXTURES, ids=[f"n{n}-d{d}" for n, d in FIXTURES])
def test_reference_agrees_with_the_oracle_and_fp32_agrees_with_float64(n, d):
    x = nf.corpus(n, d)
    q = nf.query_set(x)
    kfull = n + 50
    for metric in METRICS:
        sgn = 1.0 if metric == flat.METRIC_IP else -1.0
        for normalize_q in (False, True):
            for name, rows in _selections(n):
                what = f"n={n} d={d} metric={metric} normalize_q={normalize_q} {name}"
                exps = nf.expected(x, q, kfull, metric, normalize_q, rows=rows)
                with np.errstate(all="ignore"):
                    D64, I64 = flat.flat_search(x, q, kfull, metric=metric, normalize_q=normalize_q, rows=rows, f64=True)
                    fp32 = [flat.flat_search(x, q, nf.K_EXACT, metric=metric, normalize_q=normalize_q, rows=rows, nthreads=t)
                            for t in (1, 4)]
                for i, e in enumerate(exps):
                    # the whole ranking against the oracle's float64 scan: ids everywhere, scores where finite, signs where not
                    Dw, Iw = e.lists(kfull)
                    assert np.array_equal(I64[i], Iw), f"{what} query {i}: float64 oracle ids differ from the reference"
                    fin = np.isfinite(Dw) & (Iw >= 0)
                    np.testing.assert_allclose(D64[i][fin], Dw[fin], rtol=1e-12, atol=1e-12, err_msg=what)
                    assert np.array_equal(D64[i][~fin].astype(np.float32), Dw[~fin].astype(np.float32)), f"{what} query {i}: infinities / padding differ"
                    # no finite score anywhere near fp32 overflow
                    assert np.abs(e.fin_scores).max(initial=0.0) < 1e31, what
                    # the near-tie condition: the fp32 oracle, sequential and threaded, ranks the first K_EXACT as float64 does
                    for Do, Io in fp32:
                        assert np.array_equal(Io[i], Iw[:nf.K_EXACT]), f"{what} query {i}: the fp32 oracle and float64 disagree: change the seeds"
                        f32fin = fin[:nf.K_EXACT]
                        assert np.abs(Do[i][f32fin] - Dw[:nf.K_EXACT][f32fin]).max(initial=0.0) <= nf.TOL, what
                        assert np.array_equal(Do[i][~f32fin].astype(np.float64), np.where(np.isinf(Dw[:nf.K_EXACT][~f32fin]), Dw[:nf.K_EXACT][~f32fin],
                                                                                        sgn * -float(nf.FLT_MAX))), what
                # the classes the tests are about do occur
                if name == "all":
                    assert any(len(e.pos) for e in exps) or metric == flat.METRIC_L2, what
                    assert any(len(e.neg) for e in exps) and any(e.n_nan == len(x) for e in exps), what


def _fp32_oracle_agrees_with_float64(x, q, metric, normalize_q, what, rows=None, keep=None, k=nf.K_EXACT, exempt=()):
    """The near-tie condition for one use of a fixture: the fp32 oracle ranks the first K_EXACT entries of every query as the
    float64 reference does, so nonfinite_cases.check holds the device to the oracle id for id on every query."""
    sel = np.flatnonzero(keep).astype(np.int64) if keep is not None else rows
    exps = nf.expected(x, q, k, metric, normalize_q, rows=rows, keep=keep)
    with np.errstate(all="ignore"):
        _, Io = flat.flat_search(x, nf.normalized(q, normalize_q), k, metric=metric, rows=sel)
    if keep is not None:
        Io = np.where(Io >= 0, sel[np.maximum(Io, 0)], -1)
    for i, e in enumerate(exps):
        if i not in exempt:
            assert np.array_equal(Io[i], e.lists(k)[1]), f"{what} query {i}: the fp32 oracle and float64 disagree: change the seeds"


# every other use tests/test_nonfinite_gpu.py makes of the fixtures: (d, metrics, batch sizes (0: the 11-query set), selection)
OTHER_USES = [(d, METRICS, (0,), sel) for d in (128, 100, 3) for sel in ("bitmap", "sparse")] + [
    (64, (flat.METRIC_IP,), (5, 20), "all"), (128, METRICS, (5, 20), "all"), (128, (flat.METRIC_IP,), (5, 20), "bitmap"),
    (80, (flat.METRIC_IP,), (8,), "all"), (128, (flat.METRIC_IP,), (130,), "all"), (768, (flat.METRIC_L2,), (5,), "all")]


@pytest.mark.parametrize("use", OTHER_USES, ids=[f"d{u[0]}-nq{'_'.join(map(str, u[2]))}-{u[3]}" for u in OTHER_USES])
def test_fp32_agrees_with_float64_on_the_batches_and_under_the_bitmaps(use):
    d, metrics, nqs, sel = use
    for n in (nf.N_BIG, nf.N_SMALL):
        x = nf.corpus(n, d)
        keep = {"all": None, "bitmap": nf.keep_mask(n), "sparse": nf.sparse_keep(n)}[sel]
        for nq in nqs:
            q = nf.query_set(x) if nq == 0 else nf.batch(x, nq)[0]
            for metric in metrics:
                for normalize_q in (False, True):
                    _fp32_oracle_agrees_with_float64(x, q, metric, normalize_q, f"n={n} d={d} nq={nq} metric={metric} "
                                                     f"normalize_q={normalize_q} {sel}", keep=keep)


@pytest.mark.parametrize("nq", [40, 130])
@pytest.mark.parametrize("variant", nf.CERTIFIED_VARIANTS)
def test_fp32_agrees_with_float64_on_the_certified_pass_fixtures(variant, nq):
    x, q, q_plain, special = nf.certified_fixture(variant, nq)
    assert np.isfinite(x).all() and len(special) == 4 and np.isfinite(q_plain).all()
    metric = flat.METRIC_IP if variant == "ip" else flat.METRIC_L2
    # One query cannot meet the condition whatever the seeds: the all-zero query under L2 over NORMALISED rows.  Every distance
    # is |x|^2 = 1 up to the rounding of the normalisation, so the whole ranking is a near-tie that fp32 and float64 order
    # differently.  The GPU test holds that query to float64 through flat.adjudicate (which knows near-ties) and to its own
    # single-query search bit for bit; the id-for-id clause of nonfinite_cases.check does not apply to it.
    zero = [i for i in special if not q[i].any()]
    assert len(zero) == 1
    for qq, name in ((q, "special"), (q_plain, "plain")):
        for normalize_q in (False, True):
            exempt = zero if variant == "l2-normalised-rows" and name == "special" else ()
            _fp32_oracle_agrees_with_float64(x, qq, metric, normalize_q, f"certified {variant} nq={nq} {name} normalize_q={normalize_q}",
                                             k=32, exempt=exempt)      # (the certified pass serves k <= 32: the GPU test runs 10 and 32)


@pytest.mark.parametrize("n,d", [(nf.N_BIG, 128), (nf.N_SMALL, 128)])
def test_reference_under_a_bitmap_is_the_oracle_over_the_kept_rows(n, d):
    x = nf.corpus(n, d)
    q = nf.query_set(x)
    keep = nf.keep_mask(n)
    sel = np.flatnonzero(keep)
    for metric in METRICS:
        exps = nf.expected(x, q, n, metric, keep=keep)
        with np.errstate(all="ignore"):
            _, I64 = flat.flat_search(x, q, n, metric=metric, rows=sel, f64=True)
        for i, e in enumerate(exps):
            _, Iw = e.lists(n)
            assert np.array_equal(np.where(I64[i] >= 0, sel[np.maximum(I64[i], 0)], -1), Iw), (metric, i)


def test_small_corpus_shows_the_whole_tail_at_k_32():
    """n = 37, k = 32 (a k every batch route serves): finite rows, then -inf rows, then padding, with NaN rows absent."""
    for d in DIMS:
        x = nf.corpus(nf.N_SMALL, d)
        q = nf.query_set(x)
        for metric in METRICS:
            e = nf.expected(x, q, 32, metric)[0]      # a plain query
            D, I = e.lists(32)
            assert len(e.fin) and len(e.neg) and e.n_nan >= 8 and (I[-2:] == -1).all(), (d, metric)
            assert len(e.pos) + len(e.fin) + len(e.neg) + e.n_nan == nf.N_SMALL


def test_check_refuses_the_faults_it_is_there_for():
    """The comparer itself: a NaN row listed first, a -inf row dropped, a -inf row listed under k > n, a wrong pad."""
    n, d, k = nf.N_SMALL, 128, 32
    x = nf.corpus(n, d)
    q = nf.query_set(x)[:1]
    e = nf.expected(x, q, k)[0]
    D, I = e.lists(k)
    D, I = D.astype(np.float32)[None], I[None]
    nf.check(D, I, x, q, k)
    c = len(e.pos) + len(e.fin) + len(e.neg)
    assert c < k and len(e.neg)

    def broken(edit):
        D2, I2 = D.copy(), I.copy()
        edit(D2[0], I2[0])
        with pytest.raises(AssertionError):
            nf.check(D2, I2, x, q, k)

    def nan_first(D2, I2):
        D2[1:], I2[1:] = D2[:-1].copy(), I2[:-1].copy()
        D2[0], I2[0] = np.inf, 0

    def neg_dropped(D2, I2):
        D2[c - 1], I2[c - 1] = -nf.FLT_MAX, -1

    def nan_as_neg_inf(D2, I2):
        D2[c], I2[c] = -np.inf, 0

    def wrong_pad(D2, I2):
        D2[-1] = -np.inf

    for edit in (nan_first, neg_dropped, nan_as_neg_inf, wrong_pad):
        broken(edit)


def test_normalisation_cases_of_the_contract():
    """fvec_renorm_L2 literally: nr = inf multiplies by 0 (inf * 0 = NaN, finite * 0 = 0), nr = NaN and nr = 0 leave the query."""
    d = 8
    base = flat.synth(1, d, 5)[0]
    qi = base.copy()
    qi[nf.COL_INF] = np.inf
    got = nf.normalized(qi, True)[0]
    assert np.isnan(got[nf.COL_INF]) and not np.delete(got, nf.COL_INF).any()
    qm = base.copy()
    qm[nf.COL_INF] = -np.inf
    got = nf.normalized(qm, True)[0]
    assert np.isnan(got[nf.COL_INF]) and not np.delete(got, nf.COL_INF).any()
    qnan = base.copy()
    qnan[nf.COL_NAN] = np.nan
    assert np.array_equal(nf.normalized(qnan, True)[0], qnan, equal_nan=True)
    z = np.zeros(d, np.float32)
    assert np.array_equal(nf.normalized(z, True)[0], z)
    # ... and what they do to a search: every row scores NaN for the first three, every finite row 0 for the last
    x = nf.corpus(nf.N_SMALL, 128)
    q = nf.query_set(x)
    for metric in METRICS:
        exps = nf.expected(x, q, 10, metric, normalize_q=True)
        for i in (1, 2, 3):
            assert exps[i].n_nan == nf.N_SMALL, (metric, i)
            assert (exps[i].lists(10)[1] == -1).all()
    zero = nf.expected(x, q, 10, flat.METRIC_IP, normalize_q=True)[4]
    assert not zero.fin_scores.any() and zero.lists(3)[1].tolist() == [1, 2, 3]
