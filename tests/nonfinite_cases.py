"""Corpora, queries and the reference of the non-finite tests (tests/test_nonfinite_cpu.py, tests/test_nonfinite_gpu.py), kept
free of any GPU import so that the CPU test can check the fixtures and the reference on any machine.

The contract under test ("Non-finite rows and queries"): the key score of a row is q.x (IP) or
-sum (q_j - x_j)^2 (L2) in the DIRECT form; a row whose key score is NaN is never a result; +inf scores come first, -inf scores
after every finite one, equal scores (the infinities included) by the lower label; the slots left are I = -1, D = -/+FLT_MAX.

Every finite element is a synthetic value in (-1, 1): no finite product, square or sum can overflow, so the class of a row's
score — NaN, +inf, -inf or finite — is decided by its non-finite TERMS alone and does not depend on the summation order.

Id-for-id equality with the fp32 oracle is asked of the first K_EXACT = 64 entries of a result: the fixtures are chosen (and the
CPU test checks) so that the fp32 oracle and float64 agree there for every query.  Beyond 64 entries — the radix-select route
lists up to all 2003 rows — neighbouring float64 scores are ~1e-3 / 2003 apart, within the reach of fp32 summation order, so no
seed makes two fp32 implementations agree id for id; there the finite stretch is held to float64 by flat.adjudicate alone.
"""
import numpy as np

from oracle import flat

TOL = 1e-4                     # tests/test_flat_gpu.py: distances within 1e-4 of the float64 score
K_EXACT = 64                   # entries of a result compared id for id with the fp32 oracle
FLT_MAX = np.float32(3.4028234663852886e38)
INF = np.float32(np.inf)

N_BIG, N_SMALL = 2003, 37      # no multiple of 16 or 128, several blocks / the whole tail visible at k = 32
COL_NAN, COL_INF = 1, 2        # where the NaN rows / the inf rows and queries hold their special element (d >= 3)
DUP_SOURCE = 5                 # the plain row that the duplicate rows and the "copy" query repeat

CORPUS_SEED, QUERY_SEED = 4321, 8765
QUERY_SEED_BY_WIDTH = {768: 9533}   # widths at which QUERY_SEED leaves a near-tie among the first K_EXACT (tests/test_nonfinite_cpu.py)


def query_seed(d):
    return QUERY_SEED_BY_WIDTH.get(d, QUERY_SEED)


def special_positions(n):
    """{row: kind}.  The MFMA 16-row tile edges (0, 15, 16, 17), the wave and GEMM 128-row tile edges (63, 64, 127, 128), one
    row mid-corpus and the clamped tail (n - 2, n - 1: the tail lanes of every scan re-read the last row, a NaN row)."""
    if n >= 256:
        return {0: "nan", 15: "pinf", 16: "ninf", 17: "mixed", 63: "negzero", 64: "dup", 127: "zero", 128: "pinf0",
                n // 2: "dup", n - 2: "ninf", n - 1: "nan_last"}
    # the small corpus: six more NaN rows, so that fewer than 32 rows can be results at all
    plan = {0: "nan", 15: "pinf", 16: "ninf", 17: "mixed", n // 2: "negzero", 20: "dup", 21: "zero", 22: "dup",
            n - 2: "ninf", n - 1: "nan_last"}
    plan.update({r: "nan" for r in range(23, 29)})
    return plan


def corpus(n, d, seed=CORPUS_SEED, special=True):
    """n x d synthetic rows (oracle stream `seed`, not normalised) with the special rows of special_positions() planted."""
    assert d >= 3 and n > 30
    x = flat.synth(n, d, seed)
    if not special:
        return x
    for r, kind in special_positions(n).items():
        if kind == "nan":
            x[r, COL_NAN] = np.nan
        elif kind == "nan_last":
            x[r, d - 1] = np.nan
        elif kind == "pinf":
            x[r, COL_INF] = np.inf
        elif kind == "pinf0":
            x[r, 0] = np.inf
        elif kind == "ninf":
            x[r, COL_INF] = -np.inf
        elif kind == "mixed":
            x[r, 0] = np.inf
            x[r, COL_INF] = -np.inf
        elif kind == "negzero":
            x[r] = -0.0
        elif kind == "zero":
            x[r] = 0.0
        elif kind == "dup":
            x[r] = x[DUP_SOURCE]
    return x


QUERY_KINDS = ("plain", "nan", "pinf", "ninf", "zero", "negzero_even", "zero_at_inf", "copy", "plain", "plain", "plain")
SPECIAL_QUERIES = (1, 2, 3, 4, 5, 6, 7)     # positions of the special kinds in QUERY_KINDS
NONFINITE_OR_ZERO_QUERIES = (1, 2, 3, 4)    # ... of those the certified fp16 pass cannot bound: NaN, +inf, -inf, all zero


def query_set(x, seed=None):
    """The 11 queries of QUERY_KINDS for corpus x: a plain set plus one each of a NaN element, +inf, -inf, all zero, -0.0 on the
    even columns, exactly 0.0 in the column of the inf rows, and a copy of a stored row (which has exact duplicates)."""
    d = x.shape[1]
    seed = query_seed(d) if seed is None else seed
    q = flat.synth(len(QUERY_KINDS), d, seed)
    for i, kind in enumerate(QUERY_KINDS):
        if kind == "nan":
            q[i, COL_NAN] = np.nan
        elif kind == "pinf":
            q[i, COL_INF] = np.inf
        elif kind == "ninf":
            q[i, COL_INF] = -np.inf
        elif kind == "zero":
            q[i] = 0.0
        elif kind == "negzero_even":
            q[i, 0::2] = -0.0
        elif kind == "zero_at_inf":
            q[i, COL_INF] = 0.0
        elif kind == "copy":
            q[i] = flat.synth(1, d, CORPUS_SEED, first_row=DUP_SOURCE)[0]
    return q


def batch(x, nq, seed=None):
    """(queries [nq, d], kinds): the special queries spread over a batch of nq — every one of them from 11 queries on, the ones
    a smaller batch has room for below that — and plain queries in between."""
    seed = query_seed(x.shape[1]) if seed is None else seed
    base = query_set(x, seed)
    if nq >= len(QUERY_KINDS):
        q = flat.synth(nq, x.shape[1], seed + 1)
        kinds = ["plain"] * nq
        # special query j at slot j * nq / 7 (+ 1 for odd j): different 16-query groups, different accumulator registers
        for j, src in enumerate(SPECIAL_QUERIES):
            at = j * nq // len(SPECIAL_QUERIES) + (j & 1)
            q[at] = base[src]
            kinds[at] = QUERY_KINDS[src]
        return q, kinds
    pick = {1: (2,), 3: (2, 0, 6), 5: (1, 2, 6, 0, 7), 8: (1, 2, 3, 4, 6, 0, 7, 8)}[nq]
    return base[list(pick)].copy(), [QUERY_KINDS[i] for i in pick]


def keep_mask(n, seed=7):
    """bool[n]: about two rows in three, excluding some of the special rows (the first NaN row, a -inf row, one duplicate, the
    zero row) and keeping the others (the last NaN row, the +inf rows, the other -inf row, the other duplicate)."""
    rng = np.random.default_rng(seed + n)
    keep = rng.random(n) < 0.66
    plan = special_positions(n)
    keep[list(plan)] = True
    first_of = {}
    for r in sorted(plan):
        first_of.setdefault(plan[r], r)
    for kind in ("nan", "ninf", "dup", "zero"):
        keep[first_of[kind]] = False
    return keep


def sparse_keep(n):
    """bool[n]: every special row and one in four of row_list(n) — few enough rows that a resident row set keeps them as a list."""
    keep = np.zeros(n, dtype=bool)
    keep[np.sort(row_list(n))[::4]] = True
    keep[list(special_positions(n))] = True
    return keep


CERTIFIED_D = 256
CERTIFIED_VARIANTS = ("ip", "l2-normalised-rows", "l2-mixed-norms")


def certified_fixture(variant, nq):
    """(x, q, q_plain, special) of the certified-pass test: 2003 FINITE rows of width 256 (normalised for the norm-range
    certificate of L2), a batch with the special queries, the same batch with the four queries the pass cannot bound — NaN,
    +inf, -inf, all zero — replaced by plain ones, and the positions of those four."""
    x = corpus(N_BIG, CERTIFIED_D, special=False)
    if variant == "l2-normalised-rows":
        flat.normalize_l2(x)
    q, kinds = batch(x, nq)
    special = [i for i, kd in enumerate(kinds) if kd in ("nan", "pinf", "ninf", "zero")]
    q_plain = q.copy()
    q_plain[special] = flat.synth(len(special), CERTIFIED_D, 99)
    return x, q, q_plain, special


def row_list(n, seed=11):
    """int64[m]: a permuted row list (labels are positions in it) holding every special row, about one row in four otherwise."""
    rng = np.random.default_rng(seed + n)
    take = rng.random(n) < 0.25
    take[list(special_positions(n))] = True
    take[DUP_SOURCE] = True
    rows = np.flatnonzero(take).astype(np.int64)
    rng.shuffle(rows)
    return rows


def normalized(q, normalize_q):
    """The query as the search sees it: normalised in fp32 as the oracle does (fvec_renorm_L2: nr > 0 false leaves it, nr = inf
    multiplies by 0)."""
    q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float32).copy()
    if normalize_q:
        with np.errstate(all="ignore"):
            flat.normalize_l2(q)
    return q


class Expected:
    """One query's expected result: labels scoring +inf (ascending), the finite ones ranked in float64 (score desc, label asc)
    with their key scores, labels scoring -inf (ascending); rows scoring NaN are in none of them."""

    def __init__(self, pos, fin, fin_scores, neg, n_nan, metric):
        self.pos, self.fin, self.fin_scores, self.neg, self.n_nan, self.metric = pos, fin, fin_scores, neg, n_nan, metric

    def lists(self, k):
        """(D float64 [k], I int64 [k]) in the order of the contract; D as the API reports it (distance for L2)."""
        sgn = 1.0 if self.metric == flat.METRIC_IP else -1.0
        I = np.concatenate([self.pos, self.fin, self.neg])[:k]
        D = np.concatenate([np.full(len(self.pos), np.inf), self.fin_scores, np.full(len(self.neg), -np.inf)])[:k] * sgn
        pad = k - len(I)
        return (np.concatenate([D, np.full(pad, -sgn * float(FLT_MAX))]),
                np.concatenate([I, np.full(pad, -1)]).astype(np.int64))


def key_scores(xs, q1, metric):
    """(score float64 [m], class int8 [m]) of the rows xs against one prepared query, from the direct form term by term.
    class: 0 finite, 1 +inf, -1 -inf, 2 NaN."""
    with np.errstate(all="ignore"):
        X = xs.astype(np.float64)
        qq = q1.astype(np.float64)[None, :]
        if metric == flat.METRIC_IP:
            terms = X * qq
        else:
            t = qq - X
            terms = -(t * t)
        has_nan = np.isnan(terms).any(axis=1)
        has_p = (terms == np.inf).any(axis=1)
        has_n = (terms == -np.inf).any(axis=1)
        cls = np.zeros(len(X), dtype=np.int8)
        cls[has_p] = 1
        cls[has_n] = -1
        cls[has_nan | (has_p & has_n)] = 2
        s = np.where(np.isfinite(terms), terms, 0.0).sum(axis=1)
    s[cls == 1] = np.inf
    s[cls == -1] = -np.inf
    s[cls == 2] = np.nan
    return s, cls


def expected(x, q, k, metric=flat.METRIC_IP, normalize_q=False, rows=None, keep=None):
    """[Expected] per query.  rows: a row list (labels = positions in it); keep: bool[n] (labels = row numbers)."""
    del k   # the expectation is the whole ranking: Expected.lists(k) cuts it
    x = np.asarray(x, dtype=np.float32)
    if rows is not None:
        xs, labels = x[np.asarray(rows)], np.arange(len(rows), dtype=np.int64)
    elif keep is not None:
        labels = np.flatnonzero(keep).astype(np.int64)
        xs = x[labels]
    else:
        xs, labels = x, np.arange(len(x), dtype=np.int64)
    out = []
    for q1 in normalized(q, normalize_q):
        s, cls = key_scores(xs, q1, metric)
        f = np.flatnonzero(cls == 0)
        f = f[np.lexsort((labels[f], -s[f]))]
        out.append(Expected(labels[cls == 1], labels[f], s[f], labels[cls == -1], int((cls == 2).sum()), metric))
    return out


def check(D, I, x, q, k, metric=flat.METRIC_IP, normalize_q=False, rows=None, keep=None, what=""):
    """Assert a [nq, k] result against the contract: the non-finite placement and the padding exactly, the finite stretch through
    flat.adjudicate (restricted to the finite-scoring rows) within TOL, and the first K_EXACT ids equal to the fp32 oracle's
    wherever the oracle itself agrees with float64 there."""
    x = np.asarray(x, dtype=np.float32)
    qn = normalized(q, normalize_q)
    D, I = np.asarray(D), np.asarray(I)
    assert D.shape == (len(qn), k) and I.shape == (len(qn), k), (what, D.shape, I.shape)
    ip = metric == flat.METRIC_IP
    worst = -INF if ip else INF       # what D shows for a key score of -inf
    exps = expected(x, q, k, metric, normalize_q, rows, keep)
    if keep is not None:              # the oracle searches the ascending list of the kept rows: positions -> row numbers
        sel = np.flatnonzero(keep).astype(np.int64)
    else:
        sel = None if rows is None else np.asarray(rows, dtype=np.int64)
    ke = min(k, K_EXACT)
    with np.errstate(all="ignore"):
        Do, Io = flat.flat_search(x, qn, ke, metric=metric, rows=sel)
    if keep is not None:
        Io = np.where(Io >= 0, sel[np.maximum(Io, 0)], -1)
    for i, e in enumerate(exps):
        w = f"{what} query {i}"
        Dw, Iw = e.lists(k)
        n_pos, n_fin, n_neg = (min(k, len(e.pos)), min(max(k - len(e.pos), 0), len(e.fin)),
                               min(max(k - len(e.pos) - len(e.fin), 0), len(e.neg)))
        a, b, c = n_pos, n_pos + n_fin, n_pos + n_fin + n_neg
        got_I, got_D = I[i], D[i]
        # ---- exact: +inf head, -inf tail, padding; NaN rows nowhere -------------------------------------------------
        assert got_I[:a].tolist() == Iw[:a].tolist(), f"{w}: +inf rows {got_I[:a].tolist()} != {Iw[:a].tolist()}"
        assert (got_D[:a] == INF).all(), f"{w}: +inf scores {got_D[:a]}"
        assert got_I[b:c].tolist() == Iw[b:c].tolist(), f"{w}: -inf rows {got_I[b:c].tolist()} != {Iw[b:c].tolist()}"
        assert (got_D[b:c] == worst).all(), f"{w}: -inf scores {got_D[b:c]}"
        assert (got_I[c:] == -1).all(), f"{w}: padding ids {got_I[c:].tolist()} ({e.n_nan} rows score NaN)"
        assert (got_D[c:] == (-FLT_MAX if ip else FLT_MAX)).all(), f"{w}: padding scores {got_D[c:]}"
        # ---- the finite stretch: finite-scoring rows only, adjudicated in float64 over exactly those rows ----------------
        fin_sorted = np.sort(e.fin)
        seg_I, seg_D = got_I[a:b], got_D[a:b]
        assert np.isfinite(seg_D).all(), f"{w}: non-finite score in the finite stretch {seg_D}"
        assert np.isin(seg_I, fin_sorted).all(), f"{w}: {seg_I[~np.isin(seg_I, fin_sorted)].tolist()} do not score finite"
        if n_fin:
            phys = fin_sorted if sel is None else sel[fin_sorted] if keep is None else fin_sorted
            ok, msg = flat.adjudicate(x, qn[i], n_fin, seg_D, np.searchsorted(fin_sorted, seg_I), metric=metric, rows=phys, tol=TOL)
            assert ok, f"{w}: {msg}"
        # ---- id for id with the fp32 oracle where it agrees with float64 -------------------------------------------------
        if np.array_equal(Io[i], Iw[:ke]):
            assert got_I[:ke].tolist() == Io[i].tolist(), f"{w}: ids differ from the fp32 oracle: {got_I[:ke].tolist()} != {Io[i].tolist()}"
            fin = np.isfinite(Do[i]) & (Io[i] >= 0)
            assert np.abs(got_D[:ke][fin].astype(np.float64) - Do[i][fin]).max(initial=0.0) <= TOL, w
    return exps
