"""MaxSim search with the scoring pass on the matrix cores (index option "maxsim_mfma", csrc/maxsim_mfma.hpp) against a plain
float64 reference.  Contract (include/mvdb.h "MAXSIM SEARCH"): a score is an fp32 dot product in some summation order,
|s - s64| <= gamma * sum|q^_i x_i| with gamma = (d + 16) 2^-24; the tests allow 2 gamma (the reference's own roundings).

Corpus: 1,007 normalised Gaussian rows (31 full tiles of 32 and one of 15).  Groups: every row its own, but rows 50 .. 149 are ONE
group (it crosses the tile boundaries 64, 96, 128) and so are seven scattered rows.  Selection: all rows, a sorted list of 400
rows, and the same 400 as a bitmap (the excluded form of the other 607)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K, T_MAX = 1007, 10, 70
SCATTERED = [3, 200, 401, 402, 650, 900, 1006]
_WORLDS = {}


def world(d, poisoned=False):
    """(index, grouping, codes, q, float64 scores [T_MAX, N], float64 sum|q^ x| [T_MAX, N], row sets), built once per key."""
    if (d, poisoned) not in _WORLDS:
        from minivectordb_amd import _native
        rng = np.random.default_rng(500 + d)
        x = rng.standard_normal((N, d)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q = rng.standard_normal((T_MAX, d)).astype(np.float32)
        if poisoned:   # row 7 is NaN; row 300 holds +inf where every query vector holds 0: inf * 0, a NaN score
            x[7, 3], x[300, 5], q[:, 5] = np.nan, np.inf, 0.0
        idx = _native.FlatIndex(d)
        idx.add(x, normalize=False)
        codes = np.arange(N, dtype=np.int32)
        codes[50:150] = 50
        codes[SCATTERED] = 3
        x64 = idx.get_rows(0, N).astype(np.float64)
        qh = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            s64, a64 = qh @ x64.T, np.abs(qh) @ np.abs(x64).T
        chosen = np.sort(np.random.default_rng(9).permutation(N)[:400]).astype(np.int64)
        sets = {"all": (None, np.arange(N)), "list": (idx.rowset(chosen), chosen),
                "bitmap": (idx.rowset(np.setdiff1d(np.arange(N), chosen).astype(np.int64), excluded=True), chosen)}
        _WORLDS[(d, poisoned)] = (idx, idx.grouping(codes, N), codes, q, s64, a64, sets)
    return _WORLDS[(d, poisoned)]


def check(d, T, sel, poisoned=False):
    idx, grouping, codes, q, s64, a64, sets = world(d, poisoned)
    rs, rows = sets[sel]
    on = np.zeros(N, bool)
    on[rows] = True
    if poisoned:
        on[[7, 300]] = False   # their scores are NaN: never offered
    before = idx.maxsim_mfma_passes()
    D, G, I_tok, D_tok = idx.search_maxsim(q[:T], K, grouping, rowset=rs, normalize_q=True, matrix_cores=True)
    assert idx.maxsim_mfma_passes() - before == -(-T // 32)
    tol = 2 * (d + 16) * 2.0 ** -24 * a64[:T]                       # [T, N]
    best = np.full((T, N), -np.inf)                                   # float64 maximum of every (vector, group) over the selection
    np.maximum.at(best, (np.arange(T)[:, None], codes[on][None, :]), s64[:T, on])
    sums = np.sort(best.sum(axis=0))[::-1]                            # (a group without a selected row: -inf)
    slack = T * tol[:, on].max()
    assert np.all(G >= 0) and len(set(G.tolist())) == K
    for j in range(K):
        members = on & (codes == G[j])
        picked = I_tok[j]
        assert members[picked].all(), (j, G[j], picked)
        ref = s64[np.arange(T), picked]
        print(f"d {d} T {T} {sel} group {G[j]}: |D_tok - s64| / tol max {np.max(np.abs(D_tok[j] - ref) / tol[np.arange(T), picked]):.3f}")
        assert np.all(np.abs(D_tok[j] - ref) <= tol[np.arange(T), picked])
        assert np.all(best[:, G[j]] - ref <= tol[:, members].max(axis=1))
        assert abs(float(D[j]) - ref.sum()) <= tol[np.arange(T), picked].sum() + T * 2.0 ** -24 * abs(ref.sum())
        assert best[:, G[j]].sum() >= sums[K - 1] - slack - T * 2.0 ** -24 * abs(sums[K - 1])
    assert np.all(D[:-1] >= D[1:])
    return D, G, I_tok, D_tok


@pytest.mark.parametrize("sel", ["all", "list", "bitmap"])
@pytest.mark.parametrize("T", [1, 5, 32, 33, 70])
@pytest.mark.parametrize("d", [384, 512, 1024])
def test_matrix_core_pass_against_float64(gpu, d, T, sel):
    check(d, T, sel)


@pytest.mark.parametrize("sel", ["all", "bitmap"])
def test_nan_scores_are_never_offered(gpu, sel):
    D, G, I_tok, D_tok = check(512, 33, sel, poisoned=True)
    assert not np.isin([7, 300], G).any() and not np.isin([7, 300], I_tok).any()
    assert np.isfinite(D).all() and np.isfinite(D_tok).all()


def test_unsupported_width_takes_the_valu_pass(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(400)
    idx = _native.FlatIndex(400)
    idx.add(rng.standard_normal((N, 400)).astype(np.float32), normalize=True)
    grouping = idx.grouping((np.arange(N) // 4).astype(np.int32), N // 4 + 1)
    q = rng.standard_normal((33, 400)).astype(np.float32)
    want = idx.search_maxsim(q, K, grouping, normalize_q=True)
    idx.set_option("maxsim_mfma", 1)
    got = idx.search_maxsim(q, K, grouping, normalize_q=True)
    assert idx.maxsim_mfma_passes() == 0 and idx.maxsim_counters() == (2, 4)
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes()


def test_two_calls_give_the_same_bits(gpu):
    first, second = check(512, 33, "all"), check(512, 33, "all")
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_database_keyword_returns_the_same_documents(gpu, tmp_path):
    from minivectordb_amd import VectorDatabase
    docs, chunks, d, T = 50, 4, 64, 3
    n = docs * chunks
    rng = np.random.default_rng(12)   # (a seed whose gaps pass the assertion below)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((T, d)).astype(np.float32)
    qh = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    s = (qh @ x.astype(np.float64).T).reshape(T, docs, chunks)
    tol = 2 * (d + 16 + 3) * 2.0 ** -24 * (np.abs(qh) @ np.abs(x.astype(np.float64)).T).max()   # (+3: the store's own fp32 normalisation of a row)
    top2 = np.sort(s, axis=2)[:, :, -2:]
    sums = np.sort(s.max(axis=2).sum(axis=0))
    assert np.min(top2[:, :, 1] - top2[:, :, 0]) > 2 * tol and np.min(np.diff(sums)) > 2 * T * tol
    db = VectorDatabase(storage_file=str(tmp_path / "m.pkl"))
    db.store_embeddings_batch(list(range(n)), x, [{"doc": r // chunks} for r in range(n)])
    want = db.find_most_similar_maxsim(q, "doc", k=5)
    got = db.find_most_similar_maxsim(q, "doc", k=5, matrix_cores=True)
    assert db.index.maxsim_mfma_passes() == 1 and db.index.maxsim_counters() == (2, 2)
    assert list(got[0]) == list(want[0]) and got[2] == want[2]
    top = int(np.argmax(s.max(axis=2).sum(axis=0)))
    assert list(got[0][0]) == [top * chunks + int(c) for c in s[:, top].argmax(axis=1)]
