"""The RaBitQ index (csrc/rabitq.hip) and RabitqVectorDatabase.  The contract is a few lines of numpy: the rotation, the encode
rule, the query rule and the score, every fp32 operation on its own.  Searches are compared with array_equal, D as bits, against
the score of the codes, factors and query parameters read back from the index; only f, g and qc — fp64 sums in an order the
contract leaves open — get one fp32 ulp."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
F15 = np.float32(15)
WIDTHS = [128, 384, 1024, 3072, 4096]   # 384 and 3072: the window is not the row, odd rounds take [d - P, d)


def rotate(x, signs):
    x, d = x.copy(), x.shape[1]
    P = 1 << (d.bit_length() - 1)
    for r, s in enumerate(signs):
        neg = np.unpackbits(s).astype(bool)
        x[:, neg] = -x[:, neg]
        at = d - P if r & 1 else 0
        w = np.ascontiguousarray(x[:, at:at + P])
        h = 1
        while h < P:
            v = w.reshape(len(x), P // (2 * h), 2, h)
            a, b = v[:, :, 0].copy(), v[:, :, 1].copy()
            v[:, :, 0], v[:, :, 1] = a + b, a - b
            h *= 2
        x[:, at:at + P] = w * np.float32(1 / np.sqrt(P))
    return x


def encode(x, c, signs):
    """codes, and (f, g) in float64"""
    res = x - c
    r = rotate(res, signs).astype(np.float64)
    l1 = np.abs(r).sum(1)
    f = np.divide((r * r).sum(1), l1, out=np.zeros_like(l1), where=l1 > 0)
    return np.packbits(r > 0, axis=1), np.stack([f, (res.astype(np.float64) * c.astype(np.float64)).sum(1)], axis=1)


def query_rule(q, c, signs):
    """u, and (lo, delta, qc, U) in float64 (lo, delta and U hold fp32 values)"""
    qp = rotate(q - c, signs)
    lo, span = qp.min(1), qp.max(1) - qp.min(1)
    with np.errstate(all="ignore"):
        delta, inv = np.where(span > 0, span / F15, 0).astype(np.float32), np.where(span > 0, F15 / span, 0).astype(np.float32)
    u = np.clip(np.rint((qp - lo[:, None]) * inv[:, None]), 0, 15).astype(np.uint8)
    return u, np.stack([lo, delta, (q.astype(np.float64) * c.astype(np.float64)).sum(1), u.sum(1, dtype=np.int64)], axis=1)


def one_ulp(got, want):
    return (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


def scores(u, prm, codes, fac):
    """S [nq, n] in float32, one rounding per operation.  T runs through BLAS in float32: every partial sum is an integer below
    15 * 4096 < 2^24, exact in any order."""
    bits = np.unpackbits(codes, axis=1).astype(np.float32)
    T = u.astype(np.float32) @ bits.T
    B = 2 * bits.sum(1) - np.float32(bits.shape[1])
    lo, delta, qc, U = (prm[:, i:i + 1] for i in range(4))
    e = delta * (2 * T - U) + lo * B[None]
    return fac[None, :, 0] * e + (fac[None, :, 1] + qc)


def top64(S, selected=None):
    """per query the 64 best selected rows by (-S, row): the top k of every k <= 64 is a prefix; padding -FLT_MAX / -1"""
    rows = np.arange(S.shape[1]) if selected is None else np.flatnonzero(selected)
    D, I = np.full((len(S), 64), -FMAX, np.float32), np.full((len(S), 64), -1, np.int64)
    for i, s in enumerate(S[:, rows]):
        best = np.lexsort((rows, -s))[:64]
        D[i, :len(best)], I[i, :len(best)] = s[best], rows[best]
    return D, I, None if selected is None else rows


def check(idx, top, q, nq, k, form=0):
    from minivectordb_amd import _native
    mask = None if top[2] is None else _native.pack_row_mask(idx.ntotal, rows=top[2])
    D, I = idx.search(q[:nq], k, mask, form=form)
    assert np.array_equal(I, top[1][:nq, :k]), (idx.ntotal, nq, k, form, np.argwhere(I != top[1][:nq, :k])[:4])
    assert np.array_equal(D.view(np.uint32), top[0][:nq, :k].view(np.uint32)), (idx.ntotal, nq, k, form)


def make_index(rng, d, rounds=4, centred=True):
    from minivectordb_amd import _native
    idx = _native.RabitqIndex(d)
    idx.set_rotation(rng.integers(0, 256, (rounds, d // 8), dtype=np.uint8))
    if centred:
        idx.set_centroid(rng.standard_normal(d).astype(np.float32) / 4)
    return idx


def random_rows(rng, n, d):
    return rng.integers(0, 256, (n, d // 8), dtype=np.uint8), rng.uniform(0.5, 1.5, (n, 2)).astype(np.float32)


def handover(idx):
    return next(nq for nq in range(1, 65) if idx.geometry(nq, 10)[0] == 2)


@pytest.mark.parametrize("rounds", [0, 4])
@pytest.mark.parametrize("d", WIDTHS)
def test_encode_and_query_equal_the_rule(gpu, d, rounds):
    rng = np.random.default_rng(d + rounds)
    idx = make_index(rng, d, rounds)
    signs, c = idx.get_rotation(), idx.get_centroid()
    assert signs.shape == (rounds, d // 8)
    x = (rng.standard_normal((70, d)) * (rng.random((70, d)) > 0.2)).astype(np.float32)   # a fifth of the entries exactly 0
    idx.add(x)
    codes, fac = idx.get_rows(0, 70)
    wcodes, wfac = encode(x, c, signs)
    assert np.array_equal(codes, wcodes)
    assert one_ulp(fac, wfac)
    with pytest.raises(ValueError):
        idx.set_centroid(c)   # rows are stored
    u, prm = idx.query(x[:9])
    wu, wprm = query_rule(x[:9], c, signs)
    assert np.array_equal(u, wu)
    assert np.array_equal(prm[:, [0, 1, 3]].view(np.uint32), wprm[:, [0, 1, 3]].astype(np.float32).view(np.uint32))
    assert one_ulp(prm[:, 2], wprm[:, 2])
    idx.close()


@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("d", WIDTHS)
def test_search_equals_oracle(gpu, d, n):
    """nq: every VALU pass width, a dead query in a pass, both sides of the hand-over, two blocks of 32 queries, a ragged
    third; 9 queries through either form by force.  k = 64 > n pads."""
    rng = np.random.default_rng(d + n)
    idx = make_index(rng, d)
    codes, fac = random_rows(rng, n, d)
    idx.add_codes(codes, fac)
    assert all(np.array_equal(a, b) for a, b in zip(idx.get_rows(0, n), (codes, fac)))
    q = rng.standard_normal((70, d)).astype(np.float32)
    top = top64(scores(*idx.query(q), codes, fac))
    H = handover(idx)
    assert idx.geometry(H - 1, 10)[0] == 1
    for k in (1, 10, 64):
        for nq in (1, 3, 4, H - 1, H, 33, 70):
            check(idx, top, q, nq, k)
        check(idx, top, q, 9, k, form=1)
        check(idx, top, q, 9, k, form=2)
    with pytest.raises(ValueError):
        idx.search(q[:1], 65)
    idx.close()


def test_one_row_past_a_grid_stride(gpu):
    """The last row is the sign pattern that maximises e for query 0, with f a hundred times any other row's."""
    rng = np.random.default_rng(5)
    d = 128
    idx = make_index(rng, d)
    q = rng.standard_normal((handover(idx), d)).astype(np.float32)
    u, prm = idx.query(q)
    for nq in (1, len(q)):
        n = idx.geometry(nq, 10)[1] + 1
        codes, fac = random_rows(rng, n, d)
        codes[-1] = np.packbits(prm[0, 0] + prm[0, 1] * u[0].astype(np.float32) > 0)
        fac[-1] = 100, 0
        idx.reset()
        idx.add_codes(codes, fac)
        D, I = idx.search(q[:nq], 10)
        assert I[0, 0] == n - 1 and (I[:, 0] >= 0).all()
        assert D[0, 0].view(np.uint32) == scores(u[:1], prm[:1], codes[-1:], fac[-1:])[0, 0].view(np.uint32)
    idx.close()


@pytest.mark.parametrize("form", [1, 2])
def test_identical_rows_go_to_the_lower_row(gpu, form):
    rng = np.random.default_rng(form)
    d, n = 384, 3000
    idx = make_index(rng, d)
    codes, fac = random_rows(rng, 1, d)
    idx.add_codes(np.repeat(codes, n, axis=0), np.repeat(fac, n, axis=0))
    D, I = idx.search(rng.standard_normal((9, d)).astype(np.float32), 64, form=form)
    assert np.array_equal(I, np.tile(np.arange(64), (9, 1))) and (D == D[:, :1]).all()
    idx.close()


@pytest.mark.parametrize("nq", [3, 33])
def test_bitmap(gpu, nq):
    rng = np.random.default_rng(nq)
    d, n = 1024, 4097
    idx = make_index(rng, d)
    codes, fac = random_rows(rng, n, d)
    idx.add_codes(codes, fac)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    S = scores(*idx.query(q), codes, fac)
    for selected in (np.arange(n) % 2 == 0, np.zeros(n, bool), np.arange(n) >= 4096):
        check(idx, top64(S, selected), q, nq, 10)
    idx.close()


def test_mutations_equal_a_fresh_index(gpu):
    rng = np.random.default_rng(7)
    d, n = 384, 5000
    x = rng.standard_normal((n, d)).astype(np.float32)
    idx, fresh = make_index(rng, d), make_index(rng, d)
    fresh.set_rotation(idx.get_rotation())
    fresh.set_centroid(idx.get_centroid())
    idx.add(x[:4000])
    gone = rng.permutation(4000)[:300]
    idx.remove_rows(gone)
    x = np.delete(x, gone, axis=0)
    changed = rng.permutation(3700)[:200]
    x[changed] = rng.standard_normal((200, d)).astype(np.float32)
    idx.set_rows(changed, x[changed])
    idx.add(x[3700:4200])
    fresh.add(x)
    idx.add_codes(*fresh.get_rows(4200, len(x) - 4200))
    codes, fac = fresh.get_rows(0, len(x))
    assert all(np.array_equal(a, b) for a, b in zip(idx.get_rows(0, idx.ntotal), (codes, fac)))
    q = rng.standard_normal((40, d)).astype(np.float32)
    top = top64(scores(*idx.query(q), codes, fac))
    for nq in (3, 40):
        check(idx, top, q, nq, 10)
    idx.close(), fresh.close()


def test_rabitq_vector_database(gpu, tmp_path):
    """200 stored rows plus 0.02 N(0, 1) noise come back first: the numpy restatement gives 200 of 200, so a miss is a bug."""
    from minivectordb_amd import RabitqVectorDatabase
    rng = np.random.default_rng(11)
    d, n = 256, 3000
    x = rng.standard_normal((n, d)).astype(np.float32) + 0.05
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    path = str(tmp_path / "rabitq.pkl")
    db = RabitqVectorDatabase(d, storage_file=path, seed=3)
    db.train(x)
    signs = np.packbits(np.random.default_rng(3).integers(0, 2, (4, d), dtype=np.uint8), axis=1)
    c = x.mean(0, dtype=np.float64).astype(np.float32)
    assert np.array_equal(db.index.get_rotation(), signs) and np.array_equal(db.index.get_centroid(), c)
    ids = [f"id{i}" for i in range(n)]
    db.store_embeddings_batch(ids[:2500], list(x[:2500]), [{"even": i % 2 == 0, "i": i} for i in range(2500)])
    for i in range(2500, n):
        db.store_embedding(ids[i], x[i], {"even": i % 2 == 0, "i": i})
    assert np.array_equal(db.index.get_rows(0, n)[0], encode(x, c, signs)[0])
    planted = rng.permutation(n)[:200]
    q = (x[planted] + 0.02 * rng.standard_normal((200, d))).astype(np.float32)
    got = db.find_most_similar_batch(list(q), k=5)
    assert [g[0][0] for g in got] == [ids[p] for p in planted]
    assert db.find_most_similar(q[0], k=3)[2][0] == {"even": planted[0] % 2 == 0, "i": planted[0]}
    even = db.find_most_similar_batch(list(q), metadata_filter={"even": True}, k=5)
    assert all(int(u[2:]) % 2 == 0 for g in even for u in g[0]) and all(len(g[0]) == 5 for g in even)
    db.delete_embedding(ids[planted[0]])
    after = db.find_most_similar_batch(list(q), k=5)
    assert all(ids[planted[0]] not in g[0] for g in after) and [g[0][0] for g in after[1:]] == [ids[p] for p in planted[1:]]
    db.persist_to_disk()
    again = RabitqVectorDatabase(d, storage_file=path, seed=99)
    assert [(g[0], g[1]) for g in again.find_most_similar_batch(list(q), k=5)] == [(g[0], g[1]) for g in after]
