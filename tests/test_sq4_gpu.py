"""The 4-bit scalar-quantised index (csrc/sq4.hip) and SQ4VectorDatabase.  The whole contract is a few lines of numpy: the encode
rule, the query rule, S = q8 . code over the selected rows ordered by (-S, row), D from the device's own step and bias.  Every
comparison is array_equal, D as bits: there is no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
SMIN = np.iinfo(np.int32).min
F15 = np.float32(15)


def derived(lo, hi):
    with np.errstate(all="ignore"):
        span = hi - lo
        ok = np.isfinite(span) & (span > 0)
        return np.where(ok, F15 / span, 0).astype(np.float32), np.where(ok, span / F15, 0).astype(np.float32)


def encode(x, lo, hi):
    with np.errstate(all="ignore"):
        u = (x - lo) * derived(lo, hi)[0]
        c = np.where(u >= 15, 15, np.where(~(u > 0), 0, np.rint(u))).astype(np.uint8)
    return c[:, 0::2] | (c[:, 1::2] << 4)


def unpack(codes):
    out = np.empty((len(codes), 2 * codes.shape[1]), np.float32)
    out[:, 0::2], out[:, 1::2] = codes & 15, codes >> 4
    return out


def query_rule(q, lo, hi):
    w = q * derived(lo, hi)[1]
    amax = np.abs(w).max(1).astype(np.float64)
    with np.errstate(all="ignore"):
        q8 = np.where(amax[:, None] > 0, np.rint(w.astype(np.float64) * (127.0 / amax)[:, None]), 0).astype(np.int8)
    prod = q.astype(np.float64) * lo.astype(np.float64)
    bias = np.cumsum(np.concatenate([np.zeros((len(q), 1)), prod], axis=1), axis=1)[:, -1]   # b = 0; b += prod[i], ascending i
    return q8, amax / 127.0, bias


def top64(q8, codes, selected=None):
    """Per query the 64 best selected rows by np.lexsort((rows, -S)) and their S = q8 . code: the top k of every k <= 64 is a
    prefix.  The int64 matrix product runs through BLAS in float32, 16 queries at a time.  That is exact in ANY summation order:
    every term is an integer and the sum of the |terms| of a row is at most 127 * 15 * 4096 < 2^24, so every partial sum BLAS
    can form, whatever it groups, is an integer below 2^24 in magnitude and float32 holds it.  The sort looks only at the rows
    at or above the 64th score."""
    rows = np.arange(len(codes)) if selected is None else np.flatnonzero(selected)
    U = unpack(codes[rows])
    I, S = np.full((len(q8), 64), -1, np.int64), np.full((len(q8), 64), SMIN, np.int64)
    for i0 in range(0, len(q8), 16):
        for i, s in enumerate(q8[i0:i0 + 16].astype(np.float32) @ U.T, i0):
            keep = np.flatnonzero(s >= np.partition(s, len(s) - 64)[len(s) - 64]) if len(s) > 64 else np.arange(len(s))
            best = keep[np.lexsort((rows[keep], -s[keep]))[:64]]
            I[i, :len(best)], S[i, :len(best)] = rows[best], s[best].astype(np.int64)
    return I, S, None if selected is None else rows


def make_index(rng, d, codes=None):
    from minivectordb_amd import _native
    idx = _native.SQ4Index(d)
    lo = rng.uniform(-1, 0, d).astype(np.float32)
    idx.set_ranges(lo, lo + rng.uniform(0.5, 2, d).astype(np.float32))
    if codes is not None:
        idx.add_codes(codes)
    return idx


def check(idx, top, table, nq, k, form=0):
    """D = (float)(bias + step * S) in float64 from the device's own step and bias; padding where fewer than k rows are selected."""
    from minivectordb_amd import _native
    Io, So = top[0][:nq, :k], top[1][:nq, :k]
    Do = np.where(Io >= 0, table[2][:nq, None] + table[1][:nq, None] * So.astype(np.float64), -FMAX).astype(np.float32)
    mask = None if top[2] is None else _native.pack_row_mask(idx.ntotal, rows=top[2])
    D, I, S = idx.search(table[3][:nq], k, mask, form=form)
    assert np.array_equal(I, Io), (idx.ntotal, nq, k, form, np.argwhere(I != Io)[:4])
    assert np.array_equal(S, So), (idx.ntotal, nq, k, form)
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), (idx.ntotal, nq, k, form)


def tables(idx, rng, nq):
    q = rng.standard_normal((nq, idx.d)).astype(np.float32)
    return idx.query(q) + (q,)


@pytest.mark.parametrize("d", [32, 96, 160])
def test_encode_equals_the_rule(gpu, d):
    """Dimensions [0, 8): lo a multiple of 1/4 and hi - lo = 15 / 2^j, so inv = 2^j and lo + (c + 0.5) / inv are exact: ties."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(d)
    lo = rng.uniform(-1, 0, d).astype(np.float32)
    hi = lo + rng.uniform(0.5, 2, d).astype(np.float32)
    lo[:8] = np.arange(8, dtype=np.float32) / 4 - 1
    hi[:8] = lo[:8] + F15 / np.float32(2) ** (np.arange(8) % 4)
    hi[9] = lo[9]
    inv = derived(lo, hi)[0]
    with np.errstate(all="ignore"):
        ties = np.stack([lo + (np.float32(c) + np.float32(0.5)) / inv for c in range(15)])
    assert np.array_equal((ties[:, :8] - lo[:8]) * inv[:8], np.repeat(np.arange(15, dtype=np.float32)[:, None] + 0.5, 8, axis=1))
    special = np.stack([lo, hi, lo - 1, hi + 1, np.full(d, np.nan), np.full(d, np.inf), np.full(d, -np.inf), np.full(d, -0.0)])
    x = np.concatenate([special, ties, rng.uniform(-1.5, 2.5, (70, d))]).astype(np.float32)
    want = encode(x, lo, hi)
    assert np.array_equal(want[8:23, 0] & 15, [0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14])
    idx = _native.SQ4Index(d)
    with pytest.raises(ValueError):
        idx.add(x)   # no ranges yet
    idx.set_ranges(lo, hi)
    assert all(np.array_equal(a, b) for a, b in zip(idx.get_ranges(), (lo, hi)))
    idx.add(x)
    idx.add(np.zeros((len(x), d), np.float32))
    assert np.array_equal(idx.get_codes(0, len(x)), want)
    with pytest.raises(ValueError):
        idx.set_ranges(lo, hi)   # rows are stored
    rows = rng.permutation(2 * len(x))[:len(x)]
    idx.set_rows(rows, x)
    assert np.array_equal(idx.get_codes(0, 2 * len(x))[rows], want)
    idx.close()


@pytest.mark.parametrize("d", [96, 4096])
def test_query_equals_the_rule(gpu, d):
    rng = np.random.default_rng(d)
    idx = make_index(rng, d, rng.integers(0, 256, (100, d // 2), dtype=np.uint8))
    lo, hi = idx.get_ranges()
    q = rng.standard_normal((6, d)).astype(np.float32)
    q[2] = 0
    q[4, d // 3] = np.nan
    q8, step, bias = idx.query(q)
    fine = [0, 1, 2, 3, 5]
    w8, wstep, wbias = query_rule(q[fine], lo, hi)
    assert np.array_equal(q8[fine], w8) and not q8[2].any()
    assert np.array_equal(step[fine].view(np.uint64), wstep.view(np.uint64))
    assert np.array_equal(bias[fine].view(np.uint64), wbias.view(np.uint64))
    D, I, S = idx.search(q, 10)
    assert (I[4] == -1).all() and (S[4] == SMIN).all() and (D[4] == -FMAX).all() and (I[fine] >= 0).all()
    assert np.array_equal(I[2], np.arange(10)) and not S[2].any()
    idx.close()


@pytest.mark.parametrize("n", [1, 63, 0])
@pytest.mark.parametrize("d", [32, 96, 512, 2048, 4096])
def test_scan_equals_oracle(gpu, d, n):
    """d: G = 1, a dead lane in a quad, G = 16, the widest matrix-core shape, two chunks per lane.  n = 0 stands for one row past
    the longest grid stride of any form.  nq: every VALU pass width, a dead query in a pass, the hand-over, one and two blocks of
    32 queries, a ragged second slab; 9 through the VALU form and 1 through the matrix cores by force."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(d + n)
    idx = make_index(rng, d)
    if n == 0:
        n = max(idx.geometry(nq, 10)[1] for nq in (1, 2, 4, 33, 65)) + 1
    codes = rng.integers(0, 256, (n, d // 2), dtype=np.uint8)
    if n > 4:
        codes[n // 2], codes[n // 3] = codes[0], codes[n - 1]
    idx.add_codes(codes)
    mfma = d <= 2048
    assert idx.geometry(4, 10)[0] == _native.SQ4Index.FORM_VALU and idx.geometry(5, 10)[0] == (2 if mfma else 1)
    table = tables(idx, rng, 100)
    top = top64(table[0], codes)
    for k in (1, 10, 64):
        for nq in (1, 2, 3, 4, 5, 33, 64, 65, 100):
            check(idx, top, table, nq, k)
        check(idx, top, table, 9, k, form=1)
        if mfma:
            check(idx, top, table, 1, k, form=2)
    with pytest.raises(ValueError):
        idx.search(table[3][:1], 65)
    if not mfma:
        with pytest.raises(ValueError):
            idx.search(table[3][:8], 10, form=2)
    idx.close()


@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("d", [96, 512])
def test_mask_and_mutations(gpu, d, nq):
    rng = np.random.default_rng(d + nq)
    n = 5000
    codes = rng.integers(0, 256, (n, d // 2), dtype=np.uint8)
    idx = make_index(rng, d, codes)
    table = tables(idx, rng, nq)
    third, few = np.arange(n) % 3 == 0, np.isin(np.arange(n), [7, 4999, 64, 2048])
    for selected in (third, few):
        check(idx, top64(table[0], codes, selected), table, nq, 10)
    gone = rng.permutation(n)[:300]
    idx.remove_rows(gone)
    codes = np.delete(codes, gone, axis=0)
    changed = rng.permutation(len(codes))[:200]
    lo, hi = idx.get_ranges()
    x = rng.uniform(-1.5, 2.5, (200, d)).astype(np.float32)
    idx.set_rows(changed, x)
    codes[changed] = encode(x, lo, hi)
    idx.set_rows_codes(changed[:50], codes[changed[50:100]])
    codes[changed[:50]] = codes[changed[50:100]]
    assert np.array_equal(idx.get_codes(0, idx.ntotal), codes)
    check(idx, top64(table[0], codes), table, nq, 10)
    check(idx, top64(table[0], codes, np.arange(len(codes)) % 3 == 0), table, nq, 10)
    idx.close()


def test_search_device_replays_from_a_graph(gpu):
    import torch
    rng = np.random.default_rng(9)
    d, n, k = 512, 5000, 10
    idx = make_index(rng, d, rng.integers(0, 256, (n, d // 2), dtype=np.uint8))
    stream = torch.cuda.Stream()
    for nq in (3, 40):   # the VALU form, the matrix-core form
        qh = rng.standard_normal((nq, d)).astype(np.float32)
        De, Ie, Se = idx.search(qh, k)
        q = torch.from_numpy(qh).cuda()
        D = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        I = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        S = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        run = lambda: idx.search_device(q.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), S.data_ptr(), stream=stream.cuda_stream)
        with torch.cuda.stream(stream):   # an eager call sizes this stream's workspace: nothing is allocated inside a capture
            run()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            run()
        for _ in range(3):
            D.zero_(), I.zero_(), S.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(I.cpu().numpy(), Ie) and np.array_equal(S.cpu().numpy(), Se)
            assert np.array_equal(D.cpu().numpy().view(np.uint32), De.view(np.uint32))
        del graph
    idx.close()


@pytest.mark.parametrize("d", [32, 96])
def test_sq4_vector_database(gpu, tmp_path, d):
    """200 stored rows plus 0.02 N(0, 1) noise come back first: the numpy restatement of the quantiser gives 200 of 200 at both
    widths, so a miss is a bug."""
    from minivectordb_amd import SQ4VectorDatabase
    rng = np.random.default_rng(d)
    n = 3000
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    path = str(tmp_path / "sq4.pkl")
    db = SQ4VectorDatabase(d, storage_file=path)
    with pytest.raises(ValueError):
        db.store_embedding("early", x[0])
    db.train(x)
    lo, hi = db.index.get_ranges()
    assert np.array_equal(lo, x.min(0)) and np.array_equal(hi, x.max(0))
    ids = [f"id{i}" for i in range(n)]
    db.store_embeddings_batch(ids[:2500], list(x[:2500]), [{"even": i % 2 == 0, "i": i} for i in range(2500)])
    for i in range(2500, n):
        db.store_embedding(ids[i], x[i] if i % 2 else -x[i], {"even": i % 2 == 0, "i": i})
    for i in range(2500, n, 2):
        db.update_embedding(ids[i], x[i])
    assert np.array_equal(db.index.get_codes(0, n), encode(x, lo, hi))
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
    again = SQ4VectorDatabase(d, storage_file=path)
    assert again.is_trained and [(g[0], g[1]) for g in again.find_most_similar_batch(list(q), k=5)] == [(g[0], g[1]) for g in after]
