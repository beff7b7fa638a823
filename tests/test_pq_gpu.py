"""The product-quantised index (csrc/pq.hip) and PQVectorDatabase.  The scan's whole contract is a dozen lines of numpy: given the
codes, the device's own table u (PQIndex.lut) and a mask, S = sum_m u[m, code[m]] over the selected rows, ordered by (S, row) —
equal bit for bit on every form.  The table, the encoder and the training update are held to float64 restatements."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.int32).max
FMAX = np.finfo(np.float32).max
IP, L2 = 0, 1
SHAPES = [(32, 16), (96, 48), (512, 64), (256, 128), (512, 256)]   # G = 1, a dead lane in a quad, G = 4, 8, 16; every NQ cap


def oracle(codes, u, step, bias, metric, k, selected=None):
    rows = np.arange(len(codes)) if selected is None else np.flatnonzero(selected)
    nq, M = u.shape[:2]
    sign = -1.0 if metric == IP else 1.0
    D = np.full((nq, k), sign * FMAX, np.float32)
    I, S = np.full((nq, k), -1, np.int64), np.full((nq, k), NONE, np.int32)
    for i in range(nq):
        s = u[i][np.arange(M), codes[rows]].sum(1, dtype=np.int64)
        best = np.lexsort((rows, s))[:k]
        I[i, :len(best)], S[i, :len(best)] = rows[best], s[best]
        D[i, :len(best)] = (sign * (np.float64(bias[i]) + np.float64(step[i]) * s[best])).astype(np.float32)
    return D, I, S


def make_index(rng, d, M, metric, codes=None, cb=None):
    from minivectordb_amd import _native
    idx = _native.PQIndex(d, M, metric)
    idx.set_codebooks(rng.standard_normal((M, 256, d // M)).astype(np.float32) if cb is None else cb)
    if codes is not None:
        idx.add_codes(codes)
    return idx


def check(idx, codes, q, k, table, metric, selected=None):
    from minivectordb_amd import _native
    nq = len(q)
    u, step, bias = (t[:nq] for t in table)
    Do, Io, So = oracle(codes, u, step, bias, metric, k, selected)
    mask = None if selected is None else _native.pack_row_mask(len(codes), rows=np.flatnonzero(selected))
    D, I, S = idx.search(q, k, mask)
    assert np.array_equal(I, Io), (codes.shape, nq, k, np.argwhere(I != Io)[:4])
    assert np.array_equal(S, So), (codes.shape, nq, k)
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), (codes.shape, nq, k)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("d,M", SHAPES)
def test_scan_equals_oracle(gpu, d, M, n, metric):
    """nq = 1, 2, 4: every NQ form; 3: a dead query in a pass; 5: a ragged last pass; 9: three passes.  k = 64 > n pads."""
    rng = np.random.default_rng(d + M + n)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    q = rng.standard_normal((9, d)).astype(np.float32)
    idx = make_index(rng, d, M, metric, codes)
    table = idx.lut(q)
    assert idx.geometry(9, 10)[0] == (4 if M <= 64 else 2 if M <= 128 else 1) and idx.geometry(2, 10)[0] == min(2, idx.geometry(9, 10)[0])
    for nq in (1, 2, 3, 4, 5, 9):
        for k in (1, 10, 64):
            check(idx, codes, q[:nq], k, table, metric)
    with pytest.raises(ValueError):
        idx.search(q[:1], 65)
    idx.close()


@pytest.mark.parametrize("nq", [1, 4])
@pytest.mark.parametrize("d,M", [(32, 16), (512, 64), (512, 256)])
def test_one_row_past_a_grid_stride(gpu, d, M, nq):
    """n = one whole stride of the full grid + 1: the last row is the second trip of block 0, and it is query 0's best row."""
    rng = np.random.default_rng(M + nq)
    idx = make_index(rng, d, M, L2)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    table = idx.lut(q)
    n = idx.geometry(nq, 10)[1] + 1
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    codes[-1] = table[0][0].argmin(1)   # every sub-space at query 0's zero entry: S = 0
    idx.add_codes(codes)
    D, I, S = idx.search(q, 10)
    assert I[0, 0] == n - 1 and S[0, 0] == 0
    check(idx, codes, q, 10, table, L2)
    idx.close()


def test_identical_rows_go_to_the_lower_row(gpu):
    rng = np.random.default_rng(7)
    codes = np.repeat(rng.integers(0, 256, (1, 64), dtype=np.uint8), 200, axis=0)
    idx = make_index(rng, 512, 64, IP, codes)
    D, I, S = idx.search(rng.standard_normal((5, 512)).astype(np.float32), 64)
    assert np.array_equal(I, np.tile(np.arange(64), (5, 1))) and (S == S[:, :1]).all()
    idx.close()


@pytest.mark.parametrize("nq", [3, 5])
@pytest.mark.parametrize("d,M", [(32, 16), (512, 256)])
def test_bitmap(gpu, d, M, nq):
    rng = np.random.default_rng(M + nq)
    n = 4100
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = make_index(rng, d, M, IP, codes)
    table = idx.lut(q)
    half, none, tail = rng.random(n) < 0.5, np.zeros(n, bool), np.arange(n) >= 4096   # the tail: the last, ragged tile only
    for selected in (half, none, tail):
        check(idx, codes, q, 10, table, IP, selected)
    idx.close()


def table64(q, cb, metric):
    """include/mvdb.h's query table restated in float64."""
    qs = q.astype(np.float64).reshape(cb.shape[0], 1, -1)
    t = -(qs * cb).sum(-1) if metric == IP else ((qs - cb) ** 2).sum(-1)
    lo = t.min(1)
    span = (t.max(1) - lo).max()
    step = span / 65535 if span else 1.0
    return np.minimum(65535, np.rint((t - lo[:, None]) / step)), step, lo.sum()


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d,M", SHAPES[:3])
def test_table_against_float64(gpu, d, M, metric):
    """Within 1 unit: at dsub <= 8 an fp32 t is off by far less than step / 2, so rint moves by at most one."""
    rng = np.random.default_rng(d + metric)
    idx = make_index(rng, d, M, metric, rng.integers(0, 256, (100, M), dtype=np.uint8))
    cb = idx.get_codebooks().astype(np.float64)
    q = rng.standard_normal((5, d)).astype(np.float32)
    u, step, bias = idx.lut(q)
    for i in range(len(q)):
        u64, step64, bias64 = table64(q[i], cb, metric)
        worst = np.abs(u[i].astype(np.int64) - u64).max()
        print(d, M, metric, "worst entry", worst, "step", step[i] / step64 - 1, "bias", bias[i] / bias64 - 1)
        assert worst <= 1
        assert abs(step[i] - step64) <= 1e-5 * step64 and abs(bias[i] - bias64) <= 1e-5 * abs(bias64)
    q[1, 3] = np.inf
    D, I, S = idx.search(q[:3], 10)
    assert (I[1] == -1).all() and (S[1] == NONE).all() and (D[1] == (-FMAX if metric == IP else FMAX)).all()
    assert (I[[0, 2]] >= 0).all()
    idx.close()


@pytest.mark.parametrize("dsub", [2, 4, 8])
def test_encoding(gpu, dsub):
    """Rows planted as cb[m][code] + 0.01 N(0, 1) come back as the planted codes.  At dsub = 4 and 8 every float64 margin between
    the best and the second best centroid is above 1e-3 and nothing is excluded.  At dsub = 2 it is not: 256 N(0, 1) centroids in
    the plane lie as close as 1e-3 to each other, about 1 planted sub-vector in 80 has ANOTHER float64 argmin (numpy, three seeds:
    81, 102, 114 of 8000) and margins reach 1e-6 — there the reference is the float64 argmin of the contract, on the sub-vectors
    whose margin is above the same 1e-3."""
    rng = np.random.default_rng(dsub)
    M, n = 16, 500
    cb = rng.standard_normal((M, 256, dsub)).astype(np.float32)
    cb[:, 9] = cb[:, 5]
    planted = rng.integers(0, 256, (n, M))
    x = (cb[np.arange(M), planted] + 0.01 * rng.standard_normal((n, M, dsub))).astype(np.float32)
    x[7, 3] = np.nan
    idx = make_index(rng, M * dsub, M, IP, cb=cb)
    idx.add(x.reshape(n, -1))
    got = idx.get_codes(0, n)
    with np.errstate(invalid="ignore"):
        d2 = ((x[:, :, None, :].astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(-1)
    d2[:, :, 9] = np.inf   # the twin of centroid 5: the lower c wins
    want = np.where(planted == 9, 5, planted)
    want[7, 3] = 0
    assert got[7, 3] == 0
    d2[7, 3] = np.arange(256)
    best2 = np.sort(d2, -1)[..., :2]
    safe = best2[..., 1] - best2[..., 0] > 1e-3
    if dsub > 2:
        assert safe.all() and np.array_equal(d2.argmin(-1), want)
        assert np.array_equal(got, want)
    assert safe.mean() > 0.9 and np.array_equal(got[safe], d2.argmin(-1)[safe])
    idx.close()


def test_one_training_iteration(gpu):
    rng = np.random.default_rng(21)
    d, M, n = 64, 16, 3000
    dsub = d // M
    centres = rng.standard_normal((M, 40, dsub))
    x = (centres[np.arange(M), rng.integers(0, 40, (n, M))] + 0.1 * rng.standard_normal((n, M, dsub))).astype(np.float32)
    start = np.empty((M, 256, dsub), np.float32)
    start[:, :40] = centres + 0.05 * rng.standard_normal(centres.shape)   # the planted centres, displaced
    start[:, 40:] = 100.0 + np.arange(216)[None, :, None]                 # centroids no row is nearest to

    def trained(iters):
        idx = make_index(rng, d, M, L2, cb=start)
        idx.train(x.reshape(n, -1), iters)
        cb = idx.get_codebooks()
        idx.add(x.reshape(n, -1))
        err = ((x - cb[np.arange(M), idx.get_codes(0, n)]).astype(np.float64) ** 2).sum() / n
        idx.close()
        return cb, err

    cb1, err1 = trained(1)
    x64 = x.astype(np.float64)
    label = ((x64[:, :, None, :] - start[None].astype(np.float64)) ** 2).sum(-1).argmin(-1)   # [n, M]
    for m in range(M):
        for c in range(256):
            members = x64[label[:, m] == c, m]
            want = members.mean(0) if len(members) else start[m, c]
            assert np.allclose(cb1[m, c], want, rtol=1e-6, atol=0), (m, c, len(members))
    assert np.array_equal(cb1[:, 40:], start[:, 40:])
    cb5, err5 = trained(5)
    print("reconstruction error after 1 and 5 iterations", err1, err5)
    assert err5 <= err1 * (1 + 1e-5)
    assert np.array_equal(trained(5)[0], cb5)


def test_pq_vector_database_round_trip(gpu, tmp_path):
    from minivectordb_amd import PQVectorDatabase, _native
    rng = np.random.default_rng(5)
    d, n = 128, 600
    x = rng.standard_normal((n, d)).astype(np.float32)
    path = str(tmp_path / "pq.pkl")
    db = PQVectorDatabase(d, storage_file=path)
    assert db.n_subvectors == 16 and not db.is_trained
    with pytest.raises(ValueError):
        db.store_embedding("early", x[0])
    db.train(x, iters=3)
    ids = [f"id{i}" for i in range(n)]
    db.store_embeddings_batch(ids[:500], list(x[:500]), [{"even": i % 2 == 0, "i": i} for i in range(500)])
    for i in range(500, n):
        db.store_embedding(ids[i], x[i], {"even": i % 2 == 0, "i": i})
    q = rng.standard_normal((6, d)).astype(np.float32)

    def expect(one, ids, k, selected=None):
        codes = one.index.get_codes(0, one.index.ntotal)
        D, I, S = oracle(codes, *one.index.lut(q), IP, k, selected)
        return [([ids[r] for r in I[j]], [float(v) for v in D[j]]) for j in range(len(q))]

    def answers(one, **kw):
        return [(got[0], got[1]) for got in one.find_most_similar_batch(list(q), k=5, **kw)]

    assert answers(db) == expect(db, ids, 5)
    assert answers(db, metadata_filter={"even": True}) == expect(db, ids, 5, np.arange(n) % 2 == 0)
    assert db.find_most_similar(q[0], k=3)[2] == [{"even": int(u[2:]) % 2 == 0, "i": int(u[2:])} for u in expect(db, ids, 3)[0][0]]
    code = db.index.get_codes(4, 1)[0]
    assert np.array_equal(db.reconstruct("id4"), db.index.get_codebooks()[np.arange(16), code].reshape(-1))
    db.delete_embedding("id4")
    ids = ids[:4] + ids[5:]
    even = np.array([int(u[2:]) % 2 == 0 for u in ids])
    db.persist_to_disk()
    again = PQVectorDatabase(d, storage_file=path)
    assert again.is_trained
    for one in (db, again):
        assert answers(one, metadata_filter={"even": True}) == expect(db, ids, 5, even)


def test_search_device_replays_from_a_graph(gpu):
    import torch
    rng = np.random.default_rng(9)
    d, M, n, nq, k = 512, 64, 5000, 5, 10
    idx = make_index(rng, d, M, L2, rng.integers(0, 256, (n, M), dtype=np.uint8))
    qh = rng.standard_normal((nq, d)).astype(np.float32)
    De, Ie, Se = idx.search(qh, k)
    q = torch.from_numpy(qh).cuda()
    D = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    I = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    S = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
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
