"""The refine store (include/mvdb.h "REFINE STORE"): stored bytes against numpy's float16, the re-rank against float64 on the
stored values, and the MX search that re-ranks its own candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def gamma(d):
    return (d + 16) * 2.0 ** -24


def spread(rng, n, d):
    """Gaussian rows whose blocks of 8 differ in magnitude by up to 2^12."""
    mag = 2.0 ** rng.integers(-6, 7, (n, d // 8))
    return (rng.standard_normal((n, d)) * np.repeat(mag, 8, axis=1)).astype(np.float32)


def same_halfs(got, x):
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got.view(np.float16)), nan) and np.array_equal(got[~nan], want.view(np.uint16)[~nan])


@pytest.mark.parametrize("d", [8, 136, 512])
def test_stored_bytes(gpu, d):
    import torch
    from minivectordb_amd import _native
    rng = np.random.default_rng(d)
    x = spread(rng, 300, d)
    h = rng.integers(0, 0x7BFF, 300 * d).astype(np.uint16).view(np.float16).astype(np.float32)
    mid = (h + np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32)) / 2   # exact ties of neighbours
    x[:60] = (mid * rng.choice([-1.0, 1.0], mid.shape)).astype(np.float32).reshape(300, d)[:60]
    x[60:70] = rng.choice(np.array([65519.9, 65520.0, 1e9, -7e4, 6e-8, -3e-8, 2.98e-8, 1e-5, 0.0, -0.0, np.inf, -np.inf,
                                    np.nan], dtype=np.float32), (10, d))
    st = _native.RefineStore(d)
    st.add(x[:200])
    xd = torch.from_numpy(x[200:]).cuda()
    st.add_device(xd.data_ptr(), 100)
    assert st.ntotal == 300 and same_halfs(st.get_rows(0, 300), x)
    rows = rng.permutation(300)[:120]
    x[rows] = spread(rng, 120, d)
    st.set_rows(rows, x[rows])
    assert same_halfs(st.get_rows(0, 300), x)
    gone = rng.permutation(300)[:50]
    st.remove_rows(gone)
    x = np.concatenate([np.delete(x, gone, axis=0), spread(rng, 40, d)])
    st.add(x[250:])
    assert st.ntotal == 290 and same_halfs(st.get_rows(0, 290), x)
    for bad in (lambda: _native.RefineStore(12), lambda: st.remove_rows([3, 3]), lambda: st.remove_rows([290]),
                lambda: st.set_rows([5, 5], x[:2]), lambda: st.set_rows([1, 290], x[:2])):
        with pytest.raises(Exception):
            bad()
    assert st.ntotal == 290 and same_halfs(st.get_rows(0, 290), x)
    st.close()


@pytest.mark.parametrize("d,n,nq,m,k", [(8, 70, 1, 1, 1), (136, 1007, 17, 63, 10), (512, 1007, 65, 64, 64),
                                        (512, 1007, 1, 1024, 10), (1032, 1007, 17, 65, 64), (4096, 300, 65, 1024, 10)])
def test_rerank_against_float64(gpu, d, n, nq, m, k):
    from minivectordb_amd import _native
    rng = np.random.default_rng(d + m)
    st = _native.RefineStore(d)
    st.add(spread(rng, n, d))
    x = st.get_rows(0, n).view(np.float16).astype(np.float64)
    q = spread(rng, nq, d)
    cand = rng.integers(0, n, (nq, m))
    cand[rng.random((nq, m)) < 0.1] = -1
    junk = rng.random((nq, m)) < 0.1
    cand[junk] = rng.choice([n, n + 5, -7, 2 ** 40], int(junk.sum()))
    cand[:, min(1, m - 1)] = cand[:, 0] = rng.integers(0, n, nq)   # a row named twice (m = 1: the one slot is a row)
    D, I = st.rerank(q, cand, k)
    S = q.astype(np.float64) @ x.T
    A = np.abs(q.astype(np.float64)) @ np.abs(x).T
    for i in range(nq):
        members = np.unique(cand[i][(cand[i] >= 0) & (cand[i] < n)])
        cnt = min(k, len(members))
        got = I[i, :cnt]
        assert (I[i, cnt:] == -1).all() and (D[i, cnt:] == -np.finfo(np.float32).max).all()
        assert len(set(got)) == cnt and np.isin(got, members).all()
        assert (np.diff(D[i, :cnt]) <= 0).all()
        assert (np.abs(D[i, :cnt] - S[i, got]) <= gamma(d) * A[i, got]).all()
        if cnt:
            kth = np.sort(S[i, members])[-cnt]
            assert (S[i, got] >= kth - 2 * gamma(d) * A[i, members].max()).all()
    st.close()


@pytest.mark.parametrize("d", [136, 1032])
def test_one_pair_one_result(gpu, d):
    """A (query, row) pair scores the same bits alone, among 17 and among 65 queries, wherever it stands in whichever list."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(d)
    x = spread(rng, 1007, d)
    x[500:520] = x[100:120]
    q = spread(rng, 65, d)
    q[0] = x[100]
    st = _native.RefineStore(d)
    st.add(x)
    cand = np.stack([rng.permutation(1007)[:64] for _ in range(65)])
    cand[0, :2] = [500, 100]
    D65, I65 = st.rerank(q, cand, 64)
    assert list(I65[0, :2]) == [100, 500] and D65[0, 0] == D65[0, 1]
    score = [dict(zip(I65[j], D65[j].view(np.uint32))) for j in range(65)]
    D17, I17 = st.rerank(q[:17], cand[:17], 64)
    assert np.array_equal(I17, I65[:17]) and np.array_equal(D17.view(np.uint32), D65[:17].view(np.uint32))
    for j in (0, 16, 64):
        for lst in (cand[j], rng.permutation(cand[j])):
            D1, I1 = st.rerank(q[j:j + 1], lst[None], 64)
            assert np.array_equal(I1[0], I65[j]) and np.array_equal(D1[0].view(np.uint32), D65[j].view(np.uint32))
        wide = np.concatenate([cand[j], rng.integers(0, 1007, 960)])
        Dw, Iw = st.rerank(q[j:j + 1], wide[None], 64)
        both = np.isin(Iw[0], cand[j])
        assert all(score[j][r] == s for r, s in zip(Iw[0][both], Dw[0].view(np.uint32)[both]))
        D10, I10 = st.rerank(q[j:j + 1], np.concatenate([cand[j], I65[j, 40:], I65[j, 40:]])[None], 10)
        assert np.array_equal(I10[0], I65[j, :10]) and np.array_equal(D10[0].view(np.uint32), D65[j, :10].view(np.uint32))
    st.close()


@pytest.mark.parametrize("n", [100, 1007])
@pytest.mark.parametrize("nq", [1, 40])
@pytest.mark.parametrize("fetch_k", [10, 64, 100, 1024])
@pytest.mark.parametrize("fmt", [4, 8])
def test_mx_candidate_rule(gpu, fmt, fetch_k, nq, n):
    """search_refined is the re-rank of the union of every segment's own top f, each found by an index of that segment alone."""
    from minivectordb_amd import _native
    rng = np.random.default_rng(fmt + fetch_k + nq + n)
    d, k = 512, 10
    x = spread(rng, n, d)
    q = spread(rng, nq, d)
    idx, st = _native.MxIndex(d, fmt), _native.RefineStore(d)
    idx.add(x), st.add(x)
    S = -(-fetch_k // 64)
    f = -(-fetch_k // S)
    L = 64 * -(-n // (64 * S))
    for keep in (np.ones(n, bool), rng.random(n) < 0.4):
        mask = None if keep.all() else _native.pack_row_mask(n, rows=np.flatnonzero(keep))
        union = []
        for lo in range(0, n, L):
            hi = min(n, lo + L)
            seg = _native.MxIndex(d, fmt)
            seg.add_codes(*idx.get_codes(lo, hi - lo))
            _, Is = seg.search(q, min(f, 64), _native.pack_row_mask(hi - lo, rows=np.flatnonzero(keep[lo:hi])))
            union.append(np.where(Is >= 0, Is + lo, -1))
            seg.close()
        union = np.concatenate(union, axis=1)
        if n == 100 and fetch_k == 1024:
            assert all(set(u[u >= 0]) == set(np.flatnonzero(keep)) for u in union)
        Dr, Ir = st.rerank(q, union, k)
        D, I = idx.search_refined(q, k, st, fetch_k, mask)
        assert np.array_equal(I, Ir) and np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
        assert keep[I[I >= 0]].all() and (I[:, 0] >= 0).all()
    idx.close(), st.close()


@pytest.mark.parametrize("nq", [3, 40])
@pytest.mark.parametrize("fmt", [4, 8])
def test_search_refined_device_replays_from_a_graph(gpu, fmt, nq):
    import torch
    from minivectordb_amd import _native
    rng = np.random.default_rng(fmt + nq)
    d, n, k, fetch_k = 512, 5000, 10, 256
    x = spread(rng, n, d)
    idx, st = _native.MxIndex(d, fmt), _native.RefineStore(d)
    idx.add(x), st.add(x)
    qh = spread(rng, nq, d)
    De, Ie = idx.search_refined(qh, k, st, fetch_k)
    stream = torch.cuda.Stream()
    q = torch.from_numpy(qh).cuda()
    D = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    I = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    run = lambda: idx.search_refined_device(q.data_ptr(), nq, k, st, fetch_k, D.data_ptr(), I.data_ptr(),
                                            stream=stream.cuda_stream)
    with torch.cuda.stream(stream):   # an eager call sizes this stream's workspaces: nothing is allocated inside a capture
        run()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        run()
    for _ in range(3):
        D.zero_(), I.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(I.cpu().numpy(), Ie)
        assert np.array_equal(D.cpu().numpy().view(np.uint32), De.view(np.uint32))
    del graph
    idx.close(), st.close()


@pytest.mark.parametrize("bits", [4, 8])
def test_mx_vector_database_refined(gpu, tmp_path, bits):
    from minivectordb_amd import MXVectorDatabase
    rng = np.random.default_rng(bits)
    d, n = 128, 2000
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    path, plain_path = str(tmp_path / "mx.pkl"), str(tmp_path / "plain.pkl")
    db = MXVectorDatabase(d, element_bits=bits, storage_file=path, refine=True, fetch_k=1024)
    plain = MXVectorDatabase(d, element_bits=bits, storage_file=plain_path)
    ids = [f"id{i}" for i in range(n)]
    for each in (db, plain):
        each.store_embeddings_batch(ids, list(x), [{"even": i % 2 == 0, "i": i} for i in range(n)])
    planted = rng.permutation(n)[:100]
    q = (x[planted] + 0.01 * rng.standard_normal((100, d))).astype(np.float32)
    found = db.find_most_similar_batch(list(q), k=5)
    assert [g[0][0] for g in found] == [ids[p] for p in planted]
    x16 = x.astype(np.float16).astype(np.float64)
    for i, (uids, scores, _) in enumerate(found):
        rows = [int(u[2:]) for u in uids]
        assert (np.abs(np.array(scores) - x16[rows] @ q[i]) <= gamma(d) * (np.abs(x16[rows]) @ np.abs(q[i]))).all()
    even = db.find_most_similar_batch(list(q), metadata_filter={"even": True}, k=5)
    assert all(int(u[2:]) % 2 == 0 for g in even for u in g[0]) and all(len(g[0]) == 5 for g in even)
    db.delete_embedding(ids[planted[0]])
    db.update_embedding(ids[planted[1]], -x[planted[1]])
    after = db.find_most_similar_batch(list(q), k=5)
    assert all(ids[planted[0]] not in g[0] for g in after) and ids[planted[1]] not in after[1][0]
    assert [g[0][0] for g in after[2:]] == [ids[p] for p in planted[2:]]
    db.persist_to_disk(), plain.persist_to_disk()
    again = MXVectorDatabase(d, element_bits=bits, storage_file=path, refine=True, fetch_k=1024)
    assert [(g[0], g[1]) for g in again.find_most_similar_batch(list(q), k=5)] == [(g[0], g[1]) for g in after]
    with pytest.raises(ValueError):
        MXVectorDatabase(d, element_bits=bits, storage_file=plain_path, refine=True)
