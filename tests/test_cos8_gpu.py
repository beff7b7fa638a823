"""The int8 cosine index on the device (csrc/cos8.hip) against the exact CPU oracle (tests/cos8_oracle.py): quantiser bytes,
ids AND fp32 distances bit-identical, batches equal to single calls, filters, deletes, label_offset, hipGraph replay, the
database class, threads, and one 10M x 512 corpus."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cos8_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


def _rng(seed):
    return np.random.default_rng(seed)


def adversarial_rows(d, rng):
    rows = [np.zeros(d, np.float32), np.eye(1, d, d // 2, dtype=np.float32)[0], -np.eye(1, d, 0, dtype=np.float32)[0],
            np.full(d, 1e-30, np.float32), np.full(d, 3e30, np.float32), np.full(d, 1.0, np.float32)]
    # values on trunc boundaries: x * 127 / |x| close to integers
    b = rng.integers(-127, 128, d).astype(np.float32)
    rows += [b, b / 3.0, (b + np.float32(0.5)) * np.float32(1e-3)]
    rows += list(rng.standard_normal((8, d)).astype(np.float32))
    return np.stack(rows).astype(np.float32)


def check_equal(D, I, Do, Io, what):
    assert np.array_equal(I, Io), (what, np.argwhere(I != Io)[:5], I[:2], Io[:2])
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), (what, D[:2], Do[:2])


@pytest.mark.parametrize("d", [1, 2, 3, 17, 64, 384, 512, 1000, 1024, 2100])
def test_quantiser_bytes(gpu, d):
    from minivectordb_amd import _native
    x = adversarial_rows(d, _rng(d))
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, x.shape[0])
    oc, oa = O.quantize(x)
    assert np.array_equal(codes, oc) and np.array_equal(a2, oa)
    idx.close()


CASES = [  # (n, d, nq, k)
    (1, 2, 1, 1), (5, 2, 3, 10), (1000, 3, 7, 10), (4097, 64, 32, 64), (20000, 384, 2, 100), (3000, 512, 300, 10),
    (30000, 768, 128, 10), (9000, 1000, 7, 64), (50000, 1024, 256, 1), (100, 512, 1, 150), (2000, 2100, 5, 10), (1 << 20, 64, 32, 10),
]


@pytest.mark.parametrize("n,d,nq,k", CASES)
def test_search_bit_exact(gpu, n, d, nq, k):
    from minivectordb_amd import _native
    rng = _rng(n + d + nq + k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 8:
        x[n // 3:n // 3 + 4] = x[1]   # exact duplicates: tie at the same distance
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[0] = x[min(1, n - 1)]
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, n)
    D, I = idx.search(q, k)
    Do, Io = O.search(codes, a2, q, k)
    check_equal(D, I, Do, Io, (n, d, nq, k))
    for i in sorted({0, nq // 2, nq - 1}):   # batch row i == a single call, bit for bit
        D1, I1 = idx.search(q[i], k)
        check_equal(D1[0], I1[0], D[i], I[i], ("single", i))
    idx.close()


def test_duplicate_heavy_and_special_rows(gpu):
    from minivectordb_amd import _native
    rng = _rng(7)
    d = 384
    base = rng.standard_normal((16, d)).astype(np.float32)
    x = base[rng.integers(0, 16, 200000)]
    x[5] = 0.0                          # zero row: distance 1 (0 against a zero query)
    x[7] = np.eye(1, d, 3)[0] * 5.0
    q = np.concatenate([base[:6], np.zeros((1, d), np.float32), x[7:8]]).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x)
    codes, a2 = idx.get_codes(0, x.shape[0])
    for k in (1, 10, 64, 100):
        D, I = idx.search(q, k)
        check_equal(D, I, *O.search(codes, a2, q, k), ("dup", k))
    idx.close()


def test_filters_deletes_and_device_paths(gpu):
    import torch
    from minivectordb_amd import _native
    rng = _rng(11)
    n, d, nq = 60000, 512, 33
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x[:40000])
    idx.add(x[40000:])
    codes, a2 = idx.get_codes(0, n)
    few = np.sort(rng.choice(n, 300, replace=False))
    most = np.sort(rng.choice(n, n // 2, replace=False))
    gone = np.sort(rng.choice(n, 50, replace=False))
    for k in (10, 100):
        rs = idx.rowset(few)
        assert not rs.is_bitmap and len(rs) == 300
        check_equal(*idx.search_rowset(q, k, rs), *O.search(codes, a2, q, k, rows=few), ("list", k))
        rs2 = idx.rowset(most)
        assert rs2.is_bitmap
        check_equal(*idx.search_rowset(q, k, rs2), *O.search(codes, a2, q, k, rows=most), ("bitmap", k))
        rs3 = idx.rowset(gone, excluded=True)
        keep = np.setdiff1d(np.arange(n), gone)
        check_equal(*idx.search_rowset(q, k, rs3), *O.search(codes, a2, q, k, rows=keep), ("excluded", k))
        rs4 = idx.rowset(np.arange(n), excluded=True)    # exclude-all
        D, I = idx.search_rowset(q, k, rs4)
        assert (I == -1).all()
    # device entry point with a label offset, eager and replayed from a hipGraph
    qt = torch.from_numpy(q).cuda()
    Dt = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    It = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    Do, Io = O.search(codes, a2, q, 10)
    with torch.cuda.stream(stream):
        idx.search_device(qt.data_ptr(), nq, 10, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream, label_offset=1000)
    stream.synchronize()
    check_equal(Dt.cpu().numpy(), It.cpu().numpy(), Do, np.where(Io >= 0, Io + 1000, -1), "device")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        idx.search_device(qt.data_ptr(), nq, 10, Dt.data_ptr(), It.data_ptr(), stream=stream.cuda_stream, label_offset=1000)
    Dt.zero_()
    It.zero_()
    g.replay()
    torch.cuda.synchronize()
    check_equal(Dt.cpu().numpy(), It.cpu().numpy(), Do, np.where(Io >= 0, Io + 1000, -1), "graph")
    del g
    # deletes: a few scattered rows, then a run; stale row sets are refused
    rs = idx.rowset(few)
    doomed = np.array([0, 17, 40000, n - 1] + list(range(100, 400)), dtype=np.int64)
    idx.remove_rows(doomed)
    with pytest.raises(ValueError):
        idx.search_rowset(q, 10, rs)
    codes2, a22 = idx.get_codes(0, idx.ntotal)
    keep = np.setdiff1d(np.arange(n), doomed)
    assert np.array_equal(codes2, codes[keep]) and np.array_equal(a22, a2[keep])
    check_equal(*idx.search(q, 10), *O.search(codes2, a22, q, 10), "after delete")
    # device-resident ingest
    xt = torch.from_numpy(x[:1000]).cuda()
    idx.add_device(xt.data_ptr(), 1000)
    torch.cuda.synchronize()
    c3, a3 = idx.get_codes(idx.ntotal - 1000, 1000)
    assert np.array_equal(c3, codes[:1000]) and np.array_equal(a3, a2[:1000])
    idx.close()


def test_class_end_to_end(gpu, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    rng = _rng(3)
    d = 48
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "s"), shard_size=70)
    x = rng.standard_normal((300, d)).astype(np.float32)
    meta = [{"g": i % 3, "v": i} for i in range(300)]
    db.store_embeddings_batch(list(range(300)), x, meta)
    db.store_embedding(1000, x[5] * 2.0, {"g": 9})
    allx = np.concatenate([x, x[5:6] * 2.0])
    ids_all = list(range(300)) + [1000]
    codes, a2 = O.quantize(allx)
    q = x[5] + 0.01
    ids, dist, metas = db.find_most_similar(q, k=5)
    Do, Io = O.search(codes, a2, q[None], 5)
    assert list(ids) == [ids_all[i] for i in Io[0]]
    assert [np.float32(v) for v in dist] == list(Do[0]) and all(isinstance(v, np.float32) for v in dist)
    assert dist[0] == dist[1]    # x[5] and 2 x[5] quantise alike: zero-distance duplicates, lower row first
    ids_f, _, _ = db.find_most_similar(q, metadata_filter={"g": 1}, k=4)
    rows = np.array([i for i in range(300) if i % 3 == 1])
    Df, If = O.search(codes, a2, q[None], 4, rows=rows)
    assert list(ids_f) == [ids_all[i] for i in If[0]]
    ids_x, _, _ = db.find_most_similar(q, exclude_filter={"g": 0}, k=400)
    assert len(ids_x) == 201 and 0 not in ids_x
    batch = db.find_most_similar_batch(np.stack([q, x[7]]), k=5)
    assert batch[0] == db.find_most_similar(q, k=5) and batch[1] == db.find_most_similar(x[7], k=5)
    db.delete_embeddings_batch([5, 1000, 17])
    ids2, dist2, _ = db.find_most_similar(q, k=5)
    keep = [i for i in range(301) if ids_all[i] not in (5, 1000, 17)]
    D2, I2 = O.search(codes[keep], a2[keep], q[None], 5)
    assert list(ids2) == [ids_all[keep[i]] for i in I2[0]]
    assert np.array_equal(db.get_vector(250), x[250])
    db2 = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "s"), shard_size=70)
    assert db2.find_most_similar(q, k=5) == (ids2, dist2, db.find_most_similar(q, k=5)[2])


def test_threads(gpu, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    rng = _rng(5)
    d = 32
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "t"), shard_size=500)
    db.store_embeddings_batch(list(range(1000)), rng.standard_normal((1000, d)).astype(np.float32),
                              [{"i": i} for i in range(1000)])
    errors = []

    def worker(t):
        try:
            r = np.random.default_rng(t)
            for j in range(20):
                uid = 10000 + t * 100 + j
                db.store_embedding(uid, r.standard_normal(d).astype(np.float32), {"t": t})
                ids, dist, _ = db.find_most_similar(r.standard_normal(d).astype(np.float32), k=5)
                assert len(ids) == 5 and list(dist) == sorted(dist)
                if j % 4 == 0:
                    db.delete_embeddings_batch([uid])
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(db.unique_ids) == 1000 + 8 * 15


def test_ten_million_by_512(gpu):
    """One full-size corpus: 10M x 512 quantised from device-resident fp32 blocks, 32 queries, oracle chunked on the host."""
    import torch
    from minivectordb_amd import _native
    n, d, nq, k = 10_000_000, 512, 32, 10
    idx = _native.Cos8Index(d)
    idx.reserve(n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    block = 1 << 20
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        xb = torch.randn((m, d), generator=gen, device="cuda", dtype=torch.float32)
        idx.add_device(xb.data_ptr(), m)
        if r0 == 0:
            first = xb[:8].cpu().numpy()
    torch.cuda.synchronize()
    q = np.concatenate([first[:4], _rng(9).standard_normal((nq - 4, d)).astype(np.float32)])
    D, I = idx.search(q, k)
    codes, a2 = idx.get_codes(0, n)
    assert np.array_equal(codes[:8], O.quantize(first)[0])
    check_equal(D, I, *O.search_chunked(codes, a2, q, k), "10M x 512")
    D1, I1 = idx.search(q[5], k)
    check_equal(D1[0], I1[0], D[5], I[5], "10M single")
    idx.close()


def test_mfma_lane_maps_on_asymmetric_integer_data(gpu):
    """The 32-query matrix-core pass: rows and queries that are one-hot at distinct positions (and distinct scales per
    position) can only match their partner if every row / query / K byte lands in the right lane."""
    from minivectordb_amd import _native
    for d in (32, 48, 64, 512, 1024):
        n = min(d, 96)
        x = np.zeros((n, d), np.float32)
        x[np.arange(n), np.arange(n) % d] = 1.0
        x[np.arange(n), (np.arange(n) * 5 + 3) % d] += 0.5 + np.arange(n) / (4.0 * n)    # asymmetric second component
        q = x[(np.arange(40) * 7) % n].copy()
        idx = _native.Cos8Index(d)
        idx.add(x)
        codes, a2 = idx.get_codes(0, n)
        for k in (1, 5, 64):
            D, I = idx.search(q, k)
            check_equal(D, I, *O.search(codes, a2, q, k), ("lanes", d, k))
        assert (I[:, 0] == (np.arange(40) * 7) % n).all()
        idx.close()


def test_mutators_survive_a_destroyed_search_stream(gpu):
    import torch
    from minivectordb_amd import _native
    d = 64
    rng = _rng(21)
    x = rng.standard_normal((5000, d)).astype(np.float32)
    idx = _native.Cos8Index(d)
    idx.add(x)
    qt = torch.from_numpy(x[:8]).cuda()
    Dt = torch.empty((8, 5), dtype=torch.float32, device="cuda")
    It = torch.empty((8, 5), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    idx.search_device(qt.data_ptr(), 8, 5, Dt.data_ptr(), It.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert (It[:, 0].cpu().numpy() == np.arange(8)).all()
    del s
    import gc
    gc.collect()
    torch.cuda.synchronize()
    idx.add(x[:100])              # the workspace of the dead stream must not wedge the mutators
    idx.remove_rows([0, 1])
    idx.reserve(10000)
    assert idx.ntotal == 5098
    codes, a2 = idx.get_codes(0, idx.ntotal)
    check_equal(*idx.search(x[:8], 5), *O.search(codes, a2, x[:8], 5), "after dead stream")
    idx.close()
