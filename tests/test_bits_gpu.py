"""The binary index (csrc/bits.hip) and BinaryVectorDatabase against a numpy oracle: Hamming distances and rows equal bit for bit
on both scan forms, under bitmaps, after sign packing and across mutations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.int32).max
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint8)   # bits set in a byte


def oracle(x, q, k, selected=None):
    """Unpack bits, XOR, sum as int64; order by (H, row); pad with -1 / INT32_MAX.  That is the whole contract."""
    rows = np.arange(len(x)) if selected is None else np.flatnonzero(selected)
    D, I = np.full((len(q), k), NONE, np.int32), np.full((len(q), k), -1, np.int64)
    xs = x[rows]
    for i, qi in enumerate(q):
        H = POP[xs ^ qi].sum(1, dtype=np.int64)
        best = np.lexsort((rows, H))[:k]
        D[i, :len(best)], I[i, :len(best)] = H[best], rows[best]
    return D, I


def bits(rng, n, d_bits):
    return rng.integers(0, 256, (n, d_bits // 8), dtype=np.uint8)


def index_of(x, d_bits):
    from minivectordb_amd import _native
    idx = _native.BitsIndex(d_bits)
    idx.add(x)
    return idx


def check(idx, x, q, k, Do, Io, mask_words=None):
    D, I = idx.search(q, k, mask_words)
    assert np.array_equal(I, Io[:len(q), :k]), (x.shape, len(q), k, np.argwhere(I != Io[:len(q), :k])[:4])
    assert np.array_equal(D, Do[:len(q), :k]), (x.shape, len(q), k)


@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("d_bits", [128, 384, 1024, 3072, 4096])
def test_search_equals_oracle(gpu, d_bits, n):
    """Every NQ instantiation (1, 3 -> 4, 8), the hand-over to the matrix-core form (9), a ragged slab (33), three slabs (70);
    k = 64 > n pads.  At d = 128 and n = 4097 the k-th place always lies inside a run of ties."""
    rng = np.random.default_rng(d_bits + n)
    x, q = bits(rng, n, d_bits), bits(rng, 70, d_bits)
    idx = index_of(x, d_bits)
    Do, Io = oracle(x, q, 64)
    assert idx.geometry(8, 10)[0] == idx.FORM_VALU and idx.geometry(9, 10)[0] == idx.FORM_MFMA
    for nq in (1, 3, 8, 9, 32, 33, 70):
        for k in (1, 10, 64):
            check(idx, x, q[:nq], k, Do, Io)
    with pytest.raises(ValueError):
        idx.search(q[:1], 65)
    idx.close()


@pytest.mark.parametrize("nq", [1, 8, 9])
@pytest.mark.parametrize("d_bits", [128, 384, 1024, 3072, 4096])
def test_one_row_past_a_grid_stride(gpu, d_bits, nq):
    """n = one whole stride of the full grid + 1: the last row is the second trip of block 0, and it is the best row of query 0."""
    rng = np.random.default_rng(d_bits)
    idx = index_of(np.zeros((0, d_bits // 8), np.uint8), d_bits)
    n = idx.geometry(nq, 10)[1] + 1
    x, q = bits(rng, n, d_bits), bits(rng, nq, d_bits)
    x[-1] = q[0]
    idx.add(x)
    Do, Io = oracle(x, q, 10)
    assert Io[0, 0] == n - 1 and Do[0, 0] == 0
    check(idx, x, q, 10, Do, Io)
    idx.close()


@pytest.mark.parametrize("form", [1, 2])
def test_identical_rows_go_to_the_lower_row(gpu, form):
    rng = np.random.default_rng(7)
    x = np.repeat(bits(rng, 1, 1024), 200, axis=0)
    idx = index_of(x, 1024)
    D, I = idx.search(np.repeat(x[:1], 9, axis=0), 64, form=form)
    assert np.array_equal(I, np.tile(np.arange(64), (9, 1))) and not D.any()
    idx.close()


@pytest.mark.parametrize("nq", [3, 33])
@pytest.mark.parametrize("d_bits", [128, 3072])
def test_bitmap(gpu, d_bits, nq):
    from minivectordb_amd import _native
    rng = np.random.default_rng(d_bits + nq)
    n = 4100
    x, q = bits(rng, n, d_bits), bits(rng, nq, d_bits)
    idx = index_of(x, d_bits)
    half, none, tail = rng.random(n) < 0.5, np.zeros(n, bool), np.arange(n) >= 4096   # the tail: the last, ragged tile only
    for selected in (half, none, tail):
        Do, Io = oracle(x, q, 10, selected)
        check(idx, x, q, 10, Do, Io, _native.pack_row_mask(n, rows=np.flatnonzero(selected)))
    assert (Io[:, 4:] == -1).all() and (Do[:, 4:] == NONE).all() and (Io[:, :4] >= 4096).all()
    idx.close()


def test_sign_packing(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(3)
    d_bits, n = 384, 300
    x = rng.standard_normal((n + 9, d_bits)).astype(np.float32)
    special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45], np.float32)
    x[rng.random(x.shape) < 0.2] = 0.0
    x[:, ::5] = special[rng.integers(0, len(special), x[:, ::5].shape)]
    with np.errstate(invalid="ignore"):
        packed = np.packbits(x > 0, axis=1)
    idx = _native.BitsIndex(d_bits)
    idx.add_float(x[:n])
    assert np.array_equal(idx.get_rows(0, n), packed[:n])
    Do, Io = oracle(packed[:n], packed[n:], 10)
    D, I = idx.search_float(x[n:], 10)
    assert np.array_equal(D, Do) and np.array_equal(I, Io)
    idx.close()


def test_mutations_equal_a_fresh_index(gpu):
    from minivectordb_amd import _native
    rng = np.random.default_rng(11)
    d_bits = 1024
    x, q = bits(rng, 300, d_bits), bits(rng, 9, d_bits)
    idx = index_of(x, d_bits)
    idx.remove_rows([299, 0, 5])
    x = np.delete(x, [0, 5, 299], axis=0)
    new = bits(rng, 2, d_bits)
    idx.set_rows([100, 3], new)
    x[[100, 3]] = new
    f = rng.standard_normal((51, d_bits)).astype(np.float32)
    idx.add_float(f[:50])
    x = np.vstack([x, np.packbits(f[:50] > 0, axis=1)])
    idx.set_rows_float([1], f[50:])
    x[1] = np.packbits(f[50] > 0)
    idx.remove_rows([10])
    x = np.delete(x, [10], axis=0)
    assert idx.ntotal == len(x) and np.array_equal(idx.get_rows(0, len(x)), x)
    fresh = index_of(x, d_bits)
    Do, Io = oracle(x, q, 10)
    for nq in (3, 9):
        check(idx, x, q[:nq], 10, Do, Io)
        check(fresh, x, q[:nq], 10, Do, Io)
    idx.close()
    fresh.close()


def test_binary_vector_database_round_trip(gpu, tmp_path):
    from minivectordb_amd import BinaryVectorDatabase
    rng = np.random.default_rng(5)
    d_bits, n = 1024, 120
    f = rng.standard_normal((n, d_bits)).astype(np.float32)
    x = np.packbits(f > 0, axis=1)
    path = str(tmp_path / "bits.pkl")
    db = BinaryVectorDatabase(d_bits, storage_file=path)
    meta = [{"even": i % 2 == 0, "i": i} for i in range(n)]
    db.store_embeddings_batch([f"id{i}" for i in range(60)], list(f[:30]) + list(x[30:60]), meta[:60])   # floats, then packed
    for i in range(60, n):
        db.store_embedding(f"id{i}", x[i] if i % 3 else f[i], meta[i])
    assert np.array_equal(db.get_vector("id7"), x[7]) and np.array_equal(db.get_vector("id100"), x[100])

    def expect(rows_x, ids, q, k, selected=None):
        D, I = oracle(rows_x, q, k, selected)
        return [([ids[r] for r in I[j]], [int(h) for h in D[j]], [{"even": int(ids[r][2:]) % 2 == 0, "i": int(ids[r][2:])} for r in I[j]])
                for j in range(len(q))]

    ids = [f"id{i}" for i in range(n)]
    q = bits(rng, 12, d_bits)
    assert db.find_most_similar(f[3], k=5) == expect(x, ids, x[3:4], 5)[0]
    even = np.arange(n) % 2 == 0
    assert db.find_most_similar(q[0], metadata_filter={"even": True}, k=7) == expect(x, ids, q[:1], 7, even)[0]
    assert db.find_most_similar(q[1], exclude_filter={"i": 4}, k=7) == expect(x, ids, q[1:2], 7, np.arange(n) != 4)[0]
    assert db.find_most_similar_batch(list(q), k=5) == expect(x, ids, q, 5)
    db.delete_embedding("id4")
    with pytest.raises(ValueError):
        db.get_vector("id4")
    x, ids = np.delete(x, 4, axis=0), ids[:4] + ids[5:]
    db.persist_to_disk()
    again = BinaryVectorDatabase(d_bits, storage_file=path)
    for one in (db, again):
        assert one.find_most_similar_batch(list(q), metadata_filter={"even": True}, k=5) == \
            expect(x, ids, q, 5, np.array([int(u[2:]) % 2 == 0 for u in ids]))
