"""The int8 cosine contract without a GPU: the oracle (tests/cos8_oracle.py) against a per-element restatement and against
a float64 brute force, and ShardedVectorDatabaseUsearch's bookkeeping driven through a CPU stand-in of Cos8Index."""
import os
import pickle
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cos8_oracle as O  # noqa: E402


def adversarial(d, rng):
    rows = [np.zeros(d), np.eye(1, d, d // 2)[0], -np.eye(1, d, 0)[0], np.full(d, 1e-30), np.full(d, 1e30),
            np.full(d, 3e37), np.full(d, 1.0), np.full(d, -2.5e-42)]
    b = rng.integers(-127, 128, d).astype(np.float64)
    rows += [b, b / 3.0, (b + 0.5) * 1e-3, b * 1e20]
    one = np.zeros(d)
    one[0] = 1.0
    if d > 1:
        one[1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    rows.append(one)
    rows += list(rng.standard_normal((6, d)))
    x = np.stack(rows).astype(np.float32)
    x[-1, 0] = np.nan     # a non-finite magnitude: all zeros
    return x


@pytest.mark.parametrize("d", [1, 2, 3, 17, 384, 512, 1024])
def test_quantize_matches_per_element_restatement(d):
    x = adversarial(d, np.random.default_rng(d))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        codes, a2 = O.quantize(x)
        for i, row in enumerate(x):
            want = O.quantize_scalar(row)
            assert list(codes[i]) == want, (d, i)
            assert a2[i] == sum(c * c for c in want)
    assert np.abs(codes.astype(int)).max() <= 127
    assert not codes[0].any() and not codes[-1].any()


def test_quantize_unit_rows():
    codes, a2 = O.quantize(np.eye(4, dtype=np.float32) * 3.0)
    assert (np.diag(codes) == 127).all() and (a2 == 127 * 127).all()
    # colinear rows quantise alike whatever their length (a power-of-two scale is exact at every step)
    x = np.array([[0.3, -0.7], [0.6, -1.4], [3e-20, -7e-20]], np.float32)
    c, _ = O.quantize(x)
    assert (c[0] == c[1]).all()


def test_distance_special_cases_and_scalar_agreement():
    rng = np.random.default_rng(0)
    assert O.distance_scalar(0, 0, 0) == 0 and O.distance_scalar(0, 5, 0) == 1 and O.distance_scalar(0, 5, 7) == 1
    ab = rng.integers(-10**6, 10**6, (3, 50))
    a2 = rng.integers(0, 10**6, 50)
    b2 = rng.integers(0, 10**6, 3)
    a2[:3] = 0
    b2[0] = 0
    got = O.distance(ab, a2, b2)
    for i in range(3):
        for j in range(50):
            assert got[i, j] == O.distance_scalar(int(ab[i, j]), int(a2[j]), int(b2[i]))


@pytest.mark.parametrize("d", [2, 17, 384])
def test_search_matches_float64_full_sort(d):
    rng = np.random.default_rng(d)
    x = rng.standard_normal((500, d)).astype(np.float32)
    x[100:110] = x[3]
    x[200] = 0
    q = np.concatenate([x[3:4], rng.standard_normal((4, d)).astype(np.float32), np.zeros((1, d), np.float32)])
    codes, a2 = O.quantize(x)
    qc, qb2 = O.quantize(q)
    for k in (1, 10, 600):
        D, I = O.search(codes, a2, q, k)
        for i in range(q.shape[0]):
            dist = np.array([O.distance_scalar(int(np.dot(qc[i].astype(np.int64), codes[r].astype(np.int64))), int(a2[r]),
                                               int(qb2[i])) for r in range(500)], np.float32)
            order = sorted(range(500), key=lambda r: (float(dist[r]), r))[:k]
            take = min(k, 500)
            assert list(I[i, :take]) == order and np.array_equal(D[i, :take], dist[order])
            assert (I[i, take:] == -1).all()
        Dc, Ic = O.search_chunked(codes, a2, q, min(k, 50), chunk=128)
        assert np.array_equal(Ic, I[:, :min(k, 50)]) and np.array_equal(Dc, D[:, :min(k, 50)])


# ---- the database class through a CPU stand-in of the device index ---------------------------------------------------
class FakeCos8:
    """Cos8Index restated on the oracle (what the device computes, bit for bit, per tests/test_cos8_gpu.py)."""

    def __init__(self, d, device=0):
        self.d = d
        self.codes = np.zeros((0, d), np.int8)
        self.a2 = np.zeros(0, np.int32)

    @property
    def ntotal(self):
        return self.codes.shape[0]

    def add(self, x, normalize=None):
        c, a = O.quantize(np.atleast_2d(x))
        self.codes = np.concatenate([self.codes, c])
        self.a2 = np.concatenate([self.a2, a])

    def remove_rows(self, rows):
        self.codes = np.delete(self.codes, rows, axis=0)
        self.a2 = np.delete(self.a2, rows)

    def reset(self):
        self.__init__(self.d)

    def search(self, q, k, normalize_q=None):
        return O.search(self.codes, self.a2, np.atleast_2d(q), k)

    def rowset(self, rows, excluded=False):
        rows = np.asarray(rows, np.int64)
        return np.setdiff1d(np.arange(self.ntotal), rows) if excluded else np.sort(rows)

    def search_rowset(self, q, k, rowset, normalize_q=None):
        return O.search(self.codes, self.a2, np.atleast_2d(q), k, rows=rowset)


@pytest.fixture
def fake_index(monkeypatch):
    from minivectordb_amd import _native
    monkeypatch.setattr(_native, "Cos8Index", FakeCos8)


def test_class_bookkeeping(fake_index, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    rng = np.random.default_rng(1)
    d = 24
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=4)
    assert db.find_most_similar(np.ones(d), k=3) == ([], [], [])
    x = rng.standard_normal((10, d)).astype(np.float32)
    db.store_embeddings_batch([f"id{i}" for i in range(10)], list(x), [{"g": i % 2, "n": i} for i in range(10)])
    db.store_embedding("dup", x[2] * 4.0, {"g": 1})
    assert sorted(os.listdir(tmp_path / "u")) == ["shard_0.pkl", "shard_1.pkl", "shard_2.pkl"]
    with open(tmp_path / "u" / "shard_2.pkl", "rb") as f:
        shard = pickle.load(f)
    assert shard["unique_ids"] == ["id8", "id9", "dup"]
    assert np.array_equal(shard["embeddings"][2], x[2] * 4.0)   # raw rows: never normalised
    assert np.array_equal(db.embeddings, np.concatenate([x, x[2:3] * 4.0]))
    assert np.array_equal(db.get_vector("id9"), x[9])            # position inside the shard
    ids, dist, metas = db.find_most_similar(x[2], k=3)
    assert ids[:2] == ("id2", "dup") and dist[0] == dist[1] == np.float32(0.0)
    assert all(isinstance(v, np.float32) for v in dist) and metas[0] == {"g": 0, "n": 2}
    ids, _, _ = db.find_most_similar(x[2], metadata_filter={"g": 1}, k=20)
    assert set(ids) == {"id1", "id3", "id5", "id7", "id9", "dup"}
    ids, _, _ = db.find_most_similar(x[2], exclude_filter={"g": 0}, k=20)
    assert set(ids) == {"id1", "id3", "id5", "id7", "id9", "dup"}
    assert db.find_most_similar(x[2], metadata_filter={"g": 5}, k=3) == ([], [], [])
    batch = db.find_most_similar_batch(np.stack([x[2], x[5]]), k=4)
    assert batch == [db.find_most_similar(x[2], k=4), db.find_most_similar(x[5], k=4)]
    db.delete_embeddings_batch(["id2", "id4"])
    ids, _, _ = db.find_most_similar(x[2], k=2)
    assert ids[0] == "dup" and "id2" not in db.unique_ids
    with pytest.raises(ValueError):
        db.get_vector("id2")
    again = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=4)
    assert again.unique_ids == db.unique_ids
    assert again.find_most_similar(x[7], k=5) == db.find_most_similar(x[7], k=5)


def test_autocut_distances_quirks(fake_index, tmp_path):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "a"))
    f = np.float32
    assert db.autocut_distances([f(0.1), f(0.11), f(0.5), f(0.52)]) == [2, 3]
    assert db.autocut_distances([f(0.1), f(0.11), f(0.12)]) == []
    with pytest.warns(RuntimeWarning):
        assert db.autocut_distances([f(0.0), f(0.3), f(0.31)]) == [1, 2]     # 0.3 / 0 -> inf, as numpy float32 does
    x = np.array([[1, 0, 0], [1, 0, 0], [0.9, 0.1, 0], [0, 1, 0]], np.float32)
    db.store_embeddings_batch([1, 2, 3, 4], list(x), [{}, {}, {}, {}])
    with pytest.warns(RuntimeWarning):
        ids, dist, _ = db.find_most_similar(x[0], k=4, autocut=True)
    # two exact duplicates first: 0 / 0 is nan, and max() over a list that starts with nan returns nan, so nothing is cut
    assert ids == (1, 2, 3, 4) and dist[0] == dist[1] == 0
    with pytest.warns(RuntimeWarning):
        ids, _, _ = db.find_most_similar(x[0], exclude_filter={"x": 1}, k=4, autocut=True)
    db.store_embedding(5, np.array([1, 0.2, 0], np.float32), {"t": 1})
    ids, dist, _ = db.find_most_similar(np.array([1, 0.2, 0], np.float32), metadata_filter={"t": 1}, k=2, autocut=True)
    assert ids == (5,)
    ids, dist, _ = db.find_most_similar(x[2], k=3, autocut=True)
    assert ids == [3] and isinstance(ids, list)     # 0 then a jump: everything after the zero is cut


# ---- the case tables of the GPU tests (tests/cos8_cases.py) ----------------------------------------------------------
import cos8_cases as C  # noqa: E402


def test_expected_form_restates_the_dispatch():
    assert len(C.all_scan_forms()) == 96 and len(C.all_mfma_forms()) == 2
    assert [C.width_class(c) for c in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 256)] == \
        [(1, 1), (2, 1), (4, 1), (4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 4), (64, 4)]
    assert C.expected_form(512, 1, 10, "none") == ("scan", 32, 1, 1, 0, False)
    assert C.expected_form(512, 7, 10, "excluded") == ("scan", 32, 1, 8, 2, False)
    assert C.expected_form(512, 8, 10, "excluded") == ("mfma", 2)
    assert C.expected_form(512, 8, 64, "none") == ("mfma", 0)
    assert C.expected_form(512, 8, 65, "none") == ("scan", 32, 1, 8, 0, True)      # large k: never the matrix cores
    assert C.expected_form(512, 33, 10, "list") == ("scan", 32, 1, 8, 1, False)    # a row list: never the matrix cores
    assert C.expected_form(1024, 8, 10, "none") == ("mfma", 0)
    assert C.expected_form(1025, 8, 10, "none") == ("scan", 64, 4, 4, 0, False)    # the queries no longer fit in LDS
    assert C.expected_form(4096, 1, 200, "bitmap") == ("scan", 64, 4, 1, 2, True)
    assert C.rowset_is_bitmap(800, 99, False) is False and C.rowset_is_bitmap(800, 100, False) is True
    assert C.rowset_is_bitmap(800, 0, True) is True


def test_case_table_reaches_every_kernel_form():
    """A condition on the table: under expected_form the GPU cases launch all 96 instantiations of cos8_scan_kernel and
    both of cos8_mfma_kernel, and the matrix-core cases cover, for every row and for the bitmap: an odd and an even chunk
    count, rows of at most 8 K-steps and of more, k = 1 and k = 64."""
    assert len(set(C.CASES)) == len(C.CASES)
    forms = {}
    for case in C.CASES:
        n, d, nq, k, kind = case
        assert kind in C.FILTER_KINDS and 1 <= d <= C.MAX_D and 1 <= k <= C.MAX_K and n % 2 == 1 and n > 2048
        rows, excluded, keep = C.filter_rows(n, kind)
        if kind != "none":       # the rows of the case really are stored the way expected_form assumes
            assert C.rowset_is_bitmap(n, len(rows), excluded) == (C.FILTER_FORM[kind] == 2), case
            assert len(keep) > 200, case
        forms.setdefault(C.expected_form(d, nq, k, kind), []).append(case)
    scan = {f for f in forms if f[0] == "scan"}
    assert scan == C.all_scan_forms(), sorted(C.all_scan_forms() - scan)
    assert len(scan) == 96
    assert {f for f in forms if f[0] == "mfma"} == C.all_mfma_forms()
    for F in (0, 2):
        mf = forms[("mfma", F)]
        chunks = [C.nchunk_of(d) for _, d, _, _, _ in mf]
        strides = [16 * c for c in chunks]
        ks = [k for _, _, _, k, _ in mf]
        assert any(c % 2 == 1 for c in chunks) and any(c % 2 == 0 for c in chunks), (F, chunks)
        assert any(s <= 256 for s in strides) and any(s > 256 for s in strides), (F, strides)
        assert 1 in ks and 64 in ks, (F, ks)
        assert {nq for _, _, nq, _, _ in mf} >= {8, 33, 70}       # one pass, a partial second pass, a partial third
    # every d of the table's classes is used, both ends of each class, and the documented maximum
    assert {d for _, d, _, _, _ in C.CASES} >= {d for dims in C.CLASS_DIMS for d in dims} | {C.MAX_D}
    assert {k for _, _, _, k, _ in C.CASES} >= {1, 10, 64, 65, 200}


@pytest.mark.parametrize("d", [1, 3, 17, 64, 1000, 4096])
def test_special_rows_match_per_element_restatement(d):
    x = C.special_rows(d, np.random.default_rng(d))
    assert x.dtype == np.float32 and x.shape[1] == d
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        codes, a2 = O.quantize(x)
        for i, row in enumerate(x):
            want = O.quantize_scalar(row)
            assert list(codes[i]) == want, (d, i)
            assert a2[i] == sum(c * c for c in want)
    for i in C.SPECIAL_ZERO_ROWS:
        assert not codes[i].any(), (d, i)
    assert (codes[7] == 127).all() and a2[7] == 127 * 127 * d            # x * 127f overflows: every code clamps
    assert (codes[8] == -int(127 / np.sqrt(d))).all()                    # subnormals are kept, not flushed
    assert codes[4].any() and codes[3].any() and codes[11].any()


def test_kernel_census_lists_every_form():
    """profiles/cos8_forms_kernel_census.txt is a kernel trace of the GPU file on the device: the symbols it saw are the
    forms that expected_form() predicts, so the restatement of the dispatch above tells the truth."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "cos8_forms_kernel_census.txt")) as f:
        seen = set(re.findall(r"cos8_(?:scan|mfma)_kernel<[^>]*>", f.read()))
    want = {"cos8_mfma_kernel<%d>" % f[1] for f in C.all_mfma_forms()}
    want |= {"cos8_scan_kernel<%d, %d, %d, %d, %s>" % (f[1], f[2], f[3], f[4], "true" if f[5] else "false")
             for f in C.all_scan_forms()}
    assert len(want) == 98 and seen == want, sorted(seen ^ want)
