"""The three add entry points (include/mvdb.h: mvdb_index_add, _add_device, _add_synthetic) share one body (mvdb.hip:
append_rows) and differ only in how the new rows reach the matrix: they must leave the same index — the same stored rows bit
for bit, through a reallocation too, and the same fp16 shadow, extended in place where it fits."""
import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from conftest import assert_product_native
    assert_product_native()
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def add_through(native, idx, how, rows, seed, first, normalize):
    """`rows` = flat.synth(len(rows), d, seed, first) appended through one of the entry points."""
    if how == "host":
        idx.add(rows, normalize=normalize)
    elif how == "device":
        import torch
        t = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        idx.add_device(t.data_ptr(), rows.shape[0], normalize=normalize)
    else:
        idx.add_synthetic(rows.shape[0], seed, first_row=first, normalize=normalize)


HOW = ("host", "device", "synthetic")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("d", [30, 64])            # 30: padded rows (stride 32)
def test_add_paths_store_the_same_rows(native, d, normalize):
    n1, n2, seed = 1500, 551, 41
    x = flat.synth(n1 + n2, d, seed)
    stored = []
    for how in HOW:
        idx = native.FlatIndex(d)                  # not reserved: 1,500 rows of capacity, the second add reallocates
        add_through(native, idx, how, x[:n1], seed, 0, normalize)
        add_through(native, idx, how, x[n1:], seed, n1, normalize)
        assert idx.ntotal == n1 + n2
        stored.append(idx.get_rows(0, n1 + n2))
        idx.close()
    if not normalize:
        assert stored[0].tobytes() == x.tobytes()
    for how, got in zip(HOW[1:], stored[1:]):
        assert got.tobytes() == stored[0].tobytes(), how


def test_add_paths_extend_the_shadow_alike(native):
    n, d, nq, extra, seed = 20_001, 512, 40, 100, 43     # (test_update_gpu.test_shadow_kept_not_rebuilt: a batch that builds a shadow)
    x = flat.synth(n, d, 11)
    y = flat.synth(extra, d, seed, n)
    q = flat.synth(nq, d, 12)
    q[0] = y[5]                                    # the best row of query 0 is an appended one
    results = []
    for how in HOW:
        idx = native.FlatIndex(d)
        idx.reserve(n + extra)
        idx.add(x, normalize=True)
        idx.search(q, 10, normalize_q=True)
        assert idx.shadow_rows == n                # built by the batch
        add_through(native, idx, how, y, seed, n, True)
        assert idx.ntotal == n + extra
        assert idx.shadow_rows == n + extra, how   # extended by the add, before any search
        results.append(idx.search(q, 10, normalize_q=True))
        assert idx.shadow_rows == n + extra
        idx.close()
    assert results[0][1][0, 0] == n + 5
    for how, got in zip(HOW[1:], results[1:]):
        assert np.array_equal(got[0].view(np.uint32), results[0][0].view(np.uint32)), how
        assert np.array_equal(got[1], results[0][1]), how
