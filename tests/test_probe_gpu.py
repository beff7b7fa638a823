"""Probed search on the device (mvdb_index_search_probe, csrc/probe_scan.hpp): every comparison is exact.  The model is built
from the library's own existing routes, as in tests/test_assign_gpu.py: the probes of a query are what FlatIndex.search
returns for it alone on a second index that holds partition.centres(); the expected rows are what
idx.search_rowset(q_i, k, rowset(sorted union of the probed lists)) returns with nq = 1.  D is compared as bits, I as integers.

Corpus: test_assign_gpu.py's recipe — 64 Gaussian cluster centres + 0.35 noise, normalised on add — at N = 2,051 rows (no
multiple of any block step) and, for the dense bitmap (a sorted list becomes a bitmap only from 4,096 stored rows on), 4,099.
The centres are 70 perturbed stored rows; centre 40 is a copy of centre 5.  33 queries (a grid row of every launch
each): query 2 is all zeros, query 4 holds a NaN.  Work items are 128 list positions: the list of
1,500 rows of the caller-labelled partition is twelve of them."""
import numpy as np
import pytest

from probe_oracle import MISSING

pytestmark = pytest.mark.gpu

N, N_DENSE, CLUSTERS, C_MAX, NQ = 2051, 4099, 64, 70, 33
DIMS = [30, 100, 384, 512, 1024]
CS = [1, 7, 64, 70]
KS = [1, 10, 64]
NQS = [1, 5, 33]
ZEROQ, NANQ, TWIN, TWIN_OF = 2, 4, 40, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64, what
    assert np.array_equal(got[1], want[1]), (what, "I", np.argwhere(got[1] != want[1])[:5])
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, "D", np.argwhere(bits(got[0]) != bits(want[0]))[:5])


def make_corpus(d, n):
    rng = np.random.default_rng(2000 + d)
    centres = rng.standard_normal((CLUSTERS, d)).astype(np.float32)
    x = centres[np.arange(n) % CLUSTERS] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32)
    return x, rng


def model(idx, cidx, labels, q, k, nprobe, normalize_q=True, selected=None):
    """(D, I, probes per query) from the existing routes: nq = 1 calls only."""
    nq = q.shape[0]
    D = np.full((nq, k), MISSING, np.float32)
    I = np.full((nq, k), -1, np.int64)
    probed = []
    for i in range(nq):
        _, Ic = cidx.search(q[i:i + 1], nprobe, normalize_q=normalize_q)
        P = Ic[0][Ic[0] >= 0]
        probed.append(P)
        rows = np.flatnonzero(np.isin(labels, P) & (labels >= 0)).astype(np.int64)
        if selected is not None:
            rows = np.intersect1d(rows, selected)
        if len(rows):
            rs = idx.rowset(rows)
            D[i], I[i] = (a[0] for a in idx.search_rowset(q[i:i + 1], k, rs, normalize_q=normalize_q))
            rs.close()
    return D, I, probed


_WORLDS = {}


class World:
    """One index per (width, size), built once: centres, queries, and per C the partition labelled by the library, the index of
    its stored centres and its labels."""

    def __init__(self, d, n):
        from minivectordb_amd import _native
        x, rng = make_corpus(d, n)
        self.d, self.n = d, n
        self.idx = _native.FlatIndex(d)
        self.idx.add(x, normalize=True)
        stored = self.idx.get_rows(0, n)
        c = stored[rng.permutation(n)[:C_MAX]] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((C_MAX, d)).astype(np.float32)
        c[TWIN] = c[TWIN_OF]
        self.c = np.ascontiguousarray(c, dtype=np.float32)
        q = stored[rng.permutation(n)[:NQ]] + np.float32(0.5 / np.sqrt(d)) * rng.standard_normal((NQ, d)).astype(np.float32)
        q[ZEROQ] = 0
        q[NANQ, 1] = np.nan
        self.q = np.ascontiguousarray(q, dtype=np.float32)
        self._parts = {}

    def centre_index(self, part):
        from minivectordb_amd import _native
        cidx = _native.FlatIndex(self.d)
        cidx.add(part.centres(), normalize=False)
        return cidx

    def partition(self, C):
        """(partition labelled by the library, index of its centres, its labels)."""
        if C not in self._parts:
            part = self.idx.partition(self.c[:C], normalize_c=True)
            self._parts[C] = (part, self.centre_index(part), part.labels())
        return self._parts[C]


def world(d, n=N):
    if (d, n) not in _WORLDS:
        _WORLDS[d, n] = World(d, n)
    return _WORLDS[d, n]


# ---- widths, list counts, probes, k, batch sizes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("d", DIMS)
def test_every_width_list_count_nprobe_k_and_batch(gpu, d, C):
    w = world(d)
    part, cidx, labels = w.partition(C)
    assert len(part) == N and part.n_lists == C and int(part.sizes().sum()) == int((labels >= 0).sum())
    assert np.array_equal(part.sizes(), np.bincount(labels[labels >= 0], minlength=C))
    for nprobe in sorted({1, min(3, C), C}):
        for k in KS:
            want = model(w.idx, cidx, labels, w.q, k, nprobe)
            for nq in NQS:
                got = w.idx.search_probe(w.q[:nq], k, nprobe, part, normalize_q=True)
                same(got, (want[0][:nq], want[1][:nq]), (d, C, nprobe, k, nq))
            assert (want[1][NANQ] == -1).all() and (want[0][NANQ] == MISSING).all()    # every score NaN: all missing markers
            if nprobe == C:                                                             # the exact search over the labelled rows
                assert (labels >= 0).all()
                for i in range(NQ):                                                     # (a batch of search takes other routes: per query)
                    same((want[0][i:i + 1], want[1][i:i + 1]), w.idx.search(w.q[i:i + 1], k, normalize_q=True), ("exact", d, C, k, i))


@pytest.mark.parametrize("d", [100, 512])
def test_labels_none_equals_assign_and_queries_as_they_are(gpu, d):
    w = world(d)
    for C in (7, 70):
        part, cidx, labels = w.partition(C)
        want_labels, _ = w.idx.assign(w.c[:C], normalize_c=True)
        assert labels.dtype == np.int32 and np.array_equal(labels, want_labels)
        assert not (labels == TWIN).any()                                               # equal scores: the lower centre
        # normalize_c = False: the centres as given; normalize_q = False: the queries as given
        raw = w.idx.partition(w.c[:C], normalize_c=False)
        assert np.array_equal(bits(raw.centres()), bits(w.c[:C]))
        assert np.array_equal(raw.labels(), w.idx.assign(w.c[:C], normalize_c=False)[0])
        rcidx = w.centre_index(raw)
        for nq_norm in (False, True):
            want = model(w.idx, rcidx, raw.labels(), w.q, 10, min(3, C), normalize_q=nq_norm)
            same(w.idx.search_probe(w.q, 10, min(3, C), raw, normalize_q=nq_norm), want[:2], ("raw", d, C, nq_norm))
        raw.free()
        rcidx.close()
    assert np.array_equal(part.labels(5, 20), labels[5:25])


def test_caller_labels_a_giant_list_empty_lists_and_unlabelled_rows(gpu):
    for d in (100, 512):
        w = world(d)
        order = np.random.default_rng(3).permutation(N)
        labels = np.full(N, -1, np.int32)
        labels[order[:1500]] = 0          # twelve work items
        labels[order[1500:1800]] = 2
        labels[order[1800:1997]] = 5
        labels[order[1997:2000]] = 4      # three rows
        part = w.idx.partition(w.c[:7], labels=labels, normalize_c=True)          # lists 1, 3, 6 are empty, 51 rows are in no list
        assert part.sizes().tolist() == [1500, 0, 300, 0, 3, 197, 0] and np.array_equal(part.labels(), labels)
        cidx = w.centre_index(part)
        for nprobe in (1, 3, 7):
            for k in (1, 10, 64):
                want = model(w.idx, cidx, labels, w.q, k, nprobe)
                got = w.idx.search_probe(w.q, k, nprobe, part, normalize_q=True)
                same(got, want[:2], ("caller", d, nprobe, k))
                hit = got[1][got[1] >= 0]
                assert (labels[hit] >= 0).all()                                     # a row labelled -1 never comes back
        # fewer than k rows in the probed list: padding
        q4 = part.centres()[4:5]
        D, I = w.idx.search_probe(q4, 10, 1, part)
        want = model(w.idx, cidx, labels, q4, 10, 1, normalize_q=False)
        assert want[2][0].tolist() == [4]
        same((D, I), want[:2], "short list")
        assert (I[0, :3] >= 0).all() and (I[0, 3:] == -1).all() and (D[0, 3:] == MISSING).all()
        assert sorted(I[0, :3].tolist()) == sorted(order[1997:2000].tolist())
        part.free()
        cidx.close()


def test_a_far_centre_has_an_empty_list_and_takes_its_probe_slot(gpu):
    from minivectordb_amd import _native
    d, n = 100, 600
    x, rng = make_corpus(d, n)
    x[:, 0] = np.abs(x[:, 0]) + 10                                                  # every row leans towards +e0 ...
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    stored = idx.get_rows(0, n)
    far = np.zeros((1, d), np.float32)
    far[0, 0] = -1                                                                  # ... and -e0 is nearest to none of them
    c = np.concatenate([stored[[3, 77, 140, 205, 333, 590]] + np.float32(0.02) * rng.standard_normal((6, d)).astype(np.float32), far])
    part = idx.partition(c.astype(np.float32), normalize_c=True)
    assert part.sizes()[6] == 0 and part.sizes().sum() == n
    w = world(d)
    cidx = w.centre_index(part)
    q = np.concatenate([part.centres()[6:7], stored[:3]])
    for nprobe in (1, 2, 7):
        want = model(idx, cidx, part.labels(), q, 10, nprobe, normalize_q=False)
        assert want[2][0][0] == 6                                                   # the empty list ranks first for its own centre
        same(idx.search_probe(q, 10, nprobe, part), want[:2], ("far", nprobe))
    D, I = idx.search_probe(q[:1], 10, 1, part)
    assert (I == -1).all() and (D == MISSING).all()                                 # the slot is taken, nothing is scanned
    D, I = idx.search_probe(q[:1], 10, 2, part)
    assert I[0, 0] >= 0                                                             # ... the second probe's list is
    part.free()
    cidx.close()
    idx.close()


def test_twin_centres_go_to_the_lower_centre_and_twin_rows_to_the_lower_row(gpu):
    from minivectordb_amd import _native
    w = world(100)
    part, cidx, assigned = w.partition(C_MAX)
    labels = assigned.copy()
    members = np.flatnonzero(labels == TWIN_OF)
    assert len(members) >= 2
    labels[members[::2]] = TWIN                                                     # both twins own rows now
    twins = w.idx.partition(w.c, labels=labels, normalize_c=True)
    q = twins.centres()[TWIN_OF:TWIN_OF + 1]
    D, I = w.idx.search_probe(q, 64, 1, twins)
    same((D, I), model(w.idx, cidx, labels, q, 64, 1, normalize_q=False)[:2], "twin centres")
    hit = I[0][I[0] >= 0]
    assert len(hit) == min(64, len(members) - len(members[::2])) and (labels[hit] == TWIN_OF).all()
    D, I = w.idx.search_probe(q, 64, 2, twins)
    hit = I[0][I[0] >= 0]
    assert set(labels[hit].tolist()) == {TWIN_OF, TWIN}
    twins.free()
    # twin rows in different lists
    x, rng = make_corpus(100, 600)
    x[411] = x[17]
    idx = _native.FlatIndex(100)
    idx.add(x, normalize=True)
    lab = (np.arange(600) % 3).astype(np.int32)
    assert lab[17] != lab[411]
    p = idx.partition(w.c[:3], labels=lab)
    q = idx.get_rows(17, 1)
    D, I = idx.search_probe(q, 2, 3, p)
    assert I[0].tolist() == [17, 411] and bits(D)[0, 0] == bits(D)[0, 1]
    D, I = idx.search_probe(q, 1, 3, p)
    assert I[0].tolist() == [17]
    p.free()
    idx.close()


# ---- row sets -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 512])
def test_bitmap_row_sets(gpu, d):
    for n, kinds in ((N, ("excluded", "empty")), (N_DENSE, ("dense", "excluded"))):
        w = world(d, n)
        part, cidx, labels = w.partition(64)
        every = np.arange(n, dtype=np.int64)
        for kind in kinds:
            if kind == "dense":
                selected = np.setdiff1d(every, np.arange(5, n, 40))                 # 97.5 % of the rows, sorted: a bitmap
                rs = w.idx.rowset(selected)
            elif kind == "excluded":
                gone = np.array([99, 100, 7, n - 1] + list(range(300, 900)), np.int64)
                selected = np.setdiff1d(every, gone)
                rs = w.idx.rowset(gone, excluded=True)
            else:
                selected = np.empty(0, np.int64)
                rs = w.idx.rowset(every, excluded=True)
            assert rs.is_bitmap and len(rs) == len(selected)
            for nprobe, k in ((1, 10), (3, 64), (64, 1)):
                want = model(w.idx, cidx, labels, w.q, k, nprobe, selected=selected)
                same(w.idx.search_probe(w.q, k, nprobe, part, rowset=rs, normalize_q=True), want[:2], (d, n, kind, nprobe, k))
            rs.close()
    w = world(d)
    part, _, _ = w.partition(64)
    listed = w.idx.rowset(np.arange(0, 900, dtype=np.int64))
    assert not listed.is_bitmap
    with pytest.raises(ValueError, match="bitmap"):
        w.idx.search_probe(w.q, 10, 3, part, rowset=listed)


# ---- the device variant, staleness, argument errors ----------------------------------------------------------------------------------

def _device_call(idx, part, q, k, nprobe, rowset=None, stream=0, label_offset=0, normalize_q=True):
    """search_probe_device on prefilled tensors: (error, D, I) as numpy, whatever the call did."""
    import torch
    nq = q.shape[0]
    qt = torch.from_numpy(q).cuda()
    Dt = torch.full((nq, max(k, 1)), 7.5, dtype=torch.float32, device="cuda")
    It = torch.full((nq, max(k, 1)), 777, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        idx.search_probe_device(qt.data_ptr(), nq, k, nprobe, part, Dt.data_ptr(), It.data_ptr(), rowset=rowset, stream=stream,
                                normalize_q=normalize_q, label_offset=label_offset)
        err = None
    except ValueError as e:
        err = e
    torch.cuda.synchronize()
    return err, Dt.cpu().numpy(), It.cpu().numpy()


def _untouched(res):
    err, D, I = res
    return isinstance(err, ValueError) and (D == 7.5).all() and (I == 777).all()


def test_host_and_device_variants_agree(gpu):
    import torch
    stream = torch.cuda.Stream()
    for d, C, nprobe, k in ((30, 7, 3, 10), (384, 70, 70, 64), (512, 64, 3, 1)):
        w = world(d)
        part, _, _ = w.partition(C)
        host = w.idx.search_probe(w.q, k, nprobe, part, normalize_q=True)
        for s, off in ((0, 0), (stream.cuda_stream, 10 ** 10)):
            err, D, I = _device_call(w.idx, part, w.q, k, nprobe, stream=s, label_offset=off)
            assert err is None
            same((D, np.where(I >= 0, I - off, I)), host, ("device", d, C, s))
            assert (I[host[1] < 0] == -1).all()


def test_a_stale_partition_is_refused_and_update_follows_the_index(gpu):
    from minivectordb_amd import _native
    d = 100
    x, rng = make_corpus(d, N + 300)
    w = world(d)
    c = w.c[:64]
    idx = _native.FlatIndex(d)
    idx.add(x[:N], normalize=True)
    part = idx.partition(c, normalize_c=True)
    cidx = w.centre_index(part)
    gone = idx.rowset(np.arange(40, 700, dtype=np.int64), excluded=True)
    calls0 = idx.probe_counters()

    def check(p, what, rs=None, selected=None):
        fresh = idx.partition(c, normalize_c=True)
        labels = p.labels()
        assert len(p) == idx.ntotal and np.array_equal(labels, fresh.labels()) and np.array_equal(labels, idx.assign(c, normalize_c=True)[0])
        assert np.array_equal(p.sizes(), fresh.sizes())
        for nprobe, k in ((1, 10), (3, 64), (64, 10)):
            got = idx.search_probe(w.q, k, nprobe, p, rowset=rs, normalize_q=True)
            same(got, idx.search_probe(w.q, k, nprobe, fresh, rowset=rs, normalize_q=True), (what, "rebuild", nprobe, k))
            same(got, model(idx, cidx, labels, w.q, k, nprobe, selected=selected)[:2], (what, "model", nprobe, k))
        fresh.free()

    check(part, "created")
    # rows added: refused until update
    idx.add(x[N:], normalize=True)
    res = _device_call(idx, part, w.q, 10, 3)
    assert _untouched(res) and "mvdb_partition_update" in str(res[0])
    with pytest.raises(ValueError, match="mvdb_partition_update"):
        idx.search_probe(w.q, 10, 3, part)
    part.update()
    check(part, "added")
    # a bitmap built before the add: the new rows are not in it
    check(part, "old bitmap", rs=gone, selected=np.setdiff1d(np.arange(N, dtype=np.int64), np.arange(40, 700)))
    # rows that change their nearest centre
    moved = np.array([10, 11, 12, N + 5], np.int64)
    before = part.labels()[moved]
    donors = np.array([int(np.flatnonzero(part.labels() != b)[j * 37]) for j, b in enumerate(before)])
    idx.set_rows(moved, idx.get_rows(0, idx.ntotal)[donors], normalize=True)
    same(idx.search_probe(w.q, 10, 3, part, normalize_q=True),                            # still valid: old lists, new vectors
         model(idx, cidx, part.labels(), w.q, 10, 3)[:2], "before update")
    part.update(moved)
    assert (part.labels()[moved] != before).all()
    check(part, "moved")
    part.update()                                                                   # nothing to do
    check(part, "no-op")
    # another index
    other = world(384)
    foreign, _, _ = other.partition(7)
    res = _device_call(idx, foreign, w.q, 10, 3)
    assert _untouched(res) and "another index" in str(res[0])
    with pytest.raises(ValueError, match="another index"):
        idx.search_probe(w.q, 10, 3, foreign)
    # rows removed: update and search are refused; re-created from the labels that are left
    kept_labels = np.delete(part.labels(), [3, 500])
    calls1 = idx.probe_counters()
    idx.remove_rows(np.array([3, 500], np.int64))
    res = _device_call(idx, part, w.q, 10, 3)
    assert _untouched(res) and "removed" in str(res[0])
    with pytest.raises(ValueError, match="removed"):
        part.update()
    with pytest.raises(ValueError, match="removed"):
        idx.search_probe(w.q, 10, 3, part)
    assert idx.probe_counters() == calls1 and calls1[0] > calls0[0]
    again = idx.partition(part.centres(), labels=kept_labels)
    check(again, "re-created")
    idx.close()


def test_argument_errors_write_nothing(gpu):
    from minivectordb_amd import _native
    w = world(100)
    part, _, _ = w.partition(7)
    for k, nprobe in ((0, 3), (65, 3), (10, 0), (10, 8)):
        assert _untouched(_device_call(w.idx, part, w.q, k, nprobe)), (k, nprobe)
    with pytest.raises(ValueError, match="k <= 64"):
        w.idx.search_probe(w.q, 65, 3, part)
    with pytest.raises(ValueError, match="nprobe"):
        w.idx.search_probe(w.q, 10, 8, part)
    with pytest.raises(ValueError):
        w.idx.partition(np.zeros((4097, 100), np.float32))
    with pytest.raises(ValueError, match="out of range"):
        w.idx.partition(w.c[:7], labels=np.full(N, 7, np.int32))
    with pytest.raises(ValueError, match="out of range"):
        w.idx.partition(w.c[:7], labels=np.full(N, -2, np.int32))
    with pytest.raises(ValueError):
        w.idx.partition(w.c[:7], labels=np.zeros(N - 1, np.int32))
    l2 = _native.FlatIndex(100, metric=1)
    l2.add(w.q)
    with pytest.raises(ValueError, match="inner-product"):
        l2.partition(w.c[:7])
    l2.close()
    empty = _native.FlatIndex(100)
    p = empty.partition(w.c[:7])
    D, I = empty.search_probe(w.q, 5, 7, p)
    assert len(p) == 0 and (I == -1).all() and (D == MISSING).all()
    empty.close()


def test_results_do_not_depend_on_the_chunking(gpu):
    for d, C, nprobe, k in ((100, 70, 70, 64), (512, 64, 3, 10)):
        w = world(d)
        part, _, _ = w.partition(C)
        base = w.idx.search_probe(w.q, k, nprobe, part, normalize_q=True)
        try:
            for budget, chunks in ((1, NQ), (None, None)):
                calls0, launches0 = w.idx.probe_counters()
                if budget is None:                                                  # room for exactly two queries per chunk
                    pieces = np.sort(-(-part.sizes() // 128))[::-1][:nprobe].sum()      # work items of 128 list positions
                    budget, chunks = int(2 * (pieces * (8 + 8 * k) + 4 * C)), -(-NQ // 2)
                w.idx.set_option("probe_table_bytes", budget)
                same(w.idx.search_probe(w.q, k, nprobe, part, normalize_q=True), base, ("chunks", d, budget))
                calls1, launches1 = w.idx.probe_counters()
                assert calls1 - calls0 == 1 and launches1 - launches0 == 4 * chunks
            with pytest.raises(ValueError, match="probe_table_bytes"):
                w.idx.set_option("probe_table_bytes", 0)
        finally:
            w.idx.set_option("probe_table_bytes", 256 << 20)
        calls0, launches0 = w.idx.probe_counters()
        same(w.idx.search_probe(w.q, k, nprobe, part, normalize_q=True), base, ("default", d))
        assert w.idx.probe_counters() == (calls0 + 1, launches0 + 4)
