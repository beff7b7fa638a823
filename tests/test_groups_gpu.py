"""Group hits search on the device (mvdb_index_search_groups, csrc/group_hits.hpp): every comparison is exact.  Each case takes
the groups G from search_distinct (tested in tests/test_distinct_gpu.py) for the same call and the members from the query's
full ranking — nq = 1, k = the rows selected, on the default routing — through tests/groups_oracle.py, the contract in numpy.

Corpus: tests/test_distinct_gpu.py's, restated — 4096 rows, 64 Gaussian cluster centres + 0.35 noise (row i belongs to cluster
i % 64), normalised on add; rows 100-109 and the last 5 are copies of row 99.  Queries: perturbed stored rows; query 0 sits
near row 99, query 1 IS row 99, the others are away from it.  Groupings: MAIN (row // 8 in general; the cluster of row 99 with
the near copies is ONE group, 512; the last 5 rows sit in five groups of their own; three singletons), FEW (one big group and
40 rows of their own), OWN (every row its own group) and ONE (all rows in one group: every row matches).

Every call is held to the member_rows counter as well: it must move by exactly the model's count of selected rows whose code
is one of the query's groups, so a pass that scores non-members, or skips members, cannot pass unnoticed."""
import numpy as np
import pytest

from distinct_oracle import MISSING
from groups_oracle import member_rows, members

pytestmark = pytest.mark.gpu

N, CLUSTERS, NQ_MAX = 4096, 64, 33
COPIES = list(range(99, 110)) + list(range(N - 5, N))
DIMS = [30, 100, 384, 512, 1024]
SHAPES = [(1, 1, 1), (5, 3, 32), (10, 5, 64), (3, 16, 32), (64, 16, 64)]     # (k, group_size, fetch_k)
NQS = [1, 3, 33]
DEFAULT_PARTIALS_BYTES = 64 << 20


def make_corpus(d):
    rng = np.random.default_rng(1000 + d)
    centres = rng.standard_normal((CLUSTERS, d)).astype(np.float32)
    cluster = np.arange(N) % CLUSTERS
    x = centres[cluster] + np.float32(0.35) * rng.standard_normal((N, d)).astype(np.float32)
    x[COPIES] = x[99]
    return x, rng


def main_codes():
    codes = (np.arange(N) // 8).astype(np.int32)
    codes[np.arange(N) % CLUSTERS == 99 % CLUSTERS] = 512
    codes[100:110] = 512
    codes[N - 5:] = np.arange(513, 518)
    codes[[7, 1234, 3000]] = [518, 519, 520]
    return codes, 521


def few_codes():
    """One big group and 40 small ones: the fetch of every query is filled by group 0."""
    codes = np.zeros(N, np.int32)
    special = np.random.default_rng(3).permutation(np.setdiff1d(np.arange(N), COPIES))[:40]
    codes[special] = np.arange(1, 41)
    return codes, 41


_WORLDS = {}


class World:
    """One index per width, built once: queries, groupings, row sets and the full rankings (each computed once and never
    written to)."""

    def __init__(self, d):
        from minivectordb_amd import _native
        x, rng = make_corpus(d)
        self.d = d
        self.idx = _native.FlatIndex(d)
        self.idx.add(x, normalize=True)
        stored = self.idx.get_rows(0, N)
        rows = rng.permutation(np.setdiff1d(np.arange(N), np.flatnonzero(np.arange(N) % CLUSTERS == 99 % CLUSTERS).tolist() + COPIES))[:NQ_MAX]
        q = stored[rows] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((NQ_MAX, d)).astype(np.float32)
        q[0] = stored[99] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal(d).astype(np.float32)
        q[1] = stored[99]
        self.q = np.ascontiguousarray(q, dtype=np.float32)
        self.codes = {"main": main_codes(), "few": few_codes(), "own": (np.arange(N, dtype=np.int32), N),
                      "one": (np.zeros(N, np.int32), 1)}
        self.groupings = {}
        self.sets = {}
        self._full = {}

    def grouping(self, name):
        if name not in self.groupings:
            self.groupings[name] = self.idx.grouping(*self.codes[name])
        return self.groupings[name]

    def rowset(self, kind):
        """(RowSet or None, the selected rows in position order)."""
        if kind is None:
            return None, np.arange(N, dtype=np.int64)
        if kind not in self.sets:
            rng = np.random.default_rng(7)
            excluded = False
            if kind == "sorted":
                rows = np.arange(0, N, 3, dtype=np.int64)                       # holds 99, 102, 105, 108, 4092, 4095
            elif kind == "unsorted":
                rows = rng.permutation(N)[:1500].astype(np.int64)
                rows = np.concatenate([np.array(COPIES[::-1], np.int64), rows[~np.isin(rows, COPIES)]])   # the copies, highest row first
            elif kind == "dense":
                rows = np.setdiff1d(np.arange(N, dtype=np.int64), np.arange(5, N, 40))      # 97.5 % of the rows, sorted: a bitmap
            elif kind == "excluded":
                rows, excluded = np.array([99, 100, 7, 4095], np.int64), True
            elif kind == "twelve":
                rows = np.array([99, 5, 100, 4095, 17, 163, 227, 291, 1000, 2000, 3000, 35], np.int64)
            elif kind == "fewgroups":
                rows = np.concatenate([np.arange(8, 24), np.arange(808, 813)]).astype(np.int64)      # groups 1, 2 and (5 rows of) 101 of MAIN
            elif kind == "empty":
                rows = np.empty(0, np.int64)
            rs = self.idx.rowset(rows, excluded=excluded)
            selected = np.setdiff1d(np.arange(N, dtype=np.int64), rows) if excluded else rows
            self.sets[kind] = (rs, selected)
        return self.sets[kind]

    def full(self, i, kind=None):
        """The full ranking of the selected rows for query i alone: nq = 1, k = m on the default routing."""
        key = (i, kind)
        if key not in self._full:
            rs, selected = self.rowset(kind)
            m = len(selected)
            if kind is None:
                D, I = self.idx.search(self.q[i:i + 1], m, normalize_q=True)
            else:
                D, I = self.idx.search_rowset(self.q[i:i + 1], m, rs, normalize_q=True)
            D.setflags(write=False)
            I.setflags(write=False)
            self._full[key] = (D[0], I[0])
        return self._full[key]


def world(d):
    if d not in _WORLDS:
        _WORLDS[d] = World(d)
    return _WORLDS[d]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expect(w, queries, k, group_size, fetch_k, grouping, kind=None):
    """(D, I, G, model member_rows) of the call over the queries w.q[queries] by the contract."""
    codes = w.codes[grouping][0]
    rs, selected = w.rowset(kind)
    _, _, G = w.idx.search_distinct(w.q[queries], k, fetch_k, w.grouping(grouping), rowset=rs, normalize_q=True)
    D = np.empty((len(queries), k, group_size), np.float32)
    I = np.empty((len(queries), k, group_size), np.int64)
    for j, i in enumerate(queries):
        D[j], I[j] = members(*w.full(i, kind), codes, G[j], group_size)
    return D, I, G, member_rows(None if kind is None else selected, codes, G)


def run_and_check(w, nq, k, group_size, fetch_k, grouping="main", kind=None, what="", queries=None):
    """One call against the contract, the counters included.  Returns (D, I, G)."""
    queries = list(range(nq)) if queries is None else queries
    Dw, Iw, Gw, rows_w = expect(w, queries, k, group_size, fetch_k, grouping, kind)
    calls0, rows0 = w.idx.groups_counters()
    D, I, G = w.idx.search_groups(w.q[queries], k, group_size, fetch_k, w.grouping(grouping), rowset=w.rowset(kind)[0], normalize_q=True)
    calls1, rows1 = w.idx.groups_counters()
    tag = (what, w.d, queries if len(queries) < 4 else len(queries), k, group_size, fetch_k, grouping, kind)
    print(f"{tag}: member rows {rows1 - rows0} (model {rows_w}), groups found {(Gw >= 0).sum()}, members {(Iw >= 0).sum()}")
    assert D.shape == I.shape == (len(queries), k, group_size) and G.shape == (len(queries), k)
    assert np.array_equal(G, Gw), (tag, G, Gw)
    for j in range(len(queries)):
        assert np.array_equal(I[j], Iw[j]), (tag, j, I[j], Iw[j])
        assert np.array_equal(bits(D[j]), bits(Dw[j])), (tag, j)
    assert (D[I == -1] == MISSING).all() and (I[G == -1] == -1).all()
    assert calls1 - calls0 == 1 and rows1 - rows0 == rows_w, (tag, rows1 - rows0, rows_w)
    return D, I, G


# ---- the whole index ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", DIMS)
def test_members_are_the_first_of_the_full_ranking(gpu, d, nq):
    w = world(d)
    for k, group_size, fetch_k in SHAPES:
        D, I, G = run_and_check(w, nq, k, group_size, fetch_k, what="main")
        assert (G[:, 0] >= 0).all() and (I[:, 0, 0] >= 0).all()
        if group_size > 1 and k > 1:
            assert (I[:, :, 1] >= 0).any() and (np.diff(D.astype(np.float64), axis=2) <= 0).all()      # best first within a group
    run_and_check(w, nq, 5, 3, 32, grouping="few", what="few")            # one group fills the fetch: distinct's tier 2 picks G


@pytest.mark.parametrize("d", DIMS)
def test_group_size_one_alone_is_distinct_search(gpu, d):
    w = world(d)
    for i in (0, 1, 2):
        for k, fetch_k, grouping in ((1, 1, "main"), (5, 32, "main"), (10, 64, "main"), (64, 64, "main"), (5, 32, "few")):
            Dd, Id, Gd = w.idx.search_distinct(w.q[i:i + 1], k, fetch_k, w.grouping(grouping), normalize_q=True)
            D, I, G = run_and_check(w, 1, k, 1, fetch_k, grouping=grouping, what="gs=1", queries=[i])
            assert np.array_equal(I[:, :, 0], Id) and np.array_equal(bits(D[:, :, 0]), bits(Dd)) and np.array_equal(G, Gd), (d, i, k, fetch_k)
            # the heads of a wider call are the same rows
            D3, I3, _ = w.idx.search_groups(w.q[i:i + 1], k, 3, fetch_k, w.grouping(grouping), normalize_q=True)
            assert np.array_equal(I3[:, :, 0], Id) and np.array_equal(bits(D3[:, :, 0]), bits(Dd))


@pytest.mark.parametrize("d", DIMS)
def test_one_group_every_row_matches_and_ties_go_to_the_lower_row(gpu, d):
    w = world(d)
    # query 1 IS row 99: its 16 copies tie at the top, far-apart blocks hold them, and all 4096 rows are members
    D, I, G = run_and_check(w, 1, 1, 16, 32, grouping="one", what="one", queries=[1])
    assert I[0, 0].tolist() == COPIES and len(set(bits(D[0, 0]).tolist())) == 1 and G[0, 0] == 0
    D, I, G = run_and_check(w, 1, 5, 16, 32, grouping="one", what="one", queries=[1])
    assert I[0, 0].tolist() == COPIES and (I[0, 1:] == -1).all() and (G[0, 1:] == -1).all()
    for nq in (3, 33):
        run_and_check(w, nq, 5, 3, 32, grouping="one", what="one")
    # ties across groups and within one, MAIN: row 99 and the near copies are group 512, the far copies five groups
    D, I, G = run_and_check(w, 1, 10, 5, 64, what="ties", queries=[1])
    assert G[0, :6].tolist() == [512, 513, 514, 515, 516, 517] and I[0, 0].tolist() == [99, 100, 101, 102, 103]
    assert I[0, 1:6, 0].tolist() == list(range(N - 5, N)) and (I[0, 1:6, 1:] == -1).all()


@pytest.mark.parametrize("d", [100, 1024])
def test_every_row_its_own_group(gpu, d):
    w = world(d)
    for nq in (1, 33):
        D, I, G = run_and_check(w, nq, 10, 5, 64, grouping="own", what="own")
        assert np.array_equal(G, I[:, :, 0]) and (I[:, :, 1:] == -1).all()
        if nq == 1:
            Dp, Ip = w.idx.search(w.q[:1], 10, normalize_q=True)
            assert np.array_equal(I[:, :, 0], Ip) and np.array_equal(bits(D[:, :, 0]), bits(Dp))


# ---- row sets -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sorted", "unsorted", "dense", "excluded"])
@pytest.mark.parametrize("d", [30, 512])
def test_members_under_a_row_set(gpu, d, kind):
    w = world(d)
    rs, selected = w.rowset(kind)
    assert rs.is_bitmap == (kind in ("dense", "excluded"))
    for nq in NQS:
        for k, group_size, fetch_k in ((5, 3, 32), (10, 5, 64)):
            D, I, G = run_and_check(w, nq, k, group_size, fetch_k, kind=kind, what="set")
            assert np.isin(I[I >= 0], selected).all()
        run_and_check(w, nq, 5, 3, 32, grouping="few", kind=kind, what="set few")
    run_and_check(w, 2, 3, 16, 32, grouping="one", kind=kind, what="set one")
    if kind == "unsorted":       # exact ties go by LIST position: the copies were listed highest row first
        D, I, G = w.idx.search_groups(w.q[1:2], 10, 5, 64, w.grouping("main"), rowset=rs, normalize_q=True)
        assert G[0, :6].tolist() == [517, 516, 515, 514, 513, 512] and I[0, 5].tolist() == [109, 108, 107, 106, 105], (G[0], I[0, 5])
        D, I, G = w.idx.search_groups(w.q[1:2], 1, 16, 32, w.grouping("one"), rowset=rs, normalize_q=True)
        assert I[0, 0].tolist() == COPIES[::-1]
    if kind == "sorted":
        D, I, G = w.idx.search_groups(w.q[1:2], 1, 16, 32, w.grouping("one"), rowset=rs, normalize_q=True)
        assert I[0, 0, :6].tolist() == [99, 102, 105, 108, 4092, 4095]


@pytest.mark.parametrize("d", [30, 512])
def test_empty_set_short_groups_fewer_groups_and_a_set_the_fetch_covers(gpu, d):
    w = world(d)
    calls0, rows0 = w.idx.groups_counters()
    D, I, G = w.idx.search_groups(w.q[:3], 5, 3, 32, w.grouping("main"), rowset=w.rowset("empty")[0], normalize_q=True)
    assert (I == -1).all() and (D == MISSING).all() and (G == -1).all() and D.shape == (3, 5, 3)
    assert w.idx.groups_counters() == (calls0 + 1, rows0)
    # 21 rows in 3 groups of 8, 8 and 5: fewer groups than k, every group shorter than group_size; fetch_k = 8 is full of
    # fewer than k groups (distinct's tier 2), fetch_k = 32 covers the set (tier 1)
    for fetch_k in (8, 32):
        for nq in (1, 3):
            D, I, G = run_and_check(w, nq, 5, 16, fetch_k, kind="fewgroups", what="fewgroups")
            assert (G[:, 3:] == -1).all() and (I[:, 3:] == -1).all() and (D[:, 3:] == MISSING).all()
            assert sorted(G[0, :3].tolist()) == [1, 2, 101]
            sizes = {int(g): int((I[0, j] >= 0).sum()) for j, g in enumerate(G[0, :3])}
            assert sizes == {1: 8, 2: 8, 101: 5}
    # fetch_k >= m on a 12-row set
    for grouping in ("main", "one"):
        run_and_check(w, 3, 5, 3, 32, grouping=grouping, kind="twelve", what="twelve")
        run_and_check(w, 3, 5, 16, 12, grouping=grouping, kind="twelve", what="twelve")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 259, 1027])
def test_sizes_around_the_four_position_lanes_and_the_256_position_steps(gpu, n):
    """The member pass walks the positions four to a lane and 256 to a step, the up to three positions behind the last whole
    lane in a tail of their own: sizes below one lane, one lane exactly, and tails of 1 and 3 behind several steps, for every
    row, a bitmap and a row list."""
    from minivectordb_amd import _native
    d = 32
    rng = np.random.default_rng(50 + n)
    idx = _native.FlatIndex(d)
    idx.add(rng.standard_normal((n, d)).astype(np.float32), normalize=True)
    q = rng.standard_normal((2, d)).astype(np.float32)
    codes = (np.arange(n) % 2).astype(np.int32)
    grp = idx.grouping(codes, min(2, n))
    listed = rng.permutation(n)[:max(1, n - 1)].astype(np.int64)
    sets = [(None, None), (idx.rowset(listed), listed)]
    if n > 1:
        sets.append((idx.rowset(np.array([0], np.int64), excluded=True), np.arange(1, n, dtype=np.int64)))
        assert sets[-1][0].is_bitmap and not sets[1][0].is_bitmap
    for rs, selected in sets:
        m = n if rs is None else len(selected)
        k = min(2, m)
        _, _, Gw = idx.search_distinct(q, k, k, grp, rowset=rs, normalize_q=True)
        rows0 = idx.groups_counters()[1]
        D, I, G = idx.search_groups(q, k, 16, k, grp, rowset=rs, normalize_q=True)
        assert idx.groups_counters()[1] - rows0 == member_rows(selected, codes, Gw) == 2 * m      # both groups: every selected row
        assert np.array_equal(G, Gw)
        for i in range(2):
            Df, If = idx.search_rowset(q[i:i + 1], m, rs, normalize_q=True) if rs else idx.search(q[i:i + 1], m, normalize_q=True)
            Dw, Iw = members(Df[0], If[0], codes, Gw[i], 16)
            assert np.array_equal(I[i], Iw) and np.array_equal(bits(D[i]), bits(Dw)), (n, rs is not None, i, I[i], Iw)
    grp.free()
    idx.close()


# ---- the partials budget ------------------------------------------------------------------------------------------------------

def test_sub_tiles_give_identical_bits(gpu):
    from minivectordb_amd import _native
    w = world(384)
    nq, k, group_size, fetch_k = 33, 10, 5, 64
    base = w.idx.search_groups(w.q[:nq], k, group_size, fetch_k, w.grouping("main"), normalize_q=True)
    # the grid of the member pass: the exact-scan rule over 4096 rows of 96 chunks (8 rows per wave batch, 4 waves per block)
    # gives 128 blocks on any device with 64 CUs or more
    grid = 128
    _native.prof_enable(True)
    try:
        for slots in (1, 2):
            w.idx.set_option("groups_partials_bytes", slots * grid * k * group_size * 8)
            _native.prof_read("groups_scan")
            _native.prof_read("groups_select")
            got = run_and_check(w, nq, k, group_size, fetch_k, what=f"T={slots}")
            for a, b in zip(got, base):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
            launches = (nq + slots - 1) // slots
            assert _native.prof_read("groups_scan")[0] == launches and _native.prof_read("groups_select")[0] == launches, slots
            run_and_check(w, 3, 5, 3, 32, grouping="few", kind="unsorted", what=f"T={slots} few")
        w.idx.set_option("groups_partials_bytes", 1)                       # below one slot: T = 1 whatever the budget
        run_and_check(w, 3, 5, 3, 32, what="T=1 floor")
        with pytest.raises(ValueError):
            w.idx.set_option("groups_partials_bytes", 0)
        with pytest.raises(ValueError, match="groups_partials_bytes"):
            w.idx.set_option("no_such_option", 1)
    finally:
        _native.prof_enable(False)
        w.idx.set_option("groups_partials_bytes", DEFAULT_PARTIALS_BYTES)


# ---- non-finite rows ----------------------------------------------------------------------------------------------------------

def test_non_finite_rows(gpu):
    from minivectordb_amd import _native
    from tests import nonfinite_cases as nf
    n, d = nf.N_BIG, 64
    x = nf.corpus(n, d)
    q = nf.query_set(x)
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=False)
    nan_rows = [r for r, kind in nf.special_positions(n).items() if kind in ("nan", "nan_last")]      # NaN against every query
    fine = (np.arange(n) // 4).astype(np.int32)                  # NaN rows share groups with finite rows ...
    fine[nan_rows[0]] = fine.max() + 1                           # ... and one is a group of its own: all NaN
    coarse = (np.arange(n) % 3).astype(np.int32)
    listed_rows = nf.row_list(n)                                 # a permuted list that holds every special row
    listed = idx.rowset(listed_rows)
    assert not listed.is_bitmap
    for codes, k, group_size, fetch_k in ((fine, 8, 4, 32), (coarse, 3, 16, 16)):
        grp = idx.grouping(codes, int(codes.max()) + 1)
        for rs, selected in ((None, None), (listed, listed_rows)):
            m = n if rs is None else len(listed_rows)
            full = []
            for i in range(len(q)):
                Df, If = idx.search_rowset(q[i:i + 1], m, rs) if rs else idx.search(q[i:i + 1], m)
                full.append((Df[0], If[0]))
            for queries in [[i] for i in range(len(q))] + [list(range(len(q)))]:
                what = (len(codes), rs is not None, queries)
                _, _, Gw = idx.search_distinct(q[queries], k, fetch_k, grp, rowset=rs)
                rows0 = idx.groups_counters()[1]
                D, I, G = idx.search_groups(q[queries], k, group_size, fetch_k, grp, rowset=rs)
                assert idx.groups_counters()[1] - rows0 == member_rows(selected, codes, Gw), what     # NaN rows are counted
                assert np.array_equal(G, Gw), what
                for j, i in enumerate(queries):
                    Dw, Iw = members(*full[i], codes, Gw[j], group_size)
                    assert np.array_equal(I[j], Iw) and np.array_equal(bits(D[j]), bits(Dw)), (what, i, nf.QUERY_KINDS[i], I[j], Iw)
                    assert not np.isin(I[j], nan_rows).any(), (what, i)                              # a NaN row is never a member
                    if nf.QUERY_KINDS[i] == "nan":
                        assert (I[j] == -1).all() and (G[j] == -1).all()                             # every score is NaN
                assert not np.isnan(D).any()
        grp.free()
    # the all-zero query: every finite row ties at zero and goes by row number, the infinite rows score NaN
    one = idx.grouping(np.zeros(n, np.int32), 1)
    D, I, G = idx.search_groups(q[4:5], 1, 16, 1, one)
    Df, If = idx.search(q[4:5], n)
    assert np.array_equal(I[0, 0], If[0, :16]) and np.array_equal(bits(D[0, 0]), bits(Df[0, :16])) and (np.diff(I[0, 0]) > 0).all()
    one.free()
    idx.close()


# ---- mutations and argument errors --------------------------------------------------------------------------------------------

def _device_call(idx, q, k, group_size, fetch_k, grp, rowset=None, with_g=True, label_offset=0, stream=0):
    """search_groups_device on prefilled tensors: (error, D, I, G) as numpy, whatever the call did."""
    import torch
    nq = q.shape[0]
    qt = torch.from_numpy(q).cuda()
    Dt = torch.full((nq, max(k, 1), max(group_size, 1)), 7.0, dtype=torch.float32, device="cuda")
    It = torch.full((nq, max(k, 1), max(group_size, 1)), 77, dtype=torch.int64, device="cuda")
    Gt = torch.full((nq, max(k, 1)), 777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        idx.search_groups_device(qt.data_ptr(), nq, k, group_size, fetch_k, grp, Dt.data_ptr(), It.data_ptr(), Gt.data_ptr() if with_g else 0,
                                 rowset=rowset, stream=stream, normalize_q=True, label_offset=label_offset)
        err = None
    except ValueError as e:
        err = e
    torch.cuda.synchronize()
    return err, Dt.cpu().numpy(), It.cpu().numpy(), Gt.cpu().numpy()


def _untouched(res):
    err, D, I, G = res
    return isinstance(err, ValueError) and (D == 7.0).all() and (I == 77).all() and (G == 777).all()


def test_mutations(gpu):
    from minivectordb_amd import _native
    n, d = 600, 64
    x, rng = make_corpus(d)
    x = np.ascontiguousarray(x[:n])
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    codes = (np.arange(n) // 8).astype(np.int32)
    grp = idx.grouping(codes, 75)
    q = rng.standard_normal((2, d)).astype(np.float32)
    before = idx.search_groups(q, 5, 3, 32, grp, normalize_q=True)
    # set_rows renumbers nothing: the grouping stays valid and the answers follow the new rows
    idx.set_rows(np.array([333, 334], np.int64), np.stack([q[0], q[0] + 0.05 * q[1]]), normalize=True)
    rows0 = idx.groups_counters()[1]
    D, I, G = idx.search_groups(q, 5, 3, 32, grp, normalize_q=True)
    assert I[0, 0, :2].tolist() == [333, 334] and G[0, 0] == 333 // 8 and D[0, 0, 0] > 0.999 and before[1][0, 0, 0] != 333
    Df, If = idx.search(q[:1], n, normalize_q=True)
    Dw, Iw = members(Df[0], If[0], codes, G[0], 3)
    assert np.array_equal(I[0], Iw) and np.array_equal(bits(D[0]), bits(Dw))
    assert idx.groups_counters()[1] - rows0 == member_rows(None, codes, G)
    err, D, I, G = _device_call(idx, q, 5, 3, 32, grp)
    assert err is None and I[0, 0, 0] == 333 and G[0, 0] == 333 // 8
    # another index: refused, nothing written
    other = _native.FlatIndex(d)
    other.add(x, normalize=True)
    assert _untouched(_device_call(other, q, 5, 3, 32, grp))
    with pytest.raises(ValueError, match="another index"):
        other.search_groups(q, 5, 3, 32, grp, normalize_q=True)
    # a row set of another index too
    foreign = other.rowset(np.arange(0, n, 2, dtype=np.int64))
    assert _untouched(_device_call(idx, q, 5, 3, 32, grp, rowset=foreign))
    # rows added: the row count differs
    stale_set = idx.rowset(np.arange(0, n, 2, dtype=np.int64))
    idx.add(x[:3], normalize=True)
    assert _untouched(_device_call(idx, q, 5, 3, 32, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_groups(q, 5, 3, 32, grp, normalize_q=True)
    # ... removed again: the count is back, the rows were renumbered
    idx.remove_rows(np.array([1, 2, 3], np.int64))
    assert idx.ntotal == n
    assert _untouched(_device_call(idx, q, 5, 3, 32, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_groups(q, 5, 3, 32, grp, normalize_q=True)
    again = idx.grouping(codes, 75)                                    # re-created: one upload
    assert _untouched(_device_call(idx, q, 5, 3, 32, again, rowset=stale_set))       # the set is stale, the grouping is not
    assert (idx.search_groups(q, 5, 3, 32, again, normalize_q=True)[1][:, :, 0] >= 0).all()
    for o in (grp, again):
        o.free()
    idx.close()
    other.close()


def test_argument_errors(gpu):
    from minivectordb_amd import _native
    w = world(100)
    grp = w.grouping("main")
    calls0 = w.idx.groups_counters()[0]
    for k, group_size, fetch_k in ((65, 3, 128), (6, 3, 5), (5, 3, 1025), (0, 3, 5), (5, 0, 32), (5, 17, 32), (5, -1, 32)):
        with pytest.raises(ValueError):
            w.idx.search_groups(w.q[:2], k, group_size, fetch_k, grp, normalize_q=True)
        if k > 0 and group_size > 0:
            assert _untouched(_device_call(w.idx, w.q[:2], k, group_size, fetch_k, grp))
    with pytest.raises(ValueError, match="group_size"):
        w.idx.search_groups(w.q[:2], 5, 17, 32, grp)
    with pytest.raises(ValueError):
        w.idx.search_groups(w.q[:2, :50], 5, 3, 32, grp)
    assert w.idx.groups_counters()[0] == calls0                        # a refused call is no call
    l2 = _native.FlatIndex(100, metric=_native.METRIC_L2)
    l2.add(w.idx.get_rows(0, 64))
    g2 = l2.grouping(np.zeros(64, np.int32), 1)
    with pytest.raises(ValueError, match="inner-product"):
        l2.search_groups(w.q[:1], 1, 1, 1, g2)
    g2.free()
    l2.close()
    empty = _native.FlatIndex(100)
    g0 = empty.grouping(np.empty(0, np.int32), 0)
    D, I, G = empty.search_groups(w.q[:2], 3, 4, 8, g0)
    assert (I == -1).all() and (D == MISSING).all() and (G == -1).all() and I.shape == (2, 3, 4)
    assert empty.groups_counters() == (1, 0)
    g0.free()
    empty.close()


# ---- the device variant -------------------------------------------------------------------------------------------------------

def test_device_variant_label_offset_graph_and_repeat(gpu):
    import torch
    d, nq, off = 384, 3, 10 ** 6
    w = world(d)
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(w.q[:nq]).cuda()
    for k, group_size, fetch_k, codes, kind in ((10, 5, 64, "main", None), (5, 3, 32, "few", "unsorted"), (5, 16, 32, "one", "dense")):
        rs = w.rowset(kind)[0]
        grp = w.grouping(codes)
        Dw, Iw, Gw, rows_w = expect(w, list(range(nq)), k, group_size, fetch_k, codes, kind)
        Dt = torch.zeros((nq, k, group_size), dtype=torch.float32, device="cuda")
        It = torch.zeros((nq, k, group_size), dtype=torch.int64, device="cuda")
        Gt = torch.zeros((nq, k), dtype=torch.int32, device="cuda")

        def enqueue(offset, with_g=True):
            w.idx.search_groups_device(qt.data_ptr(), nq, k, group_size, fetch_k, grp, Dt.data_ptr(), It.data_ptr(),
                                       Gt.data_ptr() if with_g else 0, rowset=rs, stream=stream.cuda_stream, normalize_q=True,
                                       label_offset=offset)

        def check(offset, what, with_g=True):
            assert np.array_equal(bits(Dt.cpu().numpy()), bits(Dw)), what
            assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + offset, -1)), what
            assert np.array_equal(Gt.cpu().numpy(), Gw if with_g else np.full_like(Gw, 9)), what

        torch.cuda.synchronize()
        for offset in (0, off, off):                      # the label offset shifts labels only; two calls in a row: the same bits
            rows0 = w.idx.groups_counters()[1]
            with torch.cuda.stream(stream):
                enqueue(offset)
            stream.synchronize()
            check(offset, f"eager {kind} offset={offset}")
            assert w.idx.groups_counters()[1] - rows0 == rows_w
        Gt.fill_(9)                                       # G NULL: D and I as before, G not written
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue(off, with_g=False)
        stream.synchronize()
        check(off, f"no G {kind}", with_g=False)
        rows0 = w.idx.groups_counters()[1]
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue(off)
        for r in range(2):
            Dt.zero_()
            It.zero_()
            Gt.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            check(off, f"replay {r} {kind}")
        assert w.idx.groups_counters()[1] - rows0 == 2 * rows_w            # the replays count, the capture does not


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_find_most_similar_groups_returns_documents_with_their_chunks(gpu, tmp_path, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    docs, chunks, d = 60, 8, 128
    n = docs * chunks
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "m.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=128)
    rng = np.random.default_rng(71)
    centres = rng.standard_normal((docs, d)).astype(np.float32)
    x = centres[np.arange(n) // chunks] + np.float32(0.2) * rng.standard_normal((n, d)).astype(np.float32)
    meta = [{"doc": f"doc{r // chunks}", "chunk": r % chunks, "parity": r % 2} for r in range(n)]
    db.store_embeddings_batch(list(range(n)), x, meta)
    q = (centres[[3, 17]] + np.float32(0.1) * rng.standard_normal((2, d))).astype(np.float32)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    for i in range(2):
        for f, rows in (({}, np.arange(n)), ({"metadata_filter": {"parity": 1}}, np.arange(1, n, 2))):
            got = db.find_most_similar_groups(q[i], "doc", k=5, group_size=3, **f)
            heads = db.find_most_similar_distinct(q[i], "doc", k=5, **f)
            assert len(got) == 5 and [g[0][0] for g in got] == list(heads[0]) and [g[1][0] for g in got] == list(heads[1])
            # the three best chunks of each of the five best documents (float64 margins between chunks are far above fp32 rounding)
            s = xn[rows].astype(np.float64) @ (q[i] / np.linalg.norm(q[i])).astype(np.float64)
            by_doc = {}
            for r, v in zip(rows, s):
                by_doc.setdefault(r // chunks, []).append((v, int(r)))
            ranked = sorted((sorted(v, reverse=True) for v in by_doc.values()), reverse=True)[:5]
            for (ids, dist, metas), want in zip(got, ranked):
                assert list(ids) == [r for _, r in want[:3]], (i, f, ids, want[:3])
                assert isinstance(ids, tuple) and all(type(v) is np.float32 for v in dist) and list(dist) == sorted(dist, reverse=True)
                assert [m["chunk"] + chunks * int(m["doc"][3:]) for m in metas] == list(ids) and len({m["doc"] for m in metas}) == 1
    many = db.find_most_similar_groups_batch(q, "doc", k=5, group_size=3)
    assert [[g[0] for g in one] for one in many] == [[g[0] for g in db.find_most_similar_groups(q[i], "doc", k=5, group_size=3)] for i in range(2)]
    # one document of 320 chunks fills the default fetch of 32: distinct's tier 2 picks the groups; a short group follows
    big = [{"doc": "big" if r < 320 else f"doc{r // chunks}"} for r in range(n)]
    db.update_embeddings_batch(list(range(n)), metadata_dicts=big)
    xb = x.copy()
    xb[:320] = centres[0] + np.float32(0.2) * rng.standard_normal((320, d)).astype(np.float32)
    db.update_embeddings_batch(list(range(320)), embeddings=xb[:320])
    rows0 = db.index.groups_counters()[1]
    got = db.find_most_similar_groups(centres[0], "doc", k=5, group_size=16)
    assert len(got) == 5 and got[0][2][0]["doc"] == "big" and len(got[0][0]) == 16 and all(u < 320 for u in got[0][0])
    assert all(len(g[0]) == 8 and all(u >= 320 for u in g[0]) for g in got[1:])
    assert db.index.groups_counters()[1] - rows0 == 320 + 4 * 8
    db.update_embeddings_batch([n - 1], metadata_dicts=[{"doc": "lone"}])
    got = db.find_most_similar_groups(x[n - 1], "doc", k=2, group_size=4)
    assert got[0][0] == (n - 1,) and len(got[1][0]) == 4
