"""Distinct search on the device (mvdb_index_search_distinct, csrc/distinct_select.hpp): every comparison is exact — both
tiers are defined by bits the plain search already returns (tests/distinct_oracle.py is the contract in numpy).

Corpus: tests/test_mmr_gpu.py's — 4096 rows, 64 Gaussian cluster centres + 0.35 noise (row i belongs to cluster i % 64),
normalised on add; rows 100-109 and the last 5 are copies of row 99.  Queries: perturbed stored rows; query 0 sits near row
99, query 1 IS row 99, the others are away from it.

Codes (MAIN): row // 8 in general (512 groups); the whole cluster of row 99 with its copies at rows 100-109 is ONE group
(512); the last 5 rows — copies of row 99 too — sit in five DIFFERENT groups (513-517: exact ties across groups, which go to
the lower row); rows 7, 1234 and 3000 are singletons (518-520).

Every test derives the tier each query must take from the candidates themselves (distinct_oracle.tier) and asserts the
fallback counter moved by exactly the number of tier-2 queries, so a wrong tier cannot pass unnoticed.

One statement of the issue cannot hold on the whole index as it words it: with the last five copies in five groups of their
own, the candidates of a query at row 99 always hold 6 groups, so at k = 5 such a query is tier 1 (g >= k) whatever fetch_k
is.  The four (k, fetch_k) cells are all run; g < k is asserted for k = 10, and k = 5 takes tier 2 (asserted) under the row
sets that leave the far copies out, under the ONE-group grouping and under the FEW grouping.
"""
import numpy as np
import pytest

from distinct_oracle import MISSING, collapse, tier

pytestmark = pytest.mark.gpu

N, CLUSTERS, NQ_MAX = 4096, 64, 33
COPIES = list(range(99, 110)) + list(range(N - 5, N))
DIMS = [30, 100, 384, 512, 1024]
TIER1_SHAPES = [(1, 1), (5, 32), (10, 64), (64, 64), (64, 1024)]     # (k, fetch_k)
TIER2_SHAPES = [(5, 32), (5, 64), (10, 32), (10, 64)]
NQS = [1, 3, 33]
AT_99 = (0, 1)                                                        # query 0 near row 99, query 1 on it
DEFAULT_TABLE_BYTES = 256 << 20


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
    """One index per width, built once: queries, groupings, row sets, the candidate searches and the full rankings (each
    computed once and never written to)."""

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
        self._cand = {}
        self._full = {}

    def grouping(self, name):
        if name not in self.groupings:
            self.groupings[name] = self.idx.grouping(*self.codes[name])
        return self.groupings[name]

    def rowset(self, kind):
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
            elif kind == "nofar":
                rows = np.arange(0, N - 5, dtype=np.int64)[np.arange(N - 5) % 5 != 3]     # a list without the far copies (99, 100, 101, 102 ... stay)
            elif kind == "dense":
                rows = np.setdiff1d(np.arange(N, dtype=np.int64), np.arange(5, N, 40))      # 97.5 % of the rows, sorted: a bitmap
            elif kind == "excluded":
                rows, excluded = np.array([99, 100, 7, 4095], np.int64), True
            elif kind == "twelve":
                rows = np.array([99, 5, 100, 4095, 17, 163, 227, 291, 1000, 2000, 3000, 35], np.int64)
            elif kind == "fewgroups":
                rows = np.concatenate([np.arange(8, 24), np.arange(808, 816)]).astype(np.int64)      # groups 1, 2 and 101 of MAIN
            elif kind == "empty":
                rows = np.empty(0, np.int64)
            rs = self.idx.rowset(rows, excluded=excluded)
            selected = np.setdiff1d(np.arange(N, dtype=np.int64), rows) if excluded else rows
            self.sets[kind] = (rs, selected)
        return self.sets[kind]

    def candidates(self, nq, fetch_k, kind=None):
        """The plain search of the same call: (D, I) [nq, fetch_k]."""
        key = (nq, fetch_k, kind)
        if key not in self._cand:
            if kind is None:
                D, I = self.idx.search(self.q[:nq], fetch_k, normalize_q=True)
            else:
                D, I = self.idx.search_rowset(self.q[:nq], fetch_k, self.rowset(kind)[0], normalize_q=True)
            D.setflags(write=False)
            I.setflags(write=False)
            self._cand[key] = (D, I)
        return self._cand[key]

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
            self._full[key] = (D[0], I[0])
        return self._full[key]


def world(d):
    if d not in _WORLDS:
        _WORLDS[d] = World(d)
    return _WORLDS[d]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expect(w, nq, k, fetch_k, grouping, kind=None):
    """Per query of the call: (tier, D, I, G) by the contract."""
    codes = w.codes[grouping][0]
    m = len(w.rowset(kind)[1])
    Dc, Ic = w.candidates(nq, fetch_k, kind)
    out = []
    for i in range(nq):
        t = tier(Ic[i], codes, k, m)
        ranking = (Dc[i], Ic[i]) if t == 1 else w.full(i, kind)
        out.append((t,) + collapse(ranking[0], ranking[1], codes, k))
    return out


def run_and_check(w, nq, k, fetch_k, grouping="main", kind=None, what=""):
    """One call against the contract, the fallback counter included.  Returns the tiers."""
    want = expect(w, nq, k, fetch_k, grouping, kind)
    calls0, fell0 = w.idx.distinct_counters()
    D, I, G = w.idx.search_distinct(w.q[:nq], k, fetch_k, w.grouping(grouping), rowset=w.rowset(kind)[0], normalize_q=True)
    calls1, fell1 = w.idx.distinct_counters()
    tiers = [t for t, _, _, _ in want]
    print(f"{what} d={w.d} nq={nq} k={k} fetch_k={fetch_k} codes={grouping} set={kind}: tier-2 queries {tiers.count(2)}, counter {fell1 - fell0}")
    for i, (t, Dw, Iw, Gw) in enumerate(want):
        tag = (what, w.d, nq, k, fetch_k, grouping, kind, i, t)
        assert np.array_equal(I[i], Iw), (tag, I[i], Iw)
        assert np.array_equal(bits(D[i]), bits(Dw)), tag
        assert np.array_equal(G[i], Gw), tag
    assert calls1 - calls0 == 1 and fell1 - fell0 == tiers.count(2), (what, tiers, fell1 - fell0)
    return tiers


# ---- tier 1 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", DIMS)
def test_tier1_is_the_collapse_of_the_plain_search(gpu, d, nq):
    w = world(d)
    codes = w.codes["main"][0]
    not_distinct = 0
    for k, fetch_k in TIER1_SHAPES:
        tiers = run_and_check(w, nq, k, fetch_k, what="tier1")
        Dc, Ic = w.candidates(nq, fetch_k)
        for i in range(nq):
            if i not in AT_99 and (k, fetch_k) != (64, 64):
                assert tiers[i] == 1, (d, nq, k, fetch_k, i)           # away from row 99: the fetch holds k groups
            top = codes[Ic[i, :k]]
            not_distinct += tiers[i] == 1 and len(set(top.tolist())) < k
    assert not_distinct >= 1                                           # some plain top-k repeats a group: the collapse had work to do


# ---- tier 2 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_tier2_is_the_collapse_of_the_full_ranking(gpu, d):
    w = world(d)
    codes = w.codes["main"][0]
    for k, fetch_k in TIER2_SHAPES:
        for nq in (1, 2, 3, 33):                                       # alone, the two aimed at row 99, and batches that mix both tiers
            tiers = run_and_check(w, nq, k, fetch_k, what="tier2")
            Ic = w.candidates(nq, fetch_k)[1]
            for i in AT_99[:nq]:
                g = len(set(codes[Ic[i]].tolist()))
                assert g == 6, (d, k, fetch_k, i, g)                   # the cluster's group and the five far copies
                assert tiers[i] == (2 if k == 10 else 1)
            assert all(t == 1 for t in tiers[2:])
    # k = 5: one group fills every fetch
    for nq in (1, 3):
        assert run_and_check(w, nq, 5, 32, grouping="few", what="tier2 few") == [2] * nq
    # ties across groups go to the lower row: the copies 99 and 4091 .. 4095 lead query 1 in row order
    D, I, G = w.idx.search_distinct(w.q[1:2], 10, 64, w.grouping("main"), normalize_q=True)
    assert I[0, :6].tolist() == [99] + list(range(N - 5, N)) and G[0, :6].tolist() == [512, 513, 514, 515, 516, 517]
    assert len(set(bits(D[0, :6]).tolist())) == 1


@pytest.mark.parametrize("slots", [2, 1])
def test_tier2_walks_the_table_in_sub_tiles(gpu, slots):
    w = world(384)
    n_groups = w.codes["main"][1]
    w.idx.set_option("distinct_table_bytes", slots * 8 * n_groups)
    try:
        for k, fetch_k in ((10, 64), (64, 64)):
            tiers = run_and_check(w, 33, k, fetch_k, what=f"T={slots}")
            assert tiers.count(2) >= 2
        assert 1 in run_and_check(w, 33, 10, 64, what=f"T={slots}")
        assert run_and_check(w, 3, 5, 32, grouping="few", what=f"T={slots} few") == [2, 2, 2]
    finally:
        w.idx.set_option("distinct_table_bytes", DEFAULT_TABLE_BYTES)


# ---- row sets -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sorted", "unsorted", "nofar", "dense", "excluded"])
@pytest.mark.parametrize("d", [30, 512])
def test_both_tiers_under_a_row_set(gpu, d, kind):
    w = world(d)
    rs, selected = w.rowset(kind)
    assert rs.is_bitmap == (kind in ("dense", "excluded"))
    seen = []
    for nq in (1, 3, 33):
        for k, fetch_k in ((5, 32), (10, 64)):
            seen += run_and_check(w, nq, k, fetch_k, kind=kind, what="set")
        seen += run_and_check(w, nq, 5, 32, grouping="few", kind=kind, what="set few")
    assert 1 in seen and 2 in seen
    if kind == "unsorted":       # exact ties go by LIST position: the copies were listed highest row first
        D, I, G = w.idx.search_distinct(w.q[:2], 10, 64, w.grouping("main"), rowset=rs, normalize_q=True)
        assert I[1, :6].tolist() == [4095, 4094, 4093, 4092, 4091, 109], I[1]
        assert expect(w, 2, 5, 32, "few", kind)[1][0] == 2                  # ... in tier 2 as well: the big group's best row
        D, I, G = w.idx.search_distinct(w.q[:2], 5, 32, w.grouping("few"), rowset=rs, normalize_q=True)
        assert I[1, 0] == 4095 and G[1, 0] == 0, I[1]
    if kind == "nofar":          # without the far copies the cluster's group is alone in the fetch: k = 5 takes tier 2 under MAIN
        assert run_and_check(w, 2, 5, 32, kind=kind, what="set nofar") == [2, 2]


@pytest.mark.parametrize("d", [30, 512])
def test_empty_set_few_groups_and_a_set_the_fetch_covers(gpu, d):
    w = world(d)
    fell0 = w.idx.distinct_counters()[1]
    D, I, G = w.idx.search_distinct(w.q[:3], 5, 32, w.grouping("main"), rowset=w.rowset("empty")[0], normalize_q=True)
    assert (I == -1).all() and (D == MISSING).all() and (G == -1).all()
    # 24 rows in 3 groups: fetch_k = 8 is full of fewer than k groups (tier 2), fetch_k = 32 covers the set (tier 1); both pad
    assert run_and_check(w, 3, 5, 8, kind="fewgroups", what="fewgroups") == [2, 2, 2]
    assert w.idx.distinct_counters()[1] == fell0 + 3
    assert run_and_check(w, 3, 5, 32, kind="fewgroups", what="fewgroups") == [1, 1, 1]
    D, I, G = w.idx.search_distinct(w.q[:3], 5, 8, w.grouping("main"), rowset=w.rowset("fewgroups")[0], normalize_q=True)
    assert (I[:, 3:] == -1).all() and (D[:, 3:] == MISSING).all() and (G[:, 3:] == -1).all() and (I[:, :3] >= 0).all()
    assert sorted(G[0, :3].tolist()) == [1, 2, 101]
    # fetch_k >= m on a 12-row set: tier 1 whatever the groups
    for grouping in ("main", "one"):
        assert run_and_check(w, 3, 5, 32, grouping=grouping, kind="twelve", what="twelve") == [1, 1, 1]
        assert run_and_check(w, 3, 5, 12, grouping=grouping, kind="twelve", what="twelve") == [1, 1, 1]


# ---- degenerate groupings -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 1024])
def test_degenerate_groupings(gpu, d):
    w = world(d)
    for nq in (1, 33):
        # every row its own group: the plain top-k, no tier 2
        assert set(run_and_check(w, nq, 10, 64, grouping="own", what="own")) == {1}
        D, I, G = w.idx.search_distinct(w.q[:nq], 10, 64, w.grouping("own"), normalize_q=True)
        Dp, Ip = w.idx.search(w.q[:nq], 64, normalize_q=True)
        assert np.array_equal(I, Ip[:, :10]) and np.array_equal(bits(D), bits(Dp[:, :10])) and np.array_equal(G, I)
        # all rows in one group: one result and padding, through tier 2
        assert set(run_and_check(w, nq, 5, 32, grouping="one", what="one")) == {2}
        D, I, G = w.idx.search_distinct(w.q[:nq], 5, 32, w.grouping("one"), normalize_q=True)
        assert (I[:, 0] >= 0).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == MISSING).all() and (G[:, 1:] == -1).all()
        assert (G[:, 0] == 0).all()


# ---- non-finite rows ----------------------------------------------------------------------------------------------------------

def test_non_finite_rows(gpu):
    from minivectordb_amd import _native
    n, d, col = 300, 64, 3
    x, rng = make_corpus(d)
    x = x[:n] / np.linalg.norm(x[:n], axis=1, keepdims=True)
    x[:, col] = np.abs(x[:, col]) + np.float32(0.01)            # no zero meets the infinity: its products are +-inf, never NaN
    x[20, 5] = np.nan
    x[26, 5] = np.nan
    x[21, col] = np.inf
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=False)
    fine = (np.arange(n) // 4).astype(np.int32)                  # row 26 shares group 6 with finite rows
    fine[20] = 75                                                # ... row 20 is a group of its own: all NaN
    coarse = (np.arange(n) % 3).astype(np.int32)
    coarse[20] = 3
    listed_rows = np.arange(10, 40, dtype=np.int64)
    listed = idx.rowset(listed_rows)
    seen = set()
    for sign in (-1.0, 1.0):                                     # the infinite row scores -inf (last) / +inf (first)
        q = (x[25] + 0.05 * rng.standard_normal(d)).astype(np.float32)
        q[col] = sign * abs(q[col])
        for codes, ng, k, fetch_k, want_tier in ((fine, 76, 5, 32, 1), (coarse, 4, 4, 16, 2)):
            grp = idx.grouping(codes, ng)
            for rs, m in ((None, n), (listed, len(listed_rows))):
                what = (sign, ng, rs is not None)
                fetch = min(fetch_k, 16) if rs is not None else fetch_k
                Dc, Ic = idx.search_rowset(q, fetch, rs) if rs else idx.search(q, fetch)
                t = tier(Ic[0], codes, k, m)
                assert t == want_tier or (rs is not None and want_tier == 1), what
                seen.add(t)
                Df, If = idx.search_rowset(q, m, rs) if rs else idx.search(q, m)
                Dw, Iw, Gw = collapse(Dc[0], Ic[0], codes, k) if t == 1 else collapse(Df[0], If[0], codes, k)
                fell0 = idx.distinct_counters()[1]
                D, I, G = idx.search_distinct(q, k, fetch, grp, rowset=rs)
                assert idx.distinct_counters()[1] - fell0 == (t == 2), what
                assert np.array_equal(I[0], Iw) and np.array_equal(bits(D[0]), bits(Dw)) and np.array_equal(G[0], Gw), (what, I, Iw)
                assert 20 not in I and 26 not in I and codes[20] not in G, what      # a NaN row is never a result, an all-NaN group never appears
                assert not np.isnan(D).any()
                if sign > 0:
                    assert I[0, 0] == 21 and D[0, 0] == np.inf, what                 # the +inf row leads
            grp.free()
    assert seen == {1, 2}
    idx.close()


# ---- mutations and argument errors --------------------------------------------------------------------------------------------

def _device_call(idx, q, k, fetch_k, grp, rowset=None, with_g=True, label_offset=0, stream=0):
    """search_distinct_device on prefilled tensors: (D, I, G) as numpy, whatever the call did."""
    import torch
    nq = q.shape[0]
    qt = torch.from_numpy(q).cuda()
    Dt = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    It = torch.full((nq, k), 77, dtype=torch.int64, device="cuda")
    Gt = torch.full((nq, k), 777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        idx.search_distinct_device(qt.data_ptr(), nq, k, fetch_k, grp, Dt.data_ptr(), It.data_ptr(), Gt.data_ptr() if with_g else 0,
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
    assert len(grp) == n and grp.n_groups == 75
    q = rng.standard_normal((2, d)).astype(np.float32)
    # set_rows renumbers nothing: the grouping stays valid and the search sees the new row, in both tiers
    idx.set_rows(np.array([333], np.int64), q[:1], normalize=True)
    for k, fetch_k, g in ((5, 32, grp), (5, 32, idx.grouping(np.zeros(n, np.int32), 1))):
        D, I, G = idx.search_distinct(q, k, fetch_k, g, normalize_q=True)
        assert I[0, 0] == 333 and D[0, 0] > 0.999, (I, D)
    assert idx.distinct_counters()[1] == 2
    err, D, I, G = _device_call(idx, q, 5, 32, grp)
    assert err is None and I[0, 0] == 333 and G[0, 0] == 333 // 8
    # another index: refused, nothing written
    other = _native.FlatIndex(d)
    other.add(x, normalize=True)
    assert _untouched(_device_call(other, q, 5, 32, grp))
    with pytest.raises(ValueError, match="another index"):
        other.search_distinct(q, 5, 32, grp, normalize_q=True)
    # rows added: the row count differs
    idx.add(x[:3], normalize=True)
    assert _untouched(_device_call(idx, q, 5, 32, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_distinct(q, 5, 32, grp, normalize_q=True)
    # ... removed again: the count is back, the rows were renumbered
    idx.remove_rows(np.array([1, 2, 3], np.int64))
    assert idx.ntotal == n
    assert _untouched(_device_call(idx, q, 5, 32, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_distinct(q, 5, 32, grp, normalize_q=True)
    again = idx.grouping(codes, 75)                                    # re-created: one upload
    assert (idx.search_distinct(q, 5, 32, again, normalize_q=True)[1] >= 0).all()
    for o in (grp, again):
        o.free()
    idx.close()
    other.close()


def test_argument_errors(gpu):
    from minivectordb_amd import _native
    w = world(100)
    codes, ng = w.codes["main"]
    for bad, groups in ((codes[:-1], ng), (np.append(codes, 0).astype(np.int32), ng), (codes, 520), (codes, 0), (codes, N + 1),
                        (np.where(np.arange(N) == 5, -1, codes).astype(np.int32), ng)):
        with pytest.raises(ValueError):
            w.idx.grouping(bad, groups)
    grp = w.grouping("main")
    for k, fetch_k in ((65, 128), (6, 5), (5, 1025), (0, 5)):
        with pytest.raises(ValueError):
            w.idx.search_distinct(w.q[:2], k, fetch_k, grp, normalize_q=True)
        if k > 0:
            assert _untouched(_device_call(w.idx, w.q[:2], k, fetch_k, grp))
    with pytest.raises(ValueError):
        w.idx.search_distinct(w.q[:2, :50], 5, 32, grp)
    l2 = _native.FlatIndex(100, metric=_native.METRIC_L2)
    l2.add(w.idx.get_rows(0, 64))
    g2 = l2.grouping(np.zeros(64, np.int32), 1)
    with pytest.raises(ValueError, match="inner-product"):
        l2.search_distinct(w.q[:1], 1, 1, g2)
    g2.free()
    l2.close()
    empty = _native.FlatIndex(100)
    g0 = empty.grouping(np.empty(0, np.int32), 0)
    assert len(g0) == 0
    D, I, G = empty.search_distinct(w.q[:2], 3, 8, g0)
    assert (I == -1).all() and (D == MISSING).all() and (G == -1).all()
    g0.free()
    empty.close()


# ---- the device variant -------------------------------------------------------------------------------------------------------

def test_device_variant_label_offset_graph_and_repeat(gpu):
    import torch
    d, nq, off = 384, 3, 10 ** 6
    w = world(d)
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(w.q[:nq]).cuda()
    for k, fetch_k, codes, kind in ((10, 64, "main", None), (5, 32, "few", "unsorted"), (5, 32, "main", "dense")):
        rs = w.rowset(kind)[0]
        grp = w.grouping(codes)
        want = expect(w, nq, k, fetch_k, codes, kind)
        assert 2 in [t for t, _, _, _ in want] or kind == "dense"            # (the whole-index and the list call take tier 2)
        Dw = np.stack([x[1] for x in want])
        Iw = np.stack([x[2] for x in want])
        Gw = np.stack([x[3] for x in want])
        Dt = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        It = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        Gt = torch.zeros((nq, k), dtype=torch.int32, device="cuda")

        def enqueue(offset, with_g=True):
            w.idx.search_distinct_device(qt.data_ptr(), nq, k, fetch_k, grp, Dt.data_ptr(), It.data_ptr(), Gt.data_ptr() if with_g else 0,
                                         rowset=rs, stream=stream.cuda_stream, normalize_q=True, label_offset=offset)

        def check(offset, what, with_g=True):
            assert np.array_equal(bits(Dt.cpu().numpy()), bits(Dw)), what
            assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + offset, -1)), what
            assert np.array_equal(Gt.cpu().numpy(), Gw if with_g else np.full_like(Gw, 9)), what

        torch.cuda.synchronize()
        for offset in (0, off, off):                      # the label offset shifts labels only; two calls in a row: the same bits
            with torch.cuda.stream(stream):
                enqueue(offset)
            stream.synchronize()
            check(offset, f"eager {kind} offset={offset}")
        Gt.fill_(9)                                       # G NULL: D and I as before, G not written
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue(off, with_g=False)
        stream.synchronize()
        check(off, f"no G {kind}", with_g=False)
        fell0 = w.idx.distinct_counters()[1]
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
        assert w.idx.distinct_counters()[1] - fell0 == 2 * [t for t, _, _, _ in want].count(2)      # the replays count too


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_find_most_similar_distinct_returns_k_documents(gpu, tmp_path, kind):
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
        plain = db.find_most_similar(q[i], k=5)
        assert len({m["doc"] for m in plain[2]}) == 1                                 # five chunks of one document
        for f, rows in (({}, np.arange(n)), ({"metadata_filter": {"parity": 1}}, np.arange(1, n, 2))):
            ids, dist, metas = db.find_most_similar_distinct(q[i], "doc", k=5, **f)
            assert len(ids) == 5 == len({m["doc"] for m in metas}) and list(dist) == sorted(dist, reverse=True)
            assert all(type(s) is np.float32 for s in dist) and [m["chunk"] + chunks * int(m["doc"][3:]) for m in metas] == list(ids)
            # the best chunk of each of the five best documents (float64 margins between chunks are far above fp32 rounding)
            s = xn[rows].astype(np.float64) @ (q[i] / np.linalg.norm(q[i])).astype(np.float64)
            best = {}
            for r, v in zip(rows, s):
                if v > best.get(r // chunks, (-2.0, -1))[0]:
                    best[r // chunks] = (v, int(r))
            want = [r for _, r in sorted(best.values(), reverse=True)[:5]]
            assert list(ids) == want, (i, f, ids, want)
    # one document of 320 chunks fills the default fetch of 32: tier 2 through the Python layer
    big = [{"doc": "big" if r < 320 else f"doc{r // chunks}"} for r in range(n)]
    db.update_embeddings_batch(list(range(n)), metadata_dicts=big)
    xb = x.copy()
    xb[:320] = centres[0] + np.float32(0.2) * rng.standard_normal((320, d)).astype(np.float32)
    db.update_embeddings_batch(list(range(320)), embeddings=xb[:320])
    fell0 = db.index.distinct_counters()[1]
    ids, dist, metas = db.find_most_similar_distinct(centres[0], "doc", k=5)
    assert db.index.distinct_counters()[1] == fell0 + 1
    assert metas[0]["doc"] == "big" and len({m["doc"] for m in metas}) == 5 and ids[0] < 320 and all(u >= 320 for u in ids[1:])
    assert list(db.find_most_similar_distinct_batch(centres[:1], "doc", k=5)[0][0]) == list(ids)
