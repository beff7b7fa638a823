"""MaxSim search on the device (mvdb_index_search_maxsim, csrc/maxsim_scan.hpp): every comparison is exact.  The oracle's input
is the library's own single-query bits — for each query vector t the full ranking of the selected rows, idx.search /
search_rowset of q[t] alone with k = m, scattered into a [T, n] matrix (a row the ranking leaves out scored NaN) — and
tests/maxsim_oracle.py is the contract in numpy.  D, D_tok are compared as bits, G and I_tok as integers.

Corpus: tests/test_distinct_gpu.py's recipe at N = 2,051 rows (no multiple of any block step, several blocks at every shape):
64 Gaussian cluster centres + 0.35 noise, normalised on add; rows 100-109 and the last 5 are copies of row 99.  The question:
33 vectors, perturbed stored rows; vector 0 sits near row 99, vector 1 IS row 99.

Codes (MAIN): row // 8 (257 groups); the whole cluster of row 99 with its copies at rows 100-109 is ONE group (257); the last
5 rows — copies of row 99 too — sit in five groups of their own (258-262: equal sums across groups, which go to the lower
code); codes 263-269 are carried by no row.

A sorted list becomes a bitmap only from 4,096 stored rows on, so the dense-bitmap form is tested on an index of 4,099 rows
built by the same recipe (the excluded form, a bitmap at any size, on the 2,051).

Vectors per pass: Tp = min(T, 32, 128 KiB / (4 ld)) (include/mvdb.h), lowered by the index option maxsim_tokens_per_pass."""
import numpy as np
import pytest

from distinct_oracle import collapse
from maxsim_oracle import MISSING, maxsim

pytestmark = pytest.mark.gpu

N, CLUSTERS, T_MAX = 2051, 64, 33
DIMS = [30, 100, 384, 512, 1024]
TS = [1, 2, 7, 32, 33]
DEFAULT_TABLE_BYTES = 2 << 30


def tokens_per_pass(T, d, knob=0):
    ld = (d + 3) // 4 * 4
    tp = min(T, 32, max(1, (128 << 10) // (4 * ld)))
    return min(tp, knob) if knob else tp


def copies(n):
    return list(range(99, 110)) + list(range(n - 5, n))


def make_corpus(d, n=N, with_copies=True):
    rng = np.random.default_rng(2000 + d)
    centres = rng.standard_normal((CLUSTERS, d)).astype(np.float32)
    x = centres[np.arange(n) % CLUSTERS] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32)
    if with_copies:
        x[copies(n)] = x[99]
    return x, rng


def main_codes(n=N):
    big = (n + 7) // 8                                   # 257 at n = 2,051
    codes = (np.arange(n) // 8).astype(np.int32)
    codes[np.arange(n) % CLUSTERS == 99 % CLUSTERS] = big
    codes[100:110] = big
    codes[n - 5:] = np.arange(big + 1, big + 6)
    return codes, big + 13


_WORLDS = {}


class World:
    """One index per width, built once: the question, groupings, row sets and the single-query score matrices (each computed
    once and never written to)."""

    def __init__(self, d, n=N):
        from minivectordb_amd import _native
        x, rng = make_corpus(d, n)
        self.d, self.n = d, n
        N, COPIES = n, copies(n)
        self.idx = _native.FlatIndex(d)
        self.idx.add(x, normalize=True)
        stored = self.idx.get_rows(0, N)
        away = np.setdiff1d(np.arange(N), np.flatnonzero(np.arange(N) % CLUSTERS == 99 % CLUSTERS).tolist() + COPIES)
        rows = rng.permutation(away)[:T_MAX]
        q = stored[rows] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((T_MAX, d)).astype(np.float32)
        q[0] = stored[99] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal(d).astype(np.float32)
        q[1] = stored[99]
        self.q = np.ascontiguousarray(q, dtype=np.float32)
        self.codes = {"main": main_codes(n), "own": (np.arange(n, dtype=np.int32), n), "one": (np.zeros(n, np.int32), 1)}
        self.groupings = {}
        self.sets = {}
        self._scores = {}

    def grouping(self, name):
        if name not in self.groupings:
            self.groupings[name] = self.idx.grouping(*self.codes[name])
        return self.groupings[name]

    def rowset(self, kind):
        """(resident row set or None, the selected rows in position order)."""
        N, COPIES = self.n, copies(self.n)
        if kind is None:
            return None, np.arange(N, dtype=np.int64)
        if kind not in self.sets:
            rng = np.random.default_rng(7)
            excluded = False
            if kind == "unsorted":
                rows = rng.permutation(N)[:900].astype(np.int64)
                rows = np.concatenate([np.array(COPIES[::-1], np.int64), rows[~np.isin(rows, COPIES)]])   # the copies, highest row first
            elif kind == "dense":
                rows = np.setdiff1d(np.arange(N, dtype=np.int64), np.arange(5, N, 40))      # 97.5 % of the rows, sorted: a bitmap
            elif kind == "excluded":
                rows, excluded = np.array([99, 100, 7, N - 1], np.int64), True
            elif kind == "fewgroups":
                rows = np.concatenate([np.arange(8, 24), np.arange(808, 816)]).astype(np.int64)      # groups 1, 2 and 101 of MAIN
            elif kind == "empty":
                rows = np.empty(0, np.int64)
            rs = self.idx.rowset(rows, excluded=excluded)
            selected = np.setdiff1d(np.arange(N, dtype=np.int64), rows) if excluded else rows
            self.sets[kind] = (rs, selected)
        return self.sets[kind]

    def scores(self, kind=None):
        """[T_MAX, N] float32: row t is the single-query scan's full ranking of q[t] alone over the selected rows (nq = 1,
        k = m), scattered by row number; NaN where the ranking holds no entry for the row."""
        if kind not in self._scores:
            rs, selected = self.rowset(kind)
            m = len(selected)
            s = np.full((T_MAX, self.n), np.nan, np.float32)
            for t in range(T_MAX if m else 0):
                if rs is None:
                    D, I = self.idx.search(self.q[t:t + 1], m, normalize_q=True)
                else:
                    D, I = self.idx.search_rowset(self.q[t:t + 1], m, rs, normalize_q=True)
                assert (I[0] >= 0).all() and len(set(I[0].tolist())) == m
                s[t, I[0]] = D[0]
            s.setflags(write=False)
            self._scores[kind] = s
        return self._scores[kind]


N_DENSE = 4099   # a sorted list becomes a bitmap from 4,096 stored rows on: the dense form has an index of its own


def world(d, n=N):
    if (d, n) not in _WORLDS:
        _WORLDS[d, n] = World(d, n)
    return _WORLDS[d, n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    for g, w, name in zip(got, want, ("D", "G", "I_tok", "D_tok")):
        if w.dtype == np.float32:
            assert np.array_equal(bits(g), bits(w)), (what, name, g, w)
        else:
            assert np.array_equal(g, w) and g.dtype == w.dtype, (what, name, g, w)


def run_and_check(w, T, k, grouping="main", kind=None, knob=0, what=""):
    """One call against the contract, the counters included.  Returns what the call returned."""
    rs, selected = w.rowset(kind)
    want = maxsim(w.scores(kind)[:T], w.codes[grouping][0], selected, k)
    calls0, passes0 = w.idx.maxsim_counters()
    got = w.idx.search_maxsim(w.q[:T], k, w.grouping(grouping), rowset=rs, normalize_q=True)
    calls1, passes1 = w.idx.maxsim_counters()
    tp = tokens_per_pass(T, w.d, knob)
    expected = -(-T // tp) if len(selected) else 0
    print(f"{what} d={w.d} T={T} k={k} codes={grouping} set={kind} knob={knob}: passes {passes1 - passes0} (expected {expected})")
    same(got, want, (what, w.d, T, k, grouping, kind, knob))
    assert calls1 - calls0 == 1 and passes1 - passes0 == expected, (what, passes1 - passes0, expected)
    return got


# ---- widths and vector counts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("d", DIMS)
def test_every_width_and_vector_count(gpu, d, T):
    w = world(d)
    D, G, I_tok, D_tok = run_and_check(w, T, 10, what="widths")
    assert (G >= 0).all() and len(set(G.tolist())) == 10
    assert T > 2 or G[0] == 257                                                    # vectors 0 and 1 sit on the big group
    codes = w.codes["main"][0]
    assert (codes[I_tok] == G[:, None]).all()                                      # every answering row is a row of its group
    run_and_check(w, T, 64, what="widths k=64")
    D1, G1, _, _ = run_and_check(w, T, 1, what="widths k=1")
    assert G1[0] == G[0] and bits(D1)[0] == bits(D)[0]


def test_sixteen_masked_chunks(gpu):
    w = world(2304)
    assert tokens_per_pass(33, 2304) == 14
    for T in (2, 33):                                                              # 33 vectors: three passes of 14, 14 and 5
        run_and_check(w, T, 10, what="2304")
    run_and_check(w, 7, 5, kind="unsorted", what="2304 list")


@pytest.mark.parametrize("d", [100, 512])
def test_results_do_not_depend_on_the_vectors_per_pass(gpu, d):
    w = world(d)
    try:
        results = []
        for knob in (0, 1, 3):
            w.idx.set_option("maxsim_tokens_per_pass", knob)
            results.append(run_and_check(w, 7, 10, knob=knob, what="knob"))         # 1, 7 and 3 passes (asserted inside)
            run_and_check(w, 7, 10, kind="unsorted", knob=knob, what="knob list")
        for other in results[1:]:
            same(other, results[0], ("knob", d))
    finally:
        w.idx.set_option("maxsim_tokens_per_pass", 0)
    with pytest.raises(ValueError, match="maxsim_tokens_per_pass"):
        w.idx.set_option("maxsim_tokens_per_pass", 33)


# ---- groupings ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [30, 512])
def test_groupings(gpu, d):
    w = world(d)
    # MAIN, a question on row 99: the big group leads, the five far copies follow with EQUAL sums, in code order
    for T in (1, 2):
        want = maxsim(w.scores()[:T], w.codes["main"][0], np.arange(N), 10)
        assert want[1][:6].tolist() == [257, 258, 259, 260, 261, 262] and len(set(bits(want[0][1:6]).tolist())) == 1    # the tie occurs
        D, G, I_tok, D_tok = run_and_check(w, T, 10, what="ties")
        assert I_tok[1:6, 0].tolist() == list(range(N - 5, N))
        assert I_tok[0, T - 1] == 99                                               # vector T-1 ties on eleven rows of the big group: the lowest
    for T in (2, 7):
        # all rows in one group: one result and padding
        D, G, I_tok, D_tok = run_and_check(w, T, 5, grouping="one", what="one")
        assert G.tolist() == [0, -1, -1, -1, -1] and (D[1:] == MISSING).all() and (I_tok[1:] == -1).all() and (D_tok[1:] == MISSING).all()
        assert I_tok[0, 1] == 99
        # every row its own group: one row answers every vector
        D, G, I_tok, D_tok = run_and_check(w, T, 10, grouping="own", what="own")
        assert (I_tok == G[:, None]).all()
    # codes no selected row carries (263-269 of MAIN everywhere; whole groups under a set) are never results
    D, G, _, _ = run_and_check(w, 7, 64, kind="unsorted", what="unused")
    selected = w.rowset("unsorted")[1]
    assert set(G[G >= 0].tolist()) <= set(w.codes["main"][0][selected].tolist())


# ---- row sets -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unsorted", "dense", "excluded"])
@pytest.mark.parametrize("d", [30, 512])
def test_row_sets(gpu, d, kind):
    w = world(d, N_DENSE if kind == "dense" else N)
    rs, selected = w.rowset(kind)
    assert rs.is_bitmap == (kind in ("dense", "excluded"))
    codes = w.codes["main"][0]
    for T in (2, 7, 33):
        D, G, I_tok, D_tok = run_and_check(w, T, 10, kind=kind, what="set")
        assert np.isin(I_tok, selected).all() and (codes[I_tok] == G[:, None]).all()
    run_and_check(w, 2, 5, grouping="one", kind=kind, what="set one")
    if kind == "unsorted":       # equal scores inside a group go by LIST position: the copies were listed highest row first
        D, G, I_tok, D_tok = run_and_check(w, 2, 10, kind=kind, what="set ties")
        assert G[:6].tolist() == [257, 258, 259, 260, 261, 262] and I_tok[0, 1] == 109 and I_tok[1:6, 1].tolist() == list(range(N - 5, N))


@pytest.mark.parametrize("d", [30, 512])
def test_empty_set_and_padding(gpu, d):
    w = world(d)
    D, G, I_tok, D_tok = run_and_check(w, 3, 5, kind="empty", what="empty")            # no pass is enqueued (asserted inside)
    assert (G == -1).all() and (D == MISSING).all() and (I_tok == -1).all() and (D_tok == MISSING).all()
    # 24 rows in 3 groups, k = 5: three results, two rows of padding
    D, G, I_tok, D_tok = run_and_check(w, 3, 5, kind="fewgroups", what="fewgroups")
    assert sorted(G[:3].tolist()) == [1, 2, 101] and (G[3:] == -1).all() and (I_tok[3:] == -1).all() and (D_tok[3:] == MISSING).all()
    D, G, I_tok, D_tok = w.idx.search_maxsim(w.q[:3], 5, w.grouping("main"), rowset=w.rowset("fewgroups")[0], normalize_q=True, with_tokens=False)
    assert I_tok is None and D_tok is None and sorted(G[:3].tolist()) == [1, 2, 101]


# ---- one vector: distinct search's tier 2 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 384])
def test_one_vector_is_the_collapse_of_the_full_ranking(gpu, d):
    w = world(d)
    codes = w.codes["main"][0]
    distinct = 0
    for t in range(T_MAX):
        Df, If = w.idx.search(w.q[t:t + 1], N, normalize_q=True)
        Dw, Iw, Gw = collapse(Df[0], If[0], codes, 10)
        if len(set(bits(Dw).tolist())) < 10:
            continue                                                               # equal scores: the collapse orders them by row, MaxSim by code
        distinct += 1
        D, G, I_tok, D_tok = w.idx.search_maxsim(w.q[t:t + 1], 10, w.grouping("main"), normalize_q=True)
        same((D, G, I_tok[:, 0], D_tok[:, 0]), (Dw, Gw, Iw, Dw), ("collapse", d, t))
    assert distinct >= 1


# ---- non-finite rows ----------------------------------------------------------------------------------------------------------

def test_non_finite_rows(gpu):
    from minivectordb_amd import _native
    n, d, col = 300, 64, 3
    x, rng = make_corpus(d, n, with_copies=False)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    x[:, col] = np.abs(x[:, col]) + np.float32(0.01)            # no zero meets the infinity: its products are +-inf, never NaN
    x[20, 5] = np.nan
    x[26, 5] = np.nan
    x[21, col] = np.inf
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=False)
    fine = (np.arange(n) // 4).astype(np.int32)                  # row 26 shares group 6 with finite rows, row 21 group 5
    fine[20] = 75                                                # ... row 20 is a group of its own: all NaN
    lone = fine.copy()
    lone[21] = 76                                                # the infinite row alone in a group
    q = (x[[25, 40, 60]] + 0.05 * rng.standard_normal((3, d))).astype(np.float32)
    q[:, col] = np.abs(q[:, col])
    mixed = q.copy()
    mixed[1, col] = -mixed[1, col]                               # vector 1 scores the infinite row -inf, the others +inf
    listed_rows = np.arange(10, 40, dtype=np.int64)
    listed = idx.rowset(listed_rows)

    def oracle(question, codes, rs, selected, k):
        s = np.full((len(question), n), np.nan, np.float32)
        for t in range(len(question)):
            D, I = idx.search_rowset(question[t], len(selected), rs) if rs else idx.search(question[t], len(selected))
            s[t, I[0][I[0] >= 0]] = D[0][I[0] >= 0]
        return s, maxsim(s, codes, selected, k)

    for rs, selected in ((None, np.arange(n)), (listed, listed_rows)):
        for codes, ng in ((fine, 76), (lone, 77)):
            grp = idx.grouping(codes, ng)
            # every vector scores row 21 +inf: its group leads with +inf
            s, want = oracle(q, codes, rs, selected, 6)
            assert np.isnan(s[:, [20, 26]]).all() and (s[:, 21] == np.inf).all()
            got = idx.search_maxsim(q, 6, grp, rowset=rs)
            same(got, want, ("+inf", ng, rs is not None))
            D, G, I_tok, D_tok = got
            assert G[0] == codes[21] and D[0] == np.inf and (I_tok[0] == 21).all()
            assert 20 not in I_tok and 26 not in I_tok and 75 not in G and not np.isnan(D).any() and not np.isnan(D_tok).any()
            everything = idx.search_maxsim(q, 64, grp, rowset=rs)
            assert 6 in everything[1] and 75 not in everything[1]      # the NaN row does not hurt its finite group; alone it never appears
            # +inf for two vectors, -inf for one: alone in its group the row sums to NaN and is dropped; among finite rows the
            # group takes the -inf vector from another row and still leads
            s, want = oracle(mixed, codes, rs, selected, 64)
            assert s[1, 21] == -np.inf and s[0, 21] == np.inf
            got = idx.search_maxsim(mixed, 64, grp, rowset=rs)
            same(got, want, ("mixed", ng, rs is not None))
            if ng == 77:
                assert 76 not in got[1] and 21 not in got[2] and not np.isnan(got[0]).any()
            else:
                assert got[1][0] == 5 and got[0][0] == np.inf and got[2][0].tolist()[1] != 21
            # one NaN vector: no group has an offer for it — all padding
            broken = q.copy()
            broken[2, 7] = np.nan
            for normalize in (False, True):
                D, G, I_tok, D_tok = idx.search_maxsim(broken, 4, grp, rowset=rs, normalize_q=normalize)
                assert (G == -1).all() and (D == MISSING).all() and (I_tok == -1).all() and (D_tok == MISSING).all()
            grp.free()
    idx.close()


# ---- mutations and argument errors --------------------------------------------------------------------------------------------

def _device_call(idx, q, k, grp, rowset=None, with_tokens=True, label_offset=0, stream=0, T=None):
    """search_maxsim_device on prefilled tensors: (error, D, G, I_tok, D_tok) as numpy, whatever the call did."""
    import torch
    T = q.shape[0] if T is None else T
    qt = torch.from_numpy(q).cuda()
    Dt = torch.full((max(k, 1),), 7.0, dtype=torch.float32, device="cuda")
    Gt = torch.full((max(k, 1),), 777, dtype=torch.int32, device="cuda")
    It = torch.full((max(k, 1), max(T, 1)), 77, dtype=torch.int64, device="cuda")
    St = torch.full((max(k, 1), max(T, 1)), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        idx.search_maxsim_device(qt.data_ptr(), T, k, grp, Dt.data_ptr(), Gt.data_ptr(), It.data_ptr() if with_tokens else 0,
                                 St.data_ptr() if with_tokens else 0, rowset=rowset, stream=stream, normalize_q=True, label_offset=label_offset)
        err = None
    except ValueError as e:
        err = e
    torch.cuda.synchronize()
    return err, Dt.cpu().numpy(), Gt.cpu().numpy(), It.cpu().numpy(), St.cpu().numpy()


def _untouched(res):
    err, D, G, I, S = res
    return isinstance(err, ValueError) and (D == 7.0).all() and (G == 777).all() and (I == 77).all() and (S == 7.5).all()


def test_mutations(gpu):
    from minivectordb_amd import _native
    n, d = 600, 64
    x, rng = make_corpus(d, n, with_copies=False)
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=True)
    codes = (np.arange(n) // 8).astype(np.int32)
    grp = idx.grouping(codes, 75)
    q = rng.standard_normal((3, d)).astype(np.float32)
    # set_rows renumbers nothing: the grouping stays valid and the search sees the new row
    idx.set_rows(np.array([333], np.int64), q[:1], normalize=True)
    D, G, I_tok, D_tok = idx.search_maxsim(q, 5, grp, normalize_q=True)
    top = np.flatnonzero(G == 333 // 8)
    assert len(top) == 1 and I_tok[top[0], 0] == 333 and D_tok[top[0], 0] > 0.999
    err, D, G, I_tok, D_tok = _device_call(idx, q[:1], 5, grp)
    assert err is None and G[0] == 333 // 8 and I_tok[0, 0] == 333
    # another index: refused, nothing written
    other = _native.FlatIndex(d)
    other.add(x, normalize=True)
    assert _untouched(_device_call(other, q, 5, grp))
    with pytest.raises(ValueError, match="another index"):
        other.search_maxsim(q, 5, grp, normalize_q=True)
    # rows added: the row count differs
    idx.add(x[:3], normalize=True)
    assert _untouched(_device_call(idx, q, 5, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_maxsim(q, 5, grp, normalize_q=True)
    # ... removed again: the count is back, the rows were renumbered
    idx.remove_rows(np.array([1, 2, 3], np.int64))
    assert idx.ntotal == n
    assert _untouched(_device_call(idx, q, 5, grp))
    with pytest.raises(ValueError, match="another state"):
        idx.search_maxsim(q, 5, grp, normalize_q=True)
    again = idx.grouping(codes, 75)                                    # re-created: one upload
    assert (idx.search_maxsim(q, 5, again, normalize_q=True)[1] >= 0).all()
    # a row set of another state is refused the same way
    stale = other.rowset(np.arange(10, dtype=np.int64))
    assert _untouched(_device_call(idx, q, 5, again, rowset=stale))
    for o in (grp, again):
        o.free()
    idx.close()
    other.close()


def test_argument_errors(gpu):
    from minivectordb_amd import _native
    w = world(100)
    grp = w.grouping("main")
    calls0 = w.idx.maxsim_counters()
    with pytest.raises(ValueError, match="k <= 64"):
        w.idx.search_maxsim(w.q[:2], 65, grp, normalize_q=True)
    with pytest.raises(ValueError):
        w.idx.search_maxsim(w.q[:2], 0, grp, normalize_q=True)
    with pytest.raises(ValueError, match="T <= 256"):
        w.idx.search_maxsim(np.tile(w.q, (8, 1))[:257], 5, grp, normalize_q=True)
    with pytest.raises(ValueError, match="T <= 256"):
        w.idx.search_maxsim(np.empty((0, 100), np.float32), 5, grp, normalize_q=True)
    with pytest.raises(ValueError):
        w.idx.search_maxsim(w.q[:2, :50], 5, grp)                                   # a wrong width
    with pytest.raises(ValueError):
        w.idx.search_maxsim(w.q[0], 5, grp)                                         # a 1-D question
    assert _untouched(_device_call(w.idx, w.q[:2], 65, grp))
    assert _untouched(_device_call(w.idx, w.q[:2], 5, grp, T=0))
    assert _untouched(_device_call(w.idx, np.tile(w.q, (8, 1))[:257], 5, grp))
    assert w.idx.maxsim_counters() == calls0                                        # nothing was served
    # T = 256 is served: eight passes
    big = np.tile(w.q, (8, 1))[:256]
    D, G, I_tok, D_tok = w.idx.search_maxsim(big, 3, grp, normalize_q=True)
    assert w.idx.maxsim_counters()[1] - calls0[1] == 8 and (G >= 0).all() and I_tok.shape == (3, 256)
    assert np.array_equal(I_tok[:, :T_MAX], I_tok[:, T_MAX:2 * T_MAX]) and np.array_equal(bits(D_tok[:, :T_MAX]), bits(D_tok[:, T_MAX:2 * T_MAX]))
    # the table of a call against its bound
    n_groups = w.codes["main"][1]
    w.idx.set_option("maxsim_table_bytes", 7 * n_groups * 8)
    try:
        run_and_check(w, 7, 5, what="table fits")
        with pytest.raises(ValueError, match=rf"{8 * n_groups * 8} bytes.*maxsim_table_bytes"):
            w.idx.search_maxsim(w.q[:8], 5, grp, normalize_q=True)
        assert _untouched(_device_call(w.idx, w.q[:8], 5, grp))
    finally:
        w.idx.set_option("maxsim_table_bytes", DEFAULT_TABLE_BYTES)
    run_and_check(w, 8, 5, what="table default")
    l2 = _native.FlatIndex(100, metric=_native.METRIC_L2)
    l2.add(w.idx.get_rows(0, 64))
    g2 = l2.grouping(np.zeros(64, np.int32), 1)
    with pytest.raises(ValueError, match="inner-product"):
        l2.search_maxsim(w.q[:2], 1, g2)
    g2.free()
    l2.close()
    empty = _native.FlatIndex(100)
    g0 = empty.grouping(np.empty(0, np.int32), 0)
    D, G, I_tok, D_tok = empty.search_maxsim(w.q[:2], 3, g0)
    assert (G == -1).all() and (D == MISSING).all() and (I_tok == -1).all() and (D_tok == MISSING).all()
    g0.free()
    empty.close()


# ---- the device variant -------------------------------------------------------------------------------------------------------

def test_device_variant_label_offset_graph_and_repeat(gpu):
    import torch
    d, off = 384, 10 ** 6
    w = world(d)
    stream = torch.cuda.Stream()
    for T, k, codes, kind in ((7, 10, "main", None), (33, 5, "main", "unsorted"), (2, 5, "one", "dense"), (7, 5, "main", "excluded")):
        w = world(d, N_DENSE if kind == "dense" else N)
        rs, selected = w.rowset(kind)
        assert kind not in ("dense", "excluded") or rs.is_bitmap
        grp = w.grouping(codes)
        Dw, Gw, Iw, Sw = maxsim(w.scores(kind)[:T], w.codes[codes][0], selected, k)
        qt = torch.from_numpy(w.q[:T]).cuda()
        Dt = torch.zeros((k,), dtype=torch.float32, device="cuda")
        Gt = torch.zeros((k,), dtype=torch.int32, device="cuda")
        It = torch.zeros((k, T), dtype=torch.int64, device="cuda")
        St = torch.zeros((k, T), dtype=torch.float32, device="cuda")

        def enqueue(offset, with_tokens=True):
            w.idx.search_maxsim_device(qt.data_ptr(), T, k, grp, Dt.data_ptr(), Gt.data_ptr(), It.data_ptr() if with_tokens else 0,
                                       St.data_ptr() if with_tokens else 0, rowset=rs, stream=stream.cuda_stream, normalize_q=True,
                                       label_offset=offset)

        def check(offset, what, with_tokens=True):
            assert np.array_equal(bits(Dt.cpu().numpy()), bits(Dw)) and np.array_equal(Gt.cpu().numpy(), Gw), what
            if with_tokens:
                assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + offset, -1)), what
                assert np.array_equal(bits(St.cpu().numpy()), bits(Sw)), what
            else:
                assert (It.cpu().numpy() == 9).all() and (St.cpu().numpy() == 9).all(), what

        torch.cuda.synchronize()
        for offset in (0, off, off):                      # the label offset shifts labels only; two calls in a row: the same bits
            with torch.cuda.stream(stream):
                enqueue(offset)
            stream.synchronize()
            check(offset, f"eager {kind} offset={offset}")
        It.fill_(9)                                       # I_tok / D_tok NULL: D and G as before, the others not written
        St.fill_(9)
        Dt.zero_()
        Gt.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enqueue(off, with_tokens=False)
        stream.synchronize()
        check(off, f"no tokens {kind}", with_tokens=False)
        passes0 = w.idx.maxsim_counters()[1]
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue(off)
        assert w.idx.maxsim_counters()[1] - passes0 == -(-T // tokens_per_pass(T, d))       # counted on the host, at the capture
        for r in range(2):
            Dt.zero_()
            Gt.zero_()
            It.zero_()
            St.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            check(off, f"replay {r} {kind}")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_find_most_similar_maxsim_returns_documents(gpu, tmp_path, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    docs, chunks, d, T = 60, 8, 128, 3
    n = docs * chunks
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "m.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=128)
    rng = np.random.default_rng(72)
    x = rng.standard_normal((n, d)).astype(np.float32)                            # the chunks of a document are unrelated vectors
    meta = [{"doc": f"doc{r // chunks}", "chunk": r % chunks, "parity": r % 2} for r in range(n)]
    db.store_embeddings_batch(list(range(n)), x, meta)
    # the three vectors of the question sit near chunks 1, 3 and 5 of document 17 — and, weaker, near one chunk each of
    # documents 3, 30 and 44: no single chunk answers the question, document 17 does
    near = [17 * chunks + 1, 17 * chunks + 3, 17 * chunks + 5]
    decoy = [3 * chunks + 1, 30 * chunks + 7, 44 * chunks + 3]
    q = (x[near] + np.float32(0.5) * x[decoy] + np.float32(0.1) * rng.standard_normal((T, d))).astype(np.float32)
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    for f, rows in (({}, np.arange(n)), ({"metadata_filter": {"parity": 1}}, np.arange(1, n, 2))):
        ids, scores, metas = db.find_most_similar_maxsim(q, "doc", k=5, **f)
        assert len(ids) == 5 and all(type(s) is np.float32 for s in scores)
        assert [float(s) for s in scores] == sorted((float(s) for s in scores), reverse=True)
        s = qn @ xn[rows].T                                                       # float64, [T, rows]
        best = {}
        for doc in sorted(set((rows // chunks).tolist())):
            members = np.flatnonzero(rows // chunks == doc)
            pick = [int(rows[members[int(np.argmax(s[t, members]))]]) for t in range(T)]
            best[doc] = (float(sum(s[t, np.flatnonzero(rows == r)[0]] for t, r in enumerate(pick))), pick)
        ranked = sorted(best.items(), key=lambda e: -e[1][0])
        gaps = [ranked[j][1][0] - ranked[j + 1][1][0] for j in range(5)]
        assert min(gaps) > 1e-4                                                   # margins far above fp32 rounding
        for j in range(5):
            doc, (total, pick) = ranked[j]
            assert list(ids[j]) == pick and isinstance(ids[j], tuple), (f, j, ids[j], pick)
            assert abs(float(scores[j]) - total) < 1e-5
            assert [m["doc"] for m in metas[j]] == [f"doc{doc}"] * T and [m["chunk"] + chunks * doc for m in metas[j]] == pick
        assert metas[0][0]["doc"] == "doc17" and list(ids[0]) == near             # (all three chunks are odd: the filter keeps them)
        assert list(db.find_most_similar_maxsim_batch([q, q[:1]], "doc", k=5, **f)[0][0]) == list(ids)
    calls, passes = db.index.maxsim_counters()
    assert calls == 6 and passes == 6
