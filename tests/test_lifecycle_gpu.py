"""Every search route against the model of tests/index_model.py across index mutations.

A scenario is a list of events (index_model.py names them) run on ONE index with the model beside it.  After every event
`check` compares the state (ntotal, the bytes of get_rows, shadow_rows as the table above ShadowStore in csrc/mvdb.hip
predicts it) and every route — exact scan, certified batch, range batch, range join, the four forms of resident row set on
every entry point that takes one, grouping, distinct, MaxSim, assign, one k-means step, MMR, grouped search — with the mirror,
and at the end of the scenario the whole index with a rebuild from the mirror.

Shapes: d = 128 (the narrowest width with a shadow kernel) and d = 30 (padded rows, no shadow); n between 3,900 and 4,450,
crossing 4,096 (from where a sorted row list becomes a bitmap or gains a bitmap twin) in both directions, never a multiple of
the 32-row tile; batches of 40 queries (33 is the least the certified pass and the shared range pass take).

The batch search that follows every event completes the shadow wherever one can exist, so an event can only meet an EMPTIED
shadow (or L2 offsets that lag BEHIND it) when no search ran since the event before: those cells of the table are reached
by ("pair", e1, e2) events, two mutations checked once.  After a reset the index is empty: only the state and the refusal of
stale handles are checked there.  The query that equals a row of norm ~40 is sent at unit length (the tolerances of
flat.adjudicate are absolute)."""
import ctypes
import time

import numpy as np
import pytest

from index_model import ROWSET_BITMAP_MIN_ROWS, IndexModel
from oracle import flat

pytestmark = pytest.mark.gpu

NQ, K, K_RANGE = 40, 10, 200
N_VECTORS = 33                        # the score matrix: C = 33 gives assign two passes
FORMS = ("unsorted", "sparse", "dense", "excluded")
N0 = 4203

_EVENTS_1 = [("add", 97), ("set", 37), ("copy",), ("del_one",), ("pair", ("del_scatter", 9), ("add", 51)), ("del_scatter", 45),
             ("pair", ("del_one",), ("set", 20)), ("del_suffix", 260), ("add", 130), ("reset",), ("add", 4131)]
_EVENTS_2 = _EVENTS_1[:2] + [("reserve", 300)] + _EVENTS_1[2:6] + [("reserve", 0)] + _EVENTS_1[6:]
_EVENTS_3 = [("add", 97), ("set", 37), ("big",), ("set", 11), ("del_big",), ("add", 60), ("copy",), ("del_scatter", 45),
             ("del_suffix", 247), ("add", 90)]
_EVENTS_4 = [("add", 97), ("set", 37), ("pair", ("add", 40), ("set", 30)), ("pair", ("add", 23), ("add", 19)),
             ("pair", ("del_scatter", 45), ("add", 60)), ("pair", ("add", 30), ("del_one",)), ("copy",), ("del_scatter", 21),
             ("del_suffix", 350), ("add", 140)]


def random_events(seed, count=12):
    """`count` events drawn from the same kinds, n kept inside [3,900, 4,400] and off the multiples of 32."""
    rng = np.random.default_rng(seed)
    n, events, big = N0, [], False
    while len(events) < count:
        kind = str(rng.choice(["add", "set", "copy", "big", "del_big", "del_one", "del_scatter", "del_suffix", "reserve", "pair"]))
        m = int(rng.integers(5, 120))
        if kind in ("add", "del_scatter", "del_suffix"):
            after = n + m if kind == "add" else n - m
            if not 3900 <= after <= 4400:
                continue
            if after % 32 == 0:
                m, after = m + 1, after + (1 if kind == "add" else -1)
            events.append((kind, m))
            n = after
        elif kind == "set":
            events.append(("set", m))
        elif kind in ("copy", "big"):
            big |= kind == "big"
            events.append((kind,))
        elif kind in ("del_one", "del_big"):
            if (kind == "del_big" and not big) or (n - 1) % 32 == 0:
                continue
            big &= kind != "del_big"
            events.append((kind,))
            n -= 1
        elif kind == "reserve":
            events.append(("reserve", int(rng.choice([0, 150]))))
        elif (n - 1 + m) % 32 and n - 1 + m <= 4400:
            events.append(("pair", ("del_one",), ("add", m)) if rng.random() < 0.5 else ("pair", ("add", m), ("del_one",)))
            n += m - 1
    return events


# name -> d, metric, norms, reserve (0: none), seed of the model, events
SCENARIOS = {
    "unit_reserved": dict(d=128, metric=flat.METRIC_IP, norms="unit", reserve=4500, seed=1, events=_EVENTS_1),
    "unit_growing": dict(d=128, metric=flat.METRIC_IP, norms="unit", reserve=0, seed=2, events=_EVENTS_2),
    "mixed_norms": dict(d=128, metric=flat.METRIC_IP, norms="mixed", reserve=4500, seed=3, events=_EVENTS_3),
    "l2_offsets": dict(d=128, metric=flat.METRIC_L2, norms="mixed", reserve=4600, seed=4, events=_EVENTS_4),
    "padded_d30": dict(d=30, metric=flat.METRIC_IP, norms="unit", reserve=4500, seed=5, events=_EVENTS_1),
    "random_18": dict(d=128, metric=flat.METRIC_IP, norms="unit", reserve=0, seed=18, events=random_events(18)),
    "random_27": dict(d=128, metric=flat.METRIC_IP, norms="mixed", reserve=0, seed=27, events=random_events(27)),
}
ROUTES = ("state", "exact", "batch", "range", "join", "rowsets", "grouping", "distinct", "maxsim", "assign", "kmeans", "mmr", "grouped")
IP_ONLY = ("distinct", "maxsim", "assign", "kmeans", "mmr")


def routes_checked(scenario, n_after):
    """The routes `check` runs after an event that leaves n_after rows (the coverage test of test_lifecycle_cpu.py reads this)."""
    if n_after == 0:
        return ("state",)
    return tuple(r for r in ROUTES if scenario["metric"] == flat.METRIC_IP or r not in IP_ONLY)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def apply_ops(idx, ops):
    for op in ops:
        if op[0] == "add":
            idx.add(op[1], normalize=False)
        elif op[0] == "set_rows":
            idx.set_rows(op[1], op[2], normalize=False)
        elif op[0] == "remove_rows":
            idx.remove_rows(op[1])
        elif op[0] == "reserve":
            idx.reserve(op[1])
        else:
            idx.reset()


class Run:
    """One scenario in flight: the index, the model, the queries and the handles (row sets by form, one grouping)."""

    def __init__(self, native, sc, model=None, idx=None):
        self.native, self.sc = native, sc
        self.model = model or IndexModel(sc["d"], sc["metric"], sc["norms"], sc["seed"])
        self.idx = idx or native.FlatIndex(sc["d"], metric=sc["metric"])
        self.ip = sc["metric"] == flat.METRIC_IP
        self.rowsets = {}                 # form -> (RowSet, Handle)
        self.grouping = None              # (Grouping, Handle, codes)
        self.refused_l2 = False
        self.q = None

    def make_queries(self):
        m = self.model
        g = np.random.default_rng(900 + self.sc["seed"]).standard_normal((NQ, m.d)).astype(np.float32)
        q = g.copy()
        near = np.arange(8, 20)
        q[near] = m.x[near * 50 + 299] * 3.0 + 0.2 * g[near]              # inside the neighbourhoods, not normalised
        q[0], q[1], q[3] = m.x[5], 3.0 * m.x[17], m.x[N0 - 1]
        self.q = np.ascontiguousarray(q)

    def refresh_queries(self):
        """Query 2 equals a row just written (or the first row a delete shifted), query 4 the lower of two identical rows."""
        m = self.model
        r = m.x[m.touched]
        norm = float(np.linalg.norm(r))
        self.q[2] = r if norm <= 2.0 else r / np.float32(norm)
        if m.copies is not None:
            self.q[4] = m.x[m.copies[0]]

    def close(self):
        for rs, _ in self.rowsets.values():
            rs.close()
        if self.grouping:
            self.grouping[0].free()
        self.idx.close()


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def agree(model, q, k, D, I, what, selected=None):
    """The rule of benchmarks/fuzz_mutations.py and test_flat_gpu.py: equal ids with scores within 2e-6 of flat_search on the
    mirror, else flat.adjudicate at its defaults."""
    Dw, Iw = model.search(q, k, selected)
    for i in range(len(q)):
        if np.array_equal(I[i], Iw[i]) and np.abs(D[i].astype(np.float64) - Dw[i]).max() <= 2e-6:
            continue
        ok, msg = model.adjudicate(q[i], k, D[i], I[i], selected)
        assert ok, (what, i, msg, I[i].tolist(), Iw[i].tolist())


def ties_lowest_first(model, D_row, I_row, what):
    """Query 4 is a row with an exact copy at a higher row number: the two are neighbours in the result, the lower row first,
    with equal bits (unit rows: they lead it; rows of mixed norms: only a row of norm ~40 can score higher)."""
    a, b = model.copies
    at = np.flatnonzero(I_row[:K - 1] == a)
    assert len(at) == 1 and I_row[at[0] + 1] == b and bits(D_row[at])[0] == bits(D_row[at + 1])[0], (what, model.copies, I_row[:K].tolist())
    if model.norms == "unit":
        assert at[0] == 0, (what, model.copies, I_row[:K].tolist())


def contained(got_ids, sure, near, what):
    """A range result against float64: every row that surely reaches the threshold, none but those and the near ties."""
    got = set(np.asarray(got_ids).tolist())
    assert len(got) == len(got_ids), (what, "a row twice")
    missing = set(sure.tolist()) - got
    extra = got - set(sure.tolist()) - set(near.tolist())
    assert not missing and not extra, (what, "missing", sorted(missing)[:8], "extra", sorted(extra)[:8])


# ---- stale handles: refused with "another state", nothing written ----------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def refused_untouched(run, rs, grp, what):
    """Every entry point that takes a row set (or the grouping `grp`, when rs is None) refuses the stale handle and leaves the
    caller's buffers as they were."""
    native, idx, q = run.native, run.idx, run.q
    L, h = native.lib(), idx.handle
    n = idx.ntotal
    Df, If, Gi = np.full((NQ, K), 7.0, np.float32), np.full((NQ, K), 7, np.int64), np.full((NQ, K), 7, np.int32)
    cnt = np.full(NQ, 7, np.int64)
    lab, sc = np.full(max(n, 1), 7, np.int32), np.full(max(n, 1), 7.0, np.float32)
    cen, kc, it = q[:5].copy(), np.full(5, 7, np.int64), ctypes.c_int(7)
    qr = np.arange(1, 1 + NQ, dtype=np.int64)
    fresh_grp = None
    calls = []
    if rs is not None:
        rsh = rs._h
        table = (ctypes.c_void_p * NQ)(*[rsh.value] * NQ)
        calls += [("search_rowset", lambda: L.mvdb_index_search_rowset(h, _p(q), 1, K, 0, rsh, _p(Df), _p(If))),
                  ("search_rowset batch", lambda: L.mvdb_index_search_rowset(h, _p(q), NQ, K, 0, rsh, _p(Df), _p(If))),
                  ("range_search", lambda: L.mvdb_index_range_search(h, _p(q), NQ, 0.5, 0, rsh, K, _p(cnt), _p(Df), _p(If))),
                  ("search_grouped", lambda: L.mvdb_index_search_grouped(h, _p(q), NQ, K, 0, table, _p(Df), _p(If)))]
        if n > NQ:                                                       # (an empty index has no row to join from)
            calls.append(("range_join", lambda: L.mvdb_index_range_join(h, _p(qr), NQ, 0.5, rsh, K, _p(cnt), _p(Df), _p(If))))
        if run.ip and n > 0:
            codes, n_groups, _ = run.model.grouping()
            fresh_grp = idx.grouping(codes, n_groups)
            gh = fresh_grp._h
            calls += [("search_mmr", lambda: L.mvdb_index_search_mmr(h, _p(q), NQ, K, 32, 0.5, 0, rsh, _p(Df), _p(If))),
                      ("search_distinct", lambda: L.mvdb_index_search_distinct(h, _p(q), NQ, K, 32, 0, gh, rsh, _p(Df), _p(If), _p(Gi))),
                      ("search_maxsim", lambda: L.mvdb_index_search_maxsim(h, _p(q), 4, K, 0, gh, rsh, _p(Df), _p(Gi), _p(If), _p(Df))),
                      ("assign", lambda: L.mvdb_index_assign(h, _p(q), N_VECTORS, 0, rsh, _p(lab), _p(sc))),
                      ("kmeans", lambda: L.mvdb_index_kmeans(h, _p(cen), 5, 1, rsh, _p(lab), _p(sc), _p(kc), ctypes.byref(it)))]
    elif run.ip:
        gh = grp._h
        calls += [("search_distinct", lambda: L.mvdb_index_search_distinct(h, _p(q), NQ, K, 32, 0, gh, None, _p(Df), _p(If), _p(Gi))),
                  ("search_maxsim", lambda: L.mvdb_index_search_maxsim(h, _p(q), 4, K, 0, gh, None, _p(Df), _p(Gi), _p(If), _p(Df)))]
    for name, call in calls:
        with pytest.raises(ValueError, match="another state"):
            native.check(call())
        assert (Df == 7.0).all() and (If == 7).all() and (Gi == 7).all() and (cnt == 7).all(), (what, name)
        assert (lab == 7).all() and (sc == 7.0).all() and (kc == 7).all() and it.value == 7 and np.array_equal(cen, q[:5]), (what, name)
    if fresh_grp is not None:
        fresh_grp.free()


def sync_handles(run, what):
    """Stale handles are shown to be refused and dropped; missing ones are built on the index as it is now."""
    m, idx = run.model, run.idx
    for form in FORMS:
        if form in run.rowsets and not m.valid(run.rowsets[form][1]):
            rs, _ = run.rowsets.pop(form)
            refused_untouched(run, rs, None, (what, "stale row set", form))
            rs.close()
    if run.grouping and not m.valid(run.grouping[1]):
        grp = run.grouping[0]
        run.grouping = None
        refused_untouched(run, None, grp, (what, "stale grouping"))
        grp.free()
    if m.n == 0:
        return
    for form in FORMS:
        if form not in run.rowsets:
            rows, excluded, h = m.rowset(form)
            rs = idx.rowset(rows, excluded=excluded)
            assert rs.is_bitmap == (h.form == "bitmap") and len(rs) == len(h.selected), (what, form, m.n >= ROWSET_BITMAP_MIN_ROWS)
            run.rowsets[form] = (rs, h)
    if run.grouping is None:
        codes, n_groups, h = m.grouping()
        run.grouping = (idx.grouping(codes, n_groups), h, codes)


# ---- the routes -----------------------------------------------------------------------------------------------------------
def score_matrix(idx, v, n):
    """[T, n] float32, the device's own single-query bits: one search with k = n per vector."""
    S = np.full((len(v), n), np.nan, np.float32)
    order = []
    for t in range(len(v)):
        D, I = idx.search(v[t:t + 1], n, normalize_q=False)
        assert (I[0] >= 0).all() and len(set(I[0].tolist())) == n
        S[t, I[0]] = D[0]
        order.append(I[0])
    return S, order


def masked(S, selected):
    out = np.full_like(S, np.nan)
    out[:, selected] = S[:, selected]
    return out


def check_state(run, what):
    idx, m = run.idx, run.model
    assert idx.ntotal == m.n, what
    if m.n:
        assert idx.get_rows(0, m.n).tobytes() == m.x.tobytes(), (what, "get_rows differs from the mirror")
    assert idx.shadow_rows == m.shadow_rows(), (what, "shadow_rows", idx.shadow_rows, m.shadow, m.n)


def check_topk(run, what):
    idx, m, q = run.idx, run.model, run.q
    for i in range(6):                                                   # the exact scan: single queries
        D, I = idx.search(q[i:i + 1], K)
        agree(m, q[i:i + 1], K, D, I, (what, "exact", i))
        if i == 4 and m.copies is not None:
            ties_lowest_first(m, D[0], I[0], (what, "exact"))
    assert idx.shadow_rows == m.shadow_rows(), (what, "a single query touched the shadow")
    D, I = idx.search(q, K)                                              # 40 queries: the certified pass where a shadow can exist
    agree(m, q, K, D, I, (what, "batch"))
    if m.copies is not None:
        ties_lowest_first(m, D[4], I[4], (what, "batch"))
    m.after_batch_search()
    assert idx.shadow_rows == m.shadow_rows(), (what, "shadow_rows after the batch", idx.shadow_rows, m.shadow, m.n)
    return D, I


def check_range(run, what, rowset=None, selected=None, bitmap=True):
    from test_range_batch_gpu import both_routes, own_thresholds
    idx, m, q = run.idx, run.model, run.q
    shared = run.ip and m.shadow_possible() and bitmap
    if rowset is None:
        thr, top = own_thresholds(idx, q, normalize_q=False, k=K_RANGE)
        assert idx.range_counters()[0] >= 0
        calls0 = idx.range_counters()[0]
        counts, D, I = both_routes(idx, q, thr, 256, normalize_q=False, expect_shared=shared)
        assert idx.range_counters()[0] - calls0 == (1 if shared else 0), (what, "range_counters")
        for i in range(NQ):
            c, (Dw, Iw) = int(counts[i]), top[i]
            assert (1, 10, K_RANGE)[i % 3] <= c <= 256, (what, i, c)
            k_ = min(c, K_RANGE)
            assert np.array_equal(bits(D[i, :k_]), bits(Dw[:k_])) and np.array_equal(I[i, :k_], Iw[:k_]), (what, "range vs search", i)
            assert (I[i, c:] == -1).all()
        if m.copies is not None:
            ties_lowest_first(m, D[4], I[4], (what, "range"))
    else:
        Db, _ = idx.search_rowset(q, K, rowset)
        thr = np.ascontiguousarray(Db[:, K - 1])
        counts, D, I = both_routes(idx, q, thr, 64, rowset=rowset, normalize_q=False, expect_shared=shared)
        for i in (0, 2, 4, 9):
            c = int(counts[i])
            assert K <= c <= 64, (what, i, c)
            Dw, Iw = idx.search_rowset(q[i:i + 1], c, rowset)
            assert np.array_equal(bits(D[i, :c]), bits(Dw[0])) and np.array_equal(I[i, :c], Iw[0]), (what, "range vs search_rowset", i)
    # ... and against float64 on the mirror, at thresholds inside a gap of the float64 scores
    thr, sure_counts, band = m.gap_thresholds(q, selected=selected)
    assert (band * 100 < np.maximum(sure_counts, 1)).all(), (what, "near ties of the reference", band.max())
    counts, D, I = both_routes(idx, q, thr, 256, rowset=rowset, normalize_q=False, expect_shared=shared)
    for i, (sure, near) in enumerate(m.range_search(q, thr, selected)):
        contained(I[i, :counts[i]], sure, near, (what, "range vs float64", i))


def join_window(m):
    lo = int(np.clip(m.touched - 150, 1, m.n - 300))
    return np.arange(lo, lo + 300, dtype=np.int64)


def check_join(run, what, rowset=None, selected=None, bitmap=True):
    from test_join_gpu import both_routes, check_rows_against_range_search
    idx, m = run.idx, run.model
    qrows = join_window(m)
    thr = float(m.join_threshold(qrows))
    shared = run.ip and m.shadow_possible() and bitmap
    counts, D, I = both_routes(idx, qrows, thr, 2048, rowset=rowset, expect_shared=shared)
    assert counts.max() <= 2048 and (rowset is not None or counts.sum() > 300), (what, counts.max(), counts.sum())
    check_rows_against_range_search(idx, qrows, counts, D, I, thr, [*range(0, 300, 25), 149, 151, 299] if rowset is None else [0, 150, 299], rowset)
    for r, (sure, near) in enumerate(m.join(qrows, np.float32(thr), selected)):
        contained(I[r, :counts[r]], sure, near, (what, "join vs float64", int(qrows[r])))


def check_scored_routes(run, S, what, rowset=None, selected=None):
    """distinct, MaxSim, assign (and, over every row, one k-means step) against their oracles fed the device's single-query
    bits; MMR against the float64 adjudicator."""
    from test_kmeans_gpu import same
    from test_mmr_gpu import check_against_candidates
    idx, m, q = run.idx, run.model, run.q
    grp, _, codes = run.grouping
    sel = np.arange(m.n, dtype=np.int64) if selected is None else selected
    nd = 4 if rowset is None else 2
    for t, (Dw, Iw, Gw) in enumerate(m.distinct(S[:nd], codes, K, sel)):
        # (one query per call: the scores of a distinct search are those of the plain search of the same call, and only a
        #  single query's are the bits of the score matrix)
        D, I, G = idx.search_distinct(q[t:t + 1], K, 32, grp, rowset=rowset)
        assert np.array_equal(bits(D[0]), bits(Dw)) and np.array_equal(I[0], Iw) and np.array_equal(G[0], Gw), (what, "distinct", t, I[0], Iw)
    got = idx.search_maxsim(q[4:8], 5, grp, rowset=rowset)
    want = m.maxsim(S[4:8], codes, 5, sel)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (what, "maxsim", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(bits(got[3]), bits(want[3])), (what, "maxsim rows")
    labels, scores = idx.assign(q[:N_VECTORS], rowset=rowset)
    wl, ws = m.assign(S)
    assert np.array_equal(labels, wl), (what, "assign labels", np.flatnonzero(labels != wl)[:8])
    assert np.array_equal(bits(scores), bits(ws)), (what, "assign scores", np.flatnonzero(bits(scores) != bits(ws))[:8])
    if rowset is None:
        empty = idx.rowset(np.empty(0, np.int64))
        start = idx.kmeans(q[:5], 3, rowset=empty)[0]                     # the initial centres as the loop first holds them
        empty.close()
        want = m.kmeans(lambda c: score_matrix(idx, c, m.n)[0], start, 1)
        same(idx.kmeans(q[:5], 1), want, (what, "kmeans"))
    nm = 3 if rowset is None else 2
    Dc, Ic = (idx.search(q[:nm], 32, normalize_q=True) if rowset is None else idx.search_rowset(q[:nm], 32, rowset, normalize_q=True))
    D, I = idx.search_mmr(q[:nm], 5, 32, 0.5, rowset=rowset, normalize_q=True)
    assert np.isin(I, sel).all(), (what, "mmr")
    for i, picks in enumerate(check_against_candidates(D, I, Dc, Ic, 5, what)):
        ok, msg, _ = m.mmr_adjudicate(Dc[i], Ic[i], picks, 5, 0.5)
        assert ok, (what, "mmr", i, msg)


def check_rowset(run, form, S, what):
    idx, m, q = run.idx, run.model, run.q
    rs, h = run.rowsets[form]
    sel = h.selected
    what = (what, form, h.form, f"built at n = {h.n}")
    for i in (0, 2, 4):
        D, I = idx.search_rowset(q[i:i + 1], K, rs)
        agree(m, q[i:i + 1], K, D, I, (what, "search_rowset", i), sel)
    D, I = idx.search_rowset(q, K, rs)
    assert np.isin(I, sel).all(), (what, "a row outside the selection", np.setdiff1d(I, sel)[:8])
    agree(m, q, K, D, I, (what, "search_rowset batch"), sel)
    check_range(run, (what, "range"), rs, sel, bitmap=h.form == "bitmap")
    check_join(run, (what, "join"), rs, sel, bitmap=h.form == "bitmap")
    if run.ip:
        Sm = masked(S, sel)
        Dw, Iw = m.ranking(Sm[0], sel)                                   # the full ranking under the set: the bits of the exact scan
        D, I = idx.search_rowset(q[:1], len(sel), rs)
        assert np.array_equal(bits(D[0]), bits(Dw)) and np.array_equal(I[0], Iw), (what, "full ranking")
        check_scored_routes(run, Sm, what, rs, sel)


def check_grouped(run, what):
    idx, q = run.idx, run.q
    table = [(None, *(run.rowsets[f][0] for f in FORMS))[i % 5] for i in range(15)]
    D, I = idx.search_grouped(q[:15], K, table)
    for i, rs in enumerate(table):
        Dw, Iw = idx.search(q[i:i + 1], K) if rs is None else idx.search_rowset(q[i:i + 1], K, rs)
        assert np.array_equal(bits(D[i]), bits(Dw[0])) and np.array_equal(I[i], Iw[0]), (what, "grouped", i)


def check_l2_refusals(run, what):
    idx, q = run.idx, run.q
    grp = run.grouping[0]
    for call in (lambda: idx.search_mmr(q[:2], 5, 32, 0.5), lambda: idx.search_distinct(q[:2], K, 32, grp),
                 lambda: idx.search_maxsim(q[4:8], 5, grp), lambda: idx.assign(q[:N_VECTORS]), lambda: idx.kmeans(q[:5], 1)):
        with pytest.raises(ValueError, match="inner-product"):
            call()
    run.refused_l2 = True


def check(run, what):
    """Everything, after one event.  `run` holds (idx, model, handles)."""
    idx, m = run.idx, run.model
    idx.set_option("range_shared", 2)
    idx.set_option("join_shared", 2)
    check_state(run, what)
    sync_handles(run, what)
    if m.n == 0:
        return
    run.refresh_queries()
    check_topk(run, what)
    check_range(run, what)
    check_join(run, what)
    S = None
    if run.ip:
        S, order = score_matrix(idx, run.q[:N_VECTORS], m.n)
        assert np.abs(S.astype(np.float64) - m.scores64(run.q[:N_VECTORS])).max() <= 1e-4, (what, "score matrix vs float64")
        for t in (0, 4):
            assert np.array_equal(order[t], m.ranking(S[t], np.arange(m.n))[1]), (what, "order of the full ranking", t)
        check_scored_routes(run, S, what)
    elif not run.refused_l2:
        check_l2_refusals(run, what)
    for form in FORMS:
        check_rowset(run, form, S, what)
    check_grouped(run, what)
    assert idx.shadow_rows == m.shadow_rows(), (what, "shadow_rows at the end of the check")


# ---- equals a rebuild -------------------------------------------------------------------------------------------------------
def snapshot(run):
    """Every call whose result the project claims bit-identical to the exact scan, as a list of (name, arrays)."""
    from test_range_batch_gpu import both_routes, own_thresholds
    from test_join_gpu import both_routes as join_both
    idx, m, q = run.idx, run.model, run.q
    shared = run.ip and m.shadow_possible()
    out = [("exact", idx.search(q[:1], K)), ("exact 2", idx.search(q[2:3], K)), ("exact 4", idx.search(q[4:5], K))]
    thr, _ = own_thresholds(idx, q, normalize_q=False, k=K_RANGE)
    out.append(("range", both_routes(idx, q, thr, 256, normalize_q=False, expect_shared=shared)))
    qrows = join_window(m)
    out.append(("join", join_both(idx, qrows, float(m.join_threshold(qrows)), 2048, expect_shared=shared)))
    table = [(None, *(run.rowsets[f][0] for f in FORMS))[i % 5] for i in range(15)]
    out.append(("grouped", idx.search_grouped(q[:15], K, table)))
    if run.ip:
        grp = run.grouping[0]
        out.append(("distinct", idx.search_distinct(q[:4], K, 32, grp)))
        out.append(("maxsim", idx.search_maxsim(q[4:8], 5, grp)))
        out.append(("assign", idx.assign(q[:N_VECTORS])))
        out.append(("assign dense", idx.assign(q[:N_VECTORS], rowset=run.rowsets["dense"][0])))
    return out, idx.search(q, K)


def check_equals_rebuild(run, what):
    m = run.model
    other = Run(run.native, run.sc, model=m)
    other.q = run.q
    try:
        other.idx.add(m.x, normalize=False)
        for r in (run, other):                                           # handles of the same selections on both
            for rs, _ in r.rowsets.values():
                rs.close()
            r.rowsets = {}
            if r.grouping:
                r.grouping[0].free()
                r.grouping = None
            r.idx.set_option("range_shared", 2)
            r.idx.set_option("join_shared", 2)
            sync_handles(r, what)
        assert other.idx.get_rows(0, m.n).tobytes() == run.idx.get_rows(0, m.n).tobytes()
        (mine, batch_a), (theirs, batch_b) = snapshot(run), snapshot(other)
        for (name, a), (_, b) in zip(mine, theirs):
            for x, y in zip(a, b):
                same = np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y)
                assert same, (what, "differs from a rebuild", name)
        # the certified batch may nominate differently (a wider norm bound on the mutated index): then both must be right
        if not (np.array_equal(batch_a[1], batch_b[1]) and np.array_equal(bits(batch_a[0]), bits(batch_b[0]))):
            for D, I in (batch_a, batch_b):
                for i in range(NQ):
                    ok, msg = m.adjudicate(run.q[i], K, D[i], I[i])
                    assert ok, (what, "certified batch after a rebuild", i, msg)
    finally:
        other.close()


def run_scenario(native, name, tamper=None):
    """The scenario `name`; tamper(model, event number): called after each event is applied (the demonstration that a wrong
    mirror is caught perturbs the model there)."""
    sc = SCENARIOS[name]
    print(f"scenario {name}: seed {sc['seed']}, events {sc['events']}")
    run = Run(native, sc)
    try:
        if sc["reserve"]:
            run.idx.reserve(sc["reserve"])
            run.model.cap = sc["reserve"]
        apply_ops(run.idx, run.model.apply(("add", N0)))
        run.make_queries()
        check(run, (name, 0, "build"))
        for number, event in enumerate(sc["events"], 1):
            t0 = time.perf_counter()
            apply_ops(run.idx, run.model.apply(event))
            if tamper:
                tamper(run.model, number)
            check(run, (name, number, event))
            print(f"  event {number} {event}: n = {run.model.n}, cells {run.model.cells[-3:]}, {time.perf_counter() - t0:.2f} s")
        check_equals_rebuild(run, (name, "rebuild"))
    finally:
        run.close()


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_lifecycle(gpu, name):
    from minivectordb_amd import _native
    run_scenario(_native, name)
