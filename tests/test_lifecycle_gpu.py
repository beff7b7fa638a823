"""Every search route against the model of tests/index_model.py across index mutations.

A scenario is a list of events (index_model.py names them) run on ONE index with the model beside it.  After every event
`check` compares the state (ntotal, the bytes of get_rows, shadow_rows as the table above ShadowStore in csrc/mvdb.hip
predicts it) and every route — exact scan, certified batch, range batch, range join, the four forms of resident row set on
every entry point that takes one, grouping, distinct, MaxSim, assign, one k-means step, MMR, grouped search, probed search,
search by examples, boosted search — with the mirror, and at the end of the scenario the whole index with a rebuild from the
mirror.

Two more resident handles live beside the row sets and the grouping: ONE partition of 33 lists, kept in step as the model's
partition_plan says (kept, update()d, or — after a removal — read back and re-created from its labels), and two term columns,
rebuilt whenever the row count or the numbering changes.  Their labels and values are compared with the mirror's after every
change; the three routes are compared as bits with their contract oracles fed the device's own single-query scores.

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

from index_model import BOOST_WEIGHTS, N_CENTRES, ROWSET_BITMAP_MIN_ROWS, IndexModel
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
# the cells of the partition the scenarios above miss: rows reallocated under it by a reserve, then an add; an add and a set
# with no search between; a delete and an add that bring the row count back
_EVENTS_5 = [("add", 97), ("reserve", 300), ("add", 31), ("pair", ("add", 40), ("set", 30)), ("pair", ("del_scatter", 9), ("add", 9)),
             ("set", 25), ("copy",), ("reserve", 0), ("del_suffix", 300), ("add", 120), ("big",), ("del_big",)]


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
    "probe_growing": dict(d=128, metric=flat.METRIC_IP, norms="mixed", reserve=0, seed=8, events=_EVENTS_5),
}
ROUTES = ("state", "exact", "batch", "range", "join", "rowsets", "grouping", "distinct", "maxsim", "assign", "kmeans", "mmr", "grouped",
          "probe", "examples", "boost")
IP_ONLY = ("distinct", "maxsim", "assign", "kmeans", "mmr", "probe", "examples", "boost")


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
    """One scenario in flight: the index, the model, the queries and the handles (row sets by form, one grouping, one partition
    with the index of its centres, two term columns)."""

    def __init__(self, native, sc, model=None, idx=None):
        self.native, self.sc = native, sc
        self.model = model or IndexModel(sc["d"], sc["metric"], sc["norms"], sc["seed"])
        self.idx = idx or native.FlatIndex(sc["d"], metric=sc["metric"])
        self.ip = sc["metric"] == flat.METRIC_IP
        self.rowsets = {}                 # form -> (RowSet, Handle)
        self.grouping = None              # (Grouping, Handle, codes)
        self.refused_l2 = False
        self.q = None
        self.partition = None             # the Partition; the model holds its Handle and the labels it must have
        self.mirrors_partition = model is None   # (the rebuild's partition is the library's own: labels=None)
        self.centres = None               # its stored centres, as partition.centres() returns them ...
        self.cidx = None                  # ... and the index that holds exactly those: the contract's definition of the probes
        self.terms = None                 # ([RowTerm, RowTerm], Handle)
        self.coarse = None                # [6, C] the centre index's single-query bits for q[:6], per check
        self.extra_terms = None           # per check: (a term of -0.0, the tie column's term, the tie column)
        self.refused_list_probe = False
        self.pending = np.empty(0, np.int64)   # rows set_rows wrote that wait in their old lists (partition_plan: "keep")
        self.pending_checks = 0           # the checks that ran in that state

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
        if self.partition:
            self.partition.free()
        for t in (self.terms[0] if self.terms else []) + list((self.extra_terms or ())[:2]):
            t.free()
        if self.cidx is not None and self.mirrors_partition:
            self.cidx.close()
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


class DeviceBuffers:
    """Queries, examples and poisoned result buffers on the device, for the device variants of the three routes."""

    def __init__(self, q, v):
        import torch
        self.torch = torch
        self.q, self.v = torch.from_numpy(q[:6].copy()).cuda(), torch.from_numpy(v).cuda()
        self.D = torch.full((6, K), 7.5, dtype=torch.float32, device="cuda")
        self.I = torch.full((6, K), 777, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def results(self, rows=6):
        self.torch.cuda.synchronize()
        D, I = self.D.cpu().numpy(), self.I.cpu().numpy()
        assert (D[rows:] == 7.5).all() and (I[rows:] == 777).all()       # nothing behind the results is written
        self.D.fill_(7.5)
        self.I.fill_(777)
        return D[:rows], I[:rows]

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.D == 7.5).all()) and bool((self.I == 777).all())


def example_vectors(q):
    """The vectors of the search by examples: three positives, then two negatives."""
    return np.ascontiguousarray(np.concatenate([q[5:8], q[20:22]]))


def refused_untouched(run, rs, grp, what, part=None, terms=None, match="another state"):
    """Every entry point that takes a row set (or the grouping `grp`, the partition `part`, the term columns `terms`, when rs is
    None) refuses the stale handle and leaves the caller's buffers as they were."""
    if part is not None or terms is not None or (rs is not None and run.ip and run.partition is not None and run.terms is not None):
        refused_new_routes(run, rs, part, terms, what, match)
    if part is not None or terms is not None:
        return
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


def refused_new_routes(run, rs, part, terms, what, match):
    """Probed search, search by examples, boosted search and boost_combine, host and device entry points, with ONE stale
    handle — the row set rs, the partition `part` or the term columns `terms` — beside valid ones: refused with the library's
    message for it, nothing written to host or device buffers."""
    native, idx, q = run.native, run.idx, run.q
    L, h = native.lib(), idx.handle
    Df, If = np.full((NQ, K), 7.0, np.float32), np.full((NQ, K), 7, np.int64)
    T = np.full(max(idx.ntotal, 1), 7.0, np.float32)
    v = example_vectors(q)
    dev = DeviceBuffers(q, v)
    qp, vp, Dp, Ip = dev.q.data_ptr(), dev.v.data_ptr(), dev.D.data_ptr(), dev.I.data_ptr()
    rsh = rs._h if rs is not None else None
    if rs is not None:                                                   # beside the stale row set: the run's valid handles
        part, terms = run.partition, run.terms[0]
    calls = []
    if part is not None:
        ph = part._h
        calls += [("search_probe", lambda: L.mvdb_index_search_probe(h, ph, _p(q), 1, K, 5, 0, rsh, _p(Df), _p(If))),
                  ("search_probe batch", lambda: L.mvdb_index_search_probe(h, ph, _p(q), NQ, K, N_CENTRES, 0, rsh, _p(Df), _p(If))),
                  ("search_probe_device", lambda: idx.search_probe_device(qp, 6, K, 5, part, Dp, Ip, rowset=rs, label_offset=1000))]
    if rs is not None:
        calls += [("search_examples", lambda: L.mvdb_index_search_examples(h, _p(v), 3, 2, K, 0, rsh, None, 0, _p(Df), _p(If))),
                  ("search_examples_device", lambda: idx.search_examples_device(vp, 3, 2, K, Dp, Ip, rowset=rs, label_offset=1000))]
    if terms is not None:
        keep, args = idx._boost_args(terms, BOOST_WEIGHTS, None, None)
        w = ctypes.c_float(0.7)
        calls += [("search_boosted", lambda: L.mvdb_index_search_boosted(h, _p(q), 1, K, 0, w, *args, rsh, _p(Df), _p(If))),
                  ("search_boosted batch", lambda: L.mvdb_index_search_boosted(h, _p(q), NQ, K, 0, w, *args, rsh, _p(Df), _p(If))),
                  ("search_boosted_device", lambda: idx.search_boosted_device(qp, 6, K, terms, BOOST_WEIGHTS, Dp, Ip, score_weight=0.7, rowset=rs,
                                                                              label_offset=1000))]
        if rs is None:
            calls.append(("boost_combine", lambda: L.mvdb_index_boost_combine(h, *args, _p(T))))
    assert calls, what
    for name, call in calls:
        with pytest.raises(ValueError, match=match):
            native.check(call() or 0)
        assert (Df == 7.0).all() and (If == 7).all() and (T == 7.0).all(), (what, name)
    assert dev.untouched(), (what, "a refused device variant wrote to its buffers")


def sync_terms(run, what):
    """The two term columns: shown refused once stale (rows added or removed since), built from the model's columns."""
    m, idx = run.model, run.idx
    if run.terms and not m.valid(run.terms[1]):
        terms, _ = run.terms
        run.terms = None
        refused_untouched(run, None, None, (what, "stale terms"), terms=terms, match=r"holds \d+ rows, the index \d+|before rows were removed")
        for t in terms:
            t.free()
    if m.n and run.terms is None:
        cols, h = m.term_columns()
        run.terms = ([idx.rowterm(c) for c in cols], h)
        assert all(len(t) == m.n for t in run.terms[0]), what


def sync_partition(run, what):
    """The partition, as the model's partition_plan says; after every change its labels are the mirror's, integer for integer."""
    m, idx = run.model, run.idx
    if not run.mirrors_partition:                                        # the rebuild: labelled by the library, never touched
        if run.partition is None:
            run.partition = idx.partition(run.centres)
        return
    action, rows = m.partition_plan()
    run.pending = rows if action == "keep" else np.empty(0, np.int64)
    if action in ("none", "keep"):
        m.partition_done(action, rows)
        return
    part = run.partition
    if action == "create":
        run.partition = part = idx.partition(m.centres())                # labels=None: the library's own assign
        if run.cidx is None:
            run.centres = part.centres()
            assert np.array_equal(bits(run.centres), bits(m.centres())), (what, "centres as given: none is normalised")
            run.cidx = run.native.FlatIndex(m.d)
            run.cidx.add(run.centres, normalize=False)
        assert np.array_equal(bits(part.centres()), bits(run.centres)), what
        sizes = part.sizes()                                             # lists on both sides of the 128-position work item, one of three items
        assert (sizes < 128).any() and ((sizes > 128) & (sizes <= 256)).any() and (sizes > 256).any(), (what, sizes)
    elif action == "update":
        if not m.valid(m.part):                                          # rows were added: stale for a search, not for update
            refused_untouched(run, None, None, (what, "stale partition"), part=part, match="mvdb_partition_update first")
        part.update(rows if len(rows) else None)
    else:                                                                # rows were removed, or the index was reset: dead
        refused_untouched(run, None, None, (what, "dead partition"), part=part, match="rows were removed since the partition was built")
        for named in (None, np.zeros(1, np.int64)):
            with pytest.raises(ValueError, match="rows were removed since the partition was built"):
                part.update(named)
        kept = m.drop_removed(part.labels())
        assert np.array_equal(kept, m.labels), (what, "the labels read back, the removed rows' dropped", np.flatnonzero(kept != m.labels)[:8])
        part.free()
        run.partition = part = None
    assigned = idx.assign(run.centres)[0] if m.n else None
    want = m.partition_done(action, rows, assigned)
    if action == "recreate":
        run.partition = part = idx.partition(run.centres, labels=want)
    if part is None:
        return
    got = part.labels()
    assert got.dtype == np.int32 and np.array_equal(got, want), (what, action, "labels", np.flatnonzero(got != want)[:8])
    assert np.array_equal(part.sizes(), np.bincount(want, minlength=N_CENTRES)) and len(part) == m.n and part.n_lists == N_CENTRES, (what, action)


def check_partition_invariant(run, what):
    """Every row no set_rows wrote since it was labelled holds the label assign gives it NOW (a row's label depends on its own
    vector and the centres alone); a row that waits in its old list is found through that list, with its new score."""
    from probe_oracle import probes
    m, idx = run.model, run.idx
    assigned = idx.assign(run.centres)[0]
    settled = np.ones(m.n, bool)
    settled[sorted(m.set_since)] = False
    assert np.array_equal(m.labels[settled], assigned[settled]), (what, "labels of rows nobody wrote", np.flatnonzero(settled & (m.labels != assigned))[:8])
    if not len(run.pending):
        return
    run.pending_checks += 1
    moved = run.pending[m.labels[run.pending] != assigned[run.pending]]
    if not len(moved):
        return
    r = int(moved[0])
    query = m.x[r:r + 1] / np.float32(max(1.0, np.linalg.norm(m.x[r]) / 2))   # (a row of norm ~40: the scores stay small)
    coarse = score_matrix(run.cidx, query, N_CENTRES)[0][0]
    at = int(np.flatnonzero(probes(coarse, N_CENTRES) == m.labels[r])[0])  # its OLD list is the query's probe number at + 1
    alone = idx.rowset(np.delete(np.arange(m.n, dtype=np.int64), r), excluded=True)   # a bitmap that selects this row alone
    assert alone.is_bitmap and len(alone) == 1
    Dw, Iw = idx.search_rowset(query, K, alone)
    assert Iw[0, 0] == r and (Iw[0, 1:] == -1).all()
    same_bits(idx.search_probe(query, K, at + 1, run.partition, rowset=alone), (Dw, Iw), (what, "old list, new vector", r, at))
    if at:                                                               # one probe fewer: the row is in none of the probed lists
        D, I = idx.search_probe(query, K, at, run.partition, rowset=alone)
        assert (I == -1).all(), (what, "the old list is not probed", r, at, I[0])
    alone.close()


def sync_handles(run, what):
    """Stale handles are shown to be refused and dropped; missing ones are built on the index as it is now."""
    m, idx = run.model, run.idx
    if run.ip:                                                           # first: the row sets' refusals pass them as the VALID handles
        sync_terms(run, what)
        sync_partition(run, what)
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
    check_probe(run, S, what, rowset, selected)
    check_examples(run, S, what, rowset, selected)
    check_boost(run, S, what, rowset, selected)
    if rowset is None:
        check_device_variants(run, what)


def same_bits(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "rows", got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, "scores", got[0], want[0])


def copies_selected(m, selected):
    return m.copies is not None and (selected is None or np.isin(m.copies, selected).all())


def check_probe(run, S, what, rowset, selected):
    """Probed search against probe_oracle fed the device's bits: the coarse row from the index of the stored centres, the fine
    row from the score matrix, the labels from the mirror — between a set_rows and its update a changed row's OLD label."""
    idx, m, q = run.idx, run.model, run.q
    part, C = run.partition, N_CENTRES
    if rowset is not None and not rowset.is_bitmap:                      # a list-form set is refused by contract: shown once
        if not run.refused_list_probe:
            Df, If = np.full((NQ, K), 7.0, np.float32), np.full((NQ, K), 7, np.int64)
            with pytest.raises(ValueError, match="takes a bitmap-form row set"):
                run.native.check(run.native.lib().mvdb_index_search_probe(idx.handle, part._h, _p(q), NQ, K, 5, 0, rowset._h, _p(Df), _p(If)))
            assert (Df == 7.0).all() and (If == 7).all(), (what, "list-form set")
            run.refused_list_probe = True
        return
    for nprobe in (1, 5, C):
        for t in (0, 2, 4):
            got = idx.search_probe(q[t:t + 1], K, nprobe, part, rowset=rowset)
            Dw, Iw, P = m.probe(run.coarse[t], S[t], m.labels, K, nprobe, selected)
            same_bits((got[0][0], got[1][0]), (Dw, Iw), (what, "probe", nprobe, t))
            if nprobe == C:                                              # every list: the exact search over the labelled rows
                assert (m.labels >= 0).all()
                same_bits(got, idx.search(q[t:t + 1], K) if rowset is None else idx.search_rowset(q[t:t + 1], K, rowset), (what, "probe, every list", t))
            if t == 4 and copies_selected(m, selected) and np.isin(m.labels[list(m.copies)], P).all():
                ties_lowest_first(m, got[0][0], got[1][0], (what, "probe", nprobe))
    D, I = idx.search_probe(q[:6], K, 5, part, rowset=rowset)            # a batch in one call: each row its own probes
    for t in range(6):
        Dw, Iw, _ = m.probe(run.coarse[t], S[t], m.labels, K, 5, selected)
        same_bits((D[t], I[t]), (Dw, Iw), (what, "probe batch", t))


def check_examples(run, S, what, rowset, selected):
    idx, m, q = run.idx, run.model, run.q
    sel = np.arange(m.n, dtype=np.int64) if selected is None else selected
    Sx = np.concatenate([S[5:8], S[20:22]])
    skip = np.array([m.ranking(S[j], sel)[1][0] for j in (5, 6, 7)], np.int64)   # the top hit of each positive
    want = m.examples(Sx, 3, K, skip, selected)
    assert (want[1] >= 0).all() and not np.isin(skip, want[1]).any()
    try:
        idx.set_option("examples_vectors_per_pass", 2)                   # three passes that carry the packed maxima
        calls0, passes0 = idx.examples_counters()
        carried = idx.search_examples(q[5:8], q[20:22], K, rowset=rowset, skip_rows=skip)
        assert idx.examples_counters() == (calls0 + 1, passes0 + 3), (what, "examples passes")
    finally:
        idx.set_option("examples_vectors_per_pass", 0)
    same_bits(carried, want, (what, "examples, 2 vectors per pass"))
    same_bits(idx.search_examples(q[5:8], q[20:22], K, rowset=rowset, skip_rows=skip), want, (what, "examples"))
    got = idx.search_examples(q[4:5], None, K, rowset=rowset)            # one positive, no negative: the plain search
    same_bits(got, m.examples(S[4:5], 1, K, (), selected), (what, "examples, one positive"))
    if rowset is None or rowset.is_bitmap or (np.diff(sel) > 0).all():   # (an unsorted list: search_rowset's ties go by list position)
        Dw, Iw = idx.search(q[4:5], K) if rowset is None else idx.search_rowset(q[4:5], K, rowset)
        same_bits(got, (Dw[0], Iw[0]), (what, "examples vs search"))
    if copies_selected(m, selected):
        ties_lowest_first(m, got[0], got[1], (what, "examples"))


def check_boost(run, S, what, rowset, selected):
    """Boosted search against boost_oracle: the columns are the model's, recomputed — the resident terms must still hold them."""
    idx, m, q = run.idx, run.model, run.q
    terms, n = run.terms[0], m.n
    cols, special = m.term_columns()[0], m.term_special()
    zero, tie, tie_col = run.extra_terms
    inside = (lambda r: True) if selected is None else (lambda r: r in selected)
    sparse = m.sparse_entries()
    for sp in (None, sparse):
        T = m.boost_column(cols, BOOST_WEIGHTS, n, sp)
        if rowset is None:                                               # the column by itself: the NaN row compares as bits
            got_T = idx.boost_combine(terms, BOOST_WEIGHTS, *(sp or (None, None)))
            assert np.array_equal(bits(got_T), bits(T)), (what, "boost_combine", sp is not None, np.flatnonzero(bits(got_T) != bits(T))[:8])
            assert np.isnan(got_T[special["nan"]]) and got_T[special["pinf"]] == np.inf and got_T[special["ninf"]] == -np.inf
        singles = {}
        for t in (0, 2, 4):
            D, I = idx.search_boosted(q[t], K, terms, BOOST_WEIGHTS, score_weight=0.7, sparse_rows=sp and sp[0], sparse_values=sp and sp[1], rowset=rowset)
            same_bits((D[0], I[0]), m.boosted(S[t], T, 0.7, K, selected), (what, "boost", t, sp is not None))
            assert special["nan"] not in I[0] and special["ninf"] not in I[0] and (I[0] >= 0).all(), (what, "boost", t)
            if inside(special["pinf"]):
                assert I[0, 0] == special["pinf"] and D[0, 0] == np.inf, (what, "the +inf row leads", t)
            singles[t] = (D[0], I[0])
        if sp is None:                                                   # a batch shares T: each row equals its single call
            D, I = idx.search_boosted(q[:6], K, terms, BOOST_WEIGHTS, score_weight=0.7, rowset=rowset)
            for t in range(6):
                same_bits((D[t], I[t]), singles[t] if t in singles else m.boosted(S[t], T, 0.7, K, selected), (what, "boost batch", t))
    # a term of -0.0 at weight 1 with w_s = 1: the plain search
    if rowset is None or rowset.is_bitmap or (np.diff(selected) > 0).all():
        for t in (0, 2, 4):
            want = idx.search(q[t:t + 1], K) if rowset is None else idx.search_rowset(q[t:t + 1], K, rowset)
            same_bits(idx.search_boosted(q[t], K, [zero], [1.0], score_weight=1.0, rowset=rowset), want, (what, "boost, -0.0", t))
    # equal terms on the two copies: their scores tie, the lower ROW first in every form (an unsorted list too)
    D, I = idx.search_boosted(q[4], K, [tie], [BOOST_WEIGHTS[1]], score_weight=0.7, rowset=rowset)
    same_bits((D[0], I[0]), m.boosted(S[4], m.boost_column([tie_col], BOOST_WEIGHTS[1:], n), 0.7, K, selected), (what, "boost, tied copies"))
    if copies_selected(m, selected):
        ties_lowest_first(m, D[0], I[0], (what, "boost"))


def check_device_variants(run, what):
    """The device variants of the three routes on a stream of their own with label_offset = 1000: the host results, the labels
    shifted, the padding still -1."""
    import torch
    idx, m, q = run.idx, run.model, run.q
    terms = run.terms[0]
    dev = DeviceBuffers(q, example_vectors(q))
    stream = torch.cuda.Stream()
    qp, vp, Dp, Ip, s = dev.q.data_ptr(), dev.v.data_ptr(), dev.D.data_ptr(), dev.I.data_ptr(), stream.cuda_stream
    sparse = m.sparse_entries()
    skip = np.array([m.touched, 0], np.int64)
    skip_dev = torch.from_numpy(skip).cuda()
    torch.cuda.synchronize()
    for name, rows, call, host in (
            ("probe", 6, lambda: idx.search_probe_device(qp, 6, K, 1, run.partition, Dp, Ip, stream=s, label_offset=1000),
             lambda: idx.search_probe(q[:6], K, 1, run.partition)),
            ("examples", 1, lambda: idx.search_examples_device(vp, 3, 2, K, Dp, Ip, skip_rows_ptr=skip_dev.data_ptr(), n_skip=2, stream=s, label_offset=1000),
             lambda: tuple(a[None] for a in idx.search_examples(q[5:8], q[20:22], K, skip_rows=skip))),
            ("boost batch", 6, lambda: idx.search_boosted_device(qp, 6, K, terms, BOOST_WEIGHTS, Dp, Ip, score_weight=0.7, stream=s, label_offset=1000),
             lambda: idx.search_boosted(q[:6], K, terms, BOOST_WEIGHTS, score_weight=0.7)),
            ("boost sparse", 1, lambda: idx.search_boosted_device(qp, 1, K, terms, BOOST_WEIGHTS, Dp, Ip, score_weight=0.7, sparse_rows=sparse[0],
                                                                  sparse_values=sparse[1], stream=s, label_offset=1000),
             lambda: idx.search_boosted(q[0], K, terms, BOOST_WEIGHTS, score_weight=0.7, sparse_rows=sparse[0], sparse_values=sparse[1]))):
        call()
        stream.synchronize()
        D, I = dev.results(rows)
        Dh, Ih = host()
        assert ((I >= 1000) | (I == -1)).all(), (what, name, "padding stays -1 under a label offset")
        same_bits((D, np.where(I >= 0, I - 1000, -1)), (Dh, Ih), (what, name, "device variant"))


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
    idx, q, m = run.idx, run.q, run.model
    grp = run.grouping[0]
    term = idx.rowterm(np.zeros(m.n, np.float32))                        # (a column can be stored; no search takes it)
    ip = run.native.FlatIndex(m.d)                                       # a partition can only come from an inner-product index
    ip.add(m.x[:64], normalize=False)
    foreign = ip.partition(m.centres())
    for call in (lambda: idx.search_mmr(q[:2], 5, 32, 0.5), lambda: idx.search_distinct(q[:2], K, 32, grp),
                 lambda: idx.search_maxsim(q[4:8], 5, grp), lambda: idx.assign(q[:N_VECTORS]), lambda: idx.kmeans(q[:5], 1),
                 lambda: idx.partition(m.centres()), lambda: idx.partition(m.centres(), labels=np.zeros(m.n, np.int32)),
                 lambda: idx.search_probe(q[:2], K, 5, foreign), lambda: idx.search_examples(q[5:8], q[20:22], K),
                 lambda: idx.search_boosted(q[:2], K, [term], [1.0]), lambda: idx.boost_combine([term], [1.0])):
        with pytest.raises(ValueError, match="inner-product"):
            call()
    foreign.free()
    ip.close()
    term.free()
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
        run.coarse = score_matrix(run.cidx, run.q[:6], N_CENTRES)[0]
        tie_col = m.tie_column()
        run.extra_terms = (idx.rowterm(np.full(m.n, -0.0, np.float32)), idx.rowterm(tie_col), tie_col)
        check_partition_invariant(run, what)
        check_scored_routes(run, S, what)
    elif not run.refused_l2:
        check_l2_refusals(run, what)
    for form in FORMS:
        check_rowset(run, form, S, what)
    check_grouped(run, what)
    if run.extra_terms:
        for t in run.extra_terms[:2]:
            t.free()
        run.extra_terms = None
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
        part, terms = run.partition, run.terms[0]
        out.append(("partition", (part.labels(), part.sizes(), part.centres())))
        for nprobe in (1, 5, N_CENTRES):
            out.append((f"probe {nprobe}", idx.search_probe(q, K, nprobe, part)))
        out.append(("probe excluded", idx.search_probe(q, K, 5, part, rowset=run.rowsets["excluded"][0])))
        if run.rowsets["dense"][0].is_bitmap:
            out.append(("probe dense", idx.search_probe(q, K, 5, part, rowset=run.rowsets["dense"][0])))
        for form in (None, "unsorted", "dense"):
            rs = run.rowsets[form][0] if form else None
            out.append((f"examples {form}", idx.search_examples(q[5:8], q[20:22], K, rowset=rs)))
            out.append((f"boost {form}", idx.search_boosted(q[:6], K, terms, BOOST_WEIGHTS, score_weight=0.7, rowset=rs)))
        sparse = m.sparse_entries()
        out.append(("boost sparse", idx.search_boosted(q[2], K, terms, BOOST_WEIGHTS, score_weight=0.7, sparse_rows=sparse[0], sparse_values=sparse[1])))
        out.append(("boost column", (idx.boost_combine(terms, BOOST_WEIGHTS, *sparse),)))
    return out, idx.search(q, K)


def check_equals_rebuild(run, what):
    m = run.model
    other = Run(run.native, run.sc, model=m)
    other.q = run.q
    other.centres, other.cidx = run.centres, run.cidx
    m.last_set = set()                # the run's partition hears of every row set_rows wrote: update(rows) in sync_handles
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
        if run.ip:                    # kept labels may differ from a fresh assign only on rows set and never named: none is left
            assert not m.set_since and np.array_equal(other.partition.labels(), m.labels), (what, "labels of a rebuild")
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
        # a row searched in its old list with its new vector, between a set_rows and the update that names it
        assert not run.ip or tamper or run.pending_checks > 0, (name, run.model.part_cells)
        served = (run.idx.probe_counters()[0], run.idx.examples_counters()[0], run.idx.boost_counters()[0])
        assert not run.ip or min(served) > len(sc["events"]), (name, "the three routes were served", served)
    finally:
        run.close()


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_lifecycle(gpu, name):
    from minivectordb_amd import _native
    run_scenario(_native, name)
