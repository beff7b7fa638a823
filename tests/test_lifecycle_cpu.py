"""The harness of tests/test_lifecycle_gpu.py checked without a GPU: the model's reference answers against float64 brute
force written out here, and the scenarios — plain data — against the table above ShadowStore in csrc/mvdb.hip: every
(event, prior store state) cell that can be reached without the int8 code and without a capture is visited, every route is
checked after every kind of event."""
import numpy as np
import pytest

from index_model import TIE_EPS, IndexModel
from oracle import flat
from test_lifecycle_gpu import FORMS, IP_ONLY, N0, NQ, ROUTES, SCENARIOS, random_events, routes_checked

N, D = 301, 24


def small_model(metric=flat.METRIC_IP, norms="mixed"):
    m = IndexModel(D, metric, norms, seed=77)
    m.apply(("add", N))
    return m


def queries(m, nq, seed=5):
    q = np.random.default_rng(seed).standard_normal((nq, m.d)).astype(np.float32)
    q[0] = m.x[7]
    q[1] = 3.0 * m.x[11]
    return q


def brute(m, q):
    """float64 scores by the textbook formula, one pair at a time where the model uses a matrix product."""
    x, q = m.x.astype(np.float64), np.asarray(q, np.float32).astype(np.float64)
    if m.metric == flat.METRIC_IP:
        return np.array([[float(np.dot(qi, r)) for r in x] for qi in q])
    return np.array([[float(((qi - r) ** 2).sum()) for r in x] for qi in q])


# ---- reference answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2])
def test_search_and_range_references(metric):
    m = small_model(metric)
    q = queries(m, 6)
    s = brute(m, q)
    assert np.abs(m.scores64(q) - s).max() < 1e-9
    sel = np.random.default_rng(1).permutation(N)[:120]
    for selected in (None, sel):
        lab = np.arange(N) if selected is None else selected
        D_, I = m.search(q, 10, selected)
        for i in range(len(q)):
            si = s[i, lab]
            order = lab[np.argsort(-si if metric == flat.METRIC_IP else si, kind="stable")][:10]
            assert I[i].tolist() == order.tolist(), (i, I[i], order)
            assert np.abs(D_[i] - s[i, I[i]]).max() < 1e-5
            ok, msg = m.adjudicate(q[i], 10, D_[i], I[i], selected)
            assert ok, msg
            wrong = I[i].copy()
            wrong[3] = np.setdiff1d(lab, order)[0]
            assert not m.adjudicate(q[i], 10, D_[i], wrong, selected)[0]
        thr = np.array([np.sort(s[i, lab])[::-1][20] if metric == flat.METRIC_IP else np.sort(s[i, lab])[20] for i in range(len(q))])
        for i, (sure, near) in enumerate(m.range_search(q, thr, selected)):
            si = s[i, lab]
            hit = si >= thr[i] if metric == flat.METRIC_IP else si <= thr[i]
            tie = np.abs(si - thr[i]) <= TIE_EPS
            assert sorted(sure.tolist()) == sorted(lab[hit & ~tie].tolist()) and sorted(near.tolist()) == sorted(lab[tie].tolist())
            assert len(sure) == 20 and len(near) == 1          # the threshold IS the 21st score: that row is the near tie


@pytest.mark.parametrize("metric", [flat.METRIC_IP, flat.METRIC_L2])
def test_join_reference(metric):
    m = small_model(metric)
    qrows = np.arange(100, 160)
    thr = m.join_threshold(qrows, share=0.05)
    sel = np.sort(np.random.default_rng(2).permutation(N)[:200])
    total = 0
    for selected in (None, sel):
        got = m.join(qrows, thr, selected)
        for (sure, near), i in zip(got, qrows):
            want = []
            for r in (range(N) if selected is None else selected.tolist()):
                if r >= i:
                    continue
                a, b = m.x[i].astype(np.float64), m.x[r].astype(np.float64)
                s = float(np.dot(a, b)) if metric == flat.METRIC_IP else float(((a - b) ** 2).sum())
                if abs(s - float(thr)) > TIE_EPS and (s >= thr if metric == flat.METRIC_IP else s <= thr):
                    want.append(r)
            assert sorted(sure.tolist()) == want, i
            total += len(want)
    assert total > 100


def test_distinct_maxsim_assign_references():
    m = small_model()
    v = queries(m, 9)
    v[8] = v[2]                                                           # equal centres: the lower label wins
    s = brute(m, v)
    codes = (np.arange(N) // 8).astype(np.int32)
    n_groups = int(codes.max()) + 1
    sel = np.random.default_rng(3).permutation(N)[:150]
    for selected in (None, sel):
        lab = np.arange(N) if selected is None else selected
        S = m.score_matrix(v, selected)
        assert np.isnan(S[:, np.setdiff1d(np.arange(N), lab)]).all()
        assert np.abs(S[:, lab] - s[:, lab]).max() < 1e-5
        # distinct: the best row of each group, the top-k groups
        for t, (Dg, Ig, Gg) in enumerate(m.distinct(S[:3], codes, 5, lab)):
            best = {}
            for r in lab.tolist():
                g = int(codes[r])
                if g not in best or s[t, r] > s[t, best[g]]:
                    best[g] = r
            top = sorted(best.values(), key=lambda r: -s[t, r])[:5]
            assert Ig.tolist() == top and Gg.tolist() == [int(codes[r]) for r in top], (t, Ig, top)
            assert np.abs(Dg - s[t, top]).max() < 1e-5
        # MaxSim: the sum over the query vectors of the per-group maximum
        Dm, Gm, Im, Dtok = m.maxsim(S[3:7], codes, 4, lab)
        sums = np.full(n_groups, -np.inf)
        for g in range(n_groups):
            rows = lab[codes[lab] == g]
            if len(rows):
                sums[g] = sum(s[t, rows].max() for t in range(3, 7))
        top = np.argsort(-sums, kind="stable")[:4]
        assert Gm.tolist() == top.tolist() and np.abs(Dm - sums[top]).max() < 1e-4
        for j, g in enumerate(Gm):
            for t in range(4):
                rows = lab[codes[lab] == g]
                assert Im[j, t] == rows[np.argmax(s[3 + t, rows])]
        # assign: the argmax over the centres, ties to the lower label
        labels, scores = m.assign(S)
        want = np.full(N, -1)
        want[lab] = np.argmax(s[:, lab], axis=0)
        assert np.array_equal(labels, want) and not (labels == 8).any()
        assert (scores[want < 0] == np.float32(-3.4028234663852886e38)).all()
        assert np.abs(scores[lab] - s[:, lab].max(axis=0)).max() < 1e-5
    # the full ranking of a selection: ties to the lower POSITION
    x2 = m.x.copy()
    m.x[40] = m.x[30]
    S = m.score_matrix(m.x[30:31], np.array([50, 40, 30, 20]))
    assert m.ranking(S[0], np.array([50, 40, 30, 20]))[1][:2].tolist() == [40, 30]
    assert m.ranking(S[0], np.array([20, 30, 40, 50]))[1][:2].tolist() == [30, 40]
    m.x = x2


def test_mmr_and_kmeans_references_are_the_existing_oracles():
    import kmeans_oracle
    import mmr_oracle
    m = small_model(norms="unit")
    q = queries(m, 2)[:1]
    D_, I = m.search(q, 32)
    picks = mmr_oracle.select(D_[0], m.x[I[0]], 5, 0.5)
    assert m.mmr_adjudicate(D_[0], I[0], picks, 5, 0.5)[0]
    assert not m.mmr_adjudicate(D_[0], I[0], [0, 1, 1, 2, 3], 5, 0.5)[0]
    c = m.x[:4].copy()
    got = m.kmeans(lambda cc: m.score_matrix(cc), c, 1)
    labels = np.argmax(brute(m, c), axis=0)
    assert np.array_equal(kmeans_oracle.assign(m.score_matrix(c))[0], labels)
    for j in range(4):
        mean = m.x[labels == j].astype(np.float64).mean(axis=0)
        assert np.abs(got[0][j] - mean / np.linalg.norm(mean)).max() < 1e-6
    assert got[4] == 1


# ---- the mirror: events, handles, store states ---------------------------------------------------------------------------------
def test_events_on_the_mirror():
    m = IndexModel(128, seed=9)
    assert m.apply(("add", 1000))[0][0] == "add" and m.cap == 1024 and m.cells == ["add_grows"]
    keep = m.x.copy()
    m.after_batch_search()
    assert m.shadow == "complete" and m.shadow_rows() == 1000
    rs, grp = m.rowset("sparse")[2], m.grouping()[2]
    op, = m.apply(("add", 20))
    assert m.shadow == "complete" and m.shadow_rows() == 1020 and np.array_equal(m.x[:1000], keep) and np.array_equal(m.x[1000:], op[1])
    assert m.valid(rs) and not m.valid(grp)                             # a row set outlives an add, a grouping does not
    op, = m.apply(("set", 10))
    assert np.array_equal(m.x[op[1]], op[2]) and op[1][0] == 1019 and m.valid(rs) and m.shadow == "complete"
    m.apply(("copy",))
    a, b = m.copies
    assert a < b and m.x[a].tobytes() == m.x[b].tobytes()
    grp = m.grouping()[2]
    op, = m.apply(("del_scatter", 30))
    assert m.n == 990 and not m.valid(rs) and not m.valid(grp) and m.shadow == "emptied" and m.shadow_rows() == 0
    if m.copies is not None:                                            # the copies moved with the renumbering
        a2, b2 = m.copies
        assert (a2, b2) != (a, b) or not (op[1] < b).any()
        assert m.x[a2].tobytes() == m.x[b2].tobytes()
    rs = m.rowset("excluded")[2]
    m.apply(("add", 5))
    assert m.cells[-1] == "add_fits/emptied" and m.shadow == "emptied" and m.valid(rs) and len(rs.selected) == 987
    m.after_batch_search()
    m.apply(("big",))
    assert m.cells[-1] == "set_rows_scale/complete" and m.shadow == "emptied" and abs(np.linalg.norm(m.x[m.big]) - 40) < 1e-3
    m.after_batch_search()
    m.apply(("add", 40))                                               # 1035 > 1024: grows by half
    assert m.cells[-1] == "add_grows" and m.cap == 1536 and m.shadow == "absent"
    m.apply(("reserve", 0))
    m.apply(("reserve", 10))
    assert m.cells[-2:] == ["reserve_noop", "reserve_grows"] and m.cap == 1546
    gen = m.gen
    m.apply(("reset",))
    assert m.n == 0 and m.gen == gen + 1 and not m.valid(rs) and m.max_norm == 0 and m.cap == 1546
    m.apply(("add", 50))
    assert m.cells[-2:] == ["add_fits/absent", "reset_then_add"]
    # the forms of row set on either side of 4,096 rows
    for n, dense in ((4095, "list"), (4096, "bitmap")):
        m = IndexModel(8, seed=1)
        m.apply(("add", n))
        forms = {f: m.rowset(f) for f in FORMS}
        assert forms["dense"][2].form == dense and forms["excluded"][2].form == "bitmap" and forms["excluded"][1]
        assert forms["unsorted"][2].form == forms["sparse"][2].form == "list"
        assert (np.diff(forms["unsorted"][0]) < 0).any() and (np.diff(forms["sparse"][0]) > 0).all()
        assert len(forms["dense"][0]) * 10 >= n * 9 and n <= len(forms["sparse"][0]) * 64 and len(forms["sparse"][0]) * 10 < n * 9


# ---- the scenarios against the table --------------------------------------------------------------------------------------------
def replay(name):
    """The scenario on the model alone, a batch search after every event as `check` runs one: (model, n after each event)."""
    sc = SCENARIOS[name]
    m = IndexModel(sc["d"], sc["metric"], sc["norms"], sc["seed"])
    m.cap = sc["reserve"]
    ns = []
    for event in [("add", N0)] + list(sc["events"]):
        m.apply(event)
        ns.append(m.n)
        if m.n:
            m.after_batch_search()
    return m, ns


# cells of the table no scenario can reach, by name, with the reason
UNREACHABLE = {
    "capture": "a stream capture across mutations is test_update_gpu.test_row_sets_and_graphs_survive's subject (out of scope)",
    "build failure": "needs a device allocation to fail",
    "every cell of the int8 code": "the code needs 500,000 rows (kCode8MinRows); test_code8_gpu has its lifecycle",
    "free": "freed with the index: nothing can be searched afterwards",
    "every route after reset": "the index is empty: only the state and the refusal of stale handles are checked",
    "l2:reserve / reset with offsets behind": "reserve and reset drop the offsets with the shadow whatever they hold: the "
                                              "cells with offsets present are the same code",
}
REQUIRED_IP = {"add_fits/complete", "add_fits/emptied", "add_fits/absent", "add_grows", "reserve_grows", "reserve_noop",
               "set_rows/complete", "set_rows/emptied", "set_rows_scale/complete", "remove_one_early/complete",
               "remove_scattered/complete", "remove_suffix/complete", "reset/complete", "reset_then_add"}
REQUIRED_L2 = {"l2:add_fits/offsets_present", "l2:add_fits/offsets_behind", "l2:add_fits/offsets_emptied",
               "l2:set_rows/offsets_present", "l2:set_rows/offsets_behind", "l2:remove_scattered/offsets_present",
               "l2:remove_one_early/offsets_behind", "l2:remove_suffix/offsets_present"}


def test_scenarios_reach_every_cell_of_the_table():
    cells = {name: set(replay(name)[0].cells) for name in SCENARIOS}
    ip = set().union(*(c for name, c in cells.items() if SCENARIOS[name]["metric"] == flat.METRIC_IP and SCENARIOS[name]["d"] == 128))
    assert not REQUIRED_IP - ip, sorted(REQUIRED_IP - ip)
    assert not REQUIRED_L2 - cells["l2_offsets"], sorted(REQUIRED_L2 - cells["l2_offsets"])
    # the two hand-written d = 128 scenarios split the work as the issue says: one never reallocates, one does
    assert "add_grows" not in cells["unit_reserved"] and "reserve_grows" not in cells["unit_reserved"]
    assert {"add_grows", "reserve_grows", "reserve_noop"} <= cells["unit_growing"]
    assert "set_rows_scale/complete" in cells["mixed_norms"]
    # d = 30: no shadow, ever
    assert all(c.endswith("/absent") or "/" not in c for c in cells["padded_d30"]), cells["padded_d30"]
    assert all(isinstance(reason, str) and reason for reason in UNREACHABLE.values())


def test_every_route_is_checked_after_every_kind_of_event():
    seen = {}
    for name, sc in SCENARIOS.items():
        if sc["metric"] != flat.METRIC_IP:
            continue
        m, ns = replay(name)
        for kind, n_after in zip(m.kinds[1:], ns[1:]):
            seen.setdefault(kind, set()).update(routes_checked(sc, n_after))
    kinds = {"add", "set", "copy", "big", "del_big", "del_one", "del_scatter", "del_suffix", "reserve", "pair", "reset"}
    assert set(seen) == kinds, kinds ^ set(seen)
    for kind in kinds - {"reset"}:                                      # (UNREACHABLE: every route after reset)
        assert seen[kind] == set(ROUTES), (kind, set(ROUTES) - seen[kind])
    assert seen["reset"] == {"state"}
    l2 = routes_checked(SCENARIOS["l2_offsets"], 4000)
    assert set(l2) == set(ROUTES) - set(IP_ONLY)


def test_scenario_shapes():
    for name, sc in SCENARIOS.items():
        m, ns = replay(name)
        assert 10 <= len(sc["events"]) <= 14, name
        live = [n for n in ns if n]
        assert all(3900 <= n <= 4450 and n % 32 for n in live), (name, ns)
        if sc["reserve"]:
            assert "add_grows" not in m.cells and max(ns) <= sc["reserve"], name
    for name in ("unit_reserved", "unit_growing", "mixed_norms", "l2_offsets", "padded_d30"):
        ns = replay(name)[1]
        down = any(a > 4096 > b for a, b in zip(ns, ns[1:]) if b)
        up = any(a < 4096 < b for a, b in zip(ns, ns[1:]) if a)
        assert down and up, (name, ns)
    assert random_events(18) == SCENARIOS["random_18"]["events"] and random_events(27) == SCENARIOS["random_27"]["events"]
    assert random_events(18) != random_events(27)
    # exact ties exist after ("copy",) and survive the delete that follows it
    m, _ = replay("unit_reserved")
    assert "copy" in m.kinds


def test_gap_thresholds_leave_no_near_ties():
    """The float64 count check of the range routes leaves out rows within TIE_EPS of the threshold: for the reference alone
    their share stays under 1 % of the counted rows, on the corpus of every scenario and under every form of row set."""
    for name, sc in SCENARIOS.items():
        m = IndexModel(sc["d"], sc["metric"], sc["norms"], sc["seed"])
        m.apply(("add", N0))
        q = np.random.default_rng(900 + sc["seed"]).standard_normal((NQ, m.d)).astype(np.float32)
        q[8:20] = m.x[np.arange(8, 20) * 50 + 299] * 3.0 + 0.2 * q[8:20]
        q[0], q[1] = m.x[5], 3.0 * m.x[17]
        for selected in [None] + [m.rowset(f)[2].selected for f in FORMS]:
            thr, counts, band = m.gap_thresholds(q, selected=selected)
            assert (band * 100 < np.maximum(counts, 1)).all(), (name, band.max())
            assert ((counts >= 7) & (counts <= 204)).all(), (name, counts.min(), counts.max())
            s = m.scores64(q, selected)
            hit = s >= thr[:, None].astype(np.float64) if sc["metric"] == flat.METRIC_IP else s <= thr[:, None].astype(np.float64)
            assert np.array_equal(hit.sum(axis=1) - band, counts) or (band == 0).all()
