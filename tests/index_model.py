"""A plain-numpy model of a FlatIndex across its mutations: the mirror of the rows, the state of the derived stores as the
table above ShadowStore in csrc/mvdb.hip predicts it, which handles are still valid, and the reference answer of every search
route computed from the mirror.  No GPU and no product import: tests/test_lifecycle_cpu.py checks it against float64 brute
force, tests/test_lifecycle_gpu.py drives an index beside it.

EVENTS are plain tuples; IndexModel.apply(event) expands one into concrete operations (row numbers and data drawn from the
model's own seeded generator), applies them to the mirror and returns them for the index:

    ("add", m)            m new rows                      ("set", m)          set_rows of m scattered rows
    ("copy",)             set_rows: one row becomes a copy of a LOWER row (exact ties from then on)
    ("big",)              set_rows: one row of norm ~40 (moves half_xscale of the norm bound)
    ("del_big",)          remove_rows of that row         ("del_one",)        remove_rows of one early row
    ("del_scatter", m)    remove_rows of m scattered rows ("del_suffix", m)   remove_rows of the last m rows
    ("reserve", extra)    reserve(capacity + extra); extra = 0 asks for no more than is there
    ("reset",)            reset                           ("pair", e1, e2)    two events with no search between them

The store states: the shadow is "absent" (no allocation), "emptied" (allocation kept, no row converted) or "complete";
idx.shadow_rows reads n for the last and 0 for the other two.  The L2 offsets beside it are "absent", "emptied", "behind"
(fewer rows than the shadow: an add into a complete shadow extends the shadow alone) or "present".

Two resident handles have validity rules of their own (include/mvdb.h "PROBED SEARCH", "BOOSTED SEARCH").  A partition is
searchable while no row was added or removed; update() revives it after adds, nothing does after a removal or a reset (read
the labels back, drop the removed rows', re-create); set_rows leaves it valid with the changed rows in their OLD lists until
update(rows) names them.  The model keeps the labels such a partition must hold and the rows still waiting to be named
(partition_plan / partition_done); part_cells logs "action/operations since the partition was last in step".  A term column
dies with every add and every removal and survives set_rows."""
import math

import numpy as np

import boost_oracle
import distinct_oracle
import examples_oracle
import kmeans_oracle
import maxsim_oracle
import mmr_oracle
import probe_oracle
from oracle import flat

SHADOW_DIMS = (128, 256, 384, 512, 640, 768, 896, 1024)      # half_scan.hip: half_shadow_dim
TIE_EPS = 2e-6                                               # flat.adjudicate's tie_eps
ROWSET_BITMAP_MIN_ROWS = 4096                                # mvdb_rowset_create: bitmap / twin only from here
N_CENTRES = 33                                               # the partition's lists (assign takes two passes from 33 centres)
PROBE_ITEM = 128                                             # probe plan: a list is cut into work items of 128 positions
BOOST_WEIGHTS = (0.05, 0.02)                                 # the weights of the two term columns


class Handle:
    """What the model remembers of a resident handle — kind "rowset", "grouping", "partition" or "rowterm": the selection (row
    sets), the row count and the renumbering generation it was built (a partition: last brought up to date) at."""

    def __init__(self, kind, n, gen, selected=None, form=None):
        self.kind, self.n, self.gen, self.selected, self.form = kind, n, gen, selected, form


class IndexModel:
    def __init__(self, d, metric=flat.METRIC_IP, norms="unit", seed=0):
        self.d, self.metric, self.norms, self.seed = int(d), metric, norms, seed
        self.rng = np.random.default_rng(seed)
        self.centre = self.rng.standard_normal(self.d)
        self.x = np.empty((0, self.d), np.float32)
        self.cap = 0
        self.gen = 0
        self.max_norm = 0.0               # the norm bound only ever widens (note_row_norms); reset clears it
        self.shadow = "absent"
        self.shadow_exp = None            # the exponent half_xscale had when the shadow was built
        self.hn_alloc, self.hn_rows = False, 0
        self.cells = []                   # the (event, prior store state) cells visited, in order
        self.kinds = []                   # the kind of every applied event
        self.copies = None                # (lower row, higher row): identical rows written by ("copy",)
        self.big = None                   # the row ("big",) wrote
        self.touched = 0                  # a row just written, or the first row a delete shifted
        self.prev_kind = None
        # the partition (the section "the partition's labels" below)
        self.part = None                  # Handle of the partition as it was last created or updated
        self.labels = np.empty(0, np.int32)   # the labels it must hold: those of the rows [0, len) that have one
        self.part_cap = 0                 # rows its label storage has room for
        self.set_since = set()            # rows written by set_rows that no update has named yet
        self.last_set = set()             # ... those of them the last event wrote
        self.part_gone = []               # removals since it was last in step: sorted row arrays, None for a reset
        self.part_since = []              # the operations since it was last in step, by name
        self.part_cells = []              # the (action / operations since) cells the partition went through

    # ---- state ------------------------------------------------------------------------------------------------------------
    @property
    def n(self):
        return self.x.shape[0]

    @property
    def ld(self):
        return (self.d + 3) // 4 * 4

    def scale_exp(self):
        """The exponent half_xscale takes from the norm bound (None: no usable bound)."""
        if not self.max_norm > 0:
            return None
        bound = self.max_norm * 1.000001
        m, e = math.frexp(bound)
        # the device's bound comes from an fp32 sum: the model is only a prediction away from a power of two
        assert min(abs(m - 0.5), abs(m - 1.0)) > 1.5e-7, ("norm bound too near a power of two for a prediction", bound)
        return e

    def shadow_possible(self):
        return self.d in SHADOW_DIMS and self.ld == self.d and self.scale_exp() is not None and self.n > 0

    def shadow_rows(self):
        """What idx.shadow_rows must read."""
        return self.n if self.shadow == "complete" else 0

    def offsets(self):
        if not self.hn_alloc:
            return "absent"
        if self.hn_rows == 0:
            return "emptied"
        return "present" if self.hn_rows == self.n else "behind"

    def after_batch_search(self):
        """A batch of 33+ queries went through: the certified pass built or completed the shadow where one can exist."""
        if self.shadow_possible():
            self.shadow, self.shadow_exp = "complete", self.scale_exp()
            if self.metric == flat.METRIC_L2:
                self.hn_alloc, self.hn_rows = True, self.n

    def valid(self, h):
        """Row sets survive adds and set_rows; groupings, row terms and (to be searched) partitions need the very row count too."""
        if h.kind in ("grouping", "rowterm", "partition"):
            return h.gen == self.gen and h.n == self.n
        return h.gen == self.gen and h.n <= self.n

    def updatable(self, h):
        """A partition follows adds and set_rows through update; after a removal or a reset update is refused as well."""
        assert h.kind == "partition"
        return h.gen == self.gen and h.n <= self.n

    def rowset(self, form):
        """The four forms of resident row set, as (rows to pass, excluded flag, Handle)."""
        n = self.n
        every = np.arange(n, dtype=np.int64)
        big = n >= ROWSET_BITMAP_MIN_ROWS
        if form == "unsorted":
            rows = np.random.default_rng(n).permutation(n)[:min(700, n)].astype(np.int64)
            return rows, False, Handle("rowset", n, self.gen, rows, "list")
        if form == "sparse":                                     # sorted, 1 row in 5: a list (with a bitmap twin from 4,096 rows)
            rows = every[2::5].copy()
            return rows, False, Handle("rowset", n, self.gen, rows, "list")
        if form == "dense":                                      # sorted, 97.5 % of the rows: a bitmap from 4,096 rows
            rows = np.setdiff1d(every, every[5::40])
            return rows, False, Handle("rowset", n, self.gen, rows, "bitmap" if big else "list")
        assert form == "excluded"
        gone = np.array([min(99, n - 1), 7 % n, n - 1], np.int64)
        return gone, True, Handle("rowset", n, self.gen, np.setdiff1d(every, gone), "bitmap")

    def grouping(self):
        return (np.arange(self.n) // 8).astype(np.int32), (self.n + 7) // 8, Handle("grouping", self.n, self.gen)

    # ---- the partition's labels ---------------------------------------------------------------------------------------------
    # The model does not look for nearest centres: it records WHICH rows take a fresh label and which keep theirs; the fresh
    # ones come from the caller (`assigned`: what assign gives for every row now — include/mvdb.h: "integer for integer").
    def centres(self):
        """The scenario's N_CENTRES centres [C, d] float32, from a generator of their own: two thirds near the cluster of
        make_rows, the rest isotropic, none normalised — uneven lists on both sides of the 128-position work item."""
        rng = np.random.default_rng(7000 + self.seed)
        c = rng.standard_normal((N_CENTRES, self.d))
        near = 2 * N_CENTRES // 3
        c[:near] = 0.45 * c[:near] + self.centre * rng.uniform(0.4, 1.3, (near, 1))
        return np.ascontiguousarray(c, dtype=np.float32)

    def nearest64(self, centres):
        """int32[n]: the float64 nearest centre of every row (the CPU tests' stand-in for the device's assign)."""
        return np.argmax(self.x.astype(np.float64) @ np.asarray(centres, np.float32).astype(np.float64).T, axis=1).astype(np.int32)

    def partition_plan(self):
        """What the holder of the partition does before the next search, as (action, rows):
        "none" / "create" (there is none; create: labels=None), "keep" (rows: those set_rows wrote that no update has named —
        they stay in their old lists), "update" (refused by a search when rows were added; update(rows)), "recreate" (refused
        by search and update; read the labels back, drop the removed rows', create from them), "drop" (the same on an empty
        index: nothing to create from).  Rows written by the LAST event wait one check in their old lists."""
        h = self.part
        if h is None:
            return ("create" if self.n else "none"), None
        if not self.updatable(h):
            return ("recreate" if self.n else "drop"), None
        rows = np.array(sorted(r for r in self.set_since if r < len(self.labels)), np.int64)
        if self.valid(h) and (len(rows) == 0 or self.last_set):
            return "keep", rows
        return "update", rows

    def drop_removed(self, labels):
        """The labels read back from a dead partition without those of the rows removed since."""
        for gone in self.part_gone:
            labels = labels[:0] if gone is None else np.delete(labels, gone[gone < len(labels)])
        return labels

    def partition_done(self, action, rows, assigned=None):
        """The action of partition_plan was carried out; returns the labels the partition holds now."""
        since = "+".join(self.part_since)
        if action in ("none", "keep"):
            if action == "keep" and len(rows):
                self.part_cells.append("search/set_pending")
            return self.labels
        if action == "drop":
            self.part_cells.append("refused/" + since)
            self.part, self.labels, self.set_since, self.part_gone, self.part_since = None, np.empty(0, np.int32), set(), [], []
            return self.labels
        assigned = np.asarray(assigned, np.int32)
        assert assigned.shape == (self.n,)
        kept = len(self.labels)
        labels = np.concatenate([self.labels, assigned[kept:]])                  # rows without a label take a fresh one
        if action == "update":
            self.part_cells.append(("update_rows/" if len(rows) else "update/") + since)
            if self.n > self.part_cap:
                self.part_cells.append("labels_grow")
            labels[rows] = assigned[rows]                                        # ... and so do the rows named
            self.set_since = {r for r in self.set_since if r < kept} - set(np.asarray(rows).tolist())
            self.part_cap = max(self.part_cap, self.n)
        elif action == "recreate":
            self.part_cells.append(("recreate_same_count/" if self.n == self.part.n else "recreate/") + since)
            self.set_since = {r for r in self.set_since if r < kept}
            self.part_cap = self.n
        else:
            assert action == "create" and kept == 0
            self.part_cells.append("create/" + since)
            self.set_since = set()
            self.part_cap = self.n
        self.labels = labels
        self.part = Handle("partition", self.n, self.gen)
        self.part_gone, self.part_since = [], []
        return self.labels

    def _part_note(self, name, written=None, gone=None, reset=False):
        self.part_since.append(name)
        if written is not None:
            self.set_since |= set(np.asarray(written).tolist())
            self.last_set |= set(np.asarray(written).tolist())
        if gone is not None:
            self.labels = np.delete(self.labels, gone[gone < len(self.labels)])
            self.part_gone.append(gone)
            left = np.array(sorted(self.set_since), np.int64)
            left = left[~np.isin(left, gone)]
            self.set_since = set((left - np.searchsorted(gone, left)).tolist())
            self.last_set = set()
        if reset:
            self.labels = self.labels[:0]
            self.part_gone.append(None)
            self.set_since, self.last_set = set(), set()

    # ---- the term columns of boosted search ------------------------------------------------------------------------------------
    def term_special(self):
        """The rows whose second term is NaN, +inf and -inf."""
        n, g = self.n, self.gen
        return {"nan": (n // 3 + g) % n, "pinf": (n // 2 + g) % n, "ninf": (n // 5 + g) % n}

    def term_columns(self):
        """([recency, category] float32[n] each, Handle): a ramp over the rows and a column of five values (-0.0 among them) with
        one NaN, one +inf and one -inf row; functions of (n, gen) alone."""
        n, g = self.n, self.gen
        r = np.arange(n)
        ramp = (4.0 * ((r + 3 * g) % n) / n).astype(np.float32)
        few = np.array([-0.0, 0.5, -1.5, 2.0, 3.0], np.float32)[(r * 7 + g + n) % 5]
        sp = self.term_special()
        few[sp["nan"]], few[sp["pinf"]], few[sp["ninf"]] = np.nan, np.inf, -np.inf
        return [ramp, few], Handle("rowterm", n, self.gen)

    def tie_column(self):
        """The five-valued column without its non-finite rows, equal on the two copies: their boosted scores tie."""
        r = np.arange(self.n)
        col = np.array([-0.0, 0.5, -1.5, 2.0, 3.0], np.float32)[(r * 7 + self.gen + self.n) % 5]
        if self.copies is not None:
            col[self.copies[1]] = col[self.copies[0]]
        return col

    def sparse_entries(self):
        """Five (row, value) entries of a single boosted query; the lower copy is one of the rows."""
        n = self.n
        first = self.copies[0] if self.copies is not None else 11
        rows = list(dict.fromkeys([first, n - 1, 0, n // 2 + 1, n // 7, n // 9, 17]))[:5]
        return np.array(rows, np.int64), np.array([0.25, -0.125, 0.3, 0.001, -2.0], np.float32)

    # ---- events -----------------------------------------------------------------------------------------------------------
    def make_rows(self, m):
        g = self.rng.standard_normal((m, self.d))
        g[self.rng.random(m) < 0.35] += 2.0 * self.centre        # a cluster: dense neighbourhoods for range and join
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        if self.norms == "mixed":
            g *= self.rng.uniform(0.55, 1.9, (m, 1))
        return np.ascontiguousarray(g, dtype=np.float32)

    def _cell(self, name):
        self.cells.append(name)

    def _store_cells(self, event):
        self._cell(f"{event}/{self.shadow}")
        if self.metric == flat.METRIC_L2:
            self._cell(f"l2:{event}/offsets_{self.offsets()}")

    def _note_norms(self, rows):
        if len(rows):
            self.max_norm = max(self.max_norm, float(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max())))

    def _drop(self):
        self.shadow, self.shadow_exp, self.hn_alloc, self.hn_rows = "absent", None, False, 0

    def _invalidate(self):
        if self.shadow != "absent":
            self.shadow = "emptied"
        self.hn_rows = 0

    def _renumber(self, gone):
        gone = np.sort(np.asarray(gone, np.int64))
        self.gen += 1
        self._invalidate()

        def moved(r):
            return None if r is None or r in gone else int(r - np.searchsorted(gone, r))
        if self.copies is not None:
            a, b = moved(self.copies[0]), moved(self.copies[1])
            self.copies = (a, b) if a is not None and b is not None else None
        self.big = moved(self.big)
        self.x = np.ascontiguousarray(np.delete(self.x, gone, axis=0))
        self.touched = min(int(gone[0]), max(self.n - 1, 0))

    def apply(self, event):
        """Apply one event to the mirror; returns the operations for the index: ("add", X), ("set_rows", rows, X),
        ("remove_rows", rows), ("reserve", n), ("reset",)."""
        kind = event[0]
        self.last_set = set()
        if kind == "pair":
            self.kinds.append("pair")
            ops = []
            for e in event[1:]:
                ops += self._apply(e)
            return ops
        self.kinds.append(kind)
        return self._apply(event)

    def _apply(self, event):
        kind = event[0]
        n = self.n
        prev, self.prev_kind = self.prev_kind, kind
        if kind == "add":
            X = self.make_rows(event[1])
            if n + len(X) > self.cap:                                            # grow: both stores dropped first
                self._cell("add_grows")
                self._part_note("add_grows")
                self.cap = max(n + len(X), self.cap + self.cap // 2, 1024)
                self._drop()
                self._note_norms(X)
            else:
                self._store_cells("add_fits")
                self._part_note("add_fits")
                if prev == "reset":
                    self._cell("reset_then_add")
                self._note_norms(X)
                if self.shadow == "complete" and self.scale_exp() == self.shadow_exp:
                    pass                                                         # extended: stays complete (offsets stay behind)
                else:
                    self._invalidate()
            self.x = np.ascontiguousarray(np.concatenate([self.x, X]))
            self.touched = n
            return [("add", X)]
        if kind in ("set", "copy", "big"):
            if kind == "set":
                # scattered, the LAST row among them (in the L2 scenario a row the offsets do not cover yet); descending: any order is allowed
                rows = np.sort(np.append(self.rng.choice(n - 1, event[1] - 1, replace=False), n - 1)).astype(np.int64)[::-1].copy()
                X = self.make_rows(len(rows))
            elif kind == "copy":
                pool = np.arange(40, n - 40)
                if self.norms == "mixed":        # a long row: as a query it scores itself above every row but one of norm ~40
                    pool = pool[np.linalg.norm(self.x[pool].astype(np.float64), axis=1) > 1.75]
                a, b = sorted(self.rng.choice(pool, 2, replace=False).tolist())
                rows, X = np.array([b], np.int64), self.x[a:a + 1].copy()
                self.copies = (a, b)
            else:
                b = int(self.rng.integers(40, n - 40))
                rows = np.array([b], np.int64)
                g = self.rng.standard_normal((1, self.d))                        # (outside the cluster: no score beyond ~60)
                X = np.ascontiguousarray(g * (40.0 / np.linalg.norm(g)), dtype=np.float32)
                self.big = b
            if self.copies is not None and kind != "copy" and np.isin(self.copies, rows).any():
                self.copies = None
            before = self.scale_exp()
            self._note_norms(X)
            moves = self.shadow == "complete" and self.scale_exp() != before
            self._store_cells("set_rows_scale" if moves else "set_rows")
            if moves:
                self._invalidate()
            self.x[rows] = X
            self._part_note("set", written=rows)
            self.touched = int(rows[0])
            return [("set_rows", rows, X)]
        if kind in ("del_big", "del_one", "del_scatter", "del_suffix"):
            if kind == "del_big":
                assert self.big is not None
                rows = np.array([self.big], np.int64)
            elif kind == "del_one":
                rows = np.array([3], np.int64)
            elif kind == "del_scatter":
                rows = self.rng.choice(n, event[1], replace=False).astype(np.int64)
            else:
                rows = np.arange(n - event[1], n, dtype=np.int64)
            name = "remove_" + {"del_big": "one", "del_one": "one_early", "del_scatter": "scattered", "del_suffix": "suffix"}[kind]
            self._store_cells(name)
            self._part_note(name, gone=np.sort(rows))
            self._renumber(rows)
            return [("remove_rows", rows)]
        if kind == "reserve":
            want = self.cap + event[1]
            if want > self.cap:
                self._cell("reserve_grows")
                self._part_note("reserve_grows")
                self.cap = want
                self._drop()
            else:
                self._cell("reserve_noop")
                self._part_note("reserve_noop")
            return [("reserve", want)]
        if kind == "reset":
            self._store_cells("reset")
            self._part_note("reset", reset=True)
            self.gen += 1
            self._drop()
            self.x = np.empty((0, self.d), np.float32)
            self.max_norm, self.copies, self.big, self.touched = 0.0, None, None, 0
            return [("reset",)]
        raise ValueError(f"unknown event {event!r}")

    # ---- reference answers ------------------------------------------------------------------------------------------------
    def scores64(self, q, rows=None):
        """float64 scores (IP) / squared distances (L2) of every (or the listed) row against the queries: [nq, m]."""
        x = self.x.astype(np.float64) if rows is None else self.x[rows].astype(np.float64)
        q = np.atleast_2d(np.asarray(q, np.float32)).astype(np.float64)
        if self.metric == flat.METRIC_IP:
            return q @ x.T
        return ((q * q).sum(axis=1)[:, None] - 2.0 * (q @ x.T)) + (x * x).sum(axis=1)[None, :]

    def reaches(self, s, thr):
        """(rows that surely reach the threshold, rows within TIE_EPS of it) as boolean arrays."""
        thr = np.asarray(thr, np.float64)
        band = np.abs(s - thr) <= TIE_EPS
        hit = (s >= thr) if self.metric == flat.METRIC_IP else (s <= thr)
        return hit & ~band, band

    def search(self, q, k, selected=None):
        """flat_search on the mirror; under a selection the labels are ROW NUMBERS and ties go to the lower position."""
        q = np.atleast_2d(np.asarray(q, np.float32))
        if selected is None:
            return flat.flat_search(self.x, q, k, metric=self.metric)
        D, P = flat.flat_search(self.x, q, k, metric=self.metric, rows=selected)
        return D, np.where(P >= 0, np.asarray(selected)[np.maximum(P, 0)], -1)

    def adjudicate(self, q, k, D, I, selected=None):
        """flat.adjudicate at its defaults; under a selection I holds row numbers."""
        if selected is None:
            return flat.adjudicate(self.x, q, k, D, I, metric=self.metric)
        pos = {int(r): j for j, r in enumerate(np.asarray(selected).tolist())}
        I = np.asarray(I).reshape(-1)
        if any(int(r) not in pos for r in I if r >= 0):
            return False, f"a label outside the selection: {[int(r) for r in I if r >= 0 and int(r) not in pos]}"
        P = np.array([pos[int(r)] if r >= 0 else -1 for r in I], np.int64)
        return flat.adjudicate(self.x, q, k, D, P, metric=self.metric, rows=np.asarray(selected, np.int64))

    def gap_thresholds(self, q, ranks=(10, 200), selected=None):
        """Per query a float32 threshold in the widest float64 gap between neighbours of rank r - 3 .. r + 3 (r by turns from
        `ranks`): (thr float32[nq], counts int64[nq] of the rows that surely reach it, band int64[nq] of rows within TIE_EPS)."""
        s = self.scores64(q, selected)
        nq, m = s.shape
        thr, counts, band = np.empty(nq, np.float32), np.empty(nq, np.int64), np.empty(nq, np.int64)
        for i in range(nq):
            best = np.sort(s[i])[::-1] if self.metric == flat.METRIC_IP else np.sort(s[i])
            r = min(ranks[i % len(ranks)], m - 4)
            lo = max(r - 3, 1)
            gaps = np.abs(np.diff(best[lo - 1:r + 4]))
            j = lo - 1 + int(np.argmax(gaps))
            thr[i] = np.float32(0.5 * (best[j] + best[j + 1]))
            sure, near = self.reaches(s[i], thr[i])
            counts[i], band[i] = sure.sum(), near.sum()
        return thr, counts, band

    def range_search(self, q, thr, selected=None):
        """Per query (rows that surely reach thr, rows within TIE_EPS of it), as row numbers."""
        s = self.scores64(q, selected)
        thr = np.broadcast_to(np.asarray(thr, np.float64), (s.shape[0],))
        lab = np.arange(self.n) if selected is None else np.asarray(selected)
        out = []
        for i in range(s.shape[0]):
            sure, near = self.reaches(s[i], thr[i])
            out.append((lab[sure], lab[near]))
        return out

    def join(self, qrows, thr, selected=None):
        """The range join: per query row i (rows below i that surely reach thr, those within TIE_EPS)."""
        lab = np.arange(self.n) if selected is None else np.asarray(selected)
        s = self.scores64(self.x[np.asarray(qrows)], selected)
        out = []
        for j, i in enumerate(np.asarray(qrows).tolist()):
            sure, near = self.reaches(s[j], thr)
            below = lab < i
            out.append((lab[sure & below], lab[near & below]))
        return out

    def join_threshold(self, qrows, share=0.015):
        """A float32 threshold that about `share` of the window's pairs reach."""
        s = self.scores64(self.x[np.asarray(qrows)])
        pairs = s[np.arange(self.n)[None, :] < np.asarray(qrows)[:, None]]
        return np.float32(np.quantile(pairs, 1.0 - share if self.metric == flat.METRIC_IP else share))

    def score_matrix(self, v, selected=None):
        """[T, n] float32: the oracle's fp32 score of every selected row for every vector, NaN elsewhere (the input of the
        distinct, MaxSim and assign oracles; the GPU tests pass the device's own single-query bits instead)."""
        v = np.atleast_2d(np.asarray(v, np.float32))
        sel = np.arange(self.n, dtype=np.int64) if selected is None else np.asarray(selected, np.int64)
        S = np.full((v.shape[0], self.n), np.nan, np.float32)
        if len(sel):
            D, P = flat.flat_search(self.x, v, len(sel), metric=self.metric, rows=sel)
            for t in range(v.shape[0]):
                S[t, sel[P[t]]] = D[t]
        return S

    @staticmethod
    def ranking(s_row, selected):
        """(D, I) of the full ranking of the selected rows from one row of a score matrix: best first by the order-preserving
        image of the bits, ties to the lower POSITION of the selection."""
        sel = np.asarray(selected, np.int64)
        s = s_row[sel]
        keep = np.flatnonzero(s == s)
        image = maxsim_oracle.order_image(s[keep]).astype(np.int64)
        order = keep[np.lexsort((keep, -image))]
        return s[order], sel[order]

    def distinct(self, S, codes, k, selected=None):
        """Per row of the score matrix S: distinct_oracle.collapse of the full ranking."""
        sel = np.arange(self.n, dtype=np.int64) if selected is None else selected
        return [distinct_oracle.collapse(*self.ranking(S[t], sel), codes, k) for t in range(S.shape[0])]

    def maxsim(self, S, codes, k, selected=None):
        sel = np.arange(self.n, dtype=np.int64) if selected is None else selected
        return maxsim_oracle.maxsim(S, codes, sel, k)

    @staticmethod
    def assign(S):
        return kmeans_oracle.assign(S)

    def kmeans(self, scores_of, centres, max_iter):
        return kmeans_oracle.kmeans(scores_of, self.x, centres, max_iter)

    @staticmethod
    def _masked(s, selected):
        """The scores of the selected rows, NaN (no offer) elsewhere."""
        s = np.asarray(s, np.float32)
        if selected is None:
            return s
        out = np.full_like(s, np.nan)
        out[..., selected] = s[..., selected]
        return out

    def probe(self, coarse, fine, labels, k, nprobe, selected=None):
        """(D, I, probes) of one probed query: coarse [C] its scores against the centres, fine [n] against the rows."""
        return probe_oracle.probe_search(coarse, fine, labels, k, nprobe, selected)

    def examples(self, S, P, k, skip=(), selected=None):
        """(D, I) of a search by examples: S [P + N, n], the positives' rows of the score matrix first."""
        return examples_oracle.examples(self._masked(S, selected), P, k, skip)

    @staticmethod
    def boost_column(terms, weights, n, sparse=None):
        return boost_oracle.combine(terms, weights, n, sparse)

    def boosted(self, s_row, T, w_s, k, selected=None):
        """(D, I) of one boosted query: S = w_s * s + T over the selected rows, ties to the lower ROW in every form."""
        return boost_oracle.boosted(self._masked(s_row, selected), T, w_s, k)

    def mmr_adjudicate(self, rel, cand_rows, picks, k, lam):
        return mmr_oracle.adjudicate(rel, self.x[np.asarray(cand_rows)], picks, k, lam)
