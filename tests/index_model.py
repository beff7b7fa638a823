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
(fewer rows than the shadow: an add into a complete shadow extends the shadow alone) or "present"."""
import math

import numpy as np

import distinct_oracle
import kmeans_oracle
import maxsim_oracle
import mmr_oracle
from oracle import flat

SHADOW_DIMS = (128, 256, 384, 512, 640, 768, 896, 1024)      # half_scan.hip: half_shadow_dim
TIE_EPS = 2e-6                                               # flat.adjudicate's tie_eps
ROWSET_BITMAP_MIN_ROWS = 4096                                # mvdb_rowset_create: bitmap / twin only from here


class Handle:
    """What the model remembers of a row set or a grouping: the selection (row sets), the row count and the renumbering
    generation it was built at."""

    def __init__(self, kind, n, gen, selected=None, form=None):
        self.kind, self.n, self.gen, self.selected, self.form = kind, n, gen, selected, form


class IndexModel:
    def __init__(self, d, metric=flat.METRIC_IP, norms="unit", seed=0):
        self.d, self.metric, self.norms = int(d), metric, norms
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
        """Row sets survive adds and set_rows; groupings need the very row count too."""
        if h.kind == "grouping":
            return h.gen == self.gen and h.n == self.n
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
                self.cap = max(n + len(X), self.cap + self.cap // 2, 1024)
                self._drop()
                self._note_norms(X)
            else:
                self._store_cells("add_fits")
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
            self._store_cells("remove_" + {"del_big": "one", "del_one": "one_early", "del_scatter": "scattered", "del_suffix": "suffix"}[kind])
            self._renumber(rows)
            return [("remove_rows", rows)]
        if kind == "reserve":
            want = self.cap + event[1]
            if want > self.cap:
                self._cell("reserve_grows")
                self.cap = want
                self._drop()
            else:
                self._cell("reserve_noop")
            return [("reserve", want)]
        if kind == "reset":
            self._store_cells("reset")
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

    def mmr_adjudicate(self, rel, cand_rows, picks, k, lam):
        return mmr_oracle.adjudicate(rel, self.x[np.asarray(cand_rows)], picks, k, lam)
