"""MMR search on the device (mvdb_index_search_mmr, csrc/mmr_select.hpp) against the float64 oracle of tests/mmr_oracle.py.

Corpus: 4096 rows, 64 Gaussian cluster centres + 0.35 noise (row i belongs to cluster i % 64), normalised on add; rows
100-109 and the last 5 are copies of row 99.  Queries: perturbed stored rows (cosine ~0.96 to their row); query 1 IS row 99,
query 2 sits near it.

Two statements of the issue hold only away from a query that is itself a stored row, and are asserted accordingly:
  - With the query ON its first pick p, rel[j] = q.x_j and s(p, j) = x_p.x_j are the same number, so at lambda = 0.5 every
    objective of step 1 is 0 up to rounding: whatever is picked there — a second copy included — is within tau of the
    best, and the plain top-k order passes the adjudicator.  The non-vacuity assertion (the order 0..k-1 fails the
    adjudicator) needs k >= 2 (k = 1 has one answer) and covers every query but the two aimed at row 99: near it, too, the
    16 copies lead the candidates with ONE objective between them, and where that objective beats the other candidates'
    (d = 100 at fetch_k = 20) the copies in order ARE the float64 answer.
  - "No second copy while a candidate from another cluster remains" is checked as stated for query 1, with the cluster of
    every candidate known from the construction; on this corpus the candidates of the lambda = 0.5 shapes (at most 64) all
    come from row 99's own cluster of 64 + copies, so no pick is ever constrained by it.  For query 2, where the copies'
    objective (0.5 * 0.96 - 0.5 * 1) is decided by more than rounding, the adjudicator forces the same thing step by step.
"""
import numpy as np
import pytest

import mmr_oracle

pytestmark = pytest.mark.gpu

N, CLUSTERS, NQ_MAX = 4096, 64, 33
COPIES = list(range(99, 110)) + list(range(N - 5, N))
DIMS = [30, 64, 100, 384, 512, 1024, 2048]
SHAPES = [(20, 5, 0.5), (40, 10, 0.5), (64, 64, 0.5), (256, 64, 0.3), (1024, 32, 0.7), (8, 1, 0.5)]   # (fetch_k, k, lambda)
NQS = [1, 3, 33]
MISSING = np.float32(-3.4028234663852886e38)
EXACT_COPY_QUERY = 1
AIMED_AT_THE_COPIES = (1, 2)


def make_corpus(d):
    rng = np.random.default_rng(1000 + d)
    centres = rng.standard_normal((CLUSTERS, d)).astype(np.float32)
    cluster = np.arange(N) % CLUSTERS
    x = centres[cluster] + np.float32(0.35) * rng.standard_normal((N, d)).astype(np.float32)
    x[COPIES] = x[99]
    cluster[COPIES] = cluster[99]
    return x, cluster, rng


def make_queries(stored, rng):
    d = stored.shape[1]
    rows = rng.permutation(np.setdiff1d(np.arange(N), COPIES))[:NQ_MAX]
    rows[list(AIMED_AT_THE_COPIES)] = 99
    q = stored[rows] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((NQ_MAX, d)).astype(np.float32)
    q[EXACT_COPY_QUERY] = stored[99]
    return np.ascontiguousarray(q, dtype=np.float32)


_WORLDS = {}


class World:
    """One index per width, built once: the stored rows as the device holds them, the queries, and the candidate searches
    (computed once per (nq, fetch_k, set) and never written to)."""

    def __init__(self, d):
        from minivectordb_amd import _native
        x, self.cluster, rng = make_corpus(d)
        self.d = d
        self.idx = _native.FlatIndex(d)
        self.idx.add(x, normalize=True)
        self.stored = self.idx.get_rows(0, N)
        self.q = make_queries(self.stored, rng)
        self.sets = {}
        self._cand = {}

    def rowset(self, kind):
        if kind not in self.sets:
            rng = np.random.default_rng(7)
            if kind == "sorted":
                rows = np.arange(0, N, 3, dtype=np.int64)                       # holds 99, 102, 105, 108, 4092, 4095
            elif kind == "unsorted":
                rows = rng.permutation(N)[:1500].astype(np.int64)
                rows = np.concatenate([np.array(COPIES[::-1], np.int64), rows[~np.isin(rows, COPIES)]])   # the copies, highest row first
            elif kind == "dense":
                rows = np.setdiff1d(np.arange(N, dtype=np.int64), np.arange(5, N, 40))      # 97.5 % of the rows, sorted: a bitmap
            elif kind == "excluded":
                rows = np.array([99, 100, 7, 4095], np.int64)
            elif kind == "twelve":
                rows = np.array([99, 5, 100, 4095, 17, 163, 227, 291, 1000, 2000, 3000, 35], np.int64)
            elif kind == "empty":
                rows = np.empty(0, np.int64)
            rs = self.idx.rowset(rows, excluded=kind == "excluded")
            self.sets[kind] = (rs, rows)
        return self.sets[kind]

    def candidates(self, nq, fetch_k, kind=None):
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


def world(d):
    if d not in _WORLDS:
        _WORLDS[d] = World(d)
    return _WORLDS[d]


def check_against_candidates(D, I, Dc, Ic, k, what):
    """Candidates and scores: labels distinct, a subset of the candidate row, the first label first, the scores the very
    bits of the search; padding exactly behind min(k, valid candidates) picks.  Returns the picks as candidate positions."""
    out = []
    for i in range(I.shape[0]):
        valid = int((Ic[i] >= 0).sum())
        npick = min(k, valid)
        assert (I[i, npick:] == -1).all() and (D[i, npick:] == MISSING).all(), (what, i)
        labels = I[i, :npick]
        assert (labels >= 0).all() and len(set(labels.tolist())) == npick, (what, i, labels)
        pos_of = {int(r): j for j, r in enumerate(Ic[i, :valid])}
        assert len(pos_of) == valid
        assert set(labels.tolist()) <= set(pos_of), (what, i)
        picks = [pos_of[int(r)] for r in labels]
        if npick:
            assert labels[0] == Ic[i, 0], (what, i)
        assert np.array_equal(D[i, :npick].view(np.uint32), Dc[i, picks].view(np.uint32)), (what, i)
        out.append(picks)
    return out


def adjudicate_all(w, picks, Dc, Ic, k, lam, what, non_vacuity):
    worst = 0.0
    for i, p in enumerate(picks):
        valid = int((Ic[i] >= 0).sum())
        rel, rows = Dc[i, :valid], w.stored[Ic[i, :valid]]
        ok, msg, deficit = mmr_oracle.adjudicate(rel, rows, p, k, lam)
        print(f"{what} query {i}: deficit {deficit:.3e} (tau {mmr_oracle.tau(rows):.3e})")
        assert ok, (what, i, msg)
        worst = max(worst, deficit)
        if non_vacuity and i not in AIMED_AT_THE_COPIES:
            plain_ok, _, _ = mmr_oracle.adjudicate(rel, rows, list(range(min(k, valid))), k, lam)
            assert not plain_ok, (what, i, "the plain top-k order passes the adjudicator: the check would be vacuous")
    return worst


def check_duplicates(w, picks, Ic, lam, what):
    """Query 1 is row 99: the lowest of the 16 identical rows first; copies in candidate order; at lambda = 0.5 no second
    copy while a valid candidate from another cluster remains."""
    p, cand = picks[EXACT_COPY_QUERY], Ic[EXACT_COPY_QUERY]
    valid = int((cand >= 0).sum())
    is_copy = np.isin(cand[:valid], COPIES)
    assert cand[0] == 99 and p[0] == 0, what
    copy_picks = [j for j in p if is_copy[j]]
    assert copy_picks == sorted(copy_picks), (what, copy_picks)            # position order = row order (sorted candidates tie by row)
    rows_in_order = [int(cand[j]) for j in copy_picks]
    assert rows_in_order == sorted(rows_in_order), (what, rows_in_order)
    constrained = 0
    if lam == 0.5:
        other = w.cluster[cand[:valid]] != w.cluster[99]
        left = np.ones(valid, bool)
        seen_copy = False
        for j in p:
            if is_copy[j] and seen_copy:
                constrained += int((other & left).any())
                assert not (other & left).any(), (what, "a second copy was picked while another cluster's candidate remained")
            seen_copy |= bool(is_copy[j])
            left[j] = False
    return constrained


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"f{s[0]}k{s[1]}l{s[2]}")
@pytest.mark.parametrize("d", DIMS)
def test_selection_against_the_float64_oracle(gpu, d, shape):
    fetch_k, k, lam = shape
    w = world(d)
    for nq in NQS:
        what = f"d={d} fetch_k={fetch_k} k={k} lambda={lam} nq={nq}"
        Dc, Ic = w.candidates(nq, fetch_k)
        D, I = w.idx.search_mmr(w.q[:nq], k, fetch_k, lam, normalize_q=True)
        picks = check_against_candidates(D, I, Dc, Ic, k, what)
        adjudicate_all(w, picks, Dc, Ic, k, lam, what, non_vacuity=lam < 1 and 2 <= k < fetch_k)
        if fetch_k == k:
            assert all(sorted(p) == list(range(k)) for p in picks), what      # a permutation of the candidates
        if nq > EXACT_COPY_QUERY:
            check_duplicates(w, picks, Ic, lam, what)
        # lambda = 1: the first k columns of the candidate search, bit for bit
        D1, I1 = w.idx.search_mmr(w.q[:nq], k, fetch_k, 1.0, normalize_q=True)
        assert np.array_equal(I1, Ic[:, :k]) and np.array_equal(D1.view(np.uint32), Dc[:, :k].view(np.uint32)), what
        # reproducible: a second call returns the same bits
        D2, I2 = w.idx.search_mmr(w.q[:nq], k, fetch_k, lam, normalize_q=True)
        assert np.array_equal(I2, I) and np.array_equal(D2.view(np.uint32), D.view(np.uint32)), what


def test_forms(gpu):
    from minivectordb_amd import _native
    form = _native.FlatIndex.mmr_form
    for d in DIMS:
        assert form(d, 1024) == 1, d
        if d <= 512:
            assert form(d, 20) == 0, d
    assert form(2048, 256) == 1
    covered = {(d, form(d, f)) for d in DIMS for f, _, _ in SHAPES}
    exist = {(d, v) for d in DIMS for f in range(1, 1025) for v in [form(d, f)]}
    assert covered == exist and {d for d, v in exist if v == 0} == set(DIMS) == {d for d, v in exist if v == 1}, sorted(exist - covered)
    # the rule looks at the row stride: d = 30 is stored at stride 32
    assert [form(30, f) for f in range(1, 1025)] == [form(32, f) for f in range(1, 1025)]
    for bad in ((0, 20), (64, 0), (64, 1025)):
        with pytest.raises(ValueError):
            form(*bad)


@pytest.mark.parametrize("d", [100, 512])
def test_row_sets(gpu, d):
    w = world(d)
    for kind in ("sorted", "unsorted", "dense", "excluded"):
        rs, rows = w.rowset(kind)
        assert rs.is_bitmap == (kind in ("dense", "excluded")), kind
        for fetch_k, k, lam in ((20, 5, 0.5), (256, 64, 0.3)):
            for nq in (1, 3):
                what = f"d={d} set={kind} fetch_k={fetch_k} k={k} nq={nq}"
                Dc, Ic = w.candidates(nq, fetch_k, kind)
                D, I = w.idx.search_mmr(w.q[:nq], k, fetch_k, lam, rowset=rs, normalize_q=True)
                picks = check_against_candidates(D, I, Dc, Ic, k, what)
                adjudicate_all(w, picks, Dc, Ic, k, lam, what, non_vacuity=False)
                selected = np.setdiff1d(np.arange(N), rows) if kind == "excluded" else rows
                assert np.isin(I, selected).all(), what
        # ties go to the candidate position: for the unsorted list that is the LIST position (the copies stand highest row first)
        Dc, Ic = w.candidates(3, 256, kind)
        D, I = w.idx.search_mmr(w.q[:3], 64, 256, 0.3, rowset=rs, normalize_q=True)
        got = [int(r) for r in I[EXACT_COPY_QUERY] if r in COPIES]
        in_set = [int(r) for r in Ic[EXACT_COPY_QUERY] if r in COPIES]
        assert in_set == ([r for r in COPIES[::-1]] if kind == "unsorted" else sorted(in_set)) and len(in_set) >= 6, (kind, in_set)
        assert I[EXACT_COPY_QUERY, 0] == in_set[0] and got == in_set[:len(got)], (kind, got, in_set)
    # a 12-row list: 12 picks, then missing markers; the empty set: markers only
    rs, rows = w.rowset("twelve")
    Dc, Ic = w.candidates(3, 40, "twelve")
    D, I = w.idx.search_mmr(w.q[:3], 20, 40, 0.5, rowset=rs, normalize_q=True)
    picks = check_against_candidates(D, I, Dc, Ic, 20, "twelve")
    assert all(sorted(I[i, :12].tolist()) == sorted(rows.tolist()) and (I[i, 12:] == -1).all() and (D[i, 12:] == MISSING).all()
               for i in range(3))
    adjudicate_all(w, picks, Dc, Ic, 20, 0.5, "twelve", non_vacuity=False)
    rs, _ = w.rowset("empty")
    D, I = w.idx.search_mmr(w.q[:3], 5, 20, 0.5, rowset=rs, normalize_q=True)
    assert (I == -1).all() and (D == MISSING).all()


@pytest.mark.parametrize("d", DIMS)
def test_a_batch_row_equals_the_single_call(gpu, d):
    w = world(d)
    identical = 0
    for fetch_k, k, lam in ((20, 5, 0.5), (256, 64, 0.3)):
        Dc, Ic = w.candidates(3, fetch_k)
        D, I = w.idx.search_mmr(w.q[:3], k, fetch_k, lam, normalize_q=True)
        for i in range(3):
            D1c, I1c = w.idx.search(w.q[i:i + 1], fetch_k, normalize_q=True)
            D1, I1 = w.idx.search_mmr(w.q[i:i + 1], k, fetch_k, lam, normalize_q=True)
            if np.array_equal(I1c[0], Ic[i]) and np.array_equal(D1c[0].view(np.uint32), Dc[i].view(np.uint32)):
                identical += 1
                assert np.array_equal(I1[0], I[i]) and np.array_equal(D1[0].view(np.uint32), D[i].view(np.uint32)), (d, fetch_k, i)
    if d in (30, 100):      # no matrix-core pass at these widths: three queries take the per-query scan, as one does
        assert identical == 6, (d, identical)
    print(f"d={d}: {identical} of 6 (query, shape) pairs had identical candidates in the nq=3 and nq=1 calls")


def test_device_variant_label_offset_graph_and_repeat(gpu):
    import torch
    d, nq, off = 384, 3, 10 ** 6
    w = world(d)
    stream = torch.cuda.Stream()
    qt = torch.from_numpy(w.q[:nq]).cuda()
    for (fetch_k, k, lam), kind in (((40, 10, 0.5), None), ((256, 64, 0.3), "sorted"), ((1024, 32, 0.7), None)):
        rs = w.rowset(kind)[0] if kind else None
        Dw, Iw = w.idx.search_mmr(w.q[:nq], k, fetch_k, lam, rowset=rs, normalize_q=True)
        Dt = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        It = torch.zeros((nq, k), dtype=torch.int64, device="cuda")

        def enqueue(offset):
            w.idx.search_mmr_device(qt.data_ptr(), nq, k, fetch_k, lam, Dt.data_ptr(), It.data_ptr(), rowset=rs,
                                    stream=stream.cuda_stream, normalize_q=True, label_offset=offset)

        def check(offset, what):
            assert np.array_equal(Dt.cpu().numpy().view(np.uint32), Dw.view(np.uint32)), what
            assert np.array_equal(It.cpu().numpy(), np.where(Iw >= 0, Iw + offset, -1)), what

        torch.cuda.synchronize()
        for offset in (0, off, off):                      # the label offset shifts labels only; two calls in a row: the same bits
            with torch.cuda.stream(stream):
                enqueue(offset)
            stream.synchronize()
            check(offset, f"eager fetch_k={fetch_k} offset={offset}")
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            enqueue(off)
        for r in range(2):
            Dt.zero_()
            It.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            check(off, f"replay {r} fetch_k={fetch_k}")


def test_non_finite_rows(gpu):
    from minivectordb_amd import _native
    n, d, col = 300, 64, 3
    x, _, rng = make_corpus(d)
    x = x[:n] / np.linalg.norm(x[:n], axis=1, keepdims=True)
    x[:, col] = np.abs(x[:, col]) + np.float32(0.01)            # no zero meets the infinity: its products are +-inf, never NaN
    x[20, 5] = np.nan
    x[21, col] = np.inf
    idx = _native.FlatIndex(d)
    idx.add(x, normalize=False)
    stored = idx.get_rows(0, n)
    listed = idx.rowset(np.arange(10, 40, dtype=np.int64))
    for sign in (-1.0, 1.0):                                     # the infinite row scores -inf (last candidate) / +inf (first)
        q = (x[25] + 0.05 * rng.standard_normal(d)).astype(np.float32)
        q[col] = sign * abs(q[col])
        for rs, fetch_k, k in ((listed, 40, 30), (None, n, n), (None, 64, 20)):
            what = f"sign={sign} fetch_k={fetch_k} set={rs is not None}"
            Dc, Ic = (idx.search_rowset(q, fetch_k, rs) if rs else idx.search(q, fetch_k))
            assert 20 not in Ic and (21 in Ic) == (rs is not None or fetch_k == n or sign > 0), what
            D, I = idx.search_mmr(q, k, fetch_k, 0.5, rowset=rs)
            picks = check_against_candidates(D, I, Dc, Ic, k, what)[0]
            valid = int((Ic[0] >= 0).sum())
            rel, rows = Dc[0, :valid], stored[Ic[0, :valid]]
            ok, msg, _ = mmr_oracle.adjudicate(rel, rows, picks, k, 0.5)
            assert ok, (what, msg)
            if sign < 0:     # every pick with a finite float64 objective precedes every pick without one
                finite = np.isfinite(mmr_oracle.objective_trace(rel, rows, picks, 0.5))
                assert finite.any() and finite.all() == (21 not in I), (what, finite)
                assert finite.all() or not finite[np.argmin(finite):].any(), (what, finite)
    idx.close()


def test_errors_and_the_empty_index(gpu):
    from minivectordb_amd import _native
    w = world(64)
    q = w.q[:2]
    for k, fetch_k, lam in ((0, 20, 0.5), (21, 20, 0.5), (5, 1025, 0.5), (5, 20, -0.1), (5, 20, 1.5), (5, 20, float("nan"))):
        with pytest.raises(ValueError):
            w.idx.search_mmr(q, k, fetch_k, lam)
    with pytest.raises(ValueError):
        w.idx.search_mmr(w.q[:2, :32], 5, 20, 0.5)
    l2 = _native.FlatIndex(64, metric=_native.METRIC_L2)
    l2.add(w.stored[:100])
    with pytest.raises(ValueError, match="inner-product"):
        l2.search_mmr(q, 5, 20, 0.5)
    l2.close()
    empty = _native.FlatIndex(64)
    D, I = empty.search_mmr(q, 5, 20, 0.5)
    assert (I == -1).all() and (D == MISSING).all()
    empty.close()
    # a stale set (rows renumbered by a removal) and a foreign one: ValueError, the output arrays untouched
    mine = _native.FlatIndex(64)
    mine.add(w.stored[:500])
    rs = mine.rowset(np.arange(0, 500, 2, dtype=np.int64))
    D = np.full((2, 5), 7.0, np.float32)
    I = np.full((2, 5), 7, np.int64)
    with pytest.raises(ValueError, match="another index"):
        w.idx.search_mmr(q, 5, 20, 0.5, rowset=rs, out=(D, I))
    mine.search_mmr(q, 5, 20, 0.5, rowset=rs)
    mine.remove_rows(np.array([3], np.int64))
    with pytest.raises(ValueError, match="another state"):
        mine.search_mmr(q, 5, 20, 0.5, rowset=rs, out=(D, I))
    assert (D == 7.0).all() and (I == 7).all()
    mine.close()


def _metadata(n):
    return [{"tenant": i % 4, "lang": ("en", "de", "fr")[i % 3], "row": i} for i in range(n)]


PY_FILTERS = [{}, {"metadata_filter": {"tenant": 1}}, {"exclude_filter": {"lang": "de"}},
              {"or_filters": [{"tenant": 2}, {"tenant": 3}]}, {"metadata_filter": {"tenant": 0, "lang": "en"}},
              {"metadata_filter": {"tenant": 9}}]


@pytest.mark.parametrize("kind", ["flat", "sharded"])
def test_drop_in_classes(tmp_path, gpu, kind):
    from minivectordb_amd import ShardedVectorDatabase, VectorDatabase
    n, d = 2000, 128
    if kind == "flat":
        db = VectorDatabase(storage_file=str(tmp_path / "m.pkl"))
    else:
        db = ShardedVectorDatabase(storage_dir=str(tmp_path / "s"), shard_size=512)
    rng = np.random.default_rng(61)
    centres = rng.standard_normal((16, d)).astype(np.float32)
    x = centres[np.arange(n) % 16] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32)
    meta = _metadata(n)
    db.store_embeddings_batch(list(range(n)), x, meta)
    q = (x[[5, 70, 333]] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((3, d))).astype(np.float32)
    nonempty = 0
    for f in PY_FILTERS:
        rows = np.array(sorted(db.find_most_similar(q[0], k=n, **f)[0]), np.int64)      # the filter's rows (ids are row numbers here)
        assert (rows.size == n) == (not f) and all(
            (f.get("metadata_filter", {}).items() <= meta[r].items()) for r in rows[:50] if "metadata_filter" in f)
        many = db.find_most_similar_mmr_batch(q, k=6, fetch_k=30, lambda_mult=0.4, **f)
        for i in range(3):
            got = db.find_most_similar_mmr(q[i], k=6, fetch_k=30, lambda_mult=0.4, **f)
            assert list(many[i][0]) == list(got[0]) and list(many[i][2]) == list(got[2])                     # _batch equals the loop
            # (the scores of a batch are those of ITS candidate search: three queries at d = 128 share a matrix-core pass, whose
            #  summation order is not the single query's — the batch contract of mvdb_index_search, a few ulp)
            assert np.allclose(np.asarray(many[i][1], np.float32), np.asarray(got[1], np.float32), rtol=0, atol=1e-6)
            if rows.size == 0:
                assert got == ([], [], [])
                continue
            nonempty += 1
            # only rows of the filter, in the order of FlatIndex.search_mmr over the filter's rows
            rs = db.index.rowset(rows) if rows.size < n else None
            Dw, Iw = db.index.search_mmr(q[i], min(6, rows.size), min(30, rows.size), 0.4, rowset=rs, normalize_q=True)
            assert list(got[0]) == Iw[0].tolist() and set(got[0]) <= set(rows.tolist()), (f, i)
            assert [m["row"] for m in got[2]] == list(got[0]) and all(type(s) is np.float32 for s in got[1])
            assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), Dw[0].view(np.uint32)), (f, i)
            plain = db.find_most_similar(q[i], k=6, **f)
            one = db.find_most_similar_mmr(q[i], k=6, fetch_k=30, lambda_mult=1.0, **f)                      # lambda_mult = 1: the plain search
            assert list(one[0]) == list(plain[0]) and list(one[2]) == list(plain[2])
            assert np.array_equal(np.asarray(one[1], np.float32).view(np.uint32), np.asarray(plain[1], np.float32).view(np.uint32))
    assert nonempty == 15
    # the default fetch_k is max(4 k, 20)
    for k in (3, 8):
        a = db.find_most_similar_mmr(q[1], k=k)
        b = db.find_most_similar_mmr(q[1], k=k, fetch_k=max(4 * k, 20))
        c = db.find_most_similar_mmr(q[1], k=k, fetch_k=max(4 * k, 20) + 17)
        assert list(a[0]) == list(b[0]) and len(a[0]) == k
        print(f"k={k}: default {list(a[0])}, fetch_k + 17 {list(c[0])}")
    with pytest.raises(ValueError):
        db.find_most_similar_mmr(q[0], k=40, fetch_k=30)


def test_the_usearch_class_raises(tmp_path, gpu):
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    db = ShardedVectorDatabaseUsearch(storage_dir=str(tmp_path / "u"), shard_size=512)
    x = np.random.default_rng(62).standard_normal((200, 128)).astype(np.float32)
    db.store_embeddings_batch(list(range(200)), x, _metadata(200))
    with pytest.raises(NotImplementedError, match="MMR search"):
        db.find_most_similar_mmr(x[0])
    with pytest.raises(NotImplementedError, match="MMR search"):
        db.find_most_similar_mmr_batch(x[:2])
    assert len(db.find_most_similar(x[0], k=3)[0]) == 3
