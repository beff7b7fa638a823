"""The two-plane int8 prefilter against the same index with the route off, at the smallest sizes the
route serves.

`code8_scan_kernel` streams the plane of the top 6 bits of every code, stages the rows its first stage cannot reject, and
completes their integer sums from the plane of the low 2 bits, 64 staged rows at a time.  What can go wrong is what these
cases plant: rows that differ ONLY in the low plane (a), a wave whose stage fills several times, with the rows that must
win at the stage's 64th, 65th and last position (b), every writer of the two planes (c), and the candidate count of every
query against the count the one-plane prefilter of the parent commit kept for it (d: tests/golden/code8_candidate_counts.json,
written by record() below on an MI355X against a build of that commit; the zero-mean and all-positive families pin the
refined sums — on the clustered family the counts are the size of the query's cluster at every width and constrain little).  In every case D (as bits) and I must equal the
exact scan's, and no call may fall back unless the case forces it."""
import json
import os

import numpy as np
import pytest

from oracle import flat

DIMS = (384, 512, 1024)
SIZES = (500_001, 500_033)
FAMILIES = {"zero_mean": 0, "positive": flat.SYNTH_POSITIVE, "clustered": flat.SYNTH_CLUSTERED}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "code8_candidate_counts.json")
SEED = 131072   # the rows of the floor's sample: (slot * n) // SEED


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    return _native


def _query(d, flag=0, nq=1):
    q = flat.synth(nq, d, 5678 | flag)
    flat.normalize_l2(q)
    return q if nq > 1 else q[0]


def _index(native, d, n, flag=0, spare=0):
    idx = native.FlatIndex(d)
    idx.reserve(n + spare)
    idx.add_synthetic(n, 1234 | flag, normalize=True)
    return idx


def _off_then_on(native, idx, q, k, what, fallback=False, warm=3):
    idx.set_option("code8_single_query", 0)
    want = idx.search(q, k)
    idx.set_option("code8_single_query", 1)
    for _ in range(warm):   # the exact scan answers the first eligible queries after a change; the third builds the code
        idx.search(q, k)
    fallbacks = idx.code8_counters()[0]
    native.prof_enable(True)
    try:
        native.prof_read("ip_scan")
        got = idx.search(q, k)
        sym = native.prof_symbol("ip_scan")
        launches = native.prof_read("ip_scan")[0]
    finally:
        native.prof_enable(False)
    assert sym.startswith("code8_scan_kernel<"), (what, sym)
    assert launches == 1, (what, launches)
    assert idx.code8_rows == idx.ntotal, what
    if fallback is not None:
        assert idx.code8_counters()[0] - fallbacks == (1 if fallback else 0), (what, idx.code8_counters())
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    return got


# ---- (a) rows that differ only in the low plane ------------------------------------------------------------------------------------
def _low_plane_variants(q, m):
    """m rows a * c_j whose codes c_j agree with the codes of q in their top 6 bits and differ in the low 2."""
    d = q.shape[0]
    top = int(np.argmax(np.abs(q)))
    a = np.float32(np.abs(q[top]) / np.float32(127))
    c = np.clip(np.rint(q / a), -127, 127).astype(np.int64)
    H = c & ~3
    rows = []
    for j in range(m):
        low = np.random.default_rng(100 + j).integers(0, 4, d)
        low = np.where(H == -128, np.maximum(low, 1), low)   # (-128 is no code)
        cj = H + low
        cj[top] = c[top]                                      # the scale stays: one int8 step at the largest element is a
        rows.append((cj * np.float64(a)).astype(np.float32))
    rows = np.stack(rows)
    back = np.clip(np.rint(rows / (np.abs(rows).max(axis=1, keepdims=True) / np.float32(127))), -127, 127).astype(np.int64)
    assert ((back & ~3) == H).all() and len({r.tobytes() for r in (back & 3)}) == m
    return rows


def _planted_rows(n):
    """The last 9 rows, row 0, the first row of the last 64-row block, and 12 rows of the floor's sample.  With 12 planted
    rows in the sample the floor of k = 1 and k = 10 is a planted row's lower bound: every planted row then lies within
    a margin (about 0.008) of the floor, while the low plane carries up to 3 / 127 of a planted row's score (about 0.02) —
    a refinement that dropped or misplaced low bits would reject planted rows the exact scan returns.  (At k = 64 the
    floor is a synthetic row's and any T passes: there only (d) below pins the refined sum.)"""
    rows = list(range(n - 1, n - 10, -1)) + [0, ((n - 1) // 64) * 64] + [((77_777 + 1_001 * i) * n) // SEED for i in range(12)]
    return list(dict.fromkeys(rows))


@pytest.fixture(scope="module")
def planted_index(native):
    held = {}

    def get(d, n):
        if held.get("key") != (d, n):
            if "idx" in held:
                held.pop("idx").close()
            idx = _index(native, d, n)
            q = _query(d)
            rows = _planted_rows(n)
            idx.set_rows(np.asarray(rows, dtype=np.int64), _low_plane_variants(q, len(rows)))
            held.update(key=(d, n), idx=idx, rows=rows, q=q)
        return held["idx"], held["rows"], held["q"]

    yield get
    if "idx" in held:
        held.pop("idx").close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", DIMS)
def test_rows_that_differ_only_in_the_low_plane(native, planted_index, d, n, k):
    idx, rows, q = planted_index(d, n)
    D, I = _off_then_on(native, idx, q, k, f"d={d} n={n} k={k}")
    # (the planted rows score about 0.999, the best synthetic row about 0.25)
    m = min(k, len(rows))
    assert set(I.reshape(-1)[:m].tolist()) <= set(rows), (d, n, k, I, rows)
    if k >= len(rows):
        assert set(I.reshape(-1)[:len(rows)].tolist()) == set(rows), (d, n, k, I, rows)


# ---- (b) a wave whose refinement stage fills several times -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", ["positive", "clustered"])
@pytest.mark.parametrize("d", DIMS)
def test_dense_refinement(native, family, d):
    """Wave w of the launch takes the batches w, w + waves, ... (mvdb_code8_scan_geometry).  All rows of its first batches are
    replaced by (1 - j 2^-17) q: near-copies of the query, a margin apart from every other row and less than a margin from each
    other, so the first stage keeps them all and the wave stages them in batch order: 3 x 64 and one batch more (fewer
    where the wave has fewer batches: at least 64 and two batches more).  The best
    scores go to the batches that hold the stage's 64th, 65th and last entry."""
    n, k = 500_001, 64
    flag = FAMILIES[family]
    rb, waves = native.code8_scan_geometry(d, n)
    w = 5
    # three fills and one batch more, or as many full batches as the wave has at this n (d = 384: 4,096 waves of 16-row
    # batches leave a wave 8 batches — one fill, the 65th entry and a last one)
    nb = min(3 * 64 // rb + 1, (n // rb - 1 - w) // waves + 1)
    assert (w + (nb - 1) * waves + 1) * rb <= n and nb * rb >= 64 + 2 * rb, (rb, waves, nb)
    batches = [w + j * waves for j in range(nb)]
    # the order of merit: the batch of the 64th entry, of the 65th, the last, then the others
    first = [64 // rb - 1, 64 // rb, nb - 1]
    order = first + [j for j in range(nb) if j not in first]
    rows = [batches[j] * rb + i for j in order for i in range(rb)]
    q = _query(d, flag)
    x = np.stack([np.float32(1.0 - j * 2.0 ** -17) * q for j in range(len(rows))]).astype(np.float32)
    idx = _index(native, d, n, flag)
    idx.set_rows(np.asarray(rows, dtype=np.int64), x)
    D, I = _off_then_on(native, idx, q, k, f"dense {family} d={d}")
    # one more call of the route on its own: it refines every planted row (and whatever else of the corpus the first stage
    # keeps) — wave w staged all the planted rows, more than 64
    refined = idx.code8_refined()
    idx.search(q, k)
    delta = idx.code8_refined() - refined
    print(f"dense {family} d={d}: rows per batch {rb}, waves {waves}, planted {len(rows)}, refined in one call {delta}, "
          f"candidates {idx.code8_counters()[1]}")
    assert delta >= len(rows), (delta, len(rows))
    assert idx.code8_counters()[1] >= len(rows)
    got = I.reshape(-1).tolist()
    assert set(got[:3 * rb]) == set(rows[:3 * rb]), (got, rows[:3 * rb])
    assert set(got) <= set(rows)
    idx.close()


# ---- (c) every writer of the planes ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_writers(native, d):
    n, k = 500_033, 10
    idx = _index(native, d, n, spare=64)
    q = _query(d)
    _off_then_on(native, idx, q, k, "fresh")
    # set_rows after the build: rows of the partial batch and a row of the floor's sample
    variants = _low_plane_variants(q, 4)
    slot_row = (33_333 * n) // SEED
    idx.set_rows(np.array([n - 1, n - 2, slot_row], np.int64), variants[:3])
    _, I = _off_then_on(native, idx, q, k, "set_rows", warm=0)
    assert set(I.reshape(-1)[:3].tolist()) == {n - 1, n - 2, slot_row}
    # add into reserved space: the planes' offsets go by capacity, nothing moves
    extra = flat.synth(37, d, 99)
    flat.normalize_l2(extra)
    extra[5] = variants[3]
    idx.add(extra)
    assert idx.code8_rows == idx.ntotal == n + 37
    _, I = _off_then_on(native, idx, q, k, "add 37", warm=0)
    assert n + 5 in I.reshape(-1)[:4].tolist()
    # remove_rows drops the code; the third query rebuilds it
    idx.remove_rows(np.array([3, n - 1], np.int64))
    assert idx.code8_rows == 0
    _off_then_on(native, idx, q, k, "remove_rows")
    # a row with a NaN element (through the device normalisation: the norm bound stays known): always a candidate
    idx.set_rows(np.array([1234], np.int64), np.full((1, d), np.nan, np.float32), normalize=True)
    _off_then_on(native, idx, q, k, "NaN row", warm=0)
    # the zero query
    _off_then_on(native, idx, np.zeros(d, np.float32), k, "zero query", warm=0, fallback=None)   # (every row is a candidate)
    # a capacity that cannot hold the candidates: the gated exact scan answers
    idx.set_option("code8_capacity", 16)
    _off_then_on(native, idx, q, 64, "capacity 16", warm=0, fallback=True)
    idx.set_option("code8_capacity", 32768)
    idx.close()


# ---- (d) the candidate counts of the parent's one-plane prefilter -------------------------------------------------------------------
def _candidate_counts(native, family, d):
    n, k = 500_001, 10
    flag = FAMILIES[family]
    idx = _index(native, d, n, flag)
    q = _query(d, flag, nq=8)
    idx.set_option("code8_single_query", 1)
    for _ in range(3):
        idx.search(q[0], k)
    assert idx.code8_rows == n
    counts = []
    for qi in q:
        idx.search(qi, k)
        counts.append(int(idx.code8_counters()[1]))
    idx.close()
    return counts


def record(path=GOLDEN):
    """Writes the golden file: run on an MI355X against a build of the parent commit (the one-plane prefilter)."""
    from minivectordb_amd import _native
    out = {f"{family}/{d}": _candidate_counts(_native, family, d) for family in sorted(FAMILIES) for d in DIMS}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_candidate_counts_equal_the_one_plane_prefilter(native, family, d):
    with open(GOLDEN) as f:
        want = json.load(f)[f"{family}/{d}"]
    got = _candidate_counts(native, family, d)
    print(f"code8 planes {family} d={d}: candidates {got}, golden {want}")
    assert got == want, (family, d, got, want)
