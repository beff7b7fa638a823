"""Case tables of the int8 cosine index's GPU tests (tests/test_cos8_forms_gpu.py), kept free of any GPU import so that
tests/test_cos8_cpu.py can check on any machine that the tables reach every kernel form.

expected_form() restates the dispatch of minivectordb_amd/csrc/cos8.hip (queries_per_pass, mfma_pass_ok, launch_scan,
launch_g, the k <= kMaxFusedK split) and rowset_is_bitmap() the list-or-bitmap rule of mvdb_cos8_rowset_create.  That the
restatement tells the truth is checked on the device by a kernel trace of the GPU file: profiles/cos8_forms_kernel_census.txt.
"""
import numpy as np

MAX_FUSED_K = 64      # kMaxFusedK (topk_device.hpp): above it the scan writes every score and the radix select runs
MFMA_MIN_NQ = 8       # kCos8MfmaMinNq
MAX_D = 4096          # 16 * kCos8MaxChunks
MAX_K = 1 << 20       # kCos8MaxK

FILTER_KINDS = ("none", "list", "bitmap", "excluded")
FILTER_FORM = {"none": 0, "list": 1, "bitmap": 2, "excluded": 2}

# (G, NCH) of cos8_scan_kernel by chunks per row, as launch_scan picks them
WIDTH_CLASSES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 4))


def nchunk_of(d):
    return (d + 15) // 16


def width_class(nchunk):
    if nchunk > 64:
        return (64, 4)
    g = 1
    while g < nchunk:
        g *= 2
    return (g, 1)


def rowset_is_bitmap(n, m, excluded):
    """mvdb_cos8_rowset_create: an excluded set is always a bitmap; a list of m rows becomes one when m * 8 >= n."""
    return bool(excluded) or m * 8 >= n


def expected_form(d, nq, k, filter_kind):
    """The kernel one search launches: ("mfma", F) or ("scan", G, NCH, Q, F, SCORES)."""
    nchunk = nchunk_of(d)
    F = FILTER_FORM[filter_kind]
    if k <= MAX_FUSED_K and nq >= MFMA_MIN_NQ and nchunk <= 64 and F != 1:
        return ("mfma", F)
    Q = 1 if nq == 1 else (4 if nchunk > 64 else 8)
    G, NCH = width_class(nchunk)
    return ("scan", G, NCH, Q, F, k > MAX_FUSED_K)


def all_scan_forms():
    out = set()
    for G, NCH in WIDTH_CLASSES:
        for Q in (1, 4 if NCH == 4 else 8):
            for F in (0, 1, 2):
                for scores in (False, True):
                    out.add(("scan", G, NCH, Q, F, scores))
    return out


def all_mfma_forms():
    return {("mfma", 0), ("mfma", 2)}


# One or more d per width class, both ends of a class where it has two.
CLASS_DIMS = ((16,), (17, 32), (33, 64), (100, 128), (200, 256), (400, 512), (1000, 1024), (1025, 2100, 4096))
_FUSED_KS = (1, 10, 64)
_SCORES_KS = (65, 200)
_NS = (4999, 3001, 6151)     # odd: the last block of the grid is short, the last wave step partial


def _rows_for(d, i):
    return 4101 if d > 2100 else (2501 if d > 1024 else _NS[i % 3])


def _build_cases():
    cases = []
    i = 0
    # the 96 scan forms: class x {single, batch} x filter x {lists, scores}; d, k, n and the two bitmap kinds rotate
    for dims in CLASS_DIMS:
        for single in (True, False):
            for fk in range(3):
                for scores in (False, True):
                    d = dims[i % len(dims)]
                    nq = 1 if single else (9 if d > 1024 else 5)
                    k = (_SCORES_KS if scores else _FUSED_KS)[(i // 2) % (2 if scores else 3)]
                    kind = ("none", "list", ("bitmap", "excluded")[i % 2])[fk]
                    cases.append((_rows_for(d, i), d, nq, k, kind))
                    i += 1
    # the other end of each class once more (batch, k = 10 and 65) so that no d of CLASS_DIMS depends on the rotation
    for dims in CLASS_DIMS:
        for d in dims:
            for extra in ((_rows_for(d, i), d, 9 if d > 1024 else 5, 10, "none"),
                          (_rows_for(d, i + 1), d, 1, 65, "excluded")):
                if extra not in cases:
                    cases.append(extra)
            i += 2
    # the matrix-core pass: nq >= 8, k <= 64, d <= 1024, every row or a bitmap.  Odd chunk counts read the zero pad in the
    # last half K-step; stride 272 is the first row of more than 8 K-steps.
    for kinds in (("none", "none"), ("bitmap", "excluded")):
        for j, (d, nq, k) in enumerate(((16, 8, 1), (1000, 33, 64), (256, 70, 64), (1024, 33, 1), (100, 8, 10),
                                        (400, 70, 10), (272, 33, 10), (32, 33, 64), (48, 70, 1), (512, 8, 64))):
            cases.append((_NS[j % 3], d, nq, k, kinds[j % 2]))
    return cases


CASES = _build_cases()


def case_id(case):
    n, d, nq, k, kind = case
    return f"n{n}-d{d}-nq{nq}-k{k}-{kind}"


def corpus(n, d, seed=0):
    """n x d Gaussian rows with four exact copies of row 1 in the middle, one at the end, and one zero row."""
    rng = np.random.default_rng(1000003 * d + n + seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 16:
        x[n // 3:n // 3 + 4] = x[1]
        x[n - 1] = x[1]
        x[n // 2] = 0.0
    return x


def queries(x, nq, seed=0):
    """nq Gaussian queries; the first equals stored row 1 (and so its copies: a tie at distance 0)."""
    n, d = x.shape
    rng = np.random.default_rng(7919 * d + nq + seed)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[0] = x[min(1, n - 1)]
    return q


def filter_rows(n, kind, seed=0):
    """(rows given to the row set, excluded flag, rows that remain selected) for a filter kind; None for "none"."""
    if kind == "none":
        return None, False, None
    rng = np.random.default_rng(n + 31 * FILTER_KINDS.index(kind) + seed)
    if kind == "list":        # few rows: m * 8 < n, with both ends of the index
        rows = np.union1d(rng.choice(n, n // 9, replace=False), [0, n - 1])
        return rows, False, rows
    if kind == "bitmap":      # an included list long enough to be stored as a bitmap
        rows = np.union1d(rng.choice(n, n // 2, replace=False), [0, n - 1])
        return rows, False, rows
    gone = np.union1d(rng.choice(n, 50, replace=False), [1, n // 3 + 1])   # the best hit of q[0] and one of its copies
    return gone, True, np.setdiff1d(np.arange(n), gone)


def special_rows(d, rng):
    """Rows at the quantiser's edges, as fp32 [m, d]: zero, subnormals, overflow of x * 127f, non-finite values, -0.0, huge
    and tiny scales, trunc boundaries, the neighbour of 1.0, a sum of squares beyond fp32."""
    f = np.float32
    rows = [np.zeros(d), np.eye(1, d, d // 2)[0], -np.eye(1, d, 0)[0], np.full(d, 1e-30), np.full(d, 3e30),
            np.full(d, 1e30), np.full(d, 1.0), np.full(d, 3e37), np.full(d, -2.5e-42), np.full(d, -0.0)]
    sub = rng.standard_normal(d)
    sub[d // 2] = 1e-41                    # one subnormal among normal values
    rows.append(sub)
    sub2 = np.full(d, 1e-39)               # subnormal, x * 127f is normal
    sub2[0] = -3e-39
    rows.append(sub2)
    b = rng.integers(-127, 128, d).astype(np.float64)
    rows += [b, b / 3.0, (b + 0.5) * 1e-3, b * 1e20]
    one = np.zeros(d)
    one[0] = 1.0
    if d > 1:
        one[1] = np.nextafter(f(1.0), f(2.0))
    rows.append(one)
    neg0 = rng.standard_normal(d)
    neg0[0] = -0.0
    rows.append(neg0)
    for bad in (np.nan, np.inf, -np.inf):  # one non-finite value: the magnitude is not finite, the row quantises to zero
        r = rng.standard_normal(d)
        r[d - 1] = bad
        rows.append(r)
    rows += list(rng.standard_normal((4, d)))
    with np.errstate(all="ignore"):
        return np.stack(rows).astype(np.float32)


SPECIAL_ZERO_ROWS = (0, 9, 18, 19, 20)    # rows of special_rows() whose codes are all zero: zero, -0.0, NaN, +inf, -inf
