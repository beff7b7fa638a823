"""CPU restatement of the int8 cosine contract (include/mvdb.h "int8 cosine index").

quantize:  mag = sqrt(sum_i (double)x_i^2) summed column by column in index order in fp64;
           code_i = trunc((double)(float)(x_i * 127f) / mag) clamped to [-127, 127]; mag 0 or not finite -> zeros.
distance:  0 when a2 == b2 == 0; 1 when exactly one is 0 or ab == 0; else (float)(1 - ab / sqrt(a2 * b2)) in fp64.
search:    ascending fp32 distance, ties to the lower row; missing slots -1 / +FLT_MAX.

Integer dot products of int8 codes are exact in fp64 (and in an fp32 BLAS for d <= 1024: |partial sums| < 2^24), so
the oracle is exact and fast enough for millions of rows.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def quantize(x):
    """fp32 [n, d] -> (codes int8 [n, d], a2 int32 [n])."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    n, d = x.shape
    mag2 = np.zeros(n, dtype=np.float64)
    for i in range(d):
        col = x[:, i].astype(np.float64)
        mag2 += col * col
    with np.errstate(all="ignore"):
        mag = np.sqrt(mag2)
        ok = (mag > 0) & np.isfinite(mag)
        prod = (x * np.float32(127.0)).astype(np.float64)
        t = np.trunc(prod / np.where(ok, mag, 1.0)[:, None])
    t = np.clip(t, -127.0, 127.0)
    t[~ok] = 0.0
    codes = t.astype(np.int8)
    a2 = (codes.astype(np.int32) ** 2).sum(axis=1, dtype=np.int64).astype(np.int32)
    return codes, a2


def dots(qcodes, codes, exact_f32=None):
    """ab[nq, n] as int64.  exact_f32 (default: d <= 1024) uses an fp32 matmul, which is exact there."""
    d = codes.shape[1]
    if exact_f32 is None:
        exact_f32 = d <= 1024
    dt = np.float32 if exact_f32 else np.float64
    return (qcodes.astype(dt) @ codes.astype(dt).T).astype(np.int64)


def distance(ab, a2, b2):
    """Vectorised contract distance: ab [nq, n] int, a2 [n], b2 [nq] -> float32 [nq, n]."""
    ab = np.asarray(ab, dtype=np.int64)
    A = np.asarray(a2, dtype=np.int64)[None, :]
    B = np.asarray(b2, dtype=np.int64)[:, None]
    with np.errstate(all="ignore"):
        v = 1.0 - ab.astype(np.float64) / np.sqrt(A.astype(np.float64) * B.astype(np.float64))
    out = v.astype(np.float32)
    one = (A == 0) | (B == 0) | (ab == 0)
    out = np.where(one, np.float32(1.0), out)
    out = np.where((A == 0) & (B == 0), np.float32(0.0), out)
    return out.astype(np.float32)


def topk_from_distances(dist, k, rows=None):
    """dist float32 [nq, m] over `rows` (default arange(m)) -> (D [nq, k], I [nq, k]) ascending, ties to the lower row."""
    nq, m = dist.shape
    rows = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    D = np.full((nq, k), FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    take = min(k, m)
    for i in range(nq):
        kth = np.partition(dist[i], take - 1)[take - 1]
        cand = np.nonzero(dist[i] <= kth)[0]
        order = cand[np.lexsort((rows[cand], dist[i, cand]))][:take]
        D[i, :take] = dist[i, order]
        I[i, :take] = rows[order]
    return D, I


def search(codes, a2, q, k, rows=None):
    """Exact search of fp32 queries q [nq, d] over stored codes/a2, optionally restricted to `rows` (sorted)."""
    qc, qb2 = quantize(q)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        codes, a2 = codes[rows], a2[rows]
    dist = distance(dots(qc, codes), a2, qb2)
    return topk_from_distances(dist, k, rows)


def search_chunked(codes, a2, q, k, chunk=1 << 20):
    """search() for corpora too large for one [nq, n] distance matrix: per-chunk top-k, merged (ties to the lower row)."""
    qc, qb2 = quantize(q)
    nq = qc.shape[0]
    bestD = np.full((nq, 0), FLT_MAX, dtype=np.float32)
    bestI = np.full((nq, 0), -1, dtype=np.int64)
    for r0 in range(0, codes.shape[0], chunk):
        c = codes[r0:r0 + chunk]
        dist = distance(dots(qc, c), a2[r0:r0 + chunk], qb2)
        D, I = topk_from_distances(dist, k, np.arange(r0, r0 + c.shape[0]))
        bestD = np.concatenate([bestD, D], axis=1)
        bestI = np.concatenate([bestI, I], axis=1)
        Dm, Im = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
        for i in range(nq):
            key_rows = np.where(bestI[i] < 0, np.iinfo(np.int64).max, bestI[i])
            order = np.lexsort((key_rows, bestD[i]))[:k]
            Dm[i], Im[i] = bestD[i, order], bestI[i, order]
        bestD, bestI = Dm, Im
    return bestD, bestI


# ---- per-element restatement (pure Python scalars): the oracle's own check ----------------------------------------
def quantize_scalar(row):
    row = [np.float32(v) for v in row]
    mag2 = 0.0
    for v in row:
        mag2 = mag2 + float(v) * float(v)
    mag = float(np.sqrt(mag2))
    if not (mag > 0.0) or not np.isfinite(mag):
        return [0] * len(row)
    out = []
    for v in row:
        with np.errstate(over="ignore"):
            p = float(np.float32(v * np.float32(127.0)))
        t = p / mag
        t = float(np.trunc(t))
        out.append(int(max(-127.0, min(127.0, t))))
    return out


def distance_scalar(ab, a2, b2):
    if a2 == 0 and b2 == 0:
        return np.float32(0.0)
    if a2 == 0 or b2 == 0 or ab == 0:
        return np.float32(1.0)
    return np.float32(1.0 - float(ab) / float(np.sqrt(float(a2) * float(b2))))


class OracleCos8Index:
    """Cos8Index (minivectordb_amd._native) restated on this oracle: what the device computes, bit for bit
    (tests/test_cos8_gpu.py).  Lets the database class run without a GPU."""

    def __init__(self, d, device=0):
        self.d = d
        self.codes = np.zeros((0, d), np.int8)
        self.a2 = np.zeros(0, np.int32)

    @property
    def ntotal(self):
        return self.codes.shape[0]

    def add(self, x, normalize=None):
        c, a = quantize(np.atleast_2d(x))
        self.codes = np.concatenate([self.codes, c])
        self.a2 = np.concatenate([self.a2, a])

    def remove_rows(self, rows):
        self.codes = np.delete(self.codes, rows, axis=0)
        self.a2 = np.delete(self.a2, rows)

    def reset(self):
        self.__init__(self.d)

    def search(self, q, k, normalize_q=None):
        return search(self.codes, self.a2, np.atleast_2d(q), k)

    def rowset(self, rows, excluded=False):
        rows = np.asarray(rows, np.int64)
        return np.setdiff1d(np.arange(self.ntotal), rows) if excluded else np.sort(rows)

    def search_rowset(self, q, k, rowset, normalize_q=None):
        return search(self.codes, self.a2, np.atleast_2d(q), k, rows=rowset)
