"""The contract of assignment and spherical k-means as a few lines of numpy (include/mvdb.h "ASSIGN AND K-MEANS").

assign     a [C, n] score matrix -> per row the vector with the largest score.  Scores are ordered as the device orders
           them: by the order-preserving integer image of the fp32 bits (-0.0 below +0.0), never by a float comparison; equal
           scores go to the lower vector; a NaN (a row that is not selected is a column of NaN) is never a candidate.
update     the centres from the labels: members in ascending row number, chunks of 256, sequential fp64 sums that START at
           their first term (np.add.accumulate in float64 is sequential), / count, / the square root of the sequential sum of
           squares, rounded to fp32 once.
kmeans     the loop.  It takes the scores from a callback, so that the GPU tests can feed it the library's own single-query
           bits and the CPU tests a plain matrix product.
KmeansOracleIndex   the CPU stand-in index + assign / kmeans, for the tests of the Python layer."""
import numpy as np

from maxsim_oracle import MISSING, order_image
from oracle import flat
from oracle_backend import OracleIndex

CHUNK = 256
MAX_VECTORS = 4096


def vectors_per_pass(C, ld, knob=0):
    """The vectors one corpus pass scores: min(C, 32, 128 KiB / (4 ld)), at least 1, lowered by the knob (0: none)."""
    vp = min(C, 32, max(1, (128 << 10) // (4 * ld)))
    return min(vp, knob) if knob > 0 else vp


def assign(S):
    """(labels int32[n], scores float32[n]) of a [C, n] float32 score matrix."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    C, n = S.shape
    offered = S == S
    image = np.where(offered, order_image(np.where(offered, S, np.float32(0))), np.uint64(0))
    inv_j = (np.uint64(0xFFFFFFFF) - np.arange(C, dtype=np.uint64))[:, None]
    key = np.where(offered, (image << np.uint64(32)) | inv_j, np.uint64(0))        # 0: no candidate
    best = key.max(axis=0) if C else np.zeros(n, np.uint64)
    some = best != 0
    j = (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64)
    labels = np.where(some, j, -1).astype(np.int32)
    scores = np.where(some, S[np.where(some, j, 0), np.arange(n)], MISSING).astype(np.float32)
    return labels, scores


def seq_sum(a):
    """Sequential float64 sum over axis 0, starting at the first term."""
    return np.add.accumulate(np.asarray(a, dtype=np.float64), axis=0)[-1]


def update(rows, labels, centres):
    """The centres after one update.  rows [n, d] float32 (the STORED rows), labels [n], centres [C, d] float32."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.array(centres, dtype=np.float32, copy=True)
    for c in range(out.shape[0]):
        members = np.flatnonzero(labels == c)                                         # ascending row number
        if not len(members):
            continue
        partials = [seq_sum(rows[members[i:i + CHUNK]]) for i in range(0, len(members), CHUNK)]
        with np.errstate(all="ignore"):
            mean = seq_sum(np.stack(partials)) / np.float64(len(members))
            norm = np.sqrt(seq_sum(mean * mean))                                        # product rounded, then added
            if not (norm > 0 and norm < np.inf):
                continue                                                                # a zero or non-finite mean: kept
            out[c] = (mean / norm).astype(np.float32)
    return out


def kmeans(scores_of, rows, centres, max_iter):
    """(centres, labels, scores, counts, iterations).  scores_of(centres) -> [C, n] float32, NaN where a row is not selected;
    `centres`: the initial ones ALREADY normalised."""
    centres = np.array(centres, dtype=np.float32, copy=True)
    before, updates, converged = None, 0, False
    labels = scores = None
    for it in range(1, max_iter + 1):
        labels, scores = assign(scores_of(centres))
        if it > 1 and np.array_equal(labels, before):
            converged = True
            break
        centres = update(rows, labels, centres)
        updates += 1
        before = labels
    if not converged:
        labels, scores = assign(scores_of(centres))
    counts = np.bincount(labels[labels >= 0], minlength=centres.shape[0]).astype(np.int64)
    return centres, labels, scores, counts, updates


class KmeansOracleIndex(OracleIndex):
    """OracleIndex + assign / kmeans: per vector the oracle's full ranking of the selected rows, scattered into a [C, n]
    matrix, then the functions above.  normalize_c and k-means' first step normalise with the oracle's normalize_l2."""

    def _scores(self, c, rowset, normalize):
        n = self.x.shape[0]
        if rowset is not None and (rowset.n > n or rowset.gen != getattr(self, "renumbered", 0)):
            raise ValueError("the row set was built for another state of the index")
        m = n if rowset is None else len(rowset.rows)
        S = np.full((c.shape[0], n), np.nan, np.float32)
        if m == 0:
            return S
        for j in range(c.shape[0]):
            if rowset is None:
                Dr, Ir = OracleIndex.search(self, c[j:j + 1], m, normalize_q=normalize)
            else:
                Dr, Ir = OracleIndex.search_rowset(self, c[j:j + 1], m, rowset, normalize_q=normalize)
            S[j, Ir[0][Ir[0] >= 0]] = Dr[0][Ir[0] >= 0]
        return S

    def _vectors(self, c):
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float32))
        if c.ndim != 2 or c.shape[1] != self.d or not 1 <= c.shape[0] <= MAX_VECTORS:
            raise ValueError("assignment needs a [C, d] array, 1 <= C <= 4096")
        return c

    def assign(self, c, rowset=None, normalize_c=False, with_scores=True):
        c = self._vectors(c)
        self.calls.append(("assign", c.shape[0], rowset is not None))
        labels, scores = assign(self._scores(c, rowset, normalize_c))
        return labels, scores if with_scores else None

    def kmeans(self, centres, max_iter=25, rowset=None):
        centres = self._vectors(centres).copy()
        self.calls.append(("kmeans", centres.shape[0], int(max_iter), rowset is not None))
        self.last_init = centres.copy()
        if max_iter < 1:
            raise ValueError("k-means needs max_iter >= 1")
        flat.normalize_l2(centres)
        return kmeans(lambda c: self._scores(c, rowset, False), self.x, centres, int(max_iter))
