"""The contract of probed search (include/mvdb.h "PROBED SEARCH") in numpy, given the scores: coarse ranking of the centres ->
probes -> union of their member lists -> ranking of those rows with ties to the lower row.

Scores are float32 and ordered as the scan's keys order them: by the order-preserving image of the bits (-0.0 below +0.0), equal
scores to the LOWER index, a NaN never a candidate."""
import numpy as np

MISSING = np.float32(-3.402823466e+38)


def image(scores):
    """uint32 order-preserving image of float32 scores (topk_device.hpp f2ord)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ranking(scores, candidates=None):
    """Indices into `scores`, best first: larger image first, equal images to the lower index; NaN scores (and indices outside
    `candidates`, when given) left out."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    ok = ~np.isnan(scores)
    if candidates is not None:
        inside = np.zeros(scores.shape[0], bool)
        inside[np.asarray(candidates, dtype=np.int64)] = True
        ok &= inside
    idx = np.flatnonzero(ok)
    img = image(scores[idx]).astype(np.int64)
    return idx[np.lexsort((idx, -img))]


def probes(coarse, nprobe):
    """The centres a query probes, best first: the first nprobe of the coarse ranking (fewer when NaNs leave fewer)."""
    return ranking(coarse)[:nprobe]


def probe_search(coarse, fine, labels, k, nprobe, selected=None):
    """One query.  coarse [C]: its scores against the centres; fine [n]: against the rows; labels [n]: the list of each row, -1
    for none; selected: the rows of a row set, or None.  Returns (D float32[k], I int64[k], the probes)."""
    labels = np.asarray(labels)
    P = probes(coarse, nprobe)
    member = np.isin(labels, P) & (labels >= 0)
    rows = np.flatnonzero(member)                        # ascending: the union of the probed lists
    if selected is not None:
        rows = np.intersect1d(rows, np.asarray(selected, dtype=np.int64))
    best = ranking(fine, rows)[:k]
    D = np.full(k, MISSING, np.float32)
    I = np.full(k, -1, np.int64)
    D[:len(best)] = np.asarray(fine, dtype=np.float32)[best]
    I[:len(best)] = best
    return D, I, P
