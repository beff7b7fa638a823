"""The contract of search by examples as a few lines of numpy (include/mvdb.h "SEARCH BY EXAMPLES"): per row the best score
against a positive (bp) and against a negative (bn), S = bp if bp > bn else -(bn * bn), the k rows with the largest S.

Scores are ordered as the device orders them: by the order-preserving integer image of the fp32 bits (-0.0 below +0.0, -inf
the smallest, +inf the largest), never by a float comparison — except the one `bp > bn` of the rule, which IS the IEEE fp32
comparison.  -(bn * bn) is one fp32 multiply and a negation."""
import numpy as np

from maxsim_oracle import MISSING, order_image


def _best(s):
    """Per column of s [m, n] the largest non-NaN entry by order image: (values float32[n], any offer bool[n]).  m may be 0."""
    n = s.shape[1]
    offered = s == s
    img = np.where(offered, order_image(np.where(offered, s, np.float32(0))), np.uint64(0))
    if s.shape[0] == 0:
        return np.full(n, -np.inf, np.float32), np.zeros(n, bool)
    pick = img.argmax(axis=0)
    return s[pick, np.arange(n)].astype(np.float32), offered.any(axis=0)


def branches(scores, P):
    """(bp, bn, has) per row: bn is -inf where no negative offers; has: some positive offers."""
    scores = np.asarray(scores, dtype=np.float32)
    bp, has = _best(scores[:P])
    bn, any_neg = _best(scores[P:])
    bn = np.where(any_neg, bn, np.float32(-np.inf)).astype(np.float32)
    return bp, bn, has


def examples(scores, P, k, skip=()):
    """(D float32[k], I int64[k]).

    scores  [P + N, n] float32: the score of stored row r for example j (the P positives first); NaN = no offer (the row is
            not selected, or the score is NaN)
    skip    rows that are never results
    A row no positive offers to is no result; equal S goes to the lower row; fewer than k rows: padded with -FLT_MAX / -1."""
    scores = np.asarray(scores, dtype=np.float32)
    bp, bn, has = branches(scores, P)
    with np.errstate(invalid="ignore", over="ignore"):
        closer = bp > bn                                         # the IEEE fp32 comparison (bp is garbage where has is False)
        S = np.where(closer, bp, -(bn * bn).astype(np.float32)).astype(np.float32)
    has = has.copy()
    skip = np.asarray(list(skip), dtype=np.int64)
    has[skip] = False
    valid = np.flatnonzero(has)
    img = order_image(S[valid])
    order = np.lexsort((valid, np.uint64(0xFFFFFFFF) - img))[:k]  # image descending, then row ascending
    D = np.full(k, MISSING, np.float32)
    I = np.full(k, -1, np.int64)
    D[:len(order)] = S[valid[order]]
    I[:len(order)] = valid[order]
    return D, I
