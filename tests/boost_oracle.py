"""The contract of boosted search as a few lines of numpy (include/mvdb.h "BOOSTED SEARCH"): T = w_1 t_1 (+ w_j t_j in call
order) (+ the sparse values), S = w_s * s + T, the k rows with the largest S.

Float32 operations only, each rounded on its own — numpy never fuses a multiply with an add.  Scores are ordered as the
device orders them: by the order-preserving integer image of the fp32 bits (-0.0 below +0.0, -inf the smallest, +inf the
largest), then by row ascending; NaN has no place in the order and is never a result."""
import numpy as np

from maxsim_oracle import MISSING, order_image


def combine(terms, weights, n, sparse=None):
    """T float32[n].

    terms    up to four float32[n] columns, chained in this order: T = w_1 t_1, then T = T + (w_j t_j)
    weights  one per term
    sparse   None or (rows, values): T[row] = T[row] + value, rows distinct
    No terms: T starts as +0.0."""
    assert len(terms) == len(weights) <= 4
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.zeros(n, np.float32)
        for j, (t, w) in enumerate(zip(terms, weights)):
            p = (np.float32(w) * np.asarray(t, dtype=np.float32)).astype(np.float32)
            assert p.shape == (n,)
            T = p if j == 0 else (T + p).astype(np.float32)
        if sparse is not None:
            rows = np.asarray(sparse[0], dtype=np.int64)
            values = np.asarray(sparse[1], dtype=np.float32)
            assert len(set(rows.tolist())) == len(rows) == len(values)
            T = T.copy()
            T[rows] = (T[rows] + values).astype(np.float32)
    assert T.dtype == np.float32
    return T


def boosted(s_row, T, w_s, k):
    """(D float32[k], I int64[k]).

    s_row  float32[n]: the single-query scan's score of every stored row; NaN = the row is not selected or has no score
    T      float32[n]: the combined term column
    S = (w_s * s) + T, one multiply then one add.  A row whose S is NaN is no result; equal S goes to the lower row; fewer
    than k rows: padded with -FLT_MAX / -1."""
    s_row = np.asarray(s_row, dtype=np.float32)
    T = np.asarray(T, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        S = ((np.float32(w_s) * s_row).astype(np.float32) + T).astype(np.float32)
    valid = np.flatnonzero((s_row == s_row) & (S == S))
    img = order_image(S[valid])
    order = np.lexsort((valid, np.uint64(0xFFFFFFFF) - img))[:k]  # image descending, then row ascending
    D = np.full(k, MISSING, np.float32)
    I = np.full(k, -1, np.int64)
    D[:len(order)] = S[valid[order]]
    I[:len(order)] = valid[order]
    return D, I
