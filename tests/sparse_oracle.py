"""The contract of sparse and hybrid search as a few lines of numpy (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH").

Float32 operations only, each rounded on its own — numpy never fuses a multiply with an add.  The sparse score of a row is
acc = +0.0, then for the row's entries in stored order whose index is in the query acc = acc + (q[index] * value); `matched`
counts the entries used.  Scores are ordered as the device orders them (boost_oracle.py); NaN is never a result.  Hybrid
search is ``boosted(s_row, np.float32(w_s) * T, w_d, k)`` of boost_oracle.py."""
import numpy as np

from maxsim_oracle import MISSING, order_image


def scores(indptr, indices, values, q_idx, q_val):
    """(T float32[n], matched int32[n]) of one query: q_idx distinct indices in any order, q_val their weights."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    values = np.asarray(values, dtype=np.float32)
    q_idx = np.asarray(q_idx, dtype=np.int64)
    q_val = np.asarray(q_val, dtype=np.float32)
    assert len(set(q_idx.tolist())) == len(q_idx) == len(q_val)
    n = len(indptr) - 1
    order = np.argsort(q_idx, kind="stable")
    sorted_idx = q_idx[order]
    pos = np.searchsorted(sorted_idx, indices)
    pos[pos == len(sorted_idx)] = 0
    used = sorted_idx[pos] == indices if len(sorted_idx) else np.zeros(len(indices), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        products = (q_val[order][pos] * values).astype(np.float32)
        T = np.zeros(n, np.float32)
        matched = np.zeros(n, np.int32)
        for r in range(n):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            chain = np.concatenate([np.zeros(1, np.float32), products[lo:hi][used[lo:hi]]])
            T[r] = np.add.accumulate(chain, dtype=np.float32)[-1]      # sequential: ((0 + p1) + p2) + ..., each sum rounded to fp32
            matched[r] = len(chain) - 1
    return T, matched


def sparse_topk(T, matched, selected, k):
    """(D float32[k], I int64[k]): the k rows of `selected` with matched >= 1 and a score that is no NaN, best first, equal
    scores to the lower row; fewer: padded with -FLT_MAX / -1."""
    T = np.asarray(T, dtype=np.float32)
    rows = np.unique(np.asarray(selected, dtype=np.int64))
    valid = rows[(matched[rows] >= 1) & (T[rows] == T[rows])]
    img = order_image(T[valid])
    order = np.lexsort((valid, np.uint64(0xFFFFFFFF) - img))[:k]
    D = np.full(k, MISSING, np.float32)
    I = np.full(k, -1, np.int64)
    D[:len(order)] = T[valid[order]]
    I[:len(order)] = valid[order]
    return D, I


def sparse_term(T, w_s):
    """The hybrid search's per-row term: one rounded multiply."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float32(w_s) * np.asarray(T, dtype=np.float32)).astype(np.float32)
