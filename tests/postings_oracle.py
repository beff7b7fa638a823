"""The inverted form of a sparse store and its scoring route as a few lines of numpy (include/mvdb.h "SPARSE POSTINGS").

`transpose` is the layout: the stable transposition of the CSR arrays.  `scores_by_postings` performs the posting route's
arithmetic literally — the query's terms in ascending index order, and per row of a term's list acc = acc + (q * v), every
operation rounded to float32 on its own — so a test can hold it, bit for bit, to sparse_oracle.scores (the row's entries in
stored order): the indices of a stored row are strictly ascending, hence both walk a row's matching entries in one order."""
import numpy as np


def transpose(indptr, indices, values, dim=None):
    """(post_ptr int64[dim + 1], rows uint32[nnz], values float32[nnz]): list t is [post_ptr[t], post_ptr[t + 1]), rows ascending
    within a list.  dim None: one more than the largest index."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    values = np.asarray(values, dtype=np.float32)
    n = len(indptr) - 1
    if dim is None:
        dim = int(indices.max()) + 1 if len(indices) else 1
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    post_ptr = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=dim), out=post_ptr[1:])
    return post_ptr, row_of[order].astype(np.uint32), values[order]


def scores_by_postings(post_ptr, rows, values, n, q_idx, q_val):
    """(T float32[n], matched int32[n]) of one query — q_idx distinct indices in any order — term at a time."""
    q_idx = np.asarray(q_idx, dtype=np.int64)
    q_val = np.asarray(q_val, dtype=np.float32)
    assert len(set(q_idx.tolist())) == len(q_idx) == len(q_val)
    T = np.zeros(n, np.float32)
    matched = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in np.argsort(q_idx, kind="stable"):              # the terms in ascending index order
            t = int(q_idx[j])
            if t + 1 >= len(post_ptr):
                continue                                            # an index beyond the directory: no row holds it
            lo, hi = int(post_ptr[t]), int(post_ptr[t + 1])
            r = rows[lo:hi].astype(np.int64)                        # distinct rows: the fancy-indexed update touches each once
            product = (q_val[j] * values[lo:hi]).astype(np.float32)
            T[r] = (T[r] + product).astype(np.float32)
            matched[r] += 1
    return T, matched
