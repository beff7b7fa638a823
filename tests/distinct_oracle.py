"""The contract of distinct search as a few lines of numpy (include/mvdb.h "DISTINCT SEARCH"): the COLLAPSE of a ranking
keeps, in order, the first entry of every group."""
import numpy as np

MISSING = np.float32(-3.4028234663852886e38)


def collapse(D_row, I_row, codes, k):
    """(D float32[k], I int64[k], G int32[k]): the first k entries of the collapse of one ranking (scores D_row, row numbers
    I_row best first, -1 = missing), padded with -FLT_MAX / -1 / -1.  codes[row] is the group of a stored row."""
    D = np.full(k, MISSING, np.float32)
    I = np.full(k, -1, np.int64)
    G = np.full(k, -1, np.int32)
    seen = set()
    for s, r in zip(D_row, I_row):
        if r < 0:
            continue
        c = int(codes[int(r)])
        if c in seen:
            continue
        if len(seen) == k:
            break
        D[len(seen)], I[len(seen)], G[len(seen)] = s, r, c
        seen.add(c)
    return D, I, G


def tier(I_row, codes, k, m):
    """1 or 2: the tier the contract assigns to a query whose fetch_k candidates are I_row, of m selected rows."""
    fetch_k = len(I_row)
    valid = [int(r) for r in I_row if r >= 0]
    g = len({int(codes[r]) for r in valid})
    return 1 if (g >= k or len(valid) < fetch_k or fetch_k >= m) else 2
