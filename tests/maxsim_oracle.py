"""The contract of MaxSim search as a few lines of numpy (include/mvdb.h "MAXSIM SEARCH"): per query vector the best selected
row of every group, the group's score their sum in order, the k best groups.

Scores are ordered as the device orders them: by the order-preserving integer image of the fp32 bits (-0.0 below +0.0, -inf
the smallest, +inf the largest), never by a float comparison."""
import numpy as np

MISSING = np.float32(-3.4028234663852886e38)


def order_image(s):
    """uint64 image of float32 values that sorts like the values (NaN has none: callers keep it out)."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u >> np.uint64(31), np.uint64(0xFFFFFFFF) - u, u | np.uint64(0x80000000))


def maxsim(scores, codes, selection, k):
    """(D float32[k], G int32[k], I_tok int64[k, T], D_tok float32[k, T]).

    scores     [T, n] float32: the score of stored row r for query vector t; NaN = not offered
    codes      [n] group code of every stored row
    selection  the selected rows IN POSITION ORDER (all rows / a bitmap: ascending; a row list: the list) — equal scores
               inside a group go to the lower position
    A group without an offer for some vector, or whose sum is NaN, is no result; equal sums go to the lower code; fewer than
    k groups: padded with -FLT_MAX / -1 / -1 / -FLT_MAX."""
    scores = np.asarray(scores, dtype=np.float32)
    T = scores.shape[0]
    selection = np.asarray(selection, dtype=np.int64)
    codes = np.asarray(codes)
    n_groups = int(codes.max()) + 1 if len(codes) else 0
    sel_codes = codes[selection].astype(np.int64)
    pos = np.arange(len(selection), dtype=np.uint64)
    best = np.zeros((T, n_groups), dtype=np.uint64)      # (image of the score) << 32 | ~position; 0 = no offer
    for t in range(T):
        s = scores[t, selection]
        offered = s == s
        key = (order_image(np.where(offered, s, np.float32(0))) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos)
        np.maximum.at(best[t], sel_codes[offered], key[offered])
    every = (best != 0).all(axis=0) if n_groups else np.zeros(0, bool)
    best_pos = (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64)
    best_row = selection[np.minimum(best_pos, max(len(selection) - 1, 0))] if len(selection) else best_pos
    m = np.zeros((T, n_groups), dtype=np.float32)
    for t in range(T):
        m[t] = scores[t, best_row[t]] if len(selection) else 0
    with np.errstate(invalid="ignore", over="ignore"):
        S = m[0].copy() if T else np.zeros(n_groups, np.float32)
        for t in range(1, T):
            S = (S + m[t]).astype(np.float32)            # sequential fp32 adds, in order
    valid = np.flatnonzero(every & (S == S))
    ranked = sorted(valid.tolist(), key=lambda g: (-int(order_image(S[g:g + 1])[0]), g))[:k]
    D = np.full(k, MISSING, np.float32)
    G = np.full(k, -1, np.int32)
    I_tok = np.full((k, T), -1, np.int64)
    D_tok = np.full((k, T), MISSING, np.float32)
    for j, g in enumerate(ranked):
        D[j], G[j] = S[g], g
        I_tok[j] = best_row[:, g]
        D_tok[j] = m[:, g]
    return D, G, I_tok, D_tok
