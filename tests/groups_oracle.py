"""The contract of group hits search as a few lines of numpy (include/mvdb.h "GROUP HITS SEARCH"): the MEMBERS of the k
groups distinct search picked are, per group, the first group_size entries of the query's full ranking that carry the
group's code; and the model behind the member_rows counter."""
import numpy as np

from distinct_oracle import MISSING


def members(D_full, I_full, codes, G_row, group_size):
    """(D float32[k, group_size], I int64[k, group_size]) for one query: D_full / I_full are its full ranking of the
    selected rows (scores and row numbers best first, -1 = missing: a row scoring NaN is in no ranking), G_row the k group
    codes distinct search returned (-1 = no group), codes[row] the group of a stored row.  Padded with -FLT_MAX / -1."""
    k = len(G_row)
    D = np.full((k, group_size), MISSING, np.float32)
    I = np.full((k, group_size), -1, np.int64)
    slot = {int(c): j for j, c in enumerate(G_row) if c >= 0}
    assert len(slot) == int((np.asarray(G_row) >= 0).sum()), "the groups of one query are distinct"
    filled = [0] * k
    for s, r in zip(D_full, I_full):
        if r < 0:
            continue
        j = slot.get(int(codes[int(r)]))
        if j is None or filled[j] == group_size:
            continue
        D[j, filled[j]], I[j, filled[j]] = s, r
        filled[j] += 1
    return D, I


def member_rows(selected, codes, G):
    """The model count behind mvdb_index_groups_counters' member_rows for one call: over the queries, the selected rows
    (row numbers, or None for every row) whose code is one of the query's groups G[i] — whatever their score, NaN included."""
    codes = np.asarray(codes)
    sel = codes if selected is None else codes[np.asarray(selected, dtype=np.int64)]
    return int(sum(np.isin(sel, [c for c in Gi if c >= 0]).sum() for Gi in np.atleast_2d(G)))
