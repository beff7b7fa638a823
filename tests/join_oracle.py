"""Test-only stand-in: OracleIndex (oracle_backend.py) + range_join / range_join_count, stated as the contract of
mvdb_index_range_join reads — query i is STORED row qrows[i], matched by the oracle's search against the selected rows whose
row number is below it, cut where the score falls below the threshold."""
import numpy as np

from oracle import flat
from oracle_backend import OracleIndex


class JoinOracleIndex(OracleIndex):
    fail_next_join = 0

    def _join(self, threshold, first_row, rows, rowset):
        if self.fail_next_join:
            self.fail_next_join -= 1
            raise ValueError("the row set was built for another state of the index")
        x = self.x
        if rowset is not None and (rowset.n > x.shape[0] or rowset.gen != getattr(self, "renumbered", 0)):
            raise ValueError("the row set was built for another state of the index")
        qrows = np.arange(int(first_row), x.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
        if qrows.size and (qrows.min() < 0 or qrows.max() >= x.shape[0]):
            raise ValueError("query row out of range")
        selected = np.arange(x.shape[0], dtype=np.int64) if rowset is None else np.asarray(rowset.rows, dtype=np.int64)
        per = []
        for i in qrows:
            cand = selected[selected < i]
            if cand.size == 0:
                per.append((np.empty(0, np.float32), np.empty(0, np.int64)))
                continue
            Ds, Ps = flat.flat_search(x, x[i:i + 1], cand.size, metric=self.metric, normalize_q=False, rows=cand)
            keep = (Ps[0] >= 0) & (Ds[0] >= np.float32(threshold))
            assert not keep.any() or keep[:keep.sum()].all()      # sorted: the matches lead
            per.append((Ds[0][keep], cand[Ps[0][keep]]))
        return qrows, per

    def range_join(self, threshold, first_row=0, rows=None, rowset=None, cap=None, block=4096):
        self.calls.append(("range_join", rowset is not None))
        qrows, per = self._join(threshold, first_row, rows, rowset)
        lims = np.zeros(len(per) + 1, np.int64)
        np.cumsum([len(d) for d, _ in per], out=lims[1:])
        D = np.concatenate([d for d, _ in per]) if per else np.empty(0, np.float32)
        I = np.concatenate([i for _, i in per]) if per else np.empty(0, np.int64)
        return qrows, lims, D.astype(np.float32), I.astype(np.int64)

    def range_join_count(self, threshold, first_row=0, rows=None, rowset=None, block=4096):
        self.calls.append(("range_join_count", rowset is not None))
        return int(sum(len(d) for d, _ in self._join(threshold, first_row, rows, rowset)[1]))
