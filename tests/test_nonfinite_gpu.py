"""NaN, +/-inf and -0.0 rows and queries on every top-k route of the flat index (libmvdb.so through the C-ABI), against the
float64 reference of tests/nonfinite_cases.py.  The contract ("Non-finite rows and queries"): a row whose key
score is NaN is never a result, +inf first, -inf after every finite score, equal scores by the lower label, the slots left are
-1 / -+FLT_MAX — whichever kernel answers.  Every entry asserts, through the profiling labels, that the route it names ran.

Before the fix that came with this file three routes broke the contract (in brackets the cases that failed for it when this
file was run against the earlier library on an MI355X; the commit message lists them):
  * k > 64 listed NaN-scoring rows with score -inf            (radix-* cases, every shape)
  * k > 64 under a bitmap dropped rows that do score -inf      (radix-*-bitmap cases)
  * the staged MFMA pass scored L2 by |q|^2 + |x|^2 - 2 q.x   (mfma2-*-l2 cases: inf - inf = NaN where the distance is +inf)
and a fourth the issue had not listed: the gate of the batch passes (beats_key from a floor of -inf) refused rows scoring -inf
while a list still had room (mfma-ng, mfma2, masked and gemm cases on the 37-row corpus at k = 32 / 16).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import flat
from tests import nonfinite_cases as nf

pytestmark = pytest.mark.gpu

IP, L2 = flat.METRIC_IP, flat.METRIC_L2
MNAME = {IP: "ip", L2: "l2"}
NS = (nf.N_BIG, nf.N_SMALL)
LABELS = ("ip_scan", "ip_scan_scores", "ip_scan_mfma", "ip_scan_mfma_masked", "ip_scan_gemm", "ip_scan_rerun", "ip_scan_half",
          "ip_scan_half_seed")


@pytest.fixture(scope="module")
def native(gpu):
    from minivectordb_amd import _native
    assert _native.device_count() >= 1
    _native.prof_enable(True)
    yield _native
    _native.prof_enable(False)


@functools.lru_cache(maxsize=None)
def _corpus(n, d):
    x = nf.corpus(n, d)
    x.setflags(write=False)
    return x


def _launches(native):
    """{label: launches since the last call}"""
    return {name: native.prof_read(name)[0] for name in LABELS}


class Selection:
    """One way of naming the searched rows, with the search call and the reference's view of it."""

    def __init__(self, native, idx, n, kind):
        self.kind, self.idx, self.rows, self.keep, self.rs = kind, idx, None, None, None
        if kind == "list":              # labels: positions in a permuted list
            self.rows = nf.row_list(n)
        elif kind == "bitmap":          # labels: row numbers
            self.keep = nf.keep_mask(n)
            self.words = native.pack_row_mask(n, rows=np.flatnonzero(self.keep))
        elif kind == "rowset":          # resident row set in list form (an ascending sparse list; labels: row numbers)
            self.keep = nf.sparse_keep(n)
            self.rs = idx.rowset(np.flatnonzero(self.keep))
            assert not self.rs.is_bitmap
        elif kind == "rowset-excluded":  # resident row set in bitmap form
            self.keep = nf.keep_mask(n)
            self.rs = idx.rowset(np.flatnonzero(~self.keep), excluded=True)
            assert self.rs.is_bitmap
        self.size = n if kind == "all" else len(self.rows) if self.rows is not None else int(self.keep.sum())

    def search(self, q, k, normalize_q):
        if self.kind == "all":
            return self.idx.search(q, k, normalize_q=normalize_q)
        if self.kind == "list":
            return self.idx.search_subset(q, k, self.rows, normalize_q=normalize_q)
        if self.kind == "bitmap":
            return self.idx.search_masked(q, k, self.words, normalize_q=normalize_q)
        return self.idx.search_rowset(q, k, self.rs, normalize_q=normalize_q)

    def check(self, D, I, x, q, k, metric, normalize_q, what):
        return nf.check(D, I, x, q, k, metric, normalize_q, rows=self.rows, keep=self.keep, what=what)

    def close(self):
        if self.rs is not None:
            self.rs.close()


def _singles(sel, q, k, normalize_q):
    """Every query of q on its own (nq = 1), stacked."""
    parts = [sel.search(q[i], k, normalize_q) for i in range(len(q))]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _same_as_singles(D, I, Ds, Is, what):
    """The caller cannot tell: a batch row equals the single-query answer — ids bit for bit, scores within TOL where finite
    and equal where not."""
    assert np.array_equal(I, Is), f"{what}: batch ids differ from the single-query ids in rows {np.flatnonzero((I != Is).any(axis=1)).tolist()}"
    fin = np.isfinite(Ds) & (Is >= 0)
    assert np.array_equal(D[~fin], Ds[~fin]), f"{what}: batch and single-query infinities / padding differ"
    assert np.abs(D[fin].astype(np.float64) - Ds[fin]).max(initial=0.0) <= nf.TOL, what


# ---- the table of routes ---------------------------------------------------------------------------------------------------
# (name, d, metric, selection, nq, ks, label that must have launched, labels that must not have)
def _routes():
    out = []
    for d in (128, 100, 3):          # unmasked lanes / masked lanes / a padded row stride
        for metric in (IP, L2):
            for sel in ("all", "list", "bitmap", "rowset", "rowset-excluded"):
                out.append((f"single-d{d}-{MNAME[metric]}-{sel}", d, metric, sel, 1, (1, 10, 64), "ip_scan",
                            ("ip_scan_scores", "ip_scan_mfma", "ip_scan_gemm", "ip_scan_half_seed")))
    for d in (128, 100):
        for metric in (IP, L2):
            for sel in ("all", "list", "bitmap"):
                for nq in (1, 3):
                    out.append((f"radix-d{d}-{MNAME[metric]}-{sel}-nq{nq}", d, metric, sel, nq, ("65", "300", "m", "m+50"),
                                "ip_scan_scores", ("ip_scan", "ip_scan_mfma", "ip_scan_gemm", "ip_scan_half_seed")))
    for nq in (5, 20):
        out.append((f"mfma-ng-d64-ip-nq{nq}", 64, IP, "all", nq, (10, 64), "ip_scan_mfma", ("ip_scan", "ip_scan_gemm", "ip_scan_half_seed")))
        for metric in (IP, L2):
            out.append((f"mfma2-d128-{MNAME[metric]}-nq{nq}", 128, metric, "all", nq, (10, 32, 64), "ip_scan_mfma",
                        ("ip_scan", "ip_scan_gemm", "ip_scan_half_seed")))
        out.append((f"mfma2-masked-d128-ip-nq{nq}", 128, IP, "bitmap", nq, (10, 32, 64), "ip_scan_mfma_masked",
                    ("ip_scan", "ip_scan_gemm", "ip_scan_half_seed")))
    # d = 768: the widest L2 form; its non-finite epilogue fits beside the query fragments only with the 512-B stages
    out.append(("mfma2-d768-l2-nq5", 768, L2, "all", 5, (10, 32), "ip_scan_mfma", ("ip_scan", "ip_scan_gemm", "ip_scan_half_seed")))
    out.append(("gemm-d80-ip-nq8", 80, IP, "all", 8, (10, 16), "ip_scan_gemm", ("ip_scan", "ip_scan_mfma", "ip_scan_half_seed")))
    out.append(("gemm-d128-ip-nq130", 128, IP, "all", 130, (10, 16), "ip_scan_gemm", ("ip_scan", "ip_scan_half_seed")))
    return out


ROUTES = _routes()


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_route(native, route):
    name, d, metric, sel_kind, nq, ks, must, must_not = route
    for n in NS:
        x = _corpus(n, d)
        idx = native.FlatIndex(d, metric=metric)
        idx.add(x)
        sel = Selection(native, idx, n, sel_kind)
        try:
            for normalize_q in (False, True):
                # one query at a time: each of the 11 fixture queries; the select route in threes: all 11 too (the last group
                # is filled up with the first query); the batch routes: the special queries spread over a batch
                radix3 = must == "ip_scan_scores" and nq == 3
                q = nf.query_set(x) if nq == 1 or radix3 else nf.batch(x, nq)[0]
                if radix3:
                    q = np.concatenate([q, q[:1]])
                for kk in ks:
                    k = {"65": 65, "300": 300, "m": sel.size, "m+50": sel.size + 50}[kk] if isinstance(kk, str) else kk
                    if must == "ip_scan_scores" and k <= 64:
                        continue        # (the 37-row corpus under a selection: k = m is a fused-list k, the entries above run it)
                    what = f"{name} n={n} k={k} normalize_q={normalize_q}"
                    _launches(native)   # drain
                    if nq == 1:
                        D, I = _singles(sel, q, k, normalize_q)
                    elif radix3:
                        D, I = [np.concatenate(p) for p in zip(*[sel.search(q[i:i + 3], k, normalize_q) for i in range(0, len(q), 3)])]
                    else:
                        D, I = sel.search(q, k, normalize_q)
                    ran = _launches(native)
                    assert ran[must] >= 1, f"{what}: {must} did not launch ({ran})"
                    assert not any(ran[lb] for lb in must_not), f"{what}: another route answered ({ran})"
                    if must == "ip_scan_mfma" and d % 128 == 0:
                        sym = native.prof_symbol("ip_scan_mfma")
                        want_ng = 1 if nq <= 16 else 2
                        assert sym.startswith(f"flat_scan_mfma2_kernel<{d // 16}, {want_ng}, ") and sym.endswith(f", {1 if metric == L2 else 0}>"), (what, sym)
                    sel.check(D, I, x, q, k, metric, normalize_q, what)
                    if nq > 1 and k <= 64:
                        # the caller cannot tell: each row of the batch is the single-query answer
                        Ds, Is = _singles(sel, q, k, normalize_q)
                        _same_as_singles(D, I, Ds, Is, what)
        finally:
            sel.close()
            idx.close()


# ---- the certified fp16 pass: finite rows, special queries riding in a batch -------------------------------------------------
def _split_launches(native):
    native.prof_read("ip_scan_half")
    return native.prof_read("ip_scan_half_seed")[0]


@pytest.mark.parametrize("nq", [40, 130])
@pytest.mark.parametrize("variant", ["ip", "l2-normalised-rows", "l2-mixed-norms"])
def test_certified_pass_refuses_the_special_queries_and_answers_their_neighbours(native, variant, nq):
    """d = 256, 2003 FINITE rows: a batch of 40 / 130 takes the certified pass (fp16 nomination over the shadow, exact fp32
    re-score).  The non-finite and the all-zero queries cannot be bounded: they must be refused and re-run exactly, under the
    contract, while the plain queries keep their answers — each one's row equals its single-query search.

    What "the special queries are the refused ones" can be held to: the library reports refusals as a count of 256-query chunks
    that held at least one (split_rerun_count), not per query.  So: the batch with the special queries is refused (count up);
    at k = 10 the same batch with those four queries replaced by plain ones is not (count unchanged) — the four are why.  At
    k = 32 the worst-case certificate may also refuse a plain query over 2003 rows (the 32nd and the 64th approximate score
    are close), so there nothing ties the refusal to the special queries; the results are held to the contract all the same."""
    d = nf.CERTIFIED_D
    metric = IP if variant == "ip" else L2
    x, q, q_plain, special = nf.certified_fixture(variant, nq)
    assert len(special) == 4
    idx = native.FlatIndex(d, metric=metric)
    idx.add(x)
    try:
        for normalize_q in (False, True):
            for k in (10, 32):
                what = f"certified {variant} nq={nq} k={k} normalize_q={normalize_q}"
                _split_launches(native)
                before = native.split_rerun_count()
                Dp, Ip = idx.search(q_plain, k, normalize_q=normalize_q)
                assert _split_launches(native) >= 1, f"{what}: the certified pass did not run"
                if k == 10:
                    assert native.split_rerun_count() == before, f"{what}: a plain query was refused"
                before = native.split_rerun_count()
                D, I = idx.search(q, k, normalize_q=normalize_q)
                assert _split_launches(native) >= 1, f"{what}: the certified pass did not run"
                assert native.split_rerun_count() > before, f"{what}: no query was refused"
                nf.check(D, I, x, q, k, metric, normalize_q, what=what)
                nf.check(Dp, Ip, x, q_plain, k, metric, normalize_q, what=what + " (plain batch)")
                # the neighbours of the refused queries are not disturbed: the plain batch answered them the same, and each
                # query — refused or not — equals its own single-query search
                others = [i for i in range(nq) if i not in special]
                assert np.array_equal(I[others], Ip[others]) and np.array_equal(D[others], Dp[others]), what
                Ds, Is = [np.concatenate(p) for p in zip(*[idx.search(q[i], k, normalize_q=normalize_q) for i in range(nq)])]
                _same_as_singles(D, I, Ds, Is, what)
    finally:
        idx.close()


# ---- mvdb_merge_topk_device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("k", [8, 64, 70], ids=["k8", "k64", "k70"])
def test_merge_topk_device_with_infinite_scores_and_padding(native, metric, k):
    """3 lists x 4 queries: +/-inf scores, a list that is all -1, -1 padding at the end of the middle list; against a numpy
    merge by (score, list, slot).  k <= 64: merge_di_kernel, k > 64: merge_di_sort_kernel."""
    import torch
    from minivectordb_amd.distributed import PackedTopK
    dev = torch.device("cuda", 0)
    world, nq = 3, 4
    ip = metric == IP
    rs = np.random.RandomState(k)
    g = PackedTopK(nq, k, dev, world)
    miss = -nf.FLT_MAX if ip else nf.FLT_MAX
    lists = []
    for l in range(world):
        d = np.full((nq, k), miss, dtype=np.float32)
        i = np.full((nq, k), -1, dtype=np.int64)
        for qi in range(nq):
            empty = 2 if qi < 2 else 0            # the list that is all -1
            if l == empty:
                continue
            have = k - 3 if l == 1 else k         # the middle list ends in -1 padding
            s = np.round(rs.rand(have).astype(np.float32), 1)     # tenths: ties inside a list and across lists
            if ip:
                s[:2] = np.inf
                s[-2:] = -np.inf
                s[2:-2] = np.sort(s[2:-2])[::-1]
            else:
                s[-2:] = np.inf                   # a distance is never negative: +inf last
                s[:-2] = np.sort(s[:-2])
            d[qi, :have] = s
            i[qi, :have] = l * 1000 + qi * 100 + np.arange(have)
        D, I = g.views(l)
        D.copy_(torch.from_numpy(d))
        I.copy_(torch.from_numpy(i))
        lists.append((d, i))
    Dout = torch.empty((nq, k), dtype=torch.float32, device=dev)
    Iout = torch.empty((nq, k), dtype=torch.int64, device=dev)
    D0, I0 = g.views(0)
    native.check(native.lib().mvdb_merge_topk_device(
        metric, world, nq, k, ctypes.c_void_p(D0.data_ptr()), g.stride_D, ctypes.c_void_p(I0.data_ptr()), g.stride_I,
        ctypes.c_void_p(Dout.data_ptr()), ctypes.c_void_p(Iout.data_ptr()), 0,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    Dout, Iout = Dout.cpu().numpy(), Iout.cpu().numpy()
    for qi in range(nq):
        cands = sorted(((-float(d[qi, j]) if ip else float(d[qi, j])), l, j) for l, (d, i) in enumerate(lists) for j in range(k)
                       if i[qi, j] >= 0)[:k]
        want_i = [int(lists[l][1][qi, j]) for _, l, j in cands] + [-1] * (k - len(cands))
        want_d = [lists[l][0][qi, j] for _, l, j in cands] + [miss] * (k - len(cands))
        assert Iout[qi].tolist() == want_i, (qi, Iout[qi].tolist(), want_i)
        assert np.array_equal(Dout[qi], np.array(want_d, dtype=np.float32)), (qi, Dout[qi], want_d)
