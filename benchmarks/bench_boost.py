#!/usr/bin/env python3
"""Boosted search (mvdb_index_search_boosted_device) beside the exact scan it is held against, timed in the same process.
Corpus 1M x 512 and 10M x 512 normalised synthetic rows added on the device; k = 10; term columns drawn N(0, 0.1).  Device
timings: hipEvents on the current stream, the median of --reps calls after 3 warm-up calls, with the minimum and the maximum
kept (``*_ms`` / ``*_ms_min`` / ``*_ms_max``).  One record per corpus:

  exact_step_ms          the exact single-query scan (index option code8_single_query = 0), one query
  default_step_ms        the default single-query step (the int8 prefilter), for scale
  boost_1term_ms         the boosted call with one term            (ratio_* = that figure / exact_step_ms)
  boost_4terms_ms        ... with four terms
  boost_1term_sparse_ms  ... with one term and 1,000 sparse entries (the device entry point waits once for their upload)
  boost_bitmap50_ms      one term under a bitmap that selects half of the rows: held against exact_bitmap50_ms, the plain
                         search under the same set
  boost_list1_ms         one term under a row list of 1 % of the rows: held against exact_list1_ms
  boost_nq8_ms           eight queries sharing one term: one combine, one launch, eight passes over the corpus
  combine_1term_ms, combine_4terms_ms   the combine launch alone (mvdb_prof_read "boost_combine", calls of their own)
  scan_launch_ms         the scan launch of the one-term call alone ("boost_scan"), scan_symbol its instantiation
  lost_by_rerank         how many of the exact boosted top 10 lie OUTSIDE the plain top 100 — what "fetch 100 and re-rank on the
                         host" loses —, averaged over 100 queries (perturbed stored rows)

One JSON line per corpus, to stdout and to --out (default profiles/boost_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

from bench_distinct import launch_ms  # noqa: E402


def timed(fn, reps, warm=3):
    """(median, min, max) in ms over `reps` calls after `warm` warm-up calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b))
    return float(np.median(per)), float(min(per)), float(max(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quality-queries", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boost_bench.jsonl"))
    args = ap.parse_args()
    d, k = 512, 10
    stream = torch.cuda.current_stream().cuda_stream
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for n in args.rows:
        rng = np.random.default_rng(2032)
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        D = torch.empty((8, k), dtype=torch.float32, device="cuda")
        I = torch.empty((8, k), dtype=torch.int64, device="cuda")
        q8_host = np.concatenate([idx.get_rows(7 + 1000 * i, 1) for i in range(8)]) + np.float32(0.01)
        q8 = torch.from_numpy(np.ascontiguousarray(q8_host, dtype=np.float32)).cuda()
        terms = [idx.rowterm(np.float32(0.1) * rng.standard_normal(n, dtype=np.float32)) for _ in range(4)]
        weights = [1.0, 0.5, -0.25, 0.125]
        sparse_rows = np.sort(rng.choice(n, 1000, replace=False)).astype(np.int64)
        sparse_values = rng.uniform(0.0, 0.3, 1000).astype(np.float32)
        half = idx.rowset(np.flatnonzero(rng.random(n) < 0.5).astype(np.int64), excluded=True)
        one_percent = idx.rowset(np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64))
        assert half.is_bitmap and not one_percent.is_bitmap
        rec = {"bench": "boost", "n": n, "d": d, "k": k, "reps": args.reps, "bitmap_rows": len(half), "list_rows": len(one_percent)}

        def put(name, fn, reps=args.reps):
            rec[name], rec[name + "_min"], rec[name + "_max"] = (round(v, 4) for v in timed(fn, reps))

        def plain(rowset=None):
            if rowset is None:
                return lambda: idx.search_device(q8.data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)
            return lambda: idx.search_rowset_device(q8.data_ptr(), 1, k, rowset, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)

        def boost(nterms, nq=1, rowset=None, sparse=False):
            return lambda: idx.search_boosted_device(q8.data_ptr(), nq, k, terms[:nterms], weights[:nterms], D.data_ptr(), I.data_ptr(),
                                                     sparse_rows=sparse_rows if sparse else None,
                                                     sparse_values=sparse_values if sparse else None, rowset=rowset, stream=stream,
                                                     normalize_q=True)

        put("default_step_ms", plain())
        idx.set_option("code8_single_query", 0)
        put("exact_step_ms", plain())
        put("boost_1term_ms", boost(1))
        put("boost_4terms_ms", boost(4))
        put("boost_1term_sparse_ms", boost(1, sparse=True))
        put("exact_bitmap50_ms", plain(half))
        put("boost_bitmap50_ms", boost(1, rowset=half))
        put("exact_list1_ms", plain(one_percent))
        put("boost_list1_ms", boost(1, rowset=one_percent))
        put("boost_nq8_ms", boost(1, nq=8))
        put("exact_step_again_ms", plain())                       # the yardstick once more, behind the cells it is held against
        rec["combine_1term_ms"], _ = launch_ms(boost(1), "boost_combine", 5, per_call=True)
        rec["combine_4terms_ms"], _ = launch_ms(boost(4), "boost_combine", 5, per_call=True)
        rec["scan_launch_ms"], rec["scan_symbol"] = launch_ms(boost(1), "boost_scan", 5, per_call=True)
        exact = 0.5 * (rec["exact_step_ms"] + rec["exact_step_again_ms"])
        for name in ("boost_1term_ms", "boost_4terms_ms", "boost_1term_sparse_ms"):
            rec["ratio_" + name[6:-3]] = round(rec[name] / exact, 3)
        rec["ratio_scan_launch"] = round(rec["scan_launch_ms"] / exact, 3) if rec["scan_launch_ms"] else None
        rec["ratio_bitmap50"] = round(rec["boost_bitmap50_ms"] / rec["exact_bitmap50_ms"], 3)
        rec["ratio_list1"] = round(rec["boost_list1_ms"] / rec["exact_list1_ms"], 3)
        rec["ratio_nq8_per_query"] = round(rec["boost_nq8_ms"] / 8 / exact, 3)
        rec["scan_TBps"] = round(n * (d * 4 + 4) / (rec["boost_1term_ms"] * 1e-3) / 1e12, 2)

        # what "fetch 100 and re-rank on the host" loses: the exact boosted top 10 against the plain top 100
        lost = []
        picks = rng.choice(n, args.quality_queries, replace=False)
        for r in picks:
            qh = idx.get_rows(int(r), 1) + np.float32(0.02) * rng.standard_normal((1, d), dtype=np.float32)
            _, top = idx.search_boosted(qh, k, terms[:1], [1.0], normalize_q=True)
            _, fetched = idx.search(qh, 100, normalize_q=True)
            lost.append(len(set(top[0].tolist()) - set(fetched[0].tolist())))
        rec["lost_by_rerank"] = round(float(np.mean(lost)), 2)
        rec["lost_by_rerank_min_max"] = [int(min(lost)), int(max(lost))]
        idx.set_option("code8_single_query", 1)
        emit(rec)
        del terms, half, one_percent
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
