#!/usr/bin/env python3
"""Distinct search (mvdb_index_search_distinct_device) beside the searches it is made of.  Corpus 1M x 512 and 10M x 512
normalised synthetic rows added on the device; (k, fetch_k) = (5, 32) and (10, 64); nq = 1 and 64.  Device buffers, hipEvents
on the current stream, the median of --reps calls after 3 warm-up calls.

  case "chunked"   codes = row // 8 (documents of 8 chunks): every query is answered by tier 1.
      distinct_ms          search_distinct_device
      search_ms            search_device with k = fetch_k on the same index — the call's first stage, existing code
      collapse_launch_ms   the distinct_collapse launch alone (mvdb_prof_read, collected in calls of their own); beside it
      mmr_select_launch_ms the mmr_select launch at the same (k, fetch_k), measured in the same run: the collapse does
                           strictly less and reads no rows
  case "one_document_fills_the_fetch"   every row has code 0 except the 4,095 rows arange(1, 4096) * (n // 4096), which
      carry the codes 1 .. 4095: every fetch holds at most fetch_k rows of code 0 and fewer than k groups, so every query
      takes tier 2 — asserted from distinct_counters().
      distinct_ms          search_distinct_device
      exact_scan_ms        the exact single-query scan of the same index (search_device, nq = 1, k = fetch_k, index option
                           code8_single_query = 0), measured in the same run; tier 2 reads the same bytes + 4 per row
      per_query_over_scan  distinct_ms / (nq * exact_scan_ms)
      scan_launch_ms       the clear and the scan launches of a call together, select_launch_ms its top-k launches

One JSON line per cell, to stdout and to --out (default profiles/distinct_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

SHAPES = ((5, 32), (10, 64))


def timed_events(fn, reps, warm=3):
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
    return float(np.median(per))


def launch_ms(fn, label, reps, per_call=False):
    """Mean time of the launches recorded under `label` while fn runs `reps` times (profiling events on; calls of their own);
    per_call: their sum per call of fn instead (a label with several launches per call)."""
    fn()
    torch.cuda.synchronize()
    _native.prof_read(label)
    _native.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _native.prof_enable(False)
    launches, ms = _native.prof_read(label)
    return (round(ms / (reps if per_call else launches), 4) if launches else None), _native.prof_symbol(label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tier2-reps", type=int, default=5, help="calls timed per cell of the second case (a call is nq exact scans)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distinct_bench.jsonl"))
    args = ap.parse_args()
    d = 512
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2028)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        qh = rng.standard_normal((max(args.nq), d), dtype=np.float32)
        q = torch.from_numpy(qh).cuda()
        chunked = idx.grouping((np.arange(n, dtype=np.int64) // 8).astype(np.int32), (n + 7) // 8)
        codes = np.zeros(n, np.int32)
        codes[np.arange(1, 4096, dtype=np.int64) * (n // 4096)] = np.arange(1, 4096, dtype=np.int32)
        filled = idx.grouping(codes, 4096)

        for k, fetch_k in SHAPES:
            for nq in args.nq:
                D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                G = torch.empty((nq, k), dtype=torch.int32, device="cuda")
                Dc = torch.empty((nq, fetch_k), dtype=torch.float32, device="cuda")
                Ic = torch.empty((nq, fetch_k), dtype=torch.int64, device="cuda")

                def distinct(grouping):
                    idx.search_distinct_device(q.data_ptr(), nq, k, fetch_k, grouping, D.data_ptr(), I.data_ptr(), G.data_ptr(),
                                               stream=stream, normalize_q=True)

                def search(queries=nq):
                    idx.search_device(q.data_ptr(), queries, fetch_k, Dc.data_ptr(), Ic.data_ptr(), stream=stream, normalize_q=True)

                def mmr():
                    idx.search_mmr_device(q.data_ptr(), nq, k, fetch_k, 0.5, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)

                # ---- documents of 8 chunks: tier 1 ---------------------------------------------------------------------
                rec = {"bench": "distinct", "case": "chunked", "n": n, "d": d, "nq": nq, "k": k, "fetch_k": fetch_k, "reps": args.reps}
                fell0 = idx.distinct_counters()[1]
                rec["search_ms"] = round(timed_events(search, args.reps), 4)
                rec["distinct_ms"] = round(timed_events(lambda: distinct(chunked), args.reps), 4)
                rec["behind_the_search_ms"] = round(rec["distinct_ms"] - rec["search_ms"], 4)
                rec["collapse_launch_ms"], rec["collapse_symbol"] = launch_ms(lambda: distinct(chunked), "distinct_collapse", args.reps)
                rec["mmr_select_launch_ms"], _ = launch_ms(mmr, "mmr_select", args.reps)
                torch.cuda.synchronize()
                rec["tier2_queries"] = idx.distinct_counters()[1] - fell0
                groups = G.cpu().numpy()
                rec["groups_distinct"] = bool(all(len(set(r.tolist())) == k for r in groups))
                emit(rec)

                # ---- one document fills the fetch: tier 2 --------------------------------------------------------------
                reps = args.tier2_reps
                rec = {"bench": "distinct", "case": "one_document_fills_the_fetch", "n": n, "d": d, "nq": nq, "k": k, "fetch_k": fetch_k,
                       "reps": reps}
                idx.set_option("code8_single_query", 0)
                rec["exact_scan_ms"] = round(timed_events(lambda: search(1), args.reps), 4)
                idx.set_option("code8_single_query", 1)
                torch.cuda.synchronize()
                calls0, fell0 = idx.distinct_counters()
                rec["distinct_ms"] = round(timed_events(lambda: distinct(filled), reps), 4)
                torch.cuda.synchronize()
                calls1, fell1 = idx.distinct_counters()
                assert fell1 - fell0 == (calls1 - calls0) * nq, (calls1 - calls0, fell1 - fell0, nq)   # every query took tier 2
                rec["tier2_queries_per_call"] = (fell1 - fell0) // (calls1 - calls0)
                rec["per_query_over_scan"] = round(rec["distinct_ms"] / (nq * rec["exact_scan_ms"]), 3)
                rec["scan_launch_ms"], rec["scan_symbol"] = launch_ms(lambda: distinct(filled), "distinct_scan", 2, per_call=True)
                rec["select_launch_ms"], _ = launch_ms(lambda: distinct(filled), "distinct_select", 2, per_call=True)
                groups = G.cpu().numpy()
                rec["groups_distinct"] = bool(all(len(set(r.tolist())) == k for r in groups))
                emit(rec)
        for g in (chunked, filled):
            g.free()
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
