#!/usr/bin/env python3
"""Group hits search (mvdb_index_search_groups_device) beside the searches it is made of and beside what a caller writes
without it.  Corpus 1M x 512 and 10M x 512 normalised synthetic rows added on the device; (k, group_size, fetch_k) = (5, 3, 32)
and (10, 5, 64); nq = 1 and 64.  Device buffers, hipEvents on the current stream, the median of --reps calls after warm-up
calls; the launches from mvdb_prof_read, collected in calls of their own.

  case "chunked"   codes = row // 8 (documents of 8 chunks): a few dozen rows of the matrix are members.
      groups_ms            search_groups_device
      distinct_ms          search_distinct_device at the same (k, fetch_k), same process: the call's first stage
      behind_distinct_ms   groups_ms - distinct_ms
      scan_launch_ms       the groups_scan launches of a call together, select_launch_ms its groups_select launches
      codes_bytes          4 n: what the scan launch streams
      groups_host_ms       search_groups through the host entry point, wall clock (upload, call, one copy back)
      today_host_ms        what a caller writes today, wall clock: one search_distinct, then per query and returned group a
                           row-set upload (the group's 8 rows) and a search_rowset with k = group_size
  case "one_group"   every row has code 0: every row matches, the member pass reads the whole matrix.
      groups_ms            search_groups_device (distinct search answers by its tier 2: one exact pass per query, too)
      scan_launch_ms       the groups_scan launches of a call together, per query in scan_launch_per_query_ms
      distinct_scan_launch_ms   the distinct_scan launches (clear + scan) of the same calls, per query
      exact_scan_ms        the exact single-query scan of the same index (search_device, nq = 1, k = fetch_k, index option
                           code8_single_query = 0), same process

One JSON line per cell, to stdout and to --out (default profiles/groups_bench.jsonl)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

SHAPES = ((5, 3, 32), (10, 5, 64))
CHUNKS = 8


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


def timed_wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(per))


def launches_ms(fn, labels, reps):
    """{label: (summed time of its launches per call of fn, its symbol)} while fn runs `reps` times with profiling on."""
    fn()
    torch.cuda.synchronize()
    for label in labels:
        _native.prof_read(label)
    _native.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _native.prof_enable(False)
    out = {}
    for label in labels:
        launches, ms = _native.prof_read(label)
        out[label] = (round(ms / reps, 4) if launches else None, launches // reps, _native.prof_symbol(label))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dense-reps", type=int, default=3, help="calls timed per cell of the second case (a call is 2 nq passes over the matrix)")
    ap.add_argument("--today-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_bench.jsonl"))
    args = ap.parse_args()
    d = 512
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2031)
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
        chunked = idx.grouping((np.arange(n, dtype=np.int64) // CHUNKS).astype(np.int32), (n + CHUNKS - 1) // CHUNKS)
        one = idx.grouping(np.zeros(n, np.int32), 1)

        for k, group_size, fetch_k in SHAPES:
            for nq in args.nq:
                D = torch.empty((nq, k, group_size), dtype=torch.float32, device="cuda")
                I = torch.empty((nq, k, group_size), dtype=torch.int64, device="cuda")
                G = torch.empty((nq, k), dtype=torch.int32, device="cuda")
                Dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                Id = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                Dc = torch.empty((1, fetch_k), dtype=torch.float32, device="cuda")
                Ic = torch.empty((1, fetch_k), dtype=torch.int64, device="cuda")

                def groups(grouping):
                    idx.search_groups_device(q.data_ptr(), nq, k, group_size, fetch_k, grouping, D.data_ptr(), I.data_ptr(), G.data_ptr(),
                                             stream=stream, normalize_q=True)

                def distinct(grouping):
                    idx.search_distinct_device(q.data_ptr(), nq, k, fetch_k, grouping, Dd.data_ptr(), Id.data_ptr(), G.data_ptr(),
                                               stream=stream, normalize_q=True)

                def today():
                    _, _, Gh = idx.search_distinct(qh[:nq], k, fetch_k, chunked, normalize_q=True)
                    for i in range(nq):
                        for g in Gh[i]:
                            if g < 0:
                                continue
                            rows = np.arange(int(g) * CHUNKS, min((int(g) + 1) * CHUNKS, n), dtype=np.int64)
                            rs = idx.rowset(rows)
                            idx.search_rowset(qh[i:i + 1], group_size, rs, normalize_q=True)
                            rs.close()

                # ---- documents of 8 chunks -----------------------------------------------------------------------------
                rec = {"bench": "groups", "case": "chunked", "n": n, "d": d, "nq": nq, "k": k, "group_size": group_size,
                       "fetch_k": fetch_k, "reps": args.reps, "codes_bytes": 4 * n}
                torch.cuda.synchronize()
                calls0, rows0 = idx.groups_counters()
                rec["distinct_ms"] = round(timed_events(lambda: distinct(chunked), args.reps), 4)
                rec["groups_ms"] = round(timed_events(lambda: groups(chunked), args.reps), 4)
                rec["behind_distinct_ms"] = round(rec["groups_ms"] - rec["distinct_ms"], 4)
                torch.cuda.synchronize()
                calls1, rows1 = idx.groups_counters()
                rec["member_rows_per_call"] = (rows1 - rows0) // (calls1 - calls0)
                prof = launches_ms(lambda: groups(chunked), ("groups_scan", "groups_select"), args.reps)
                rec["scan_launch_ms"], rec["scan_launches"], rec["scan_symbol"] = prof["groups_scan"]
                rec["select_launch_ms"], rec["select_launches"], _ = prof["groups_select"]
                rec["groups_host_ms"] = round(timed_wall(lambda: idx.search_groups(qh[:nq], k, group_size, fetch_k, chunked, normalize_q=True),
                                                         args.today_reps), 4)
                rec["today_host_ms"] = round(timed_wall(today, args.today_reps), 4)
                members = I.cpu().numpy()
                rec["groups_full"] = bool((members >= 0).all())
                emit(rec)

                # ---- every row in one group ----------------------------------------------------------------------------
                reps = args.dense_reps
                rec = {"bench": "groups", "case": "one_group", "n": n, "d": d, "nq": nq, "k": k, "group_size": group_size,
                       "fetch_k": fetch_k, "reps": reps, "matrix_bytes": 4 * n * d}
                idx.set_option("code8_single_query", 0)
                rec["exact_scan_ms"] = round(timed_events(lambda: idx.search_device(q.data_ptr(), 1, fetch_k, Dc.data_ptr(), Ic.data_ptr(),
                                                                                    stream=stream, normalize_q=True), args.reps), 4)
                idx.set_option("code8_single_query", 1)
                torch.cuda.synchronize()
                calls0, rows0 = idx.groups_counters()
                rec["groups_ms"] = round(timed_events(lambda: groups(one), reps, warm=1), 4)
                torch.cuda.synchronize()
                calls1, rows1 = idx.groups_counters()
                assert rows1 - rows0 == (calls1 - calls0) * nq * n, (calls1 - calls0, rows1 - rows0)      # every row matched
                prof = launches_ms(lambda: groups(one), ("groups_scan", "groups_select", "distinct_scan"), 2)
                rec["scan_launch_ms"], rec["scan_launches"], rec["scan_symbol"] = prof["groups_scan"]
                rec["select_launch_ms"] = prof["groups_select"][0]
                rec["distinct_scan_launch_ms"], _, rec["distinct_scan_symbol"] = prof["distinct_scan"]
                rec["scan_launch_per_query_ms"] = round(rec["scan_launch_ms"] / nq, 4)
                rec["distinct_scan_launch_per_query_ms"] = round(rec["distinct_scan_launch_ms"] / nq, 4)
                rec["scan_over_distinct_scan"] = round(rec["scan_launch_ms"] / rec["distinct_scan_launch_ms"], 3)
                rec["scan_per_query_over_exact_scan"] = round(rec["scan_launch_per_query_ms"] / rec["exact_scan_ms"], 3)
                emit(rec)
        for g in (chunked, one):
            g.free()
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
