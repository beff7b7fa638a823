#!/usr/bin/env python3
"""Search by examples (mvdb_index_search_examples_device) beside the passes it is built from.  Corpus 1M x 512 and 10M x 512
normalised synthetic rows added on the device; k = 10; (P, N) = (1, 0), (4, 2), (16, 16), (64, 64).  Device timings: hipEvents
on the current stream, the median of --reps calls after 3 warm-up calls.

  examples_ms          one search_examples_device call (D and I to device arrays, the examples' rows as skip rows), passes: its
                       corpus passes; this call and the assign call are timed alternately, two rounds each (*_ms_rounds), and a
                       figure is the mean of its two medians
  assign_ms            mvdb_index_assign_device with the same P + N vectors on the same index (labels and scores to device
                       arrays): the pass this one is modelled on, with as many passes; per_pass_ratio = examples_ms / assign_ms
                       (both divided by the same number of passes)
  scan_launch_ms       the clear and the scan launches of a call together, select_launch_ms the two selection launches
                       (mvdb_prof_read, calls of their own)
  exact_step_ms        the exact single-query scan (int8 prefilter switched off), one query: what a caller pays P + N times
                       when ranking per example; loop_of_scans_ms = (P + N) x exact_step_ms, without the n scores per example
                       such a caller would also copy down
  default_step_ms      the default single-query step (the int8 prefilter), for scale

One JSON line per cell, to stdout and to --out (default profiles/examples_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

from bench_distinct import launch_ms, timed_events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 0, 4, 2, 16, 16, 64, 64], help="P N pairs")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "examples_bench.jsonl"))
    args = ap.parse_args()
    d, k = 512, 10
    shapes = list(zip(args.shapes[0::2], args.shapes[1::2]))
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
        labels = torch.empty((n,), dtype=torch.int32, device="cuda")
        scores = torch.empty((n,), dtype=torch.float32, device="cuda")
        D = torch.empty((k,), dtype=torch.float32, device="cuda")
        I = torch.empty((k,), dtype=torch.int64, device="cuda")
        q = torch.from_numpy(idx.get_rows(7, 1) + np.float32(0.01)).cuda()

        def single():
            idx.search_device(q.data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)

        default_ms = timed_events(single, args.reps)
        idx.set_option("code8_single_query", 0)
        exact_ms = timed_events(single, args.reps)
        idx.set_option("code8_single_query", 1)

        for P, N in shapes:
            V = P + N
            # examples as a user has them: stored rows, slightly perturbed
            picks = rng.choice(n, V, replace=False)
            v_host = np.concatenate([idx.get_rows(int(r), 1) for r in picks]) + np.float32(0.02) * rng.standard_normal((V, d), dtype=np.float32)
            v = torch.from_numpy(np.ascontiguousarray(v_host, dtype=np.float32)).cuda()
            skip = torch.from_numpy(np.sort(picks).astype(np.int64)).cuda()

            def examples():
                idx.search_examples_device(v.data_ptr(), P, N, k, D.data_ptr(), I.data_ptr(), skip_rows_ptr=skip.data_ptr(), n_skip=V,
                                           stream=stream, normalize=True)

            def assign():
                idx.assign_device(v.data_ptr(), V, labels.data_ptr(), scores.data_ptr(), stream=stream, normalize_c=True)

            rec = {"bench": "examples", "n": n, "d": d, "P": P, "N": N, "k": k, "reps": args.reps}
            # the two calls alternate, two rounds each: a figure is the mean of its two medians, the rounds are in the record
            calls0, passes0 = idx.examples_counters()
            a0, ap0 = idx.assign_counters()
            rounds = [(timed_events(examples, args.reps), timed_events(assign, args.reps)) for _ in range(2)]
            calls1, passes1 = idx.examples_counters()
            a1, ap1 = idx.assign_counters()
            rec["examples_ms_rounds"] = [round(r[0], 4) for r in rounds]
            rec["assign_ms_rounds"] = [round(r[1], 4) for r in rounds]
            rec["examples_ms"] = round(float(np.mean([r[0] for r in rounds])), 4)
            rec["assign_ms"] = round(float(np.mean([r[1] for r in rounds])), 4)
            rec["passes"] = (passes1 - passes0) // (calls1 - calls0)
            rec["assign_passes"] = (ap1 - ap0) // (a1 - a0)
            rec["scan_launch_ms"], rec["scan_symbol"] = launch_ms(examples, "examples_scan", 2, per_call=True)
            rec["select_launch_ms"], _ = launch_ms(examples, "examples_select", 2, per_call=True)
            rec["assign_scan_launch_ms"], _ = launch_ms(assign, "assign_scan", 2, per_call=True)
            rec["per_pass_ms"] = round(rec["examples_ms"] / rec["passes"], 4)
            rec["assign_per_pass_ms"] = round(rec["assign_ms"] / rec["assign_passes"], 4)
            rec["per_pass_ratio"] = round(rec["per_pass_ms"] / rec["assign_per_pass_ms"], 3)
            rec["pass_TBps"] = round(n * (d * 4 + 8) / (rec["per_pass_ms"] * 1e-3) / 1e12, 2)
            rec["default_step_ms"] = round(default_ms, 4)
            rec["exact_step_ms"] = round(exact_ms, 4)
            rec["loop_of_scans_ms"] = round(V * exact_ms, 3)
            rec["speedup_over_loop_of_scans"] = round(V * exact_ms / rec["examples_ms"], 1)
            emit(rec)
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
