#!/usr/bin/env python3
"""Assignment (mvdb_index_assign_device) and one k-means iteration (mvdb_index_kmeans) beside what they replace.  Corpus 1M x 512
and 10M x 512 normalised synthetic rows added on the device; C = 8, 32, 256 vectors.  Device timings: hipEvents on the current
stream, the median of --reps calls after 3 warm-up calls; host timings: wall clock around synchronous calls.

  assign_ms            one assign_device call (labels and scores to device arrays), passes: its corpus passes
  maxsim_ms            baseline (a): search_maxsim_device with T = min(C, 32) vectors on the same index (documents of 8 rows,
                       k = 10) — the pass this one is modelled on; per_pass_ratio = (assign_ms / passes) / maxsim_ms
  scan_launch_ms       the clear and the scan launches of an assign call together (mvdb_prof_read, calls of their own)
  kmeans_iter_ms       one k-means iteration: (wall of mvdb_index_kmeans with max_iter = 3 - wall with max_iter = 1) / 2 — an
                       assignment, the changed-label count with its 8-byte read, the list build, the chunk sums, the finalise;
                       kmeans_call_ms: the whole max_iter = 1 call with its copies back (8 bytes per row)
  pull_search_ms       baseline (b), what a user wrote before: a second index over the C vectors, the stored rows pulled with
                       get_rows and pushed back up as query batches of --block rows (search, k = 1); measured on --pull-blocks
                       blocks and scaled to the corpus (pull_rows_measured)
  numpy_iter_ms        baseline (c), 1M rows only: one Lloyd iteration in numpy on the host's threads (--threads) over a host
                       copy of the rows — a matrix product, an argmax, a sorted segment sum — without the copy down

One JSON line per cell, to stdout and to --out (default profiles/kmeans_bench.jsonl)."""
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

from bench_distinct import launch_ms, timed_events  # noqa: E402


def wall_ms(fn, reps):
    fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(per))


def numpy_iteration(x, c):
    labels = np.argmax(x @ c.T, axis=1)
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=c.shape[0])
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    live = counts > 0
    sums = np.add.reduceat(x[order], starts[live], axis=0)
    out = c.copy()
    out[live] = sums / np.linalg.norm(sums, axis=1, keepdims=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--C", type=int, nargs="+", default=[8, 32, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kmeans-reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--pull-blocks", type=int, default=8)
    ap.add_argument("--numpy-rows", type=int, default=1_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    args = ap.parse_args()
    d, k = 512, 10
    torch.set_num_threads(args.threads)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2030)
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
        grouping = idx.grouping((np.arange(n, dtype=np.int64) // 8).astype(np.int32), (n + 7) // 8)
        labels = torch.empty((n,), dtype=torch.int32, device="cuda")
        scores = torch.empty((n,), dtype=torch.float32, device="cuda")
        D = torch.empty((k,), dtype=torch.float32, device="cuda")
        G = torch.empty((k,), dtype=torch.int32, device="cuda")
        host_rows = idx.get_rows(0, n) if n <= args.numpy_rows else None
        for C in args.C:
            c_host = rng.standard_normal((C, d), dtype=np.float32)
            c_host /= np.linalg.norm(c_host, axis=1, keepdims=True)
            c = torch.from_numpy(c_host).cuda()
            T = min(C, 32)

            def assign():
                idx.assign_device(c.data_ptr(), C, labels.data_ptr(), scores.data_ptr(), stream=stream, normalize_c=True)

            def maxsim():
                idx.search_maxsim_device(c.data_ptr(), T, k, grouping, D.data_ptr(), G.data_ptr(), stream=stream, normalize_q=True)

            rec = {"bench": "kmeans", "n": n, "d": d, "C": C, "reps": args.reps}
            calls0, passes0 = idx.assign_counters()
            rec["assign_ms"] = round(timed_events(assign, args.reps), 4)
            calls1, passes1 = idx.assign_counters()
            rec["passes"] = (passes1 - passes0) // (calls1 - calls0)
            rec["scan_launch_ms"], rec["scan_symbol"] = launch_ms(assign, "assign_scan", 2, per_call=True)
            rec["maxsim_T"] = T
            rec["maxsim_ms"] = round(timed_events(maxsim, args.reps), 4)
            rec["per_pass_ratio"] = round(rec["assign_ms"] / rec["passes"] / rec["maxsim_ms"], 3)

            one = wall_ms(lambda: idx.kmeans(c_host, 1), args.kmeans_reps)
            three = wall_ms(lambda: idx.kmeans(c_host, 3), args.kmeans_reps)
            rec["kmeans_updates_of_3"] = idx.kmeans(c_host, 3)[4]   # (3: the loop ran out, every iteration did an update)
            rec["kmeans_call_ms"] = round(one, 3)
            rec["kmeans_iter_ms"] = round((three - one) / 2, 3)

            # (b) a second index over the vectors, the stored rows as query batches
            centres_index = _native.FlatIndex(d)
            centres_index.add(c_host)
            blocks = min(args.pull_blocks, (n + args.block - 1) // args.block)
            measured = min(n, blocks * args.block)

            def pull():
                for r0 in range(0, measured, args.block):
                    rows = idx.get_rows(r0, min(args.block, n - r0))
                    centres_index.search(rows, 1)

            rec["pull_rows_measured"] = measured
            rec["pull_search_ms"] = round(wall_ms(pull, 1) * n / measured, 2)
            centres_index.close()
            rec["speedup_over_pull_search"] = round(rec["pull_search_ms"] / rec["assign_ms"], 1)

            if host_rows is not None:
                rec["numpy_threads"] = args.threads
                rec["numpy_iter_ms"] = round(wall_ms(lambda: numpy_iteration(host_rows, c_host), 1), 1)
                rec["speedup_over_numpy"] = round(rec["numpy_iter_ms"] / rec["kmeans_iter_ms"], 1)
            emit(rec)
        grouping.free()
        idx.close()
        del host_rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
