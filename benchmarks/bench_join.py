#!/usr/bin/env python3
"""Duplicate-pair search (mvdb_index_range_join) beside what a user had to write without it.  Corpora: 1M x 512, and 200k x 384
as a short cell; normalised Gaussian rows of which 1 % are near-copies (cosine ~0.995) of an earlier row.  Threshold 0.95.

Per cell three forms that do the same job — every (earlier, later) pair at or above the threshold — with the pair count of
each recorded, so that the forms provably agree:

  join          FlatIndex.range_join over all rows (option join_shared = 1, the default): row numbers up, pairs down
  loop_shared   get_rows + range_search in blocks of 256 queries with range_shared = 2, keeping I < i on the host: the rows
                come down and go up again, every pair is found from both ends
  loop_exact    the same with range_shared = 0 (one fp32 pass per query) — the 200k cell only: at 1M rows it is hours

Wall-clock seconds of whole calls (time.perf_counter around host entry points that return host arrays: the device is idle
when they return), one un-timed warm-up call of each form over the first 4,096 rows, then the median of --reps runs
(loop_exact: one run).  One JSON line per cell, to stdout and to --out (default profiles/join_bench.jsonl)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

CELLS = {"200k": (200_000, 384, True), "1M": (1_000_000, 512, False)}
THRESHOLD = 0.95


def corpus(n, d, seed=2029):
    rng = np.random.default_rng(seed)
    x = np.empty((n, d), np.float32)
    for b0 in range(0, n, 65536):
        x[b0:b0 + 65536] = rng.standard_normal((min(65536, n - b0), d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    later = np.sort(rng.choice(np.arange(1, n), n // 100, replace=False))
    earlier = (rng.random(later.shape[0]) * later).astype(np.int64)          # each a near-copy of some earlier ORIGINAL row
    earlier = np.where(np.isin(earlier, later), 0, earlier)
    x[later] = x[earlier] + 0.1 / np.sqrt(d) * rng.standard_normal((later.shape[0], d), dtype=np.float32)
    x[later] /= np.linalg.norm(x[later], axis=1, keepdims=True)
    return x


def loop(idx, rows, shared):
    """what a user writes without the join: the pairs whose later member is in `rows`"""
    idx.set_option("range_shared", shared)
    pairs = 0
    for b0 in range(0, len(rows), 256):
        part = rows[b0:b0 + 256]
        q = idx.get_rows(int(part[0]), len(part))
        lims, D, I = idx.range_search(q, THRESHOLD, normalize_q=False, cap=64)
        pairs += int((I < np.repeat(part, np.diff(lims))).sum())
    return pairs


def timed(fn, reps):
    per, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        per.append(time.perf_counter() - t0)
    return float(np.median(per)), out


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=["200k", "1M"], choices=sorted(CELLS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=commit(), help="recorded with every line (default: git's HEAD, if this is a checkout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_bench.jsonl"))
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    for cell in args.cells:
        n, d, with_exact = CELLS[cell]
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add(corpus(n, d))
        every = np.arange(n, dtype=np.int64)
        warm = every[:4096]
        rec = {"bench": "join", "cell": cell, "n": n, "d": d, "threshold": THRESHOLD, "reps": args.reps, "commit": args.commit}
        idx.range_join(THRESHOLD, rows=warm)
        calls0, fell0 = idx.join_counters()
        rec["join_s"], (_, lims, _, _) = timed(lambda: idx.range_join(THRESHOLD), args.reps)
        rec["join_pairs"] = int(lims[-1])
        calls1, fell1 = idx.join_counters()
        rec["join_shared_calls_per_run"] = (calls1 - calls0) / args.reps
        rec["join_fallback_rows_per_run"] = (fell1 - fell0) / args.reps
        rec["count_s"], count = timed(lambda: idx.range_join_count(THRESHOLD), args.reps)
        rec["count_pairs"] = count
        loop(idx, warm, 2)
        rec["loop_shared_s"], rec["loop_shared_pairs"] = timed(lambda: loop(idx, every, 2), max(1, args.reps - 1))
        if with_exact:
            loop(idx, warm, 0)
            rec["loop_exact_s"], rec["loop_exact_pairs"] = timed(lambda: loop(idx, every, 0), 1)
        else:
            rec["loop_exact_s"] = None   # not measured: n fp32 passes over n rows
        rec["forms_agree"] = len({v for k, v in rec.items() if k.endswith("_pairs")}) == 1
        rec["loop_shared_over_join"] = round(rec["loop_shared_s"] / rec["join_s"], 2)
        for k in ("join_s", "count_s", "loop_shared_s", "loop_exact_s"):
            rec[k] = round(rec[k], 4) if rec[k] is not None else None
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
        idx.close()


if __name__ == "__main__":
    main()
