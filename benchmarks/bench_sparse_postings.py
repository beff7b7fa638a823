#!/usr/bin/env python3
"""The sparse scoring launch through the posting lists (include/mvdb.h "SPARSE POSTINGS") beside the CSR pass, in one process on
one store: bench_sparse.py's corpus — log-uniform indices over dim = 2^18, about 64 and about 128 distinct non-zeros per row, 1M
and 10M rows at d = 512 — and queries of 4, 16, 128 and 1,024 distinct terms drawn the same way.  One record per (rows, mean,
query terms):

  csr_launch_ms         sparse_scan_kernel through mvdb_index_sparse_scores, index option sparse_postings = 0 (mvdb_prof_read
                        "sparse_scan"): the parent's unchanged kernel, the yardstick
  postings_launch_ms    sparse_postings_kernel through the same call, option 1 (mvdb_prof_read "sparse_postings")
  launch_ratio          csr_launch_ms / postings_launch_ms (above 1: the posting launch is faster)
  entries               list entries of the query's terms (mvdb_index_sparse_postings_counters), entries_of_nnz = entries / nnz
  postings_GBps         8 bytes per touched entry per second
  bits_equal            the two launches' columns compared as bits, and their matched counts
  sparse_search_ms      mvdb_index_search_sparse, host entry point, wall clock, median: csr_ / postings_
  hybrid_search_ms      mvdb_index_search_hybrid, host entry point, wall clock, median: csr_ / postings_
  build_s               mvdb_sparse_build_postings (device build and the host copy of the directory), wall clock
  postings_bytes        8 nnz + 8 (dim + 1)

One JSON line per record, to stdout and to --out (default profiles/sparse_postings_bench.jsonl)."""
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

from bench_distinct import launch_ms  # noqa: E402
from bench_sparse import DIM, make_csr, make_query, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--means", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--terms", type=int, nargs="+", default=[4, 16, 128, 1024])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_postings_bench.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it anew")
    args = ap.parse_args()
    d, k, w_d, w_s = 512, 10, 1.0, 0.05
    sink = open(args.out, "a" if args.append else "w") if args.out else None

    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        idx.set_option("code8_single_query", 0)
        rng = np.random.default_rng(2040)
        dense = np.ascontiguousarray(idx.get_rows(int(rng.integers(n)), 1) + np.float32(0.02) * rng.standard_normal((1, d), dtype=np.float32))
        for mean in args.means:
            indptr, indices, values = make_csr(n, mean, 7 + mean)
            store = idx.sparse(indptr, indices, values, DIM)
            del indptr, indices, values
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store.build_postings()
            build_s = time.perf_counter() - t0
            for m in args.terms:
                query = make_query(m, rng)
                rec = {"bench": "sparse_postings", "n": n, "d": d, "k": k, "dim": DIM, "mean_nnz": round(store.nnz / n, 2), "nnz": store.nnz,
                       "query_terms": m, "reps": args.reps, "build_s": round(build_s, 3), "postings_bytes": 8 * store.nnz + 8 * (DIM + 1)}
                before = idx.sparse_postings_counters()[2]
                T1, m1 = idx.sparse_scores(store, *query)
                rec["entries"] = idx.sparse_postings_counters()[2] - before
                rec["entries_of_nnz"] = round(rec["entries"] / store.nnz, 5)
                for option, name, label in ((0, "csr", "sparse_scan"), (1, "postings", "sparse_postings")):
                    idx.set_option("sparse_postings", option)
                    if option == 0:
                        T0, m0 = idx.sparse_scores(store, *query)
                        rec["bits_equal"] = bool(np.array_equal(T0.view(np.uint32), T1.view(np.uint32)) and np.array_equal(m0, m1))
                    rec[f"{name}_launch_ms"], rec[f"{name}_symbol"] = launch_ms(lambda: idx.sparse_scores(store, *query, with_matched=False),
                                                                                label, args.reps, per_call=True)
                    rec[f"{name}_sparse_search_ms"] = wall(lambda: idx.search_sparse(store, [query], k), args.reps)
                    rec[f"{name}_hybrid_search_ms"] = wall(lambda: idx.search_hybrid(store, dense, [query], k, dense_weight=w_d, sparse_weight=w_s,
                                                                                     normalize_q=True), args.reps)
                rec["launch_ratio"] = round(rec["csr_launch_ms"] / rec["postings_launch_ms"], 2)
                rec["postings_GBps"] = round(rec["entries"] * 8 / (rec["postings_launch_ms"] * 1e-3) / 1e9, 1)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
            del store
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
