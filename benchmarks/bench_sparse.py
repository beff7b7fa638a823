#!/usr/bin/env python3
"""Sparse and hybrid search (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH") beside the exact dense scan and beside what a user
writes without them, timed in the same process.  Corpus: 1M and 10M normalised synthetic rows at d = 512 added on the device;
sparse rows with log-uniform ("Zipf", exponent 1) indices over dim = 2^18 and a mean of about 64 and of about 128 distinct
non-zeros per row (drawn on the device, made distinct per row; ``mean_nnz`` is what came out); queries of 16 and of 128 distinct
terms drawn the same way, weights uniform in (0, 1); k = 10.  One record per (rows, mean, query terms):

  exact_step_ms         (a) the exact dense single-query scan (index option code8_single_query = 0), device time, median
  exact_GBps            ... its rows' bytes per second
  score_launch_ms       the scoring launch alone (sparse_scan_kernel through mvdb_index_sparse_scores; mvdb_prof_read "sparse_scan")
  score_GBps            ... 8 bytes per stored non-zero per second; score_vs_exact = score_GBps / exact_GBps
  sparse_search_ms      mvdb_index_search_sparse, host entry point (query upload, launch, merge, results back), wall clock, median
  hybrid_search_ms      mvdb_index_search_hybrid, host entry point, wall clock, median — what find_most_similar_sparse /
                        find_most_similar_hybrid resolve to once the store is resident
  host_csr_ms           (b) scipy.sparse ``csr @ q`` on the host (float32) ...
  host_boosted_ms       ... then a freshly uploaded row term and mvdb_index_search_boosted; host_total_ms is their sum
  rerank_ms             (c) the dense top 100, then the hybrid score of those 100 rows on the host
  rerank_lost           ... and how many of the exact hybrid top 10 that misses, mean over --quality-queries queries (min, max beside it)
  store_build_s         mvdb_sparse_create: checks, tiles, interleaving and upload

Hybrid weights: dense 1.0, sparse 0.05.  One JSON line per record, to stdout and to --out (default profiles/sparse_bench.jsonl)."""
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

from bench_boost import timed  # noqa: E402
from bench_distinct import launch_ms  # noqa: E402

DIM = 1 << 18
CHUNK = 500_000


def draw(rows, per_row, gen):
    """Sorted keys row * DIM + index of `per_row` log-uniform draws per row, duplicates removed (device tensor)."""
    u = torch.rand(rows * per_row, device="cuda", generator=gen)
    idx = torch.clamp(torch.exp(u * float(np.log(DIM))).long() - 1, 0, DIM - 1)
    key = torch.arange(rows, device="cuda").repeat_interleave(per_row) * DIM + idx
    return torch.unique(key)


def make_csr(n, mean, seed):
    """(indptr int64, indices int32, values float32) with about `mean` distinct indices per row."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    per_row = mean
    for _ in range(3):      # calibrate the draws per row on 20,000 rows
        got = draw(20_000, per_row, gen).numel() / 20_000
        per_row = max(1, int(round(per_row * mean / got)))
    counts, indices = [], []
    for r0 in range(0, n, CHUNK):
        rows = min(CHUNK, n - r0)
        key = draw(rows, per_row, gen)
        counts.append(torch.bincount(key // DIM, minlength=rows).cpu().numpy())
        indices.append((key % DIM).to(torch.int32).cpu().numpy())
        del key
    indptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    indices = np.concatenate(indices)
    values = np.random.default_rng(seed).random(len(indices), dtype=np.float32)
    return indptr, indices, values


def make_query(m, rng):
    """m distinct log-uniform indices (ascending) and their weights."""
    idx = np.empty(0, np.int64)
    while len(idx) < m:
        more = (np.exp(rng.random(4 * m) * np.log(DIM)).astype(np.int64) - 1).clip(0, DIM - 1)
        idx = np.unique(np.concatenate([idx, more]))
    idx = np.sort(rng.permutation(idx)[:m])
    return idx, rng.random(m).astype(np.float32)


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(per)), 4)


def main():
    import scipy.sparse as sp
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--means", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--terms", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quality-queries", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it anew")
    args = ap.parse_args()
    d, k, w_d, w_s = 512, 10, 1.0, 0.05
    stream = torch.cuda.current_stream().cuda_stream
    sink = open(args.out, "a" if args.append else "w") if args.out else None

    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        idx.set_option("code8_single_query", 0)
        D = torch.empty((1, k), dtype=torch.float32, device="cuda")
        I = torch.empty((1, k), dtype=torch.int64, device="cuda")
        rng = np.random.default_rng(2040)
        picks = rng.choice(n, args.quality_queries, replace=False)
        dense = np.concatenate([idx.get_rows(int(r), 1) for r in picks]) + np.float32(0.02) * rng.standard_normal((len(picks), d), dtype=np.float32)
        dense = np.ascontiguousarray(dense, dtype=np.float32)
        qd = torch.from_numpy(dense[:1]).cuda()
        for mean in args.means:
            indptr, indices, values = make_csr(n, mean, 7 + mean)
            t0 = time.perf_counter()
            store = idx.sparse(indptr, indices, values, DIM)
            build_s = time.perf_counter() - t0
            csr = sp.csr_matrix((values, indices, indptr), shape=(n, DIM))
            for m in args.terms:
                q_idx, q_val = make_query(m, rng)
                query = (q_idx, q_val)
                rec = {"bench": "sparse", "n": n, "d": d, "k": k, "dim": DIM, "mean_nnz": round(store.nnz / n, 2), "nnz": store.nnz,
                       "query_terms": m, "reps": args.reps, "dense_weight": w_d, "sparse_weight": w_s, "store_build_s": round(build_s, 2)}
                exact = timed(lambda: idx.search_device(qd.data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True),
                              args.reps)[0]
                rec["exact_step_ms"] = round(exact, 4)
                rec["exact_GBps"] = round(n * d * 4 / (exact * 1e-3) / 1e9, 1)
                rec["score_launch_ms"], rec["score_symbol"] = launch_ms(lambda: idx.sparse_scores(store, *query, with_matched=False),
                                                                        "sparse_scan", 5, per_call=True)
                rec["score_GBps"] = round(store.nnz * 8 / (rec["score_launch_ms"] * 1e-3) / 1e9, 1)
                rec["score_vs_exact"] = round(rec["score_GBps"] / rec["exact_GBps"], 3)
                rec["sparse_search_ms"] = wall(lambda: idx.search_sparse(store, [query], k), args.reps)
                rec["hybrid_search_ms"] = wall(lambda: idx.search_hybrid(store, dense[:1], [query], k, dense_weight=w_d, sparse_weight=w_s,
                                                                         normalize_q=True), args.reps)
                # (b) what a user writes today: the sparse scores on the host, uploaded as a row term of a boosted search
                qvec = np.zeros(DIM, np.float32)
                qvec[q_idx] = q_val
                rec["host_csr_ms"] = wall(lambda: csr @ qvec, 3, warm=1)
                T = (csr @ qvec).astype(np.float32)
                rec["host_boosted_ms"] = wall(lambda: idx.search_boosted(dense[:1], k, [idx.rowterm(T)], [w_s], score_weight=w_d, normalize_q=True),
                                              3, warm=1)
                rec["host_total_ms"] = round(rec["host_csr_ms"] + rec["host_boosted_ms"], 4)
                # (c) the dense top 100 re-ranked on the host, against the exact hybrid top 10
                lost, rerank = [], []
                for j in range(len(picks)):
                    _, top = idx.search_hybrid(store, dense[j], [query], k, dense_weight=w_d, sparse_weight=w_s, normalize_q=True)
                    t0 = time.perf_counter()
                    Df, If = idx.search(dense[j:j + 1], 100, normalize_q=True)
                    S = np.float32(w_d) * Df[0] + np.float32(w_s) * (csr[If[0]] @ qvec)
                    kept = If[0][np.argsort(-S, kind="stable")[:k]]
                    rerank.append((time.perf_counter() - t0) * 1e3)
                    lost.append(len(set(top[0].tolist()) - set(kept.tolist())))
                rec["rerank_ms"] = round(float(np.median(rerank)), 4)
                rec["rerank_lost"] = round(float(np.mean(lost)), 2)
                rec["rerank_lost_min_max"] = [int(min(lost)), int(max(lost))]
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
            del store, csr, indptr, indices, values
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
