#!/usr/bin/env python3
"""Probed search (mvdb_index_search_probe_device) beside the routes that read the whole corpus.  Corpus: 1M and 10M x 512 rows
drawn from a mixture of 2,048 Gaussian directions (+ 0.35 noise per element, normalised on add), generated on the device;
queries: fresh draws from the same mixture.  Partition: spherical k-means (--kmeans-iter updates) on a sample of 256 C rows,
then every row labelled on the device.  Device timings: hipEvents on the current stream, the median of --reps calls after 3
warm-up calls, with the spread (min, max); host timings: wall clock around synchronous calls.

One "build" record per (n, C):
  kmeans_ms            k-means on the sample (mvdb_index_kmeans under a list-form row set), wall clock
  assign_ms            one assign of every row to the C centres (assign_device), device time
  create_ms            mvdb_partition_create with labels = NULL: that assign, the list build, the copies back, wall clock
  default_step_ms      in the same process: one single-query search on the default route (the int8 prefilter where it applies)
  exact_step_ms        ... and with that route switched off: the exact scan
One "cell" record per (n, C, nprobe, nq):
  ms, ms_min, ms_max   one search_probe_device call, k = 10
  rows_touched         mean per query, from the labels and the probes: the sizes of the lists of the query's nprobe best centres
  bytes_touched        per call: nq x (rows_touched x (4 d + 4) + C x 4 d)
  tb_per_s             bytes_touched / ms
  model_ms             bytes_touched / 6.4 TB/s (the grouped scan's measured gather rate): the launches come on top
  recall_at_10         against the exact search of the same queries in the same run
  ratio_to_default     default_step_ms x nq / ms: how many default single-query steps one call replaces, per query
  launch_ms            nq = 1 only: the time under each profiling label of the call (calls of their own)

One JSON line per record, to stdout and to --out (default profiles/probe_bench.jsonl)."""
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

GATHER_TB_S = 6.4
LABELS = ("ip_scan_scores", "probe_plan", "probe_scan", "probe_merge")


def spread_events(fn, reps, warm=3):
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


def mixture(gen, directions, n, noise=0.35):
    pick = torch.randint(directions.shape[0], (n,), device="cuda", generator=gen)
    return directions[pick] + noise * torch.randn((n, directions.shape[1]), device="cuda", generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--C", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kmeans-iter", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.jsonl"))
    args = ap.parse_args()
    d, k, chunk = 512, 10, 1_000_000
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2031)
    rng = np.random.default_rng(2031)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    directions = torch.randn((2048, d), device="cuda", generator=gen)
    nq_max = max(args.nq)
    q = mixture(gen, directions, nq_max).contiguous()
    q_host = q.cpu().numpy()
    D = torch.empty((nq_max, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq_max, k), dtype=torch.int64, device="cuda")

    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        for r0 in range(0, n, chunk):
            block = mixture(gen, directions, min(chunk, n - r0)).contiguous()
            torch.cuda.synchronize()
            idx.add_device(block.data_ptr(), block.shape[0], normalize=True)
            del block
        torch.cuda.empty_cache()

        def single():
            idx.search_device(q.data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)

        default_ms = spread_events(single, 50, warm=40)[0]   # (the first eligible queries build the int8 code)
        idx.set_option("code8_single_query", 0)
        exact_ms = spread_events(single, args.reps)[0]
        idx.set_option("code8_single_query", 1)
        _, exact_I = idx.search(q_host, k, normalize_q=True)

        labels_dev = torch.empty((n,), dtype=torch.int32, device="cuda")
        for C in args.C:
            m = min(n, 256 * C)
            sample = np.sort(rng.choice(n, m, replace=False)) if m < n else None
            picked = rng.choice(sample if sample is not None else n, C, replace=False)
            start = np.concatenate([idx.get_rows(int(r), 1) for r in picked])
            rs = idx.rowset(sample) if sample is not None else None
            t0 = time.perf_counter()
            centres = idx.kmeans(start, args.kmeans_iter, rowset=rs)[0]
            kmeans_ms = (time.perf_counter() - t0) * 1e3
            c_dev = torch.from_numpy(centres).cuda()
            assign_ms = spread_events(lambda: idx.assign_device(c_dev.data_ptr(), C, labels_dev.data_ptr(), stream=stream), 1, warm=1)[0]
            t0 = time.perf_counter()
            part = idx.partition(centres)
            create_ms = (time.perf_counter() - t0) * 1e3
            sizes = part.sizes()
            emit({"bench": "probe_build", "n": n, "d": d, "C": C, "train_rows": m, "kmeans_iter": args.kmeans_iter,
                  "kmeans_ms": round(kmeans_ms, 1), "assign_ms": round(assign_ms, 1), "create_ms": round(create_ms, 1),
                  "list_min": int(sizes.min()), "list_max": int(sizes.max()), "list_mean": round(float(sizes.mean()), 1),
                  "default_step_ms": round(default_ms, 4), "exact_step_ms": round(exact_ms, 4)})
            cidx = _native.FlatIndex(d)
            cidx.add(part.centres())
            for nprobe in args.nprobe:
                _, P = cidx.search(q_host, nprobe, normalize_q=True)
                touched = sizes[P].sum(axis=1)
                for nq in args.nq:
                    def probe():
                        idx.search_probe_device(q.data_ptr(), nq, k, nprobe, part, D.data_ptr(), I.data_ptr(), stream=stream,
                                                normalize_q=True)

                    ms, lo, hi = spread_events(probe, args.reps)
                    torch.cuda.synchronize()
                    got = I[:nq].cpu().numpy()
                    recall = float(np.mean([len(np.intersect1d(got[i], exact_I[i])) / k for i in range(nq)]))
                    rows = float(touched[:nq].mean())
                    nbytes = nq * (rows * (4 * d + 4) + C * 4 * d)
                    rec = {"bench": "probe", "n": n, "d": d, "C": C, "nprobe": nprobe, "nq": nq, "k": k, "reps": args.reps,
                           "ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "rows_touched": round(rows, 1),
                           "bytes_touched": int(nbytes), "tb_per_s": round(nbytes / ms / 1e9, 3),
                           "model_ms": round(nbytes / GATHER_TB_S / 1e9, 4), "recall_at_10": round(recall, 4),
                           "default_step_ms": round(default_ms, 4), "exact_step_ms": round(exact_ms, 4),
                           "ratio_to_default": round(default_ms * nq / ms, 2)}
                    if nq == 1:
                        rec["launch_ms"] = {label: launch_ms(probe, label, 5, per_call=True)[0] for label in LABELS}
                    emit(rec)
            cidx.close()
            part.free()
        idx.close()
        del labels_dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
