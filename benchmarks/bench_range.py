#!/usr/bin/env python3
"""Range search (mvdb_index_range_search_device) against the only way to get the same answer before it existed: a top-k
search with k = the count rounded up to the next power of two (the k > 64 route).  Corpus 10M x 512 and 1M x 512 normalised
synthetic rows; one threshold per cell, chosen from the normal approximation of the cosine of random unit vectors so that
about 10 / 1,000 / 100,000 rows of the whole corpus pass, plus a dense cell (about a quarter of the rows); no filter, a 30 %
row list, a 90 % bitmap (the thresholds stay, so fewer rows pass under a filter: the measured counts are in the record);
nq = 1 and 16.  Per cell, device buffers, hipEvents, medians of --reps after 3 warm-up calls:

  a  range_search_device, cap = the largest count rounded up to a power of two; beside it the range scan launch alone
     (mvdb_prof_read("ip_scan_range"), collected in calls of its own)
  b  search_device / search_rowset_device with k = that power of two            (--columns parent)
  c  the k = 10 single-query search of the same session, and its scan launch ("ip_scan") — nq = 1 cells only: the nq = 16
     cells carry no scan-launch ratio

Two runs: `--columns range --out A.jsonl` on this build, then `--columns parent --merge-from A.jsonl --out B.jsonl` with
MVDB_LIBMVDB naming the parent commit's library (column b needs nothing this build adds); B holds the merged records.

`--batch`: the BATCH cells of the shared pass instead — 1M x 512 and 10M x 512, 8 / 32 / 128 / 256
queries, thresholds for about 10 and about 1,000 passing rows per query and one dense cell (1 % of the rows).  Per cell, the same
device call under option "range_shared" = 0 (one fp32 pass per query: the route every batch took before the shared pass
existed, same kernels) and = 1 (the automatic rule), the nomination launch alone ("ip_scan_range_half"), and beside it the
certified top-k call (k = 10) of the same (nq, n, d), which streams the same shadow.  The "per_query" column is THIS build
with the route switched off, not the parent commit's library: the parent has no option to switch, and its range_scan_kernel
lacks the two branches this build adds at the top of the kernel (the per-query threshold pointer and the device gate, both
NULL on that column)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

RANGE_SYMBOLS = ("mvdb_index_range_search", "mvdb_index_range_search_device")


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


def launch_ms(fn, label, reps):
    """Mean time of the launches recorded under `label` while fn runs `reps` times (profiling events on; calls of their own)."""
    fn()
    torch.cuda.synchronize()
    _native.prof_read(label)
    _native.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _native.prof_enable(False)
    launches, ms = _native.prof_read(label)
    return (ms / launches if launches else None), _native.prof_symbol(label)


def pow2ceil(v):
    p = 2
    while p < v:
        p <<= 1
    return p


def cell_key(c):
    return (c["n"], c["target"], c["filter"], c["nq"])


def batch_cells(args):
    d = 512
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    sd = 1.0 / np.sqrt(d)
    sink = open(args.out, "w") if args.out else None
    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        qh = rng.standard_normal((max(args.batch_nq), d), dtype=np.float32)
        q = torch.from_numpy(qh).cuda()
        for target in (10, 1_000, n // 100):
            t = float(sd * statistics.NormalDist().inv_cdf(1.0 - target / n))
            for nq in args.batch_nq:
                idx.set_option("range_shared", 1)
                counts = idx.range_count(qh[:nq], t, normalize_q=True)
                cap = pow2ceil(int(counts.max()))
                ct = torch.empty(nq, dtype=torch.int64, device="cuda")
                D = torch.empty((nq, cap), dtype=torch.float32, device="cuda")
                I = torch.empty((nq, cap), dtype=torch.int64, device="cuda")

                def ranged():
                    idx.range_search_device(q.data_ptr(), nq, t, cap, ct.data_ptr(), D.data_ptr(), I.data_ptr(), stream=stream,
                                            normalize_q=True)

                rec = {"bench": "range_batch", "n": n, "d": d, "target": target, "threshold": round(t, 6), "nq": nq,
                       "counts_min": int(counts.min()), "counts_max": int(counts.max()), "cap": cap}
                idx.set_option("range_shared", 0)
                slow_reps = max(2, min(args.reps, int(2e9 // (n * nq)) or 2))     # (256 fp32 passes over 10M rows: 0.7 s a call)
                rec["per_query_ms"] = round(timed_events(ranged, slow_reps, warm=1), 4)
                ref = (ct.cpu().numpy().copy(), D.cpu().numpy().view(np.uint32).copy(), I.cpu().numpy().copy())
                idx.set_option("range_shared", 1)
                calls, fb0 = idx.range_counters()[:2]
                rec["auto_ms"] = round(timed_events(ranged, args.reps), 4)
                torch.cuda.synchronize()
                after = idx.range_counters()
                rec["auto_took_shared"] = after[0] > calls
                rec["fallback_queries_per_call"] = round((after[1] - fb0) / (args.reps + 3), 2)
                rec["candidates"] = after[2]
                rec["identical"] = bool(np.array_equal(ct.cpu().numpy(), ref[0]) and np.array_equal(D.cpu().numpy().view(np.uint32), ref[1])
                                        and np.array_equal(I.cpu().numpy(), ref[2]))
                rec["speedup"] = round(rec["per_query_ms"] / rec["auto_ms"], 2)
                if rec["auto_took_shared"]:
                    for label, key in (("ip_scan_range_half", "nominate_launch_ms"), ("ip_scan_range_rescore", "rescore_launch_ms"),
                                       ("ip_scan_range_fallback", "fallback_launch_ms")):
                        ms, sym = launch_ms(ranged, label, args.reps)
                        rec[key] = round(ms, 4) if ms is not None else None
                    Dk = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
                    Ik = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
                    k10 = lambda: idx.search_device(q.data_ptr(), nq, 10, Dk.data_ptr(), Ik.data_ptr(), stream=stream, normalize_q=True)
                    rec["topk10_device_ms"] = round(timed_events(k10, args.reps), 4)
                    ms, sym = launch_ms(k10, "ip_scan_half", args.reps)
                    rec["topk10_half_launch_ms"], rec["topk10_half_symbol"] = (round(ms, 4) if ms is not None else None), sym
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
                del D, I
                torch.cuda.empty_cache()
        idx.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="the batch cells of the shared pass")
    ap.add_argument("--batch-nq", type=int, nargs="+", default=[8, 32, 128, 256])
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000_000, 1_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--columns", choices=("range", "parent"), default="range")
    ap.add_argument("--merge-from", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.batch:
        return batch_cells(args)
    if args.columns == "parent":
        for name in RANGE_SYMBOLS:          # the parent's library does not export them
            _native.PROTOTYPES.pop(name, None)
    known = {}
    if args.merge_from:
        for line in open(args.merge_from):
            rec = json.loads(line)
            known[cell_key(rec)] = rec
    d = 512
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2025)
    sd = 1.0 / np.sqrt(d)
    sink = open(args.out, "w") if args.out else None
    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        perm = rng.permutation(n)
        filters = {"none": None, "list30": idx.rowset(np.sort(perm[:n * 3 // 10])), "bitmap90": idx.rowset(np.sort(perm[:n * 9 // 10]))}
        assert not filters["list30"].is_bitmap and filters["bitmap90"].is_bitmap
        qh = rng.standard_normal((max(args.nq), d), dtype=np.float32)
        q = torch.from_numpy(qh).cuda()
        for target in (10, 1_000, 100_000, n // 4):
            t = float(sd * statistics.NormalDist().inv_cdf(1.0 - target / n))
            for fname, rs in filters.items():
                for nq in args.nq:
                    rec = {"bench": "range", "n": n, "d": d, "target": target, "threshold": round(t, 6), "filter": fname, "nq": nq,
                           "reps": args.reps}
                    rec.update(known.get(cell_key(rec), {}))
                    rec["library_" + args.columns] = os.path.basename(os.path.dirname(_native.LIB_PATH)) + "/" + os.path.basename(_native.LIB_PATH)

                    def topk(kk, nn):
                        D = torch.empty((nn, kk), dtype=torch.float32, device="cuda")
                        I = torch.empty((nn, kk), dtype=torch.int64, device="cuda")
                        if rs is None:
                            return lambda: idx.search_device(q.data_ptr(), nn, kk, D.data_ptr(), I.data_ptr(), stream=stream, normalize_q=True)
                        return lambda: idx.search_rowset_device(q.data_ptr(), nn, kk, rs, D.data_ptr(), I.data_ptr(), stream=stream,
                                                                normalize_q=True)

                    if args.columns == "range":
                        counts = idx.range_count(qh[:nq], t, rowset=rs, normalize_q=True)
                        cap = pow2ceil(int(counts.max()))
                        ct = torch.empty(nq, dtype=torch.int64, device="cuda")
                        D = torch.empty((nq, cap), dtype=torch.float32, device="cuda")
                        I = torch.empty((nq, cap), dtype=torch.int64, device="cuda")

                        def ranged():
                            idx.range_search_device(q.data_ptr(), nq, t, cap, ct.data_ptr(), D.data_ptr(), I.data_ptr(), rowset=rs,
                                                    stream=stream, normalize_q=True)

                        rec["counts_min"], rec["counts_max"], rec["cap"] = int(counts.min()), int(counts.max()), cap
                        rec["a_range_device_ms"] = round(timed_events(ranged, args.reps), 4)
                        ms, sym = launch_ms(ranged, "ip_scan_range", args.reps)
                        rec["a_scan_launch_ms"], rec["a_scan_symbol"] = (round(ms, 4) if ms is not None else None), sym
                        del D, I
                        if nq == 1:
                            k10 = topk(10, 1)
                            rec["c_k10_device_ms"] = round(timed_events(k10, args.reps), 4)
                            ms, sym = launch_ms(k10, "ip_scan", args.reps)
                            rec["c_scan_launch_ms"], rec["c_scan_symbol"] = (round(ms, 4) if ms is not None else None), sym
                            if rec["a_scan_launch_ms"] and rec["c_scan_launch_ms"]:
                                rec["a_over_c_scan_launch"] = round(rec["a_scan_launch_ms"] / rec["c_scan_launch_ms"], 4)
                    else:
                        kk = rec.get("cap") or pow2ceil(int(target * 1.1))
                        rec["b_k"] = kk
                        rec["b_topk_device_ms"] = round(timed_events(topk(kk, nq), args.reps), 4)
                        if "a_range_device_ms" in rec:
                            rec["b_over_a"] = round(rec["b_topk_device_ms"] / rec["a_range_device_ms"], 2)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if sink:
                        sink.write(line + "\n")
                        sink.flush()
                    torch.cuda.empty_cache()
        for rs in filters.values():
            if rs is not None:
                rs.close()
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
