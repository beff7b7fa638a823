#!/usr/bin/env python3
"""The MX index (csrc/mx.hip) -> profiles/mx_bench.jsonl, one JSON line per cell group.

timings   10M rows at d = 512 and 1024, MXFP4 and MXFP8, k = 10, nq = 1, 4, 8, 32, 64, 256: the whole device call (query encode +
          scan + merge; hipEvent medians, device buffers) and the same call on a ONE-row index, whose difference is reported as
          the scan's share, with the bytes the scan reads (codes + scale planes) over that time.  In the same process: SQ4Index,
          Cos8Index and BitsIndex over the same number of rows of the same width, and benchmarks/micro/stream_read's best rate
          (run first, as a child process, when the binary has been built).
recall    1M x 512 rows of bench_pq.py's clustered mixture: the share of the exact flat top 10 inside the MX top 10 and top 64,
          both formats.
QB and the tiles in flight are first guesses, not swept."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from benchmarks.bench_sq4 import stream_read_gbps  # noqa: E402

N, K = 10_000_000, 10
NQS = (1, 4, 8, 32, 64, 256)


def main():
    n = int(os.environ.get("MVDB_BENCH_MX_ROWS", N))
    ceiling = stream_read_gbps()
    import torch
    from minivectordb_amd import _native

    def timed(fn, reps=15, warm=3):
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

    def fill(idx, d, rows):
        gen = torch.Generator(device="cuda").manual_seed(d)
        step = 1 << 18
        for r0 in range(0, rows, step):
            x = torch.randn((min(step, rows - r0), d), generator=gen, device="cuda", dtype=torch.float32)
            idx.add_device(x.data_ptr(), x.shape[0])
        torch.cuda.synchronize()

    def call_times(idx, one, d):
        out = {}
        for nq in NQS:
            q = torch.randn((nq, d), device="cuda", dtype=torch.float32)
            D = torch.empty((nq, K), device="cuda", dtype=torch.float32)
            I = torch.empty((nq, K), device="cuda", dtype=torch.int64)
            full = timed(lambda: idx.search_device(q.data_ptr(), nq, K, D.data_ptr(), I.data_ptr()))
            base = timed(lambda: one.search_device(q.data_ptr(), nq, K, D.data_ptr(), I.data_ptr()))
            out[nq] = (full, full - base)
        return out

    rows_out = []
    for d in (512, 1024):
        sq, sq1 = _native.SQ4Index(d), _native.SQ4Index(d)
        for s in (sq, sq1):
            s.set_ranges(np.full(d, -4, np.float32), np.full(d, 4, np.float32))
        fill(sq, d, n), fill(sq1, d, 1)
        sq_t = call_times(sq, sq1, d)
        sq.close(), sq1.close()
        torch.cuda.empty_cache()
        other = {"bench": "mx_vs_cos8_bits", "n": n, "d": d, "k": K}
        c8, bx = _native.Cos8Index(d), _native.BitsIndex(d)
        c8.reserve(n), bx.reserve(n)
        gen = torch.Generator(device="cuda").manual_seed(d)
        for r0 in range(0, n, 1 << 18):
            xb = torch.randn((min(1 << 18, n - r0), d), generator=gen, device="cuda")
            c8.add_device(xb.data_ptr(), xb.shape[0])
            bx.add_float_device(xb.data_ptr(), xb.shape[0])
        qs = torch.randn((256, d), device="cuda")
        qb = torch.randint(0, 256, (256, d // 8), dtype=torch.uint8, device="cuda")
        Dv = torch.empty((256, K), dtype=torch.float32, device="cuda")
        Hv = torch.empty((256, K), dtype=torch.int32, device="cuda")
        Iv = torch.empty((256, K), dtype=torch.int64, device="cuda")
        for nq in NQS:
            other[f"cos8_nq{nq}_call_ms"] = round(timed(lambda: c8.search_device(qs.data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr())), 4)
            other[f"bits_nq{nq}_call_ms"] = round(timed(lambda: bx.search_device(qb.data_ptr(), nq, K, Hv.data_ptr(), Iv.data_ptr())), 4)
        c8.close(), bx.close()
        torch.cuda.empty_cache()
        rows_out.append(other)
        print(json.dumps(other), flush=True)
        for fmt in (4, 8):
            idx, one = _native.MxIndex(d, fmt), _native.MxIndex(d, fmt)
            fill(idx, d, n), fill(one, d, 1)
            row_bytes = d * fmt // 8 + 4 * ((d // 128 + 3) & ~3)
            for nq, (full, scan) in call_times(idx, one, d).items():
                per = idx.geometry(nq, K)[0]
                passes = -(-nq // per)
                rows_out.append({"bench": "mx", "d": d, "format": fmt, "n": n, "nq": nq, "k": K, "call_ms": round(full, 4),
                                 "scan_ms": round(scan, 4), "queries_per_read": per, "row_bytes": row_bytes,
                                 "scan_GBps": round(passes * n * row_bytes / scan / 1e6, 1),
                                 "stream_read_GBps": ceiling,
                                 "scan_frac_of_stream_read": round(passes * n * row_bytes / scan / 1e6 / ceiling, 3) if ceiling else None,
                                 "sq4_call_ms": round(sq_t[nq][0], 4),
                                 "sq4_scan_ms": round(sq_t[nq][1], 4), "sq4_row_bytes": d // 2})
                print(json.dumps(rows_out[-1]), flush=True)
            idx.close(), one.close()
            torch.cuda.empty_cache()

    # ---- recall: bench_pq.py's clustered mixture ----
    n_recall = int(os.environ.get("MVDB_BENCH_MX_RECALL_ROWS", 1_000_000))
    D = 512
    gen = torch.Generator(device="cuda").manual_seed(1234)
    centres = torch.randn((1000, D), generator=gen, device="cuda")
    pick = torch.randint(0, 1000, (n_recall + 256,), device="cuda", generator=gen)
    x = centres[pick] + 0.5 * torch.randn((n_recall + 256, D), generator=gen, device="cuda")
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    rows, qh = x[:n_recall].contiguous(), x[n_recall:].contiguous().cpu().numpy()
    torch.cuda.synchronize()
    flat = _native.FlatIndex(D, device=0)
    flat.add_device(rows.data_ptr(), n_recall)
    truth = flat.search(qh, K)[1]
    flat.close()
    rec = {"bench": "mx_recall", "n": n_recall, "d": D, "queries": 256}
    for fmt in (4, 8):
        idx = _native.MxIndex(D, fmt)
        rec[f"fp{fmt}_encode_ms"] = round(timed(lambda: (idx.reset(), idx.add_device(rows.data_ptr(), n_recall))), 4)
        for top in (10, 64):
            I = idx.search(qh, top)[1]
            rec[f"fp{fmt}_top{top}_recall_at_10"] = round(float(np.mean([len(set(truth[i]) & set(I[i])) / K for i in range(256)])), 4)
        idx.close()
    rows_out.append(rec)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mx_bench.jsonl"), "w") as f:
        for r in rows_out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
