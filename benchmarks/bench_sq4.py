#!/usr/bin/env python3
"""The 4-bit scalar-quantised index (csrc/sq4.hip) -> profiles/sq4_bench.jsonl, one JSON line per cell group.

timings   10M rows at d = 512 and 1024, k = 10, nq = 1, 4, 8, 32, 64, 256: the whole device call (query launch + scan + merge;
          hipEvent medians, device buffers) and the same call on a ONE-row index, whose difference is reported as the scan
          launch's share; host calls with the VALU form and the matrix-core form forced at nq = 4, 5, 8, 16 (the hand-over);
          64 queries in one call (two blocks of 32 per row read) against two calls of 32.  In the same process:
          benchmarks/micro/stream_read's best rate (run first, as a child process, when the binary has been built), and
          Cos8Index and BitsIndex over the same number of rows of the same width.
recall    1M x 512 rows of bench_pq.py's clustered mixture: the share of the exact flat top 10 inside the 4-bit top 10 and
          top 64, with min/max ranges and with ranges at the 0.1 % / 99.9 % quantiles, both set through
          SQ4VectorDatabase.train on all the rows (clip_quantile None and 0.999).
ingest    the encode of those 1M rows (reset + add_device, the wait included; median of 15 calls)."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, K = 10_000_000, 10
NQS = (1, 4, 8, 32, 64, 256)
FORCED = (4, 5, 8, 16)


def stream_read_gbps():
    exe = os.path.join(ROOT, "benchmarks", "micro", "stream_read")
    if not os.path.exists(exe):
        return None   # not measured: build it with the line at the top of stream_read.hip
    text = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=300).stdout
    m = re.search(r"best streaming read: (\d+) GB/s", text)
    return int(m.group(1)) if m else None


def main():
    n = int(os.environ.get("MVDB_BENCH_SQ4_ROWS", N))
    n_recall = int(os.environ.get("MVDB_BENCH_SQ4_RECALL_ROWS", 1_000_000))
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

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    block = 1 << 20

    def emit(out):
        lines.append(out)
        print(json.dumps(out), flush=True)

    for d in (512, 1024):
        out = {"bench": "sq4_scan", "n": n, "d": d, "k": K, "stream_read_gbps": ceiling}
        lo, hi = -np.ones(d, np.float32), np.ones(d, np.float32)
        idx, one = _native.SQ4Index(d), _native.SQ4Index(d)
        for ix in (idx, one):
            ix.set_ranges(lo, hi)
        one.add_codes(np.zeros((1, d // 2), np.uint8))
        idx.reserve(n)
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            idx.add_codes(torch.randint(0, 256, (m, d // 2), dtype=torch.uint8, device="cuda", generator=gen).cpu().numpy())
        qs = torch.randn((256, d), generator=gen, device="cuda")
        Dv = torch.empty((256, K), dtype=torch.float32, device="cuda")
        Iv = torch.empty((256, K), dtype=torch.int64, device="cuda")
        call = lambda ix, nq, off=0: ix.search_device(qs[off:].data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr(), stream=stream)
        for nq in NQS:
            ms, base = timed(lambda: call(idx, nq)), timed(lambda: call(one, nq))
            out[f"nq{nq}_call_ms"], out[f"nq{nq}_one_row_call_ms"] = round(ms, 4), round(base, 4)
            out[f"nq{nq}_scan_ms"], out[f"nq{nq}_form"] = round(ms - base, 4), idx.geometry(nq, K)[0]
        out["nq1_scan_rows_gbps"] = round(n * (d // 2) / (out["nq1_scan_ms"] * 1e-3) / 1e9, 1)
        out["nq1_scan_frac_of_stream_read"] = round(out["nq1_scan_rows_gbps"] / ceiling, 3) if ceiling else None
        out["two_calls_of_32_ms"] = round(timed(lambda: (call(idx, 32), call(idx, 32, 32))), 4)
        qh = qs.cpu().numpy()
        for nq in FORCED:   # host calls: staging and the copy back included, the same for both forms
            got = {}
            for form, name in ((1, "valu"), (2, "mfma")):
                out[f"nq{nq}_{name}_host_call_ms"] = round(timed(lambda: got.__setitem__(form, idx.search(qh[:nq], K, form=form))), 4)
            assert all(np.array_equal(a, b) for a, b in zip(got[1], got[2]))
        idx.close()
        one.close()
        torch.cuda.empty_cache()
        emit(out)

        other = {"bench": "sq4_vs_cos8_bits", "n": n, "d": d, "k": K}
        c8, bx = _native.Cos8Index(d), _native.BitsIndex(d)
        c8.reserve(n)
        bx.reserve(n)
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            xb = torch.randn((m, d), generator=gen, device="cuda")
            c8.add_device(xb.data_ptr(), m)
            bx.add_float_device(xb.data_ptr(), m)
        Hv = torch.empty((256, K), dtype=torch.int32, device="cuda")
        qb = torch.randint(0, 256, (256, d // 8), dtype=torch.uint8, device="cuda", generator=gen)
        for nq in NQS:
            other[f"cos8_nq{nq}_call_ms"] = round(timed(lambda: c8.search_device(qs.data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr(),
                                                                                 stream=stream)), 4)
            other[f"bits_nq{nq}_call_ms"] = round(timed(lambda: bx.search_device(qb.data_ptr(), nq, K, Hv.data_ptr(), Iv.data_ptr(),
                                                                                 stream=stream)), 4)
            other[f"sq4_over_cos8_nq{nq}"] = round(out[f"nq{nq}_call_ms"] / other[f"cos8_nq{nq}_call_ms"], 3)
        c8.close()
        bx.close()
        torch.cuda.empty_cache()
        emit(other)

    # ---- recall and ingest ----
    D = 512
    rec = {"bench": "sq4_recall", "n": n_recall, "d": D, "queries": 256}
    centres = torch.randn((1000, D), generator=gen, device="cuda")
    pick = torch.randint(0, 1000, (n_recall + 256,), device="cuda", generator=gen)
    x = centres[pick] + 0.5 * torch.randn((n_recall + 256, D), generator=gen, device="cuda")
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    rows, q = x[:n_recall].contiguous(), x[n_recall:].contiguous()
    torch.cuda.synchronize()
    flat = _native.FlatIndex(D, device=0)
    flat.add_device(rows.data_ptr(), n_recall)
    qh = q.cpu().numpy()
    truth = flat.search(qh, K)[1]
    flat.close()

    def recall(I):
        return float(np.mean([len(set(truth[i]) & set(I[i])) / K for i in range(len(truth))]))

    from minivectordb_amd import SQ4VectorDatabase
    sample = rows.cpu().numpy()
    for name, clip in (("minmax", None), ("clip999", 0.999)):   # the ranges come from the class's own train, all rows
        db = SQ4VectorDatabase(D)
        t0 = time.perf_counter()
        db.train(sample, clip_quantile=clip)
        rec[f"train_{name}_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)   # minmax: the upload of the rows included
        sq = db.index

        def encode():   # add_device waits for the encode launch; reset keeps the ranges
            sq.reset()
            sq.add_device(rows.data_ptr(), n_recall)

        rec[f"{name}_encode_ms"] = round(timed(encode), 4)
        rec[f"{name}_top10_recall_at_10"] = round(recall(sq.search(qh, 10)[1]), 4)
        rec[f"{name}_top64_recall_at_10"] = round(recall(sq.search(qh, 64)[1]), 4)
        sq.close()
    emit(rec)

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    target = os.environ.get("MVDB_BENCH_SQ4_OUT", os.path.join(ROOT, "profiles", "sq4_bench.jsonl"))
    with open(target, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
