#!/usr/bin/env python3
"""The product-quantised index (csrc/pq.hip) -> profiles/pq_bench.jsonl, one JSON line per cell group.

timings   10M rows at d = 512, M = 64 and M = 128, k = 10, nq = 1, 4, 8, 256: the whole device call (table launch + scan +
          merge; hipEvent medians, device buffers) and the same call on a ONE-row index with the same codebooks — the table
          launch, a one-tile scan and the merge — whose difference is reported as the scan launch's share.  In the same process:
          benchmarks/micro/stream_read's best rate (run first, as a child process, when the binary has been built) and BitsIndex
          at 512 bits, whose rows are the same 64 bytes as M = 64.
recall    1M x 512 rows of a clustered mixture, codebooks trained on 65,536 rows for 25 iterations: recall@10 of the PQ top 10
          and of the PQ top 64 (k <= 64 is the index's limit; the top 100 cannot be asked for) against the exact flat index, and the
          same two figures for BitsIndex over the sign bits of the same rows.
ingest    the encode of those 1M rows (add_device) and one training iteration on the 65,536-row sample (train's upload included)."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, K, D = 10_000_000, 10, 512
NQS = (1, 4, 8, 256)


def stream_read_gbps():
    exe = os.path.join(ROOT, "benchmarks", "micro", "stream_read")
    if not os.path.exists(exe):
        return None   # not measured: build it with the line at the top of stream_read.hip
    text = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=300).stdout
    m = re.search(r"best streaming read: (\d+) GB/s", text)
    return int(m.group(1)) if m else None


def main():
    n = int(os.environ.get("MVDB_BENCH_PQ_ROWS", N))
    n_recall = int(os.environ.get("MVDB_BENCH_PQ_RECALL_ROWS", 1_000_000))
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

    def fill(idx, add, width, dtype=torch.uint8):
        block = 1 << 20
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            add(torch.randint(0, 256, (m, width), dtype=dtype, device="cuda", generator=gen), m)

    # ---- timings ----
    for M in (64, 128):
        out = {"bench": "pq_scan", "n": n, "d": D, "M": M, "k": K, "stream_read_gbps": ceiling}
        cb = torch.randn((M, 256, D // M), generator=gen, device="cuda").cpu().numpy()
        idx, one = _native.PQIndex(D, M, _native.METRIC_IP), _native.PQIndex(D, M, _native.METRIC_IP)
        for ix in (idx, one):
            ix.set_codebooks(cb)
        one.add_codes(np.zeros((1, M), np.uint8))
        idx.reserve(n)
        fill(idx, lambda xb, m: idx.add_codes(xb.cpu().numpy()), M)
        for nq in NQS:
            q = torch.randn((nq, D), generator=gen, device="cuda")
            Dv = torch.empty((nq, K), dtype=torch.float32, device="cuda")
            Iv = torch.empty((nq, K), dtype=torch.int64, device="cuda")
            call = lambda ix: ix.search_device(q.data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr(), stream=stream)
            ms, base = timed(lambda: call(idx)), timed(lambda: call(one))
            out[f"nq{nq}_call_ms"], out[f"nq{nq}_one_row_call_ms"] = round(ms, 4), round(base, 4)
            out[f"nq{nq}_scan_ms"] = round(ms - base, 4)
            out[f"nq{nq}_queries_per_pass"] = idx.geometry(nq, K)[0]
        out["nq1_scan_rows_gbps"] = round(n * M / (out["nq1_scan_ms"] * 1e-3) / 1e9, 1)
        out["nq1_scan_frac_of_stream_read"] = round(out["nq1_scan_rows_gbps"] / ceiling, 3) if ceiling else None
        idx.close()
        one.close()
        torch.cuda.empty_cache()
        lines.append(out)
        print(json.dumps(out), flush=True)

    bits = {"bench": "pq_vs_bits", "n": n, "d_bits": 512, "k": K}
    bx = _native.BitsIndex(512)
    bx.reserve(n)
    fill(bx, lambda xb, m: bx.add_device(xb.data_ptr(), m), 64)
    for nq in NQS:
        q = torch.randint(0, 256, (nq, 64), dtype=torch.uint8, device="cuda", generator=gen)
        Dv = torch.empty((nq, K), dtype=torch.int32, device="cuda")
        Iv = torch.empty((nq, K), dtype=torch.int64, device="cuda")
        bits[f"bits_nq{nq}_call_ms"] = round(timed(lambda: bx.search_device(q.data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr(),
                                                                            stream=stream)), 4)
        bits[f"pq64_over_bits_nq{nq}"] = round(lines[0][f"nq{nq}_call_ms"] / bits[f"bits_nq{nq}_call_ms"], 3)
    bx.close()
    torch.cuda.empty_cache()
    lines.append(bits)
    print(json.dumps(bits), flush=True)

    # ---- recall and ingest ----
    rec = {"bench": "pq_recall", "n": n_recall, "d": D, "M": 64, "train_rows": 65536, "train_iters": 25, "queries": 256}
    centres = torch.randn((1000, D), generator=gen, device="cuda")
    pick = torch.randint(0, 1000, (n_recall + 256,), device="cuda", generator=gen)
    x = centres[pick] + 0.5 * torch.randn((n_recall + 256, D), generator=gen, device="cuda")
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    rows, q = x[:n_recall].contiguous(), x[n_recall:].contiguous()
    torch.cuda.synchronize()
    flat = _native.FlatIndex(D, device=0)
    flat.add_device(rows.data_ptr(), n_recall)
    truth = flat.search(q.cpu().numpy(), K)[1]
    flat.close()
    sample = rows[torch.randperm(n_recall, generator=gen, device="cuda")[:65536]].cpu().numpy()
    start = np.ascontiguousarray(sample[:256].reshape(256, 64, -1).transpose(1, 0, 2))
    pq = _native.PQIndex(D, 64, _native.METRIC_IP)
    pq.set_codebooks(start)
    t0 = time.perf_counter()
    pq.train(sample, 1)
    rec["train_one_iteration_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    pq.set_codebooks(start)
    t0 = time.perf_counter()
    pq.train(sample, 25)
    rec["train_25_iterations_call_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rec["train_per_iteration_ms"] = round((rec["train_25_iterations_call_ms"] - rec["train_one_iteration_call_ms"]) / 24, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pq.add_device(rows.data_ptr(), n_recall)
    rec["encode_ms"] = round((time.perf_counter() - t0) * 1e3, 2)

    def recall(I):
        return float(np.mean([len(set(truth[i]) & set(I[i])) / K for i in range(len(truth))]))

    qh = q.cpu().numpy()
    rec["pq_top10_recall_at_10"] = round(recall(pq.search(qh, 10)[1]), 4)
    rec["pq_top64_recall_at_10"] = round(recall(pq.search(qh, 64)[1]), 4)
    pq.close()
    bx = _native.BitsIndex(512)
    bx.add_float_device(rows.data_ptr(), n_recall)
    rec["bits_top10_recall_at_10"] = round(recall(bx.search_float(qh, 10)[1]), 4)
    rec["bits_top64_recall_at_10"] = round(recall(bx.search_float(qh, 64)[1]), 4)
    bx.close()
    lines.append(rec)
    print(json.dumps(rec), flush=True)

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    target = os.environ.get("MVDB_BENCH_PQ_OUT", os.path.join(ROOT, "profiles", "pq_bench.jsonl"))
    with open(target, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
