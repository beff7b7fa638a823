#!/usr/bin/env python3
"""The RaBitQ index (csrc/rabitq.hip) -> profiles/rabitq_bench.jsonl, one JSON line per cell group.

timings   10M rows at d = 512 and 1024, k = 10, nq = 1, 4, 8, 32, 64, 256: the whole device call (query launch + scan + merge;
          hipEvent medians, device buffers) and the same call on a ONE-row index, whose difference is reported as the scan
          launch's share; BitsIndex over the same number of rows of the same bit width beside it, each time as a ratio;
          host calls with the VALU form and the matrix-core form forced at nq = 4, 5, 8, 16 (the hand-over); 64 queries in one
          call (two blocks of 32 per row read) against two calls of 32.  benchmarks/micro/stream_read's best rate is taken
          first, as a child process, when the binary has been built.
recall    1M x 512 rows of bench_pq.py's clustered mixture, 256 queries against the flat index: the share of the exact top 10
          inside the top 10 and the top 64, with and without train (the centroid), BitsIndex and SQ4Index beside it, and the
          mean |S - exact inner product| over the returned rows.
ingest    the encode of those 1M rows (reset + add_device, the wait included; median of 15 calls)."""
import json
import os
import re
import subprocess
import sys

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
    n = int(os.environ.get("MVDB_BENCH_RABITQ_ROWS", N))
    n_recall = int(os.environ.get("MVDB_BENCH_RABITQ_RECALL_ROWS", 1_000_000))
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

    def signs(d):
        return np.packbits(np.random.default_rng(0).integers(0, 2, (4, d), dtype=np.uint8), axis=1)

    for d in (512, 1024):
        out = {"bench": "rabitq_scan", "n": n, "d": d, "k": K, "stream_read_gbps": ceiling}
        idx, one, bx = _native.RabitqIndex(d), _native.RabitqIndex(d), _native.BitsIndex(d)
        for ix in (idx, one):
            ix.set_rotation(signs(d))
        one.add_codes(np.zeros((1, d // 8), np.uint8), np.ones((1, 2), np.float32))
        idx.reserve(n)
        bx.reserve(n)
        for r0 in range(0, n, block):   # the same code rows in both indexes
            m = min(block, n - r0)
            rows = torch.randint(0, 256, (m, d // 8), dtype=torch.uint8, device="cuda", generator=gen)
            idx.add_codes(rows.cpu().numpy(), torch.rand((m, 2), generator=gen, device="cuda").cpu().numpy() + 0.5)
            bx.add_device(rows.data_ptr(), m)
        qs = torch.randn((256, d), generator=gen, device="cuda")
        qb = torch.randint(0, 256, (256, d // 8), dtype=torch.uint8, device="cuda", generator=gen)
        Dv = torch.empty((256, K), dtype=torch.float32, device="cuda")
        Hv = torch.empty((256, K), dtype=torch.int32, device="cuda")
        Iv = torch.empty((256, K), dtype=torch.int64, device="cuda")
        call = lambda ix, nq, off=0: ix.search_device(qs[off:].data_ptr(), nq, K, Dv.data_ptr(), Iv.data_ptr(), stream=stream)
        for nq in NQS:
            ms, base = timed(lambda: call(idx, nq)), timed(lambda: call(one, nq))
            bits = timed(lambda: bx.search_device(qb.data_ptr(), nq, K, Hv.data_ptr(), Iv.data_ptr(), stream=stream))
            out[f"nq{nq}_call_ms"], out[f"nq{nq}_one_row_call_ms"] = round(ms, 4), round(base, 4)
            out[f"nq{nq}_scan_ms"], out[f"nq{nq}_form"] = round(ms - base, 4), idx.geometry(nq, K)[0]
            out[f"bits_nq{nq}_call_ms"], out[f"rabitq_over_bits_nq{nq}"] = round(bits, 4), round(ms / bits, 3)
        out["nq1_scan_rows_gbps"] = round(n * (d // 8 + 12) / (out["nq1_scan_ms"] * 1e-3) / 1e9, 1)   # code + (f, g) + B
        out["nq1_scan_frac_of_stream_read"] = round(out["nq1_scan_rows_gbps"] / ceiling, 3) if ceiling else None
        out["two_calls_of_32_ms"] = round(timed(lambda: (call(idx, 32), call(idx, 32, 32))), 4)
        qh = qs.cpu().numpy()
        for nq in FORCED:   # host calls: staging and the copy back included, the same for both forms
            got = {}
            for form, name in ((1, "valu"), (2, "mfma")):
                out[f"nq{nq}_{name}_host_call_ms"] = round(timed(lambda: got.__setitem__(form, idx.search(qh[:nq], K, form=form))), 4)
            assert all(np.array_equal(a, b) for a, b in zip(got[1], got[2]))
        for ix in (idx, one, bx):
            ix.close()
        torch.cuda.empty_cache()
        emit(out)

    # ---- recall and ingest ----
    D = 512
    rec = {"bench": "rabitq_recall", "n": n_recall, "d": D, "queries": 256}
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
    sample = rows.cpu().numpy()

    def recall(I):
        return float(np.mean([len(set(truth[i]) & set(I[i])) / K for i in range(len(truth))]))

    from minivectordb_amd import RabitqVectorDatabase, SQ4VectorDatabase
    for name, train in (("untrained", False), ("trained", True)):
        db = RabitqVectorDatabase(D)
        if train:
            db.train(sample)
        rb = db.index

        def encode():   # add_device waits for the encode launch; reset keeps the rotation and the centroid
            rb.reset()
            rb.add_device(rows.data_ptr(), n_recall)

        rec[f"{name}_encode_ms"] = round(timed(encode), 4)
        S, I = rb.search(qh, 64)
        rec[f"{name}_top10_recall_at_10"], rec[f"{name}_top64_recall_at_10"] = round(recall(I[:, :10]), 4), round(recall(I), 4)
        rec[f"{name}_mean_abs_score_error"] = round(float(np.mean(np.abs(S - np.einsum("qd,qkd->qk", qh, sample[I])))), 5)
        rb.close()
    bx = _native.BitsIndex(D)
    bx.add_float_device(rows.data_ptr(), n_recall)
    I = bx.search_float(qh, 64)[1]
    rec["bits_top10_recall_at_10"], rec["bits_top64_recall_at_10"] = round(recall(I[:, :10]), 4), round(recall(I), 4)
    bx.close()
    sq = SQ4VectorDatabase(D)
    sq.train(sample)
    sq.index.add_device(rows.data_ptr(), n_recall)
    I = sq.index.search(qh, 64)[1]
    rec["sq4_top10_recall_at_10"], rec["sq4_top64_recall_at_10"] = round(recall(I[:, :10]), 4), round(recall(I), 4)
    emit(rec)

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    target = os.environ.get("MVDB_BENCH_RABITQ_OUT", os.path.join(ROOT, "profiles", "rabitq_bench.jsonl"))
    with open(target, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
