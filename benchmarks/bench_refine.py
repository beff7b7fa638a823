#!/usr/bin/env python3
"""The refine store (csrc/refine.hip) behind the MX index -> profiles/refine_bench.jsonl, one JSON line per cell.

timings   10M rows at d = 512 and 1024, MXFP4 and MXFP8, k = 10, nq = 1, 8, 64, 256, fetch_k = 64, 256, 1024: the whole refined
          device call (query encode + S segment scans and merges + re-rank) and, alternating with it in the same loop, the plain
          search at k = 10 on the same index — what a caller had before.  The re-rank launches alone over lists of fetch_k random
          rows, with the bytes they gather (candidates x 2 d) over their time, beside benchmarks/micro/stream_read's best rate
          (run first, as a child process, when the binary has been built).  hipEvent medians around whole device calls.
recall    1M x 512 rows of bench_pq.py's clustered mixture, 256 queries: recall@10 of the refined answer against FlatIndex's exact
          top 10, per format and fetch_k, beside the un-refined top 10 and top 64 of the same run.
Rows in flight per wave, slices per query and waves per block are first guesses, not swept."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from benchmarks.bench_sq4 import stream_read_gbps  # noqa: E402

N, K = 10_000_000, 10
NQS = (1, 8, 64, 256)
FETCH = (64, 256, 1024)


def main():
    n = int(os.environ.get("MVDB_BENCH_REFINE_ROWS", N))
    ceiling = stream_read_gbps()
    import torch
    from minivectordb_amd import _native

    def timed_pair(fa, fb, reps=15, warm=3):
        """medians of two calls timed alternately"""
        for _ in range(warm):
            fa(), fb()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = ([], [])
        for _ in range(reps):
            for fn, out in zip((fa, fb), per):
                a.record()
                fn()
                b.record()
                b.synchronize()
                out.append(a.elapsed_time(b))
        return float(np.median(per[0])), float(np.median(per[1]))

    rows_out = []

    def emit(rec):
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)

    for d in (512, 1024):
        st = _native.RefineStore(d)
        idxs = {fmt: _native.MxIndex(d, fmt) for fmt in (4, 8)}
        st.reserve(n)
        gen = torch.Generator(device="cuda").manual_seed(d)
        for r0 in range(0, n, 1 << 18):
            x = torch.randn((min(1 << 18, n - r0), d), generator=gen, device="cuda", dtype=torch.float32)
            st.add_device(x.data_ptr(), x.shape[0])
            for idx in idxs.values():
                idx.add_device(x.data_ptr(), x.shape[0])
        torch.cuda.synchronize()
        for nq in NQS:
            q = torch.randn((nq, d), device="cuda", dtype=torch.float32)
            D = torch.empty((nq, K), device="cuda", dtype=torch.float32)
            I = torch.empty((nq, K), device="cuda", dtype=torch.int64)
            for fetch_k in FETCH:
                cand = torch.randint(0, n, (nq, fetch_k), device="cuda", dtype=torch.int64)
                rerank = lambda: st.rerank_device(q.data_ptr(), nq, cand.data_ptr(), fetch_k, K, D.data_ptr(), I.data_ptr())
                rec = {"bench": "refine", "n": n, "d": d, "nq": nq, "k": K, "fetch_k": fetch_k, "stream_read_GBps": ceiling}
                for fmt, idx in idxs.items():
                    plain = lambda: idx.search_device(q.data_ptr(), nq, K, D.data_ptr(), I.data_ptr())
                    refined = lambda: idx.search_refined_device(q.data_ptr(), nq, K, st, fetch_k, D.data_ptr(), I.data_ptr())
                    t_ref, t_plain = timed_pair(refined, plain)
                    rec[f"fp{fmt}_refined_call_ms"], rec[f"fp{fmt}_plain_call_ms"] = round(t_ref, 4), round(t_plain, 4)
                t_rr, _ = timed_pair(rerank, rerank)
                rec["rerank_ms"] = round(t_rr, 4)
                rec["rerank_gather_GBps"] = round(nq * fetch_k * 2 * d / t_rr / 1e6, 1)
                emit(rec)
        st.close()
        for idx in idxs.values():
            idx.close()
        torch.cuda.empty_cache()

    # ---- recall: bench_pq.py's clustered mixture ----
    n_recall = int(os.environ.get("MVDB_BENCH_REFINE_RECALL_ROWS", 1_000_000))
    Dm = 512
    gen = torch.Generator(device="cuda").manual_seed(1234)
    centres = torch.randn((1000, Dm), generator=gen, device="cuda")
    pick = torch.randint(0, 1000, (n_recall + 256,), device="cuda", generator=gen)
    x = centres[pick] + 0.5 * torch.randn((n_recall + 256, Dm), generator=gen, device="cuda")
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    rows, qh = x[:n_recall].contiguous(), x[n_recall:].contiguous().cpu().numpy()
    torch.cuda.synchronize()
    flat = _native.FlatIndex(Dm, device=0)
    flat.add_device(rows.data_ptr(), n_recall)
    truth = flat.search(qh, K)[1]
    flat.close()
    recall = lambda I: round(float(np.mean([len(set(truth[i]) & set(I[i])) / K for i in range(256)])), 4)
    st = _native.RefineStore(Dm)
    st.add_device(rows.data_ptr(), n_recall)
    rec = {"bench": "refine_recall", "n": n_recall, "d": Dm, "queries": 256}
    for fmt in (4, 8):
        idx = _native.MxIndex(Dm, fmt)
        idx.add_device(rows.data_ptr(), n_recall)
        for top in (10, 64):
            rec[f"fp{fmt}_unrefined_top{top}_recall_at_10"] = recall(idx.search(qh, top)[1])
        for fetch_k in FETCH:
            rec[f"fp{fmt}_fetch{fetch_k}_refined_recall_at_10"] = recall(idx.search_refined(qh, K, st, fetch_k)[1])
        idx.close()
    emit(rec)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "refine_bench.jsonl"), "w") as f:
        for r in rows_out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
