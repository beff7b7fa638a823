#!/usr/bin/env python3
"""The int8 cosine index (csrc/cos8.hip, ShardedVectorDatabaseUsearch): 10M x 512, k = 10 — one query per call (ms and the
fraction of 8 TB/s over the N * stride + 4 N bytes a scan reads) and 32 / 128 / 256 queries per call (q/s), device
buffers, timed with hipEvents; quantising ingest of device-resident fp32 rows (GB/s of fp32 read); and the drop-in
class at 1M x 512 per find_most_similar call.  One JSON line."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402


def timed(fn, reps, warm=3):
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


def main():
    n, d, k = 10_000_000, 512, 10
    stride = (d + 15) // 16 * 16
    out = {"bench": "cos8", "n": n, "d": d, "k": k}
    idx = _native.Cos8Index(d)
    idx.reserve(n)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    block = 1 << 20
    xb = torch.empty((block, d), dtype=torch.float32, device="cuda")
    t_ing = 0.0
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        xb[:m].normal_(generator=gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.add_device(xb.data_ptr(), m)   # synchronises on return
        t_ing += time.perf_counter() - t0
    out["ingest_gbps_fp32_read"] = round(n * d * 4 / t_ing / 1e9, 2)
    out["ingest_ms"] = round(t_ing * 1e3, 1)
    del xb

    stream = torch.cuda.current_stream()
    for nq in (1, 32, 128, 256):
        q = torch.randn((nq, d), generator=gen, device="cuda")
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        ms = timed(lambda: idx.search_device(q.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(),
                                             stream=stream.cuda_stream), reps=20 if nq == 1 else 5)
        if nq == 1:
            out["single_ms"] = round(ms, 4)
            out["single_frac_of_8tbps"] = round((n * stride + 4 * n) / (ms * 1e-3) / 8e12, 3)
        else:
            out[f"batch{nq}_ms"] = round(ms, 3)
            out[f"batch{nq}_qps"] = round(nq / (ms * 1e-3), 1)
    idx.close()
    torch.cuda.empty_cache()

    # the drop-in class at 1M x 512: per find_most_similar call, host in / host out
    from minivectordb_amd import ShardedVectorDatabaseUsearch
    rng = np.random.default_rng(5)
    nd = 1_000_000
    x = rng.standard_normal((nd, d), dtype=np.float32)
    db = ShardedVectorDatabaseUsearch(storage_dir=os.path.join(tempfile.mkdtemp(), "u"), shard_size=250_000)
    db.store_embeddings_batch(list(range(nd)), x, [{"b": i % 100} for i in range(nd)])
    qs = rng.standard_normal((64, d), dtype=np.float32)
    t0 = time.perf_counter()
    db.find_most_similar(qs[0], k=k)
    out["dropin_first_query_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    lat = []
    for i in range(64):
        t0 = time.perf_counter()
        db.find_most_similar(qs[i], k=k)
        lat.append(time.perf_counter() - t0)
    out["dropin_1m_ms_p50"] = round(float(np.median(lat)) * 1e3, 3)
    latf = []
    for i in range(32):
        t0 = time.perf_counter()
        db.find_most_similar(qs[i], metadata_filter={"b": 7}, k=k)
        latf.append(time.perf_counter() - t0)
    out["dropin_1m_filtered_ms_p50"] = round(float(np.median(latf)) * 1e3, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
