#!/usr/bin/env python3
"""The binary index (csrc/bits.hip): 10M rows x 1024 bits and 10M x 4096 bits, k = 10, nq = 1 .. 256 per call, device buffers,
hipEvent medians — BOTH scan forms wherever both can serve, which is where the shape table's crossover comes from; the bytes of
rows per second of the nq = 1 launch beside benchmarks/micro/stream_read's best rate on the same box (run first, as a child
process, when the binary has been built); the int8 cosine index over the same number of rows at d = 1024, nq = 1 and 256, in
the same process; one clock / power sample under the nq = 1 load.  One JSON line per width -> profiles/bits_bench.jsonl."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, K = 10_000_000, 10
NQS = (1, 2, 4, 8, 9, 16, 32, 64, 256)


def stream_read_gbps():
    exe = os.path.join(ROOT, "benchmarks", "micro", "stream_read")
    if not os.path.exists(exe):
        return None   # not measured: build it with the line at the top of stream_read.hip
    text = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=300).stdout
    m = re.search(r"best streaming read: (\d+) GB/s", text)
    return int(m.group(1)) if m else None


def main():
    n = int(os.environ.get("MVDB_BENCH_BITS_ROWS", N))
    ceiling = stream_read_gbps()
    import torch
    import bench
    from minivectordb_amd import _native

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

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    lines = []
    for d_bits in (1024, 4096):
        rb = d_bits // 8
        out = {"bench": "bits", "n": n, "d_bits": d_bits, "k": K, "stream_read_gbps": ceiling}
        idx = _native.BitsIndex(d_bits)
        idx.reserve(n)
        block = 1 << 20
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            xb = torch.randint(0, 256, (m, rb), dtype=torch.uint8, device="cuda", generator=gen)
            idx.add_device(xb.data_ptr(), m)
        del xb
        for nq in NQS:
            q = torch.randint(0, 256, (nq, rb), dtype=torch.uint8, device="cuda", generator=gen)
            D = torch.empty((nq, K), dtype=torch.int32, device="cuda")
            I = torch.empty((nq, K), dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            ms = timed(lambda: idx.search_device(q.data_ptr(), nq, K, D.data_ptr(), I.data_ptr(), stream=stream), reps=15)
            out[f"nq{nq}_ms"] = round(ms, 4)
            out[f"nq{nq}_form"] = "mfma" if idx.geometry(nq, K)[0] == idx.FORM_MFMA else "valu"
            # each form forced, through the host call (host queries in, host results out: its copies are in both figures)
            qh = q.cpu().numpy()
            first = None
            for form, name in ((idx.FORM_VALU, "valu"), (idx.FORM_MFMA, "mfma")):
                Df, If = idx.search(qh, K, form=form)
                first = (Df, If) if first is None else first
                assert np.array_equal(Df, first[0]) and np.array_equal(If, first[1]), (d_bits, nq, name)
                assert np.array_equal(Df, D.cpu().numpy()) and np.array_equal(If, I.cpu().numpy()), (d_bits, nq, name)
                out[f"nq{nq}_{name}_host_ms"] = round(timed(lambda: idx.search(qh, K, form=form), reps=9), 4)
            if nq == 1:
                out["nq1_rows_gbps"] = round(n * rb / (ms * 1e-3) / 1e9, 1)
                out["nq1_frac_of_stream_read"] = round(out["nq1_rows_gbps"] / ceiling, 3) if ceiling else None
                out["power"] = bench.power_probe(
                    lambda: idx.search_device(q.data_ptr(), 1, K, D.data_ptr(), I.data_ptr(), stream=stream),
                    f"bits nq=1 d_bits={d_bits}", torch.cuda.synchronize)
        idx.close()
        torch.cuda.empty_cache()
        lines.append(out)

    # the cheapest way to hold such vectors before this index: int8 codes, d = 1024, same number of rows, same process
    d = 1024
    c8 = _native.Cos8Index(d)
    c8.reserve(n)
    block = 1 << 19
    xb = torch.empty((block, d), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        xb[:m].normal_(generator=gen)
        torch.cuda.synchronize()
        c8.add_device(xb.data_ptr(), m)
    del xb
    cos8 = {"bench": "bits_vs_cos8", "n": n, "d": d, "k": K}
    for nq in (1, 256):
        q = torch.randn((nq, d), generator=gen, device="cuda")
        D = torch.empty((nq, K), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, K), dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        cos8[f"cos8_nq{nq}_ms"] = round(timed(lambda: c8.search_device(q.data_ptr(), nq, K, D.data_ptr(), I.data_ptr(),
                                                                       stream=stream), reps=9), 4)
        cos8[f"bits1024_over_cos8_nq{nq}"] = round(lines[0][f"nq{nq}_ms"] / cos8[f"cos8_nq{nq}_ms"], 4)
    c8.close()
    lines.append(cos8)

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    target = os.environ.get("MVDB_BENCH_BITS_OUT", os.path.join(ROOT, "profiles", "bits_bench.jsonl"))
    with open(target, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
