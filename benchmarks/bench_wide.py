#!/usr/bin/env python3
"""The certified batch pass at d = 1536 / 2048 / 3072 / 4096 (index option "wide_shadow", csrc/half_wide_scan.hip) beside the route
the same index takes without it (the GEMM-tiled exact fp32 scan): one index, one process, the two settings alternating --rounds
times (3 warm-up calls and --reps timed calls a time; hipEvents on the current stream, device buffers; a cell reports the median
of its rounds' medians).  Shapes: 1M rows at the four widths and 10M x 1536; 33, 128 and 256 queries per call, k = 10.

      exact_ms, wide_ms    the call with wide_shadow = 0 / 1
      main_launch_ms       the launches under "ip_scan_half_wide" of one call with the option on (mvdb_prof_read, calls of their own)
      alg_bytes, alg_tbs   slabs x n x d x 2 — a workgroup serves QW = 64 / 32 queries, every slab of QW queries streams the
                           shadow itself — and that over main_launch_ms
      reruns_before/after  mvdb_split_rerun_count around the option-1 calls (chunks that held a refused query)
      agree                D and I of the two settings under tests/bigcheck.compare (near-ties adjudicated in float64)

One JSON line per cell, to stdout and appended to --out (default profiles/wide_batch_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

import bigcheck  # noqa: E402
from bench_distinct import launch_ms, timed_events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000000x1536", "1000000x2048", "1000000x3072", "1000000x4096", "10000000x1536"])
    ap.add_argument("--nq", type=int, nargs="+", default=[33, 128, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_batch_bench.jsonl"))
    args = ap.parse_args()
    k = args.k
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2031)
    for shape in args.shapes:
        n, d = (int(v) for v in shape.split("x"))
        qw = _native.half_wide_queries(d)
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        qh = rng.standard_normal((max(args.nq), d), dtype=np.float32)
        qh /= np.linalg.norm(qh, axis=1, keepdims=True)
        q = torch.from_numpy(qh).cuda()
        for nq in args.nq:
            D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            I = torch.empty((nq, k), dtype=torch.int64, device="cuda")

            def call():
                idx.search_device(q.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream=stream)

            rounds, out = {0: [], 1: []}, {}
            reruns_before = _native.split_rerun_count()
            for _ in range(args.rounds):
                for on in (0, 1):
                    idx.set_option("wide_shadow", on)
                    rounds[on].append(round(timed_events(call, args.reps), 4))
                    torch.cuda.synchronize()
                    out[on] = (D.cpu().numpy().copy(), I.cpu().numpy().copy())
            main_ms, symbol = launch_ms(call, "ip_scan_half_wide", 3, per_call=True)   # (the option is still on)
            reruns_after = _native.split_rerun_count()
            idx.set_option("wide_shadow", 0)
            slabs = sum(-(-min(128, nq - c0) // qw) for c0 in range(0, nq, 128))
            rec = {"bench": "wide_batch", "n": n, "d": d, "nq": nq, "k": k, "reps": args.reps, "exact_ms": float(np.median(rounds[0])),
                   "wide_ms": float(np.median(rounds[1])), "exact_rounds": rounds[0], "wide_rounds": rounds[1], "main_launch_ms": main_ms,
                   "symbol": symbol, "slabs": slabs, "alg_bytes": slabs * n * d * 2, "reruns_before": reruns_before, "reruns_after": reruns_after}
            rec["speedup"] = round(rec["exact_ms"] / rec["wide_ms"], 3)
            rec["alg_tbs"] = round(rec["alg_bytes"] / main_ms / 1e9, 3) if main_ms else None
            try:
                bigcheck.compare(idx, qh[:nq], out[1][0], out[1][1], out[0][0], out[0][1], f"wide {shape} nq={nq}")
                rec["agree"] = True
            except AssertionError as e:
                rec["agree"], rec["disagreement"] = False, str(e)[:300]
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
