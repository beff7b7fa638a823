#!/usr/bin/env python3
"""Grids of the single-query int8 route's small launches, one process on 10M x 512, k = 10.

The seed launch's grid (`MVDB_CODE8_SEED_BLOCKS` x `MVDB_CODE8_SEED_THREADS`: CUs x 256, CUs x 512, 2 CUs x 256; 0 = the
default) and the re-score's candidates per block (`MVDB_CODE8_RESCORE_ROWS`: 16 / 32 / 64), set through `reload_env` and
visited round-robin ROUNDS times, so that the spread of the session shows beside the differences.  Per cell one JSON line:
ms per query over 200 calls with the library's timers off, then the seed, prefilter and re-score launches under the timers
(they add ~3 us each), fallbacks and calls.  (`profiles/code8_headmerge_sweep.jsonl`)

usage: code8_headmerge_sweep.py [ROUNDS = 3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from minivectordb_amd import _native as native

n, d, k, W, K = 10_000_000, 512, 10, 20, 200
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda", 0)
cus = torch.cuda.get_device_properties(0).multi_processor_count
idx = native.FlatIndex(d, device=0)
idx.reserve(n)
idx.add_synthetic(n, 1234, normalize=True)
queries = torch.empty((W + K, d), dtype=torch.float32, device=dev)
native.check(native.lib().mvdb_synth_fill_device(queries.data_ptr(), W + K, d, 5678, 0, 1, 0, torch.cuda.current_stream().cuda_stream))
D = torch.empty((1, k), dtype=torch.float32, device=dev)
I = torch.empty((1, k), dtype=torch.int64, device=dev)
stream = torch.cuda.current_stream().cuda_stream


def run(first, count):
    for i in range(first, first + count):
        idx.search_device(queries[i].data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream)
    torch.cuda.synchronize()


idx.set_option("code8_single_query", 1)
run(0, 4)
assert idx.code8_rows == n
configs = [(0, 0, 0), (cus, 256, 0), (cus, 512, 0), (2 * cus, 256, 0), (0, 0, 16), (0, 0, 32), (0, 0, 64)]
LABELS = ("ip_scan_code8_seed", "ip_scan", "ip_scan_code8_rescore")
for rnd in range(ROUNDS):
    for sb, st, rr in configs:
        for name, v in (("MVDB_CODE8_SEED_BLOCKS", sb), ("MVDB_CODE8_SEED_THREADS", st), ("MVDB_CODE8_RESCORE_ROWS", rr)):
            if v:
                os.environ[name] = str(v)
            else:
                os.environ.pop(name, None)
        idx.reload_env()
        run(0, W)
        t0 = time.perf_counter()
        run(W, K)
        dt = time.perf_counter() - t0
        fb0, _, c0 = idx.code8_counters()
        for l in LABELS:
            native.prof_read(l)
        native.prof_enable(True)
        run(W, K)
        native.prof_enable(False)
        fb1, _, c1 = idx.code8_counters()
        rec = {"round": rnd, "rows": n, "dim": d, "k": k, "cus": cus, "seed_blocks": sb, "seed_threads": st, "rescore_rows": rr,
               "ms_per_query_untimed": round(dt / K * 1e3, 5), "fallbacks_calls": [fb1 - fb0, c1 - c0]}
        for l in LABELS:
            cnt, ms = native.prof_read(l)
            rec[l + "_us"] = round(ms / max(cnt, 1) * 1e3, 2)
        print(json.dumps(rec), flush=True)
idx.close()
