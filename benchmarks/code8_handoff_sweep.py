#!/usr/bin/env python3
"""The survivor wave of the int8 prefilter's front form ("The survivor wave"), one process on
10M x 512, k = 10.

Cells: the parent's instantiation (`MVDB_CODE8_HANDOFF=1`) and the hand-off form (`=2`) with a ring of 256, 1,024 and 4,096
entries (`MVDB_CODE8_RING`), set through `reload_env` and visited round-robin ROUNDS times, so that the spread of the session
shows beside the differences.  Per cell one JSON line: ms per query over 200 calls with the library's timers off, then the
seed, prefilter and re-score launches under the timers, fallbacks and calls.  (`profiles/code8_handoff_sweep.jsonl`)

MVDB_LIBMVDB=<library> runs another build of the library (the ablations of the Makefile); every line names the library it ran.

usage: code8_handoff_sweep.py [ROUNDS = 3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from minivectordb_amd import _native as native

n, d, k, W, K = 10_000_000, 512, 10, 20, 200
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda", 0)
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
library = os.path.basename(os.environ.get("MVDB_LIBMVDB", "") or "libmvdb.so")
configs = [(1, 0), (2, 256), (2, 1024), (2, 4096)]
LABELS = ("ip_scan_code8_seed", "ip_scan", "ip_scan_code8_rescore")
for rnd in range(ROUNDS):
    for handoff, ring in configs:
        os.environ["MVDB_CODE8_HANDOFF"] = str(handoff)
        if ring:
            os.environ["MVDB_CODE8_RING"] = str(ring)
        else:
            os.environ.pop("MVDB_CODE8_RING", None)
        idx.reload_env()
        run(0, W)
        t0 = time.perf_counter()
        run(W, K)
        dt = time.perf_counter() - t0
        fb0, _, c0 = idx.code8_counters()
        s0 = idx.code8_front_counters()[0]
        for l in LABELS:
            native.prof_read(l)
        native.prof_enable(True)
        run(W, K)
        native.prof_enable(False)
        fb1, _, c1 = idx.code8_counters()
        rec = {"round": rnd, "library": library, "rows": n, "dim": d, "k": k, "handoff": handoff, "ring": ring,
               "ms_per_query_untimed": round(dt / K * 1e3, 5), "fallbacks_calls": [fb1 - fb0, c1 - c0],
               "front_survivors_per_call": round((idx.code8_front_counters()[0] - s0) / K, 1)}
        for l in LABELS:
            cnt, ms = native.prof_read(l)
            rec[l + "_us"] = round(ms / max(cnt, 1) * 1e3, 2)
        print(json.dumps(rec), flush=True)
idx.close()
