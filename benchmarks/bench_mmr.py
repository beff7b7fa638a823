#!/usr/bin/env python3
"""MMR search (mvdb_index_search_mmr_device) beside the plain search it starts with.  Corpus 1M x 512 and 10M x 512
normalised synthetic rows; nq = 1 and 64; (k, fetch_k) = (5, 20), (10, 100), (64, 1024); lambda = 0.5.  Per cell, device
buffers, hipEvents on the current stream, the median of --reps calls after 3 warm-up calls:

  mmr_ms      search_mmr_device
  search_ms   search_device with k = fetch_k on the same index — existing code the MMR call runs unchanged as its first stage
  select_ms   mmr_ms - search_ms: the selection stage; beside it select_launch_ms, the mmr_select launch alone
              (mvdb_prof_read("mmr_select"), collected in calls of their own) and the form it took (mvdb_mmr_form)

One JSON line per cell, to stdout and to --out (default profiles/mmr_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

SHAPES = ((5, 20), (10, 100), (64, 1024))


def timed_events(fn, reps, warm=3):
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


def launch_ms(fn, label, reps):
    """Mean time of the launches recorded under `label` while fn runs `reps` times (profiling events on; calls of their own)."""
    fn()
    torch.cuda.synchronize()
    _native.prof_read(label)
    _native.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    _native.prof_enable(False)
    launches, ms = _native.prof_read(label)
    return (ms / launches if launches else None), _native.prof_symbol(label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-mult", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_bench.jsonl"))
    args = ap.parse_args()
    d = 512
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2027)
    sink = open(args.out, "w") if args.out else None
    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        qh = rng.standard_normal((max(args.nq), d), dtype=np.float32)
        q = torch.from_numpy(qh).cuda()
        for k, fetch_k in SHAPES:
            for nq in args.nq:
                D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                Dc = torch.empty((nq, fetch_k), dtype=torch.float32, device="cuda")
                Ic = torch.empty((nq, fetch_k), dtype=torch.int64, device="cuda")

                def mmr():
                    idx.search_mmr_device(q.data_ptr(), nq, k, fetch_k, args.lambda_mult, D.data_ptr(), I.data_ptr(), stream=stream,
                                          normalize_q=True)

                def search():
                    idx.search_device(q.data_ptr(), nq, fetch_k, Dc.data_ptr(), Ic.data_ptr(), stream=stream, normalize_q=True)

                rec = {"bench": "mmr", "n": n, "d": d, "nq": nq, "k": k, "fetch_k": fetch_k, "lambda": args.lambda_mult,
                       "reps": args.reps, "form": _native.FlatIndex.mmr_form(d, fetch_k)}
                rec["search_ms"] = round(timed_events(search, args.reps), 4)
                rec["mmr_ms"] = round(timed_events(mmr, args.reps), 4)
                rec["select_ms"] = round(rec["mmr_ms"] - rec["search_ms"], 4)
                ms, sym = launch_ms(mmr, "mmr_select", args.reps)
                rec["select_launch_ms"], rec["select_symbol"] = (round(ms, 4) if ms is not None else None), sym
                torch.cuda.synchronize()
                picked = I.cpu().numpy()
                first = Ic.cpu().numpy()
                rec["first_pick_is_the_best_hit"] = bool((picked[:, 0] == first[:, 0]).all())
                rec["picks_outside_the_top_k"] = int((~np.isin(picked, first[:, :k])).sum())   # (isin over the batch: a rough count)
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
