#!/usr/bin/env python3
"""The single-query int8 route beside the exact fp32 scan, in ONE process and on one corpus.

Per configuration one JSON line: the prefilter launch's own mean duration (the library's `ip_scan` timer), its true rate on
its own bytes — N (3 d / 4 + 8) for the high plane and (a, r), plus d / 4 for every row whose low plane it fetched (the rows
its first stage could not reject: `refined_per_query`) — the wall time per query, the candidates of the timed queries
(min / median / max), and whether (D, I) of the first queries equal the exact scan's bit for bit.  The last line is the exact
scan (`code8_single_query = 0`): its launch time and rate on N d 4 bytes.  (Run from a checkout from before the two planes —
this file copied into its benchmarks/ — the index has no count of refined rows and the launch is rated on N (d + 8).)

  python3 benchmarks/code8_route_probe.py                              # 10M x 512, the grid the library picks
  python3 benchmarks/code8_route_probe.py --blocks 2,3,4               # MVDB_SCAN_BLOCKS_PER_CU swept in-process
  python3 benchmarks/code8_route_probe.py --front 2 --front-u 1,2,4 --blocks 1,2,3,4   # the front form's tiles per batch x its grid
  python3 benchmarks/code8_route_probe.py --family positive            # the all-positive corpus (or: clustered)
  python3 benchmarks/code8_route_probe.py --front 2 --lift 0,-1,0,-1   # the front form's survivors: lifted from the bit plane, gathered from
                                                                       # the 6-bit plane (no bit plane), in ONE process
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 benchmarks/code8_route_probe.py --timers 0
      (one trace session with both kernels: 200 route steps, then 40 exact scans; --timers 0 keeps the library's event
       pairs out of the stream, so the gaps in the trace are the route's own)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--exact-steps", type=int, default=40)
    ap.add_argument("--blocks", default="0", help="comma list of MVDB_SCAN_BLOCKS_PER_CU values (0 = the library's choice)")
    ap.add_argument("--family", default="zero_mean", choices=["zero_mean", "positive", "clustered"], help="the synthetic corpus and its queries")
    ap.add_argument("--timers", type=int, default=1, help="0: no per-launch event timers (for runs under a tracer)")
    ap.add_argument("--front-u", default="0", help="comma list of MVDB_CODE8_FRONT_U values, tiles per batch of the front form (0 = the library's "
                    "choice; d = 512, the quad layout: 1, 2, 4; the other widths: 4, 8), swept in-process with --blocks")
    ap.add_argument("--front", type=int, default=1, help="index option code8_front_plane: 1 the library decides, 2 always the front form, "
                    "3 the plane kept and never streamed, 0 no plane")
    ap.add_argument("--lift", default="0", help="comma list, swept in-process outside --front-u and --blocks: 0 the library's choice (the survivors of "
                    "the front form are lifted from the bit plane), -1 index option code8_bit_plane = 0 (gathered from the 6-bit plane); "
                    "a list that begins with -1 is written --lift=-1,0")
    args = ap.parse_args()

    import numpy as np
    import torch
    from minivectordb_amd import _native as native

    n, d, k = args.rows, args.dim, args.k
    flag = {"zero_mean": 0, "positive": 1 << 56, "clustered": 2 << 56}[args.family]   # (oracle.flat.SYNTH_*)
    W, K = args.warmup, args.steps
    dev = torch.device("cuda", 0)
    idx = native.FlatIndex(d, device=0)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flag, normalize=True)
    nqs = W + K
    queries = torch.empty((nqs, d), dtype=torch.float32, device=dev)
    native.check(native.lib().mvdb_synth_fill_device(queries.data_ptr(), nqs, d, 5678 | flag, 0, 1, 0, torch.cuda.current_stream().cuda_stream))
    D = torch.empty((1, k), dtype=torch.float32, device=dev)
    I = torch.empty((1, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(first, count):
        for i in range(first, first + count):
            idx.search_device(queries[i].data_ptr(), 1, k, D.data_ptr(), I.data_ptr(), stream)
        torch.cuda.synchronize()

    def results(count):
        out = []
        for i in range(W, W + count):
            run(i, 1)
            out.append((D.cpu().numpy().view(np.uint32).copy(), I.cpu().numpy().copy()))
        return out

    planes = hasattr(idx, "code8_refined")
    fronted = hasattr(idx, "code8_front_counters")
    lifted = hasattr(idx, "code8_bit_plane_held")
    if fronted:
        idx.set_option("code8_front_plane", args.front)

    def measure(steps, bytes_per_launch, label):
        run(0, W)
        native.prof_read("ip_scan")
        refined = idx.code8_refined() if planes else 0
        front0 = idx.code8_front_counters() if fronted else None
        native.prof_enable(bool(args.timers))
        t0 = time.perf_counter()
        run(W, steps)
        dt = time.perf_counter() - t0
        native.prof_enable(False)
        if label["route"] == "code8" and planes:
            label = dict(label, refined_per_query=round((idx.code8_refined() - refined) / steps, 1))
            bytes_per_launch = n * (d // 4 * 3 + 8) + int(label["refined_per_query"] * (d // 4))
            if fronted:
                # the front form streams 5 d / 8 + 8 bytes per row and gathers 3 d / 4 + 8 for every row its stage 0 keeps; the
                # launches of this measurement that ran it (the library's window may have suspended it for some)
                front1 = idx.code8_front_counters()
                fcalls = front1[1] - front0[1]
                per_front = (front1[0] - front0[0]) / max(fcalls, 1)
                label = dict(label, front_option=args.front, front_launches=fcalls, front_suspensions=front1[2],
                             front_survivors_per_launch=round(per_front, 1))
                per_survivor = d // 8 if lifted and idx.code8_bit_plane_held() else d // 4 * 3 + 8   # (the bit plane's row, or the gather)
                label = dict(label, bit_plane=bool(lifted and idx.code8_bit_plane_held()))
                front_bytes = n * (d // 8 * 5 + 8) + int(per_front * per_survivor) + int(label["refined_per_query"] * (d // 4))
                bytes_per_launch = (fcalls * front_bytes + (steps - fcalls) * bytes_per_launch) // steps
        launches, ms = native.prof_read("ip_scan")
        avg = ms / max(launches, 1)
        rec = dict(label, rows=n, dim=d, k=k, steps=steps, kernel=native.prof_symbol("ip_scan"), launches=launches,
                   launch_ms=round(avg, 5), true_bytes_per_launch=bytes_per_launch,
                   true_tb_per_s=round(bytes_per_launch / (avg * 1e-3) / 1e12, 4) if avg > 0 else None,
                   ms_per_query=round(dt / steps * 1e3, 5))
        return rec

    idx.set_option("code8_single_query", 0)
    want = results(8)
    idx.set_option("code8_single_query", 1)
    run(0, 3)   # the third eligible query builds the code
    for lift, front_u, blocks in [(l, u, b) for l in args.lift.split(",") for u in args.front_u.split(",") for b in args.blocks.split(",")]:
        os.environ["MVDB_SCAN_BLOCKS_PER_CU"] = blocks if int(blocks) > 0 else ""
        os.environ["MVDB_CODE8_FRONT_U"] = front_u if int(front_u) > 0 else ""
        idx.reload_env()
        if lifted:
            idx.set_option("code8_bit_plane", 0 if int(lift) < 0 else 1)
            run(0, 3)   # (a code that lacks the plane is rebuilt)
        got = results(8)
        same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, want))
        rec = measure(K, n * (d + 8), {"route": "code8", "blocks_per_cu": int(blocks), "front_u": int(front_u), "lift": int(lift)})
        fb, cand, calls = idx.code8_counters()
        cands = []
        for i in range(W, W + min(K, 32)):
            run(i, 1)
            cands.append(idx.code8_counters()[1])
        rec.update(bit_equal_exact_scan=bool(same), fallbacks=fb, last_candidates=cand, family=args.family,
                   candidates_min_median_max=[int(min(cands)), float(np.median(cands)), int(max(cands))], candidates=cands)
        print(json.dumps(rec), flush=True)
    os.environ["MVDB_SCAN_BLOCKS_PER_CU"] = ""
    os.environ["MVDB_CODE8_FRONT_U"] = ""
    idx.reload_env()
    idx.set_option("code8_single_query", 0)
    if args.exact_steps > 0:
        print(json.dumps(measure(args.exact_steps, n * d * 4, {"route": "exact"})), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
