#!/usr/bin/env python3
"""MaxSim search (mvdb_index_search_maxsim_device) beside the exact single-query scan it repeats per query vector.  Corpus
1M x 512 and 10M x 512 normalised synthetic rows added on the device, documents of 8 consecutive rows, k = 10; T = 1, 4, 8, 32
query vectors.  Device buffers, hipEvents on the current stream, the median of --reps calls after 3 warm-up calls.

  case "chunked"   codes = row // 8.  Each cell is run twice in the same process:
      maxsim_ms            the default rule of the vectors per pass (Tp = min(T, 32) at d = 512: one pass)
      per_vector_ms        index option maxsim_tokens_per_pass = 1: one corpus pass PER VECTOR with everything else equal —
                           what T calls of a one-vector search cost on the device today, without their transfers
      exact_scan_ms        the exact single-query scan of the same index (search_device, nq = 1, k = 10, index option
                           code8_single_query = 0), measured in the same run: a pass reads the same row bytes + 4 per row
      passes               corpus passes of one call under each setting (from maxsim_counters)
      scan_launch_ms       the clear and the scan launches of a default call together (mvdb_prof_read, calls of their own),
      select_launch_ms     its top-k and emit launches
      bound_bytes_ms       passes x exact_scan_ms: a pass is no faster than the row bytes at the scan's own achieved rate
      bound_fma_ms         n x d x T FMAs at 64 FMA / clk / CU, the plain fp32 vector rate (--cus, --mhz: 256 CUs at 2400 MHz)
  case "one_group"   every row in group 0, 10M x 512 only, T = 8: every offer of a pass goes to the 8 words of one cache line.

One JSON line per cell, to stdout and to --out (default profiles/maxsim_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd import _native  # noqa: E402

from bench_distinct import launch_ms, timed_events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--T", type=int, nargs="+", default=[1, 4, 8, 32])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--adversarial-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_bench.jsonl"))
    args = ap.parse_args()
    d, k = 512, args.k
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2029)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        q = torch.from_numpy(rng.standard_normal((max(args.T), d), dtype=np.float32)).cuda()
        Dc = torch.empty((1, k), dtype=torch.float32, device="cuda")
        Ic = torch.empty((1, k), dtype=torch.int64, device="cuda")
        D = torch.empty((k,), dtype=torch.float32, device="cuda")
        G = torch.empty((k,), dtype=torch.int32, device="cuda")

        def exact_scan():
            idx.search_device(q.data_ptr(), 1, k, Dc.data_ptr(), Ic.data_ptr(), stream=stream, normalize_q=True)

        idx.set_option("code8_single_query", 0)
        exact_ms = round(timed_events(exact_scan, args.reps), 4)
        idx.set_option("code8_single_query", 1)

        cases = [("chunked", (np.arange(n, dtype=np.int64) // 8).astype(np.int32), (n + 7) // 8, args.T)]
        if n == args.adversarial_rows:
            cases.append(("one_group", np.zeros(n, np.int32), 1, [8]))
        for case, codes, n_groups, Ts in cases:
            grouping = idx.grouping(codes, n_groups)
            for T in Ts:
                I_tok = torch.empty((k, T), dtype=torch.int64, device="cuda")
                D_tok = torch.empty((k, T), dtype=torch.float32, device="cuda")

                def maxsim():
                    idx.search_maxsim_device(q.data_ptr(), T, k, grouping, D.data_ptr(), G.data_ptr(), I_tok.data_ptr(), D_tok.data_ptr(),
                                             stream=stream, normalize_q=True)

                def timed(knob):
                    idx.set_option("maxsim_tokens_per_pass", knob)
                    calls0, passes0 = idx.maxsim_counters()
                    ms = round(timed_events(maxsim, args.reps), 4)
                    torch.cuda.synchronize()
                    calls1, passes1 = idx.maxsim_counters()
                    return ms, (passes1 - passes0) // (calls1 - calls0), (D.cpu().numpy().copy(), G.cpu().numpy().copy(), I_tok.cpu().numpy().copy())

                rec = {"bench": "maxsim", "case": case, "n": n, "d": d, "T": T, "k": k, "n_groups": n_groups, "reps": args.reps,
                       "exact_scan_ms": exact_ms}
                rec["maxsim_ms"], rec["passes"], got = timed(0)
                rec["per_vector_ms"], rec["per_vector_passes"], base = timed(1)
                idx.set_option("maxsim_tokens_per_pass", 0)
                rec["same_results"] = bool(all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                              b.view(np.uint32) if b.dtype == np.float32 else b) for a, b in zip(got, base)))
                rec["speedup_over_per_vector"] = round(rec["per_vector_ms"] / rec["maxsim_ms"], 3)
                rec["scan_launch_ms"], rec["scan_symbol"] = launch_ms(maxsim, "maxsim_scan", 2, per_call=True)
                rec["select_launch_ms"], _ = launch_ms(maxsim, "maxsim_select", 2, per_call=True)
                rec["bound_bytes_ms"] = round(rec["passes"] * exact_ms, 4)
                rec["bound_fma_ms"] = round(n * d * T / (64.0 * args.cus * args.mhz * 1e3), 4)
                rec["over_bound"] = round(rec["maxsim_ms"] / max(rec["bound_bytes_ms"], rec["bound_fma_ms"]), 3)
                rec["table_mb"] = round(T * n_groups * 8 / 1e6, 1)
                emit(rec)
            grouping.free()
        idx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
