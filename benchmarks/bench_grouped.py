#!/usr/bin/env python3
"""A batch in which every query has its own resident row set: mvdb_index_search_grouped against the loop of single-query
calls it replaces.  Corpus 1M x 512 and 10M x 512 synthetic rows, k = 10, nq in {8, 64, 256}; T disjoint tenants of equal
size for T in {nq, nq / 8} at 0.1 %, 1 % and 10 % of the corpus per tenant where that fits, plus one skewed case (one set of
half the corpus, the rest 0.1 %).  Per cell, sets resident, medians of --reps repetitions after warm-up:

  a  search_grouped_device                     hipEvents around device-buffer calls
  b  nq x search_rowset_device with nq = 1     hipEvents
  c  search_grouped                            host to host, wall clock
  d  nq x search_rowset with nq = 1            host to host, wall clock

--columns loop times b and d only (entry points that exist before the grouped search: run it on the parent build, library
chosen with MVDB_LIBMVDB), --columns grouped times a and c.  One JSON line per cell; --dropin adds find_most_similar_each
against a loop of find_most_similar at 1M x 512 with 64 tenants."""
import argparse
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


def timed_wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(per))


def cells(n, nqs):
    for nq in nqs:
        for tenants in sorted({nq, max(1, nq // 8)}, reverse=True):
            for frac in (0.001, 0.01, 0.1):
                if tenants * frac <= 1.0:
                    yield {"nq": nq, "tenants": tenants, "frac": frac, "skew": False}
        yield {"nq": nq, "tenants": nq, "frac": 0.001, "skew": True}


def tenant_lists(n, cell, rng):
    """Disjoint tenants of equal size (a random partition's first T parts), each list sorted."""
    m = int(n * cell["frac"])
    t = cell["tenants"]
    if cell["skew"]:
        perm = rng.permutation(n)
        lists = [np.sort(perm[:n // 2])]
        lists += [np.sort(perm[n // 2 + i * m:n // 2 + (i + 1) * m]) for i in range(t - 1)]
        return lists
    perm = rng.permutation(n)[:t * m]
    return [np.sort(perm[i * m:(i + 1) * m]) for i in range(t)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--columns", choices=("all", "loop", "grouped"), default="all")
    ap.add_argument("--dropin", action="store_true")
    args = ap.parse_args()
    d, k = 512, 10
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2024)
    for n in args.rows:
        idx = _native.FlatIndex(d)
        idx.reserve(n)
        idx.add_synthetic(n, 1234)
        for cell in cells(n, args.nq):
            nq = cell["nq"]
            lists = tenant_lists(n, cell, rng)
            rowsets = [idx.rowset(r) for r in lists]
            assert not any(rs.is_bitmap for rs in rowsets)
            sets = [rowsets[i % len(rowsets)] for i in range(nq)]
            touched = sum(len(lists[i % len(lists)]) for i in range(nq))
            qh = rng.standard_normal((nq, d), dtype=np.float32)
            q = torch.from_numpy(qh).cuda()
            D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            out = {"bench": "grouped", "n": n, "d": d, "k": k, **cell, "rows_touched": touched, "reps": args.reps,
                   "library": os.path.basename(_native.LIB_PATH),
                   "hooks": {v: os.environ[v] for v in ("MVDB_GROUPED_ITEMS_PER_CU", "MVDB_GROUPED_MIN_BATCHES") if v in os.environ}}
            if args.columns in ("all", "grouped"):
                a = timed_events(lambda: idx.search_grouped_device(q.data_ptr(), nq, k, sets, D.data_ptr(), I.data_ptr(),
                                                                   stream=stream, normalize_q=True), args.reps)
                out["a_grouped_device_ms"] = round(a, 4)
                out["a_tbps_rows_touched"] = round(touched * d * 4 / (a * 1e-3) / 1e12, 3)
                out["c_grouped_host_ms"] = round(timed_wall(lambda: idx.search_grouped(qh, k, sets, normalize_q=True), args.reps), 4)
            if args.columns in ("all", "loop"):
                def loop_device():
                    for i in range(nq):
                        idx.search_rowset_device(q.data_ptr() + i * d * 4, 1, k, sets[i], D.data_ptr() + i * k * 4,
                                                 I.data_ptr() + i * k * 8, stream=stream, normalize_q=True)

                def loop_host():
                    for i in range(nq):
                        idx.search_rowset(qh[i:i + 1], k, sets[i], normalize_q=True)

                out["b_loop_device_ms"] = round(timed_events(loop_device, args.reps), 4)
                out["d_loop_host_ms"] = round(timed_wall(loop_host, args.reps), 4)
            print(json.dumps(out), flush=True)
            for rs in rowsets:
                rs.close()
        idx.close()
        torch.cuda.empty_cache()

    if args.dropin:
        from minivectordb_amd import VectorDatabase
        nd, tenants = 1_000_000, 64
        x = rng.standard_normal((nd, d), dtype=np.float32)
        db = VectorDatabase(storage_file=os.path.join(tempfile.mkdtemp(), "g.pkl"))
        db.store_embeddings_batch(list(range(nd)), x, [{"tenant": i % tenants} for i in range(nd)])
        qs = rng.standard_normal((64, d), dtype=np.float32)
        filters = [{"metadata_filter": {"tenant": i % tenants}} for i in range(64)]
        out = {"bench": "grouped_dropin", "n": nd, "d": d, "k": k, "nq": 64, "tenants": tenants, "reps": args.reps}
        if hasattr(db, "find_most_similar_each"):
            out["each_ms"] = round(timed_wall(lambda: db.find_most_similar_each(qs, filters, k=k), args.reps), 3)
        out["loop_ms"] = round(timed_wall(lambda: [db.find_most_similar(qs[i], k=k, **filters[i]) for i in range(64)], args.reps), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
