#!/usr/bin/env python3
"""Changing m stored rows of a large index: mvdb_index_set_rows against the remove_rows + add pair it replaces, and what the
first searches afterwards cost.  Corpus 1M x 512 and 10M x 512 synthetic normalised rows; before every repetition the fp16
shadow and the int8 code are built (one 64-query batch, four single queries).  m in {1, 100, 10000} scattered rows.  Per cell,
medians over --reps repetitions (and their spread, max - min):

  a  set_rows, host to host                              wall clock
  b  remove_rows of the same rows + add of the new ones   wall clock
  c  the FIRST 64-query batch search and the FIRST single query after a / after b   wall clock

--columns update times a (+ c after a); --columns parent times b (+ c after b) through entry points that exist before
set_rows: run it on the parent build (library chosen with MVDB_LIBMVDB).  --dropin: column d, through VectorDatabase at
1M x 512 — update_embedding followed by a filtered find_most_similar (--columns update), delete_embedding + store_embedding
followed by the same query (--columns parent).  One JSON line per cell, appended to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from minivectordb_amd import _native  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(values):
    return {"median_ms": round(float(np.median(values)), 4), "spread_ms": round(float(max(values) - min(values)), 4)}


def unit_rows(m, d, seed):
    x = np.random.default_rng(seed).standard_normal((m, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def index_cells(args, emit):
    d = 512
    for n in args.n:
        idx = _native.FlatIndex(d)
        idx.reserve(n + 10_000)
        idx.add_synthetic(n, 1234, normalize=True)
        idx.set_option("code8_single_query", 1)
        qb, q1 = unit_rows(64, d, 1), unit_rows(4, d, 2)

        def derived():
            idx.search(qb, 10)
            for qi in q1:
                idx.search(qi, 10)

        for m in args.m:
            rng = np.random.default_rng(m)
            op, batch, single = [], [], []
            shadow = code = None
            for rep in range(args.reps + 1):           # the first repetition warms up and is dropped
                derived()
                rows = np.sort(rng.choice(idx.ntotal, m, replace=False)).astype(np.int64)
                y = unit_rows(m, d, 100 + rep)
                if args.columns == "update":
                    t = wall(lambda: idx.set_rows(rows, y, normalize=True))
                else:
                    t = wall(lambda: (idx.remove_rows(rows), idx.add(y, normalize=True)))
                shadow, code = idx.shadow_rows, idx.code8_rows
                tb = wall(lambda: idx.search(qb, 10))
                ts = wall(lambda: idx.search(q1[0], 10))
                if rep:
                    op.append(t), batch.append(tb), single.append(ts)
            emit({"bench": "update", "column": "a_set_rows" if args.columns == "update" else "b_remove_add", "n": n, "d": d, "m": m,
                  "reps": args.reps, "op": stats(op), "first_batch64": stats(batch), "first_single": stats(single),
                  "shadow_rows_after": shadow, "code8_rows_after": code, "library": os.path.basename(_native.LIB_PATH)})
        idx.close()


def dropin_cell(args, emit):
    from minivectordb_amd import VectorDatabase
    n, d = 1_000_000, 512
    x = unit_rows(n, d, 3)
    with tempfile.TemporaryDirectory() as tmp:
        db = VectorDatabase(storage_file=os.path.join(tmp, "db.pkl"))
        db.store_embeddings_batch(list(range(n)), x, [{"tenant": i % 100} for i in range(n)])
        q = unit_rows(1, d, 4)[0]
        f = {"tenant": 7}
        db.find_most_similar(q, metadata_filter=f, k=10)
        per = []
        for rep in range(args.reps + 1):
            uid = 7 + 100 * (rep + 1)
            y = unit_rows(1, d, 50 + rep)[0]
            if args.columns == "update":
                t = wall(lambda: (db.update_embedding(uid, embedding=y), db.find_most_similar(q, metadata_filter=f, k=10)))
            else:
                t = wall(lambda: (db.delete_embedding(uid), db.store_embedding(uid, y, {"tenant": 7}),
                                  db.find_most_similar(q, metadata_filter=f, k=10)))
            if rep:
                per.append(t)
        emit({"bench": "update", "column": "d_update_then_query" if args.columns == "update" else "d_delete_store_then_query",
              "n": n, "d": d, "reps": args.reps, "op": stats(per), "library": os.path.basename(_native.LIB_PATH)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", choices=["update", "parent"], required=True)
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--m", type=int, nargs="+", default=[1, 100, 10_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dropin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_bench.jsonl"))
    args = ap.parse_args()
    if args.columns == "parent":
        # a library from before set_rows exports none of its symbols: nothing here calls them
        for name in [k for k in _native.PROTOTYPES if "set_rows" in k]:
            del _native.PROTOTYPES[name]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    index_cells(args, emit)
    if args.dropin:
        dropin_cell(args, emit)


if __name__ == "__main__":
    main()
