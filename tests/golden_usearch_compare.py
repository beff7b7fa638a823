"""Replay of tests/golden/golden_usearch.json (recorded from the REFERENCE's ShardedVectorDatabaseUsearch by
tests/golden/make_golden_usearch.py) and its comparison: every record identical — ids, float32 distances bit for bit,
metadata, return types, errors, id maps, shard bookkeeping — and every shard file the reference left behind
byte-identical (or, for shards holding string ids, whose pickled sets follow a per-process hash order, identical in
content).  One deliberate deviation: where the reference's get_vector fails by indexing a shard with the stacked row
number (sharded_vector_database_usearch.py:84-95), the drop-in returns the row."""
import hashlib
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import replay  # noqa: E402


def load():
    with open(os.path.join(HERE, "golden", "golden_usearch.json")) as f:
        return json.load(f)


def canonical(data):
    """sha256 of a shard's content with sets sorted (independent of the per-process string hash order)."""
    emb = np.ascontiguousarray(data["embeddings"])
    h = hashlib.sha256()
    h.update(str(emb.dtype).encode() + str(emb.shape).encode() + emb.tobytes())
    h.update(repr(data["metadata"]).encode())
    h.update(repr(data["unique_ids"]).encode())
    h.update(repr([(k, sorted(map(repr, v))) for k, v in data["inverted_index"].items()]).encode())
    return h.hexdigest()


def shard_digests(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in sorted(files):
            if not f.startswith("shard_"):
                continue
            path = os.path.join(dirpath, f)
            blob = open(path, "rb").read()
            data = pickle.loads(blob)
            rel = os.path.relpath(path, root)
            if all(isinstance(u, int) for u in data["unique_ids"]):
                out[rel] = {"raw": hashlib.sha256(blob).hexdigest()}
            else:
                out[rel] = {"content": canonical(data)}
    return out


def make_db(kind, path, **kw):
    from minivectordb_amd import ShardedVectorDatabaseUsearch, VectorDatabase
    if kind == "flat":
        return VectorDatabase(storage_file=path)
    return ShardedVectorDatabaseUsearch(storage_dir=path, **kw)


def _norm(rec):
    r = dict(rec)
    if "inverse_id_map" in r:
        r["inverse_id_map"] = sorted(r["inverse_id_map"], key=lambda kv: str(kv[0]))
    return r


def check_scenario(scenario, workdir, flat_tol=0.0):
    """flat_tol: the fp32 VectorDatabase a migration starts from scores in fp32 on the device, in another summation order
    than the oracle's; its searches (before the "migrate" op) are compared as tests/test_golden_gpu.py does."""
    import golden_compare
    got = replay.run(make_db, scenario["ops"], workdir)
    want = scenario["expected"]
    assert len(got) == len(want)
    flat = any(op["op"] == "open" and op["kind"] == "flat" for op in scenario["ops"])
    for i, (g, w) in enumerate(zip(got, want)):
        if w["op"] == "migrate":
            flat = False
        if flat and flat_tol and w["op"] == "search":
            golden_compare.compare_search(g, w, flat_tol, exact=False)
            continue
        if w["op"] == "get_vector" and w.get("error") == "IndexError":
            assert "vector" in g, (i, g)       # the deliberate get_vector fix
            continue
        assert _norm(g) == _norm(w), (i, g, w)
    has_flat = any(op["op"] == "open" and op["kind"] == "flat" for op in scenario["ops"])
    if not (flat_tol and has_flat):
        # (a migration's shards hold the rows the fp32 VectorDatabase normalised on the device, within an ulp of the
        #  oracle's normalisation: byte identity of those files is checked on the CPU, where both sides use the oracle)
        assert shard_digests(workdir) == scenario["shards"]
