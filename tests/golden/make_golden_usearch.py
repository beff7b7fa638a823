#!/usr/bin/env python3
"""Generate tests/golden/golden_usearch.json by replaying tests/golden/scenarios_usearch.py through the REFERENCE's own
minivectordb.sharded_vector_database_usearch.ShardedVectorDatabaseUsearch (and VectorDatabase for the migration),
imported from the reference tree at generation time only; the tests read the committed JSON and never import it.

usearch is absent from this image, so `usearch.index` is bound to a stand-in: an exact brute force under the int8 cosine
contract of tests/cos8_oracle.py (ties to the lower key), which is what HNSW returns wherever HNSW is exact.  faiss and
thefuzz get make_golden.py's stand-ins.  Everything above that boundary is the reference's real code: filters, k
clamping, key -> row mapping, autocut over float32 distances, tuple / list returns, shard files, errors.

Besides the records, the fixture keeps the sha256 of every shard file the reference left behind at the end of each
scenario, so that the tests can require byte-identical files without the reference.  Pickled sets of STRING ids iterate
in a per-process hash order, so only shards whose ids are all integers are hashed ("raw"); the rest are compared after
loading ("content")."""
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import cos8_oracle  # noqa: E402
from golden_usearch_compare import shard_digests  # noqa: E402
import make_golden  # noqa: E402
import replay  # noqa: E402
import scenarios_usearch  # noqa: E402

REFERENCE = "/root/reference"


def install_usearch_stand_in():
    usearch = types.ModuleType("usearch")
    index = types.ModuleType("usearch.index")

    class Match:
        def __init__(self, key, distance):
            self.key = key
            self.distance = distance

    class Matches:
        def __init__(self, keys, distances):
            self.keys, self.distances = keys, distances

        def __len__(self):
            return len(self.keys)

        def __iter__(self):
            return (Match(int(k), d) for k, d in zip(self.keys, self.distances))

    class Index:
        def __init__(self, ndim, metric, dtype):
            assert metric == "cos" and dtype == "int8"
            self.ndim = ndim
            self.keys = np.zeros(0, np.int64)
            self.codes = np.zeros((0, ndim), np.int8)
            self.a2 = np.zeros(0, np.int32)

        def add(self, keys, vectors, copy=True):
            c, a = cos8_oracle.quantize(np.asarray(vectors, dtype=np.float32))
            self.keys = np.concatenate([self.keys, np.asarray(keys, np.int64)])
            self.codes = np.concatenate([self.codes, c])
            self.a2 = np.concatenate([self.a2, a])

        def search(self, query, count):
            query = np.atleast_2d(np.asarray(query, dtype=np.float32))
            assert query.shape[0] == 1
            order = np.argsort(self.keys, kind="stable")   # ties to the lower KEY
            D, I = cos8_oracle.search(self.codes[order], self.a2[order], query, count)
            found = I[0] >= 0
            return Matches(self.keys[order][I[0][found]], D[0][found])

    index.Index, index.Matches, index.Match = Index, Matches, Match
    usearch.index = index
    sys.modules["usearch"] = usearch
    sys.modules["usearch.index"] = index


def main():
    make_golden.install_stand_ins()
    install_usearch_stand_in()
    sys.path.insert(0, REFERENCE)
    from minivectordb.sharded_vector_database_usearch import ShardedVectorDatabaseUsearch
    from minivectordb.vector_database import VectorDatabase

    def make_db(kind, path, **kw):
        if kind == "flat":
            return VectorDatabase(storage_file=path)
        return ShardedVectorDatabaseUsearch(storage_dir=path, **kw)

    out = {}
    for name, build in scenarios_usearch.SCENARIOS.items():
        with tempfile.TemporaryDirectory() as tmp:
            ops = json.loads(json.dumps(build()))   # exactly the inputs the tests will read back
            expected = replay.run(make_db, ops, tmp)
            out[name] = {"ops": ops, "expected": expected, "shards": shard_digests(tmp)}
        errs = sum(1 for r in expected if "error" in r)
        print(f"{name}: {len(ops)} ops, {errs} recorded errors, {len(out[name]['shards'])} shard files")
    path = os.path.join(HERE, "golden_usearch.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
