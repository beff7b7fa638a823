#!/usr/bin/env python3
"""The rows stage 0 of the prefilter's front form cannot reject, per call: 3 corpora x 8 queries at
the smallest size the route serves plus one, d = 512, the front form forced (code8_front_plane = 2).  One JSON object:
{"<family>/<d>": [survivors of query 0, ..., of query 7]}.

T5 is an exact integer and the floor is the same bits in every build, so the counts are a property of the stored plane and
the unpacking, not of the launch's shape.  tests/golden/code8_front_survivors.json was written by this script from a checkout
of the commit BEFORE the quad layout of the plane (this file copied into its benchmarks/); tests/test_code8_front_quad_gpu.py
requires every later build to reproduce it.

  python3 benchmarks/code8_front_survivors.py > tests/golden/code8_front_survivors.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N, D, K, NQ = 500_001, 512, 10, 8
FAMILIES = {"zero_mean": 0, "positive": 1 << 56, "clustered": 2 << 56}   # (oracle.flat.SYNTH_*)


def survivors_per_call(native, family, n=N, d=D, k=K, nq=NQ):
    from oracle import flat
    flag = FAMILIES[family]
    idx = native.FlatIndex(d)
    idx.reserve(n)
    idx.add_synthetic(n, 1234 | flag, normalize=True)
    qs = flat.synth(nq, d, 5678 | flag)
    flat.normalize_l2(qs)
    idx.set_option("code8_front_plane", 2)
    for _ in range(3):   # the third eligible query builds the code
        idx.search(qs[0], k)
    out = []
    for q in qs:
        before = idx.code8_front_counters()
        idx.search(q, k)
        after = idx.code8_front_counters()
        assert after[1] - before[1] == 1, "the front form did not serve the call"
        out.append(int(after[0] - before[0]))
    idx.close()
    return out


def main():
    from minivectordb_amd import _native as native
    print(json.dumps({f"{family}/{D}": survivors_per_call(native, family) for family in sorted(FAMILIES)}))


if __name__ == "__main__":
    main()
