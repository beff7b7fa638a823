"""Scenario definitions (inputs only) for tests/golden/golden_usearch.json: what ShardedVectorDatabaseUsearch must do
like the reference's class.  New scenarios for the int8 cosine path, plus the sharded ones of scenarios.py run through
the usearch class ("sharded" opens it)."""
import scenarios
from scenarios import q


def colinear_d2():
    """d = 2 colinear rows (identical codes: zero distances, ties to the lower row), k > n, autocut over zeros."""
    rows = [[1.0, 2.0], [2.0, 4.0], [0.5, 1.0], [-1.0, -2.0], [2.0, -1.0], [1.0, 2.1], [3.0, 6.0]]
    ops = [{"op": "wipe", "path": "u_col"}, {"op": "open", "kind": "sharded", "path": "u_col", "kw": {"shard_size": 3}},
           {"op": "store_batch", "ids": list(range(len(rows))), "vecs": {"rows": [{"list": r} for r in rows]},
            "metas": [{"side": "pos" if r[0] > 0 else "neg", "i": i} for i, r in enumerate(rows)]}]
    for qv in ([1.0, 2.0], [-2.0, -4.0], [2.0, -1.0], [0.3, 0.9]):
        ops += [{"op": "search", "q": {"list": qv}, "k": 3},
                {"op": "search", "q": {"list": qv}, "k": 20},
                {"op": "search", "q": {"list": qv}, "k": 5, "autocut": True},
                {"op": "search", "q": {"list": qv}, "k": 4, "filter": {"side": "pos"}}]
    ops += [{"op": "state"}, {"op": "get_vector", "id": 4}, {"op": "get_vector", "id": 6}]
    return ops


def duplicates_zero_odd():
    """Exact duplicates (zero distance, autocut), a zero vector as row and as query, odd d, filters, exclude-all."""
    d = 17
    ops = [{"op": "wipe", "path": "u_dup"}, {"op": "open", "kind": "sharded", "path": "u_dup", "kw": {"shard_size": 6}}]
    ops.append({"op": "store_batch", "ids": list(range(10)), "vecs": {"synth_block": [61, 0, 10, d]},
                "metas": [{"g": i % 3, "keep": True} for i in range(10)]})
    for i in range(4):   # duplicates of row 2 (scaled by powers of two: identical codes)
        ops.append({"op": "store", "id": 100 + i, "vec": {"synth": [61, 2, d], "scale": 2.0 ** i}, "meta": {"g": 7}})
    ops.append({"op": "store", "id": 200, "vec": {"list": [0.0] * d}, "meta": {"g": 0, "zero": True}})
    ops += [{"op": "search", "q": {"synth": [61, 2, d]}, "k": 6},
            {"op": "search", "q": {"synth": [61, 2, d]}, "k": 6, "autocut": True},
            {"op": "search", "q": {"synth": [61, 2, d], "add": [62, 0, 0.3]}, "k": 8, "autocut": True},
            {"op": "search", "q": {"list": [0.0] * d}, "k": 4},
            {"op": "search", "q": q(1, d), "k": 30},
            {"op": "search", "q": q(1, d), "k": 5, "filter": {"g": 1}},
            {"op": "search", "q": q(1, d), "k": 5, "filter": {"g": {"$gte": 1}}, "exclude": {"g": 7}},
            {"op": "search", "q": q(1, d), "k": 5, "or": [{"g": 7}, {"zero": True}]},
            {"op": "search", "q": q(1, d), "k": 5, "exclude": [{"g": 0}, {"g": 1}, {"g": 2}, {"g": 7}]},
            {"op": "search", "q": q(1, d), "k": 5, "filter": {"g": 99}},
            {"op": "delete_batch", "ids": [2, 100, 200]},
            {"op": "search", "q": {"synth": [61, 2, d]}, "k": 6},
            {"op": "state"}, {"op": "reopen"}, {"op": "state"},
            {"op": "search", "q": {"synth": [61, 2, d]}, "k": 6, "autocut": True},
            {"op": "get_vector", "id": 103}]
    return ops


SCENARIOS = {
    "u_colinear_d2": colinear_d2,
    "u_duplicates_zero_odd": duplicates_zero_odd,
    "sharded": scenarios.sharded,
    "fuzz_sharded_3": lambda: scenarios._fuzz("sharded", 3),
    "delete_everything_sharded": lambda: scenarios.delete_everything("sharded"),
    "migrate": scenarios.migrate,
}
