"""ShardedVectorDatabaseUsearch against the records made from the REFERENCE class (tests/golden/make_golden_usearch.py),
with the device index replaced by its oracle restatement: every record identical, shard files byte-identical."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cos8_oracle  # noqa: E402
import golden_usearch_compare  # noqa: E402

GOLDEN = golden_usearch_compare.load()


@pytest.fixture
def oracle_backend(monkeypatch):
    from minivectordb_amd import _native
    from oracle_backend import OracleIndex
    monkeypatch.setattr(_native, "Cos8Index", cos8_oracle.OracleCos8Index)
    monkeypatch.setattr(_native, "FlatIndex", OracleIndex)    # the flat source database of the migration


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_usearch_scenario_matches_reference(name, tmp_path, oracle_backend):
    golden_usearch_compare.check_scenario(GOLDEN[name], str(tmp_path))


def test_fixture_covers_the_issue_scenarios():
    assert {"u_colinear_d2", "u_duplicates_zero_odd", "sharded", "fuzz_sharded_3", "delete_everything_sharded",
            "migrate"} <= set(GOLDEN)
    assert sum(1 for sc in GOLDEN.values() for s in sc["shards"].values() if "raw" in s) >= 20
