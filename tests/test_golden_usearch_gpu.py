"""The golden usearch scenarios (recorded from the REFERENCE class) replayed through the HIP index: every record
identical — float32 distances bit for bit — and the shard files byte-identical."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import golden_usearch_compare  # noqa: E402

GOLDEN = golden_usearch_compare.load()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_usearch_scenario_through_hip(name, tmp_path, gpu):
    golden_usearch_compare.check_scenario(GOLDEN[name], str(tmp_path), flat_tol=1e-4)
