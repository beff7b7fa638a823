"""bench.py --gpus 1 as the plain headline run: `--steps` timed steps, one JSON line without the --full blocks, and
`--dump-outputs DIR` holding what the last timed step returned — the same from run to run, and the same as a single-index
search of that step's query."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import flat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("host_api_qps", "power", "opt_in_single_query_over_fp16_shadow", "certified_passes_on_unfriendly_data",
             "encoder", "config5")


def _bench(out_dir, rows, d, k, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--rows", str(rows), "--dim", str(d), "--k", str(k), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True,
                       timeout=int(os.environ.get("MVDB_TEST_SUBPROCESS_TIMEOUT", "600")))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_bench_dumps_the_last_timed_step(gpu, tmp_path):
    from minivectordb_amd import _native as native
    rows, d, k, steps, warmup = 300_000, 512, 10, 7, 3
    a = _bench(tmp_path / "a", rows, d, k, steps, warmup)
    assert a["steps"] == steps and a["warmup"] == warmup and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(1e3 / a["ms_per_step"], rel=5e-3)
    assert a["unit"] == "queries/s" and a["higher_is_better"] is True and a["metric"] and a["dtype"].startswith("f32")
    assert not [key for key in FULL_ONLY if key in a], a.keys()
    assert a["cpu_baseline"] is None
    D, I = np.load(tmp_path / "a" / "D.npy"), np.load(tmp_path / "a" / "I.npy")
    assert D.dtype == np.float32 and I.dtype == np.float64 and D.shape == I.shape == (1, k)
    # the same arguments give the same inputs, so the same outputs
    _bench(tmp_path / "b", rows, d, k, steps, warmup)
    assert np.load(tmp_path / "b" / "D.npy").tobytes() == D.tobytes()
    assert np.load(tmp_path / "b" / "I.npy").tobytes() == I.tobytes()
    # ... which are the top-k of the last timed query: query warmup + steps - 1 of stream 5678 over rows of stream 1234
    q = flat.synth(warmup + steps, d, 5678)
    flat.normalize_l2(q)
    idx = native.FlatIndex(d, device=0)
    idx.add_synthetic(rows, 1234, normalize=True)
    D1, I1 = idx.search(q[warmup + steps - 1], k)
    idx.close()
    assert np.array_equal(I[0].astype(np.int64), I1[0]), (I, I1)
    np.testing.assert_allclose(D[0], D1[0], atol=2e-6, rtol=0)
