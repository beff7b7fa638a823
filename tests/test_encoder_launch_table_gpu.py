"""The encoder's launch table on the device: which kernel instantiation, grid and LDS size every op of a layer launches.

The parity suites pass with any GEMM form, attention family or LayerNorm route: a slip in the rules that choose them costs
10 - 30 % on a shape and fails none of them.  This file pins the table.  Every case creates a fresh encoder under the case's
switches (read when the encoder is created), turns profiling on, runs ONE forward and asserts

  1. the results: the golden cases of tests/golden/encoder_golden.npz against transformers' stored outputs at the tolerance of
     tests/test_encoder_gpu.py (2e-5); the shapes beyond the golden set — e5-small widths, two layers, 256 sentences — are
     finite in every row and agree in rows 0, 1, 63, 64, 127, 128, 200, 255 with the float64 restatement of that sentence
     alone (2e-5: the reference semantics are B = 1, and a sentence's row does not depend on the batch);
  2. the symbols recorded under the labels of a forward (LABELS; "" for an op that was not launched) against
     tests/golden/encoder_launch_symbols.json.

The rules depend on the CU count: the fixture is for 256 CUs, and the cases skip on anything else.

The fixture is written by `record()` below (PYTHONPATH=. python tests/test_encoder_launch_table_gpu.py) and was recorded ONCE,
from a build of the commit BEFORE the launchers were rewritten around one form table — that commit's launch code with one
recording line beside every launch.  It states what the hand-written `if` chains launched.  Re-record it only with a change that
means to launch other kernels, from a build without that change's launch code.  record() runs every case in a child process of
its own: before this file existed most switches were read once per process, and a label kept its last symbol for good."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from encoder_cases import load_cases
from oracle import encoder as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_launch_symbols.json")
OPS = ["enc_pack", "enc_embed", "enc_qkv", "enc_qkv_epi", "enc_attn", "enc_ctx_split", "enc_wo", "enc_ln1", "enc_ffn1", "enc_ffn1_epi",
       "enc_ffn2", "enc_ln2", "enc_pool"]
PAIRED = ["enc_qkv", "enc_wo", "enc_ffn1", "enc_ffn2"]   # GEMMs that may be launched as (256-row form, fallback)
LABELS = OPS + [op + "_fallback" for op in PAIRED]
CUS = 256
CHECKED_ROWS = [0, 1, 63, 64, 127, 128, 200, 255]
WSEED, ISEED = 61, 62   # of the shapes beyond the golden set (seed 62, ragged: 15,659 of the 32,768 token slots are tokens)

_GOLDEN_CASES = load_cases()


def golden_case(i, compute, env=None):
    return {"golden": i, "compute": compute, "env": dict(env or {})}


def wide_case(S, ragged, compute, env=None):
    return {"S": S, "ragged": ragged, "compute": compute, "env": dict(env or {})}


def case_id(c):
    what = f"golden{c['golden']}" if "golden" in c else f"256x{c['S']}-{'ragged' if c['ragged'] else 'full'}"
    env = "".join(f"-{k[5:]}={v}" for k, v in sorted(c["env"].items()))
    return f"{what}-compute{c['compute']}{env}"


SPREAD_OFF = {"MVDB_GEMM_X3_SPREAD": "0", "MVDB_GEMM_X3_SPREAD_SMALL": "0", "MVDB_GEMM_LN_SPREAD": "0"}
SWITCH_SETS = [{"MVDB_GEMM_LN_FUSED": "2"},
               {"MVDB_GEMM_LN_FUSED": "0", "MVDB_ATTENTION_IMG": "0"},
               {"MVDB_GEMM_X3_BIG": "1"},
               {"MVDB_GEMM_X3_BIG": "1", "MVDB_GEMM_X3_PERSIST": "0"},
               SPREAD_OFF,
               {"MVDB_GEMM_X3_SPLITK": "0"},
               {"MVDB_GEMM_X3_SPLITK_PARTS": "3", "MVDB_GEMM_X3_SPLITK_WIDE": "0"},
               {"MVDB_ENCODER_ATTENTION": "valu"}]
CASES = (
    # golden cases, split-precision mode.  Forms on 256 CUs, restated for the reader — the fixture is what is asserted:
    [golden_case(4, 2),    # 4 x 32: 64 x 64 GEMM tiles, wo / FFN2 split over K into 3 / 8 planes, one-wave attention
     golden_case(5, 2),    # 2 x 130: eight-wave attention
     golden_case(8, 2),    # 256 x 32: 128 x 128 four-wave tiles for QKV and FFN1, the default 64 x 128 for N = 384, ln_kernel
     golden_case(9, 2),    # wide shape, 4 x 33: split-K QKV / FFN1 with partials_image, VPT 16, head width 64
     golden_case(11, 2),   # h96, 70 x 13: lane-masked LayerNorm, N no multiple of 64
     # 2 x 17 slots would take the layer-walking launch, which launches none of these: per-op kernels, head width 64
     golden_case(2, 2, {"MVDB_ENCODER_WALK": "0"}),
     golden_case(4, 0), golden_case(8, 0)]
    # 32,768 padded slots: both 256-row pairs (N = 1152 -> 192, N = 1536 -> 256), the LayerNorm-fused GEMM at 128 rows; the
    # full batch makes the 256-row form do the work on the device, the ragged one its fallback; exact mode: the two-lane split
    + [wide_case(128, False, 2), wide_case(128, True, 2), wide_case(128, True, 0)]
    # 16,384 padded slots with the fused GEMM forced: its 64-row band
    + [wide_case(64, False, 2, {"MVDB_GEMM_LN_FUSED": "2"})]
    + [golden_case(i, 2, env) for env in SWITCH_SETS for i in (4, 8)]
    # three planes forced on the wide shape: FFN1 split over K too (by itself it is at 65 ... 128 token slots), the GELU partials_image
    + [golden_case(9, 2, {"MVDB_GEMM_X3_SPLITK_PARTS": "3"})]
    + [golden_case(i, 0, {"MVDB_GEMM_DMA": "0"}) for i in (4, 8)])

_WEIGHTS = {}
_WIDE = {}


def weights(cfg, name, seed):
    """Seeded weights, computed once per (config, seed) and shared: nothing writes to them (an encoder copies them to the device)."""
    key = (name, cfg["num_hidden_layers"], seed)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = E.make_weights(cfg, seed)
    return _WEIGHTS[key]


def wide_inputs(S, ragged):
    """(cfg, weights, ids, mask, float64 reference of CHECKED_ROWS, each sentence alone): once per shape, shared read-only."""
    if (S, ragged) not in _WIDE:
        cfg = dict(E.make_config("e5-small-dims"), num_hidden_layers=2)
        w = weights(cfg, "e5-small-dims", WSEED)
        ids, mask = E.make_inputs(cfg, 256, S, ISEED, ragged=ragged)
        ref = np.concatenate([E.numpy_forward(cfg, w, ids[r:r + 1], mask[r:r + 1])[1] for r in CHECKED_ROWS])
        for a in (ids, mask, ref):
            a.setflags(write=False)
        _WIDE[(S, ragged)] = (cfg, w, ids, mask, ref)
    return _WIDE[(S, ragged)]


def run_case(native, c):
    """One forward of a fresh encoder under profiling: results asserted, {label: symbol} returned.  The case's switches are
    already in the environment."""
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    if "golden" in c:
        g = _GOLDEN_CASES[c["golden"]]
        cfg = E.make_config(g["name"])
        w, ids, mask = weights(cfg, g["name"], g["wseed"]), g["ids"], g["mask"]
    else:
        cfg, w, ids, mask, ref = wide_inputs(c["S"], c["ragged"])
    enc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0)
    native.prof_enable(False)
    native.prof_enable(True)   # (off -> on: forgets the symbols of earlier launches)
    try:
        emb = enc.forward(ids, mask, compute=c["compute"])
        symbols = {label: native.prof_symbol(label) for label in LABELS}
    finally:
        native.prof_enable(False)
        enc.close()
    if "golden" in c:
        np.testing.assert_allclose(emb, g["emb"], atol=2e-5, rtol=0)
    else:
        assert np.isfinite(emb).all(axis=1).all(), np.flatnonzero(~np.isfinite(emb).all(axis=1))
        np.testing.assert_allclose(emb[CHECKED_ROWS], ref, atol=2e-5, rtol=0)
    return symbols


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_results_and_launched_kernels(gpu, golden, c, monkeypatch):
    import torch
    from minivectordb_amd import _native
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != CUS:
        pytest.skip(f"the fixture states the launches of a {CUS}-CU device; this one has {cus}")
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)   # read when the encoder is created
    want = golden[case_id(c)]
    got = run_case(_native, c)
    assert got == want, {l: (got.get(l), want.get(l)) for l in LABELS if got.get(l) != want.get(l)}


def test_fixture_covers_the_table(golden):
    """Every form of the tables is in the fixture (read by eye against the hand-written `if` chains when it was recorded; the six
    spelled out are named there)."""
    assert sorted(golden) == sorted(case_id(c) for c in CASES)
    seen = {s for v in golden.values() for s in v.values()}

    def has(prefix):
        return any(s.startswith(prefix) for s in seen)
    # the seven forms of the split-precision GEMM (BM, NST, waves, BN / the persistent kernel's BN), and the split-K launch
    for form in ("gemm_x3_dma_kernel<EPI_BIAS_RESIDUAL, 64, 3, 4, 128, 1, 0>", "gemm_x3_dma_kernel<EPI_BIAS_QKV, 64, 3, 4, 64, 1, 0>",
                 "gemm_x3_dma_kernel<EPI_BIAS_QKV, 128, 2, 4, 128, 1, 0>", "gemm_x3_big_kernel<EPI_BIAS_GELU, 256, 1, 0>",
                 "gemm_x3_big_kernel<EPI_BIAS_QKV, 192, 1, 0>", "gemm_x3_dma_kernel<EPI_BIAS_GELU, 256, 2, 8, 256, 0, 0>",
                 "gemm_x3_dma_kernel<EPI_BIAS_QKV, 256, 2, 8, 192, 0, 0>", "gemm_x3_dma_kernel<EPI_PARTIAL, 64, 3, 4, 128, 1, 0>",
                 "partials_image_kernel<EPI_BIAS_QKV, ", "partials_image_kernel<EPI_BIAS_GELU, "):
        assert has(form), form
    # the LayerNorm-fused GEMM's band heights (H = 384: TN = 3): 128 / 64 rows on eight waves, 32 on four
    for band in ("gemm_x3_ln_kernel<128, 2, 3, ", "gemm_x3_ln_kernel<64, 2, 3, ", "gemm_x3_ln_kernel<32, 1, 3, "):
        assert has(band), band
    # the four attention families and the three wave counts
    for attn in ("attention_kernel<32>", "attention_mfma_kernel<32>", "attention_x3_kernel<32, 1>", "attention_x3i_kernel<32, 1>",
                 "attention_x3i_kernel<32, 4>", "attention_x3i_kernel<32, 8>", "attention_x3i_kernel<64, 4>"):
        assert has(attn), attn
    full, ragged = golden["256x128-full-compute2"], golden["256x128-ragged-compute2"]
    assert full == ragged   # the host knows the padded count only: the device chooses between the pair
    assert golden["golden4-compute2"]["enc_qkv"] == "gemm_x3_dma_kernel<EPI_BIAS_QKV, 64, 3, 4, 64, 1, 0> grid=(18,2,1) block=256 lds=49152 sel=0"
    assert golden["golden4-compute2"]["enc_ffn2"] == "gemm_x3_dma_kernel<EPI_PARTIAL, 64, 3, 4, 128, 1, 0> grid=(3,2,8) block=256 lds=73728 sel=0"
    assert golden["golden8-compute2"]["enc_ffn1"] == "gemm_x3_dma_kernel<EPI_BIAS_GELU, 128, 2, 4, 128, 1, 0> grid=(12,64,1) block=256 lds=65536 sel=0"
    assert full["enc_ffn1"] == "gemm_x3_big_kernel<EPI_BIAS_GELU, 256, 1, 0> grid=(256,1,1) block=512 lds=131072 sel=256"
    assert full["enc_ffn1_fallback"] == "gemm_x3_dma_kernel<EPI_BIAS_GELU, 128, 2, 4, 128, 1, 0> grid=(12,256,1) block=256 lds=65536 sel=-256"
    assert full["enc_wo"] == "gemm_x3_ln_kernel<128, 2, 3, 2, 1, 0> grid=(256,1,1) block=512 lds=135168"


def record(path=GOLDEN):
    """Write the fixture from the library that is loaded (see the module docstring for which build that must be): every case in
    a child process of its own, its switches in that process's environment."""
    out = {}
    for c in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case_id(c)], env=dict(os.environ, **c["env"]),
                           capture_output=True, text=True)
        assert r.returncode == 0, (case_id(c), r.stdout[-2000:], r.stderr[-2000:])
        out[case_id(c)] = json.loads(r.stdout.strip().splitlines()[-1])
        print(case_id(c), out[case_id(c)], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--case"]:
        from minivectordb_amd import _native
        print(json.dumps(run_case(_native, next(c for c in CASES if case_id(c) == sys.argv[2]))))
    else:
        record(*sys.argv[1:2])
