"""BGE-M3's heads on the device (csrc/m3_heads.hpp, mvdb_encoder_forward_multi_device) against tests/m3_oracle.py.

Per (shape, compute mode) ONE run on the device is shared by the assertions below; the float64 forward of a shape is computed
once for both modes.  Bounds (none is a measured number):
  * lexical structure: exact — the oracle's dedupe of the device's own token weights gives the device's counts, ids, values;
  * heads on the device's own hidden states: token weights within the any-order fp32 dot-product bound
    gamma_{H+2} (sum |x_i w_i| + |b|); ColBERT rows within 2e-5 (test_encoder_gpu.py's tolerance for unit-norm vectors);
  * end to end against oracle.encoder.numpy_forward: hidden states are within 1e-4 (test_encoder_gpu.py), so token weights
    within 1e-4 |w|_1 + the bound above, ColBERT rows within 2 sqrt(C) 1e-4 max_j |colbert_w[j]|_1 / |u|_2 + 2e-5
    (normalisation is 2 / |u| - Lipschitz).
The maxima seen go to profiles/m3_parity.jsonl (MVDB_M3_PARITY_OUT moves the file)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import m3_oracle as M
from oracle import encoder as E

pytestmark = pytest.mark.gpu

# name: (config, B, S, colbert_dim, inputs)
SHAPES = {
    "edge": ("xlmr-tiny", 3, 19, 128),        # lengths 19 / 1 / 7, planted special ids, a triple repeat; <= 64 slots
    "ragged-40": ("xlmr-tiny", 40, 16, 128),  # ragged; still packed by pack_small_kernel (kPackSmallB is 64, not below 40)
    "past-small-pack": ("xlmr-tiny", 70, 8, 128),  # B > kPackSmallB: seq_rank / seq_scan / pack_fill and the flag's memset node
    "h96": ("h96", 2, 33, 96),                # H = C = 96: the lane tail; S = 33 is no power of two for the sort
    "large": ("xlmr-large-dims", 2, 512, 1024),  # lengths 512 / 300 over a vocabulary of 300: longest sort, widest rows
    "c64": ("xlmr-tiny", 5, 24, 64),          # colbert_dim < H
}
CASES = [(s, c) for s in SHAPES for c in (0, 2)]
IDS = [f"{s}-{'fp32' if c == 0 else 'fp16x3'}" for s, c in CASES]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    name, B, S, C = SHAPES[shape]
    cfg = E.make_config(name)
    w = E.make_weights(cfg, 7)
    if shape == "edge":
        ids, mask = M.edge_batch(cfg["vocab_size"])
    else:
        ids, mask = E.make_inputs(cfg, B, S, 11)
        if shape == "large":
            mask = (np.arange(S)[None, :] < np.array([[512], [300]])).astype(np.int32)
            ids = np.random.RandomState(2).randint(4, cfg["vocab_size"], size=(B, S)).astype(np.int32)
        lens = mask.sum(axis=1)
        ids[:, 0] = 0
        for b in range(B):
            if lens[b] >= 2:
                ids[b, lens[b] - 1] = 2
            if lens[b] >= 6:
                ids[b, 2], ids[b, 3] = 3, ids[b, 4]  # an unused id mid-sentence and a repeat
        ids = np.where(mask == 1, ids, cfg["pad_token_id"]).astype(np.int32)
    assert ids.shape == (B, S)
    heads = M.make_heads(cfg["hidden_size"], C, 164)
    return cfg, w, ids, mask, heads


@functools.lru_cache(maxsize=None)
def _reference(shape):
    cfg, w, ids, mask, heads = _problem(shape)
    x, emb = E.numpy_forward(cfg, w, ids, mask)
    if cfg["model_type"] != "bert":  # the encoders below pool CLS for XLM-R (BGE-M3's dense vector), mean for BERT
        emb = x[:, 0] / np.maximum(np.linalg.norm(x[:, 0], axis=1, keepdims=True), 1e-12)
    return x, emb


def _encoder(shape, heads=True):
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    cfg, w, _, _, hd = _problem(shape)
    enc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0,
                     pooling="mean" if cfg["model_type"] == "bert" else "cls")
    if heads:
        enc.set_heads(*M.state_dicts(hd))
    return enc


def _to_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _run(shape, compute):
    """Everything the device gives for one (shape, mode): two multi forwards, plain forwards around them, the hidden states."""
    import torch
    cfg, w, ids, mask, heads = _problem(shape)
    dev = torch.device("cuda", 0)
    enc = _encoder(shape)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    before = enc.forward(ids, mask, compute=compute)
    first = enc.forward_multi_device(ids_d, mask_d, compute=compute)
    torch.cuda.synchronize()
    flag = int(enc.overflow_flag().item())
    second = enc.forward_multi_device(ids_d, mask_d, compute=compute)
    torch.cuda.synchronize()
    after = enc.forward(ids, mask, compute=compute)
    dense_plain, hidden = enc.forward_device(ids_d, mask_d, compute=compute, want_hidden=True)
    torch.cuda.synchronize()
    host = enc.forward_multi(ids, mask, compute=compute)
    out = {"first": _to_numpy(first), "second": _to_numpy(second), "before": before, "after": after, "flag": flag,
           "dense_plain": dense_plain.cpu().numpy(), "hidden": hidden.cpu().numpy(), "host": host, "walks": enc.walks(*ids.shape)}
    enc.close()
    return out


def _record(rec):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.environ.get("MVDB_M3_PARITY_OUT", os.path.join(root, "profiles", "m3_parity.jsonl"))
    print("[m3 parity]", json.dumps(rec))
    try:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("shape,compute", CASES, ids=IDS)
def test_lexical_structure_is_exact(shape, compute, gpu):
    _, _, ids, mask, _ = _problem(shape)
    got = _run(shape, compute)["first"]
    assert _run(shape, compute)["flag"] == 0
    tw = got["token_weights"]
    assert tw.dtype == np.float32 and not tw[mask == 0].any() and (tw >= 0).all()
    want = M.dedupe(ids, mask, tw)
    lens = mask.sum(axis=1)
    dropped = 0
    for b, (keys, vals) in enumerate(want):
        n = int(got["lex_count"][b])
        assert n == len(keys), (b, n, len(keys))
        assert got["lex_indices"][b, :n].tolist() == keys
        assert got["lex_values"][b, :n].tobytes() == np.asarray(vals, dtype=np.float32).tobytes()
        assert not got["lex_indices"][b, n:].any() and not got["lex_values"][b, n:].any()
        assert not set(keys) & set(M.UNUSED)
        dropped += int(lens[b]) - n
        if lens[b] == 1:
            assert n == 0 and int(got["colbert_count"][b]) == 0
    assert dropped > 0  # unused ids, repeats or zero weights were there to drop
    # the host entry trims the same outputs into dicts
    host = _run(shape, compute)["host"]
    for b, (keys, vals) in enumerate(want):
        assert list(host["lexical_weights"][b]) == keys
        assert [np.float32(v) for v in host["lexical_weights"][b].values()] == [np.float32(v) for v in vals]
        assert host["colbert_vecs"][b].shape == (max(int(lens[b]) - 1, 0), SHAPES[shape][3])
        assert np.array_equal(host["colbert_vecs"][b], got["colbert"][b, :max(int(lens[b]) - 1, 0)])
    assert np.array_equal(host["token_weights"], tw) and np.array_equal(host["dense"], got["dense"])


@pytest.mark.parametrize("shape,compute", [c for c in CASES if SHAPES[c[0]][1] * SHAPES[c[0]][2] > 64],
                         ids=[i for i, c in zip(IDS, CASES) if SHAPES[c[0]][1] * SHAPES[c[0]][2] > 64])
def test_heads_match_float64_on_the_devices_hidden_states(shape, compute, gpu):
    cfg, _, ids, mask, heads = _problem(shape)
    run = _run(shape, compute)
    assert not run["walks"]  # the hidden states below come from the same per-op kernels
    got, x = run["first"], run["hidden"]
    H, C = cfg["hidden_size"], SHAPES[shape][3]
    want = M.token_weights(x, mask, heads["sparse_w"], heads["sparse_b"])
    bound = M.token_weight_bound(x, mask, heads["sparse_w"], heads["sparse_b"], H)
    err = np.abs(got["token_weights"].astype(np.float64) - want)
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))
    lens = mask.sum(axis=1)
    vecs = M.colbert_vecs(x, mask, heads["colbert_w"], heads["colbert_b"])
    cerr = 0.0
    for b in range(ids.shape[0]):
        n = max(int(lens[b]) - 1, 0)
        assert int(got["colbert_count"][b]) == n
        assert not got["colbert"][b, n:].any()  # exactly 0 behind the count
        if n:
            cerr = max(cerr, float(np.abs(got["colbert"][b, :n] - vecs[b]).max()))
    assert got["colbert"].shape == (ids.shape[0], ids.shape[1] - 1, C)
    assert cerr <= 2e-5, cerr
    _record({"check": "heads_on_device_hidden", "shape": shape, "compute": compute, "tw_err_max": float(err.max()),
             "tw_err_over_bound_max": float((err[bound > 0] / bound[bound > 0]).max()), "colbert_err_max": cerr})


@pytest.mark.parametrize("shape,compute", CASES, ids=IDS)
def test_end_to_end_against_the_float64_forward(shape, compute, gpu):
    cfg, _, ids, mask, heads = _problem(shape)
    got = _run(shape, compute)["first"]
    x, emb = _reference(shape)
    H, C = cfg["hidden_size"], SHAPES[shape][3]
    want = M.token_weights(x, mask, heads["sparse_w"], heads["sparse_b"])
    tol = 1e-4 * float(np.abs(heads["sparse_w"].astype(np.float64)).sum()) + M.token_weight_bound(x, mask, heads["sparse_w"], heads["sparse_b"], H)
    err = np.abs(got["token_weights"].astype(np.float64) - want)
    assert (err[mask == 1] <= tol[mask == 1]).all(), float(err.max())
    assert not err[mask == 0].any()
    u = M.colbert_pre(x, heads["colbert_w"], heads["colbert_b"])
    unorm = np.linalg.norm(u, axis=-1)
    w1 = float(np.abs(heads["colbert_w"].astype(np.float64)).sum(axis=1).max())
    lens = mask.sum(axis=1)
    vecs = M.colbert_vecs(x, mask, heads["colbert_w"], heads["colbert_b"])
    cerr, cratio = 0.0, 0.0
    for b in range(ids.shape[0]):
        n = max(int(lens[b]) - 1, 0)
        assert int(got["colbert_count"][b]) == n
        if not n:
            continue
        ctol = 2.0 * np.sqrt(C) * 1e-4 * w1 / unorm[b, 1:n + 1] + 2e-5
        e = np.abs(got["colbert"][b, :n] - vecs[b]).max(axis=1)
        assert (e <= ctol).all(), (b, float(e.max()))
        cerr, cratio = max(cerr, float(e.max())), max(cratio, float((e / ctol).max()))
    derr = float(np.abs(got["dense"] - emb).max())
    assert derr <= 2e-5, derr
    _record({"check": "end_to_end", "shape": shape, "compute": compute, "tw_err_max": float(err.max()),
             "tw_err_over_tol_max": float((err[mask == 1] / tol[mask == 1]).max()), "colbert_err_max": cerr,
             "colbert_err_over_tol_max": cratio, "dense_err_max": derr})


@pytest.mark.parametrize("shape,compute", CASES, ids=IDS)
def test_dense_output_and_repeatability(shape, compute, gpu):
    run = _run(shape, compute)
    if not run["walks"]:
        assert run["first"]["dense"].tobytes() == run["dense_plain"].tobytes()  # the same per-op kernels: the same bits
    else:
        assert np.abs(run["first"]["dense"] - run["dense_plain"]).max() <= 2e-5  # the plain call walks the layers in one launch
    assert sorted(run["first"]) == sorted(run["second"]) == ["colbert", "colbert_count", "dense", "lex_count", "lex_indices",
                                                             "lex_values", "token_weights"]
    for k in run["first"]:
        assert run["first"][k].tobytes() == run["second"][k].tobytes(), k
    assert run["before"].tobytes() == run["after"].tobytes()  # a plain forward is what it was


def test_nonfinite_token_weights_raise_the_overflow_word(gpu):
    import torch
    _, _, ids, mask, heads = _problem("ragged-40")
    dev = torch.device("cuda", 0)
    enc = _encoder("ragged-40")
    sparse, colbert = M.state_dicts(heads)
    sparse["bias"] = torch.tensor([float("nan")])
    enc.set_heads(sparse, colbert)
    res = enc.forward_multi_device(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), compute=0)
    torch.cuda.synchronize()
    assert int(enc.overflow_flag().item()) == 1
    res = _to_numpy(res)
    assert not res["lex_count"].any()
    assert np.isnan(res["token_weights"][mask == 1]).all() and not res["token_weights"][mask == 0].any()
    clean = _run("ragged-40", 0)["first"]
    assert res["colbert"].tobytes() == clean["colbert"].tobytes() and res["dense"].tobytes() == clean["dense"].tobytes()
    # the heads back in place: the word is cleared by the next forward
    enc.set_heads(*M.state_dicts(heads))
    enc.forward_multi_device(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), compute=0)
    torch.cuda.synchronize()
    assert int(enc.overflow_flag().item()) == 0
    enc.close()


def test_argument_errors_enqueue_nothing(gpu):
    import torch
    from minivectordb_amd import _native
    cfg, _, ids, mask, heads = _problem("c64")
    dev = torch.device("cuda", 0)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    B, S = ids.shape
    H = cfg["hidden_size"]
    enc = _encoder("c64", heads=False)
    sparse, colbert = M.state_dicts(heads)
    SENT = 12345.0
    dense = torch.full((B, H), SENT, device=dev)
    bufs = {k: torch.full(shape, 77, dtype=dt, device=dev) for k, (shape, dt) in {
        "token_weights": ((B, S), torch.float32), "lex_count": ((B,), torch.int32), "lex_indices": ((B, S), torch.int32),
        "lex_values": ((B, S), torch.float32), "colbert": ((B, S - 1, 64), torch.float32), "colbert_count": ((B,), torch.int32)}.items()}

    def call(fields, S_arg=S):
        out = _native.M3Out(**{k: bufs[k].data_ptr() for k in fields})
        rc = _native.lib().mvdb_encoder_forward_multi_device(
            enc._h, ctypes.c_void_p(ids_d.data_ptr()), ctypes.c_void_p(mask_d.data_ptr()), B, S_arg, 0, ctypes.c_void_p(dense.data_ptr()),
            ctypes.byref(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, _native.last_error()

    def untouched():
        torch.cuda.synchronize()
        return bool((dense == SENT).all()) and all(bool((t == 77).all()) for t in bufs.values())

    rc, msg = call(["token_weights"])
    assert rc == _native.ERR_ARG and "heads" in msg and untouched()                       # heads not set
    with pytest.raises(ValueError, match="heads"):
        enc.forward_multi_device(ids_d, mask_d)
    enc.set_heads(sparse)                                                                   # the sparse head alone
    rc, msg = call(["colbert", "colbert_count"])
    assert rc == _native.ERR_ARG and "ColBERT" in msg and untouched()                     # a ColBERT output without its head
    with pytest.raises(ValueError, match="ColBERT"):
        enc.forward_multi_device(ids_d, mask_d)
    for part in (["lex_count"], ["lex_indices", "lex_values"], ["lex_count", "lex_values"]):
        rc, msg = call(part)
        assert rc == _native.ERR_ARG and "go together" in msg and untouched()              # lexical outputs in part
    rc, msg = call(["token_weights"], S_arg=1025)
    assert rc == _native.ERR_ARG and "1024" in msg and untouched()                        # S > 1024
    for bad in (48, 160):                                                                   # no multiple of 32 / wider than H
        with pytest.raises(ValueError, match="colbert_dim"):
            enc.set_heads(sparse, {"weight": torch.zeros(bad, H), "bias": torch.zeros(bad)})
    # the sparse head alone still serves the sparse outputs
    res = enc.forward_multi_device(ids_d, mask_d, compute=0, return_colbert=False)
    torch.cuda.synchronize()
    assert sorted(res) == ["dense", "lex_count", "lex_indices", "lex_values", "token_weights"]
    assert res["token_weights"].cpu().numpy().tobytes() == _run("c64", 0)["first"]["token_weights"].tobytes()
    enc.close()
