"""SPLADE's head on the device (csrc/splade_head.hpp, mvdb_encoder_forward_splade_device) against tests/splade_oracle.py.
Per (shape, compute mode) ONE run on the device is shared by the assertions; the float64 forward of a shape is computed once.
Bounds (none is a measured number).  w = max_t f(z_t) with f = log1p . relu, 1-Lipschitz, so |dw| <= max_t |dz_t|, and for
z = t . E_v + b_v as three fp16 x fp16 products per 16-deep step with fp32 accumulation (splade_oracle.logit_bound)
    |dz| <= sum_i eps_t[i] |E_vi|                  the transform's own error, carried through the product
          + (2^-21 + gamma_H) sum_i |t_i E_vi|     the split (2^-22 per operand, two operands), an any-order fp32 sum of H terms
          + 8 ulp (sum_i |t_i E_vi| + |b_v| + 1)   the power-of-two scale, the bias add, log1pf
  * on the device's OWN hidden states eps_t = 1e-4: test_encoder_gpu.py's tolerance for a LayerNorm output (the transform is that op chain);
  * end to end against oracle.encoder.numpy_forward the hidden states are within 1e-4 (test_encoder_gpu.py), which
    splade_oracle.transform_bound carries through |W_t|_1 and |g| / sigma of every token, plus the 1e-4 above.
The pruning's structure is exact.  The maxima seen go to profiles/splade_parity.jsonl (MVDB_SPLADE_PARITY_OUT moves it)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import splade_oracle as SO
from oracle import encoder as E

pytestmark = pytest.mark.gpu

# name: (config, overrides, B, S, lengths (None: ragged by make_inputs), tied decoder, max_terms, unused ids)
SHAPES = {
    "edge": ("xlmr-tiny", {}, 4, 19, [19, 1, 7, 0], True, 16, (0, 1, 2, 3)),  # one token; all padding; one band, 4 sentences; V = 150: a column tail
    "band": ("tiny", {"max_position_embeddings": 256}, 3, 200, [200, 1, 77], False, 20, (0,)),  # a sentence across bands; own decoder, two equal rows
    "h96": ("h96", {}, 2, 33, None, True, 1024, (0, 5)),                          # the K tail (H = 96); max_terms above the positives
    "v301": ("tiny", {"vocab_size": 301}, 5, 24, None, True, 40, ()),            # three column tiles, the last one 45 wide
    "past-small-pack": ("e5-small-dims", {}, 70, 8, None, True, 256, (0, 100, 101)),  # B > 64: the three packing kernels
}
CASES = pytest.mark.parametrize("shape,compute", [(s, c) for s in SHAPES for c in (0, 2)])


@functools.lru_cache(maxsize=None)
def _problem(shape):  # -> cfg, weights, ids, mask, head, numpy_forward's float64 hidden states (0 on the padding) and embeddings
    name, over, B, S, lens, tied, max_terms, unused = SHAPES[shape]
    cfg = dict(E.make_config(name), **over)
    w = E.make_weights(cfg, 7)
    ids, mask = E.make_inputs(cfg, B, S, 11)
    if lens is not None:
        mask = (np.arange(S)[None, :] < np.asarray(lens)[:, None]).astype(np.int32)
        ids = np.where(mask == 1, ids, cfg["pad_token_id"]).astype(np.int32)
    with np.errstate(invalid="ignore"):  # (the all-padding sentence's own rows are NaN in float64 too; nothing reads them)
        x, emb = E.numpy_forward(cfg, w, ids, mask)
    x = np.where(mask[..., None] == 1, x, 0.0)
    hd = SO.make_head(cfg, 5, tied=tied)
    if not tied:  # equal weights at the cut: in sentence 0 the first weight the pruning drops becomes a copy of the last one kept
        w0 = SO.weights(SO.logits(x, w, hd, cfg["layer_norm_eps"])[1], mask)[0]
        w0[list(unused)] = 0
        order = sorted(range(len(w0)), key=lambda i: (-w0[i], i))
        keep, drop = order[max_terms - 1], order[max_terms]
        hd["dec_w"][drop], hd["dec_b"][drop] = hd["dec_w"][keep], hd["dec_b"][keep]
    return cfg, w, ids, mask, hd, x, emb


def _encoder(shape, hd="own"):
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    cfg, w = _problem(shape)[:2]
    enc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0)
    if hd is not None:
        enc.set_mlm_head(SO.state_dict(cfg, _problem(shape)[4] if hd == "own" else hd), SHAPES[shape][7])
    return enc


def _device(enc, shape, compute):  # one SPLADE forward with every output, as numpy, and the overflow word behind it
    import torch
    ids, mask = (torch.from_numpy(a).to("cuda:0") for a in _problem(shape)[2:4])
    res = enc.forward_splade_device(ids, mask, compute=compute, max_terms=SHAPES[shape][6], return_weights=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}, int(enc.overflow_flag().item())


@functools.lru_cache(maxsize=None)
def _run(shape, compute):
    """Everything the device gives for one (shape, mode): two SPLADE forwards, plain forwards around them, the hidden states."""
    import torch
    ids, mask = _problem(shape)[2:4]
    enc = _encoder(shape)
    before = enc.forward(ids, mask, compute=compute)
    first, flag = _device(enc, shape, compute)
    second, _ = _device(enc, shape, compute)
    after = enc.forward(ids, mask, compute=compute)
    dense_plain, hidden = enc.forward_device(torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(mask).to("cuda:0"), compute=compute, want_hidden=True)
    torch.cuda.synchronize()
    out = {"first": first, "second": second, "same_plain": before.tobytes() == after.tobytes(), "flag": flag, "dense_plain": dense_plain.cpu().numpy(),
           "hidden": hidden.cpu().numpy(), "host": enc.forward_splade(ids, mask, compute=compute, max_terms=SHAPES[shape][6]), "walks": enc.walks(*ids.shape)}
    enc.close()
    return out


def _check_weights(check, shape, compute, x, eps_t):  # the device's [B, V] weights against float64 on x, within logit_bound(eps_t)
    cfg, w, _, mask, hd = _problem(shape)[:5]
    t, z = SO.logits(x, w, hd, cfg["layer_norm_eps"])
    bound = np.where(mask[..., None] == 1, SO.logit_bound(t, SO.decoder(w, hd), hd, eps_t), 0.0).max(axis=1)
    err = np.abs(_run(shape, compute)["first"]["weights"].astype(np.float64) - SO.weights(z, mask))
    rec = {"check": check, "shape": shape, "compute": compute, "err_max": float(err.max()), "err_over_bound_max": float((err[bound > 0] / bound[bound > 0]).max())}
    default = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "splade_parity.jsonl")
    with open(os.environ.get("MVDB_SPLADE_PARITY_OUT", default), "a") as f:
        f.write(json.dumps(rec) + "\n")
    assert (err <= bound).all(), (float(err.max()), float(bound[err > bound].min()))


@CASES
def test_structure_is_exact(shape, compute, gpu):
    mask, (max_terms, unused), run = _problem(shape)[3], SHAPES[shape][6:8], _run(shape, compute)
    got, wts = run["first"], run["first"]["weights"]
    assert run["flag"] == 0 and wts.dtype == np.float32 and wts.shape == (len(mask), _problem(shape)[0]["vocab_size"]) and (wts >= 0).all()
    pruned = 0
    for b in range(len(mask)):
        keys, vals = SO.prune(wts[b], max_terms, unused)  # the oracle's pruning of the device's OWN weights
        n = int(got["count"][b])
        assert n == len(keys) and got["indices"][b, :n].tolist() == keys and got["values"][b, :n].tobytes() == np.asarray(vals, np.float32).tobytes(), b
        assert not got["indices"][b, n:].any() and not got["values"][b, n:].any() and not set(keys) & set(unused)
        assert mask[b].any() or (n == 0 and not wts[b].any())  # an all-padding sentence: count 0
        pruned += int((wts[b] > 0).sum()) > max_terms
        assert list(run["host"][b]) == keys and [np.float32(v) for v in run["host"][b].values()] == [np.float32(v) for v in vals]
    assert pruned == (0 if max_terms == 1024 else int(mask.any(axis=1).sum()))  # the cut bites where it is meant to
    if shape == "band":  # the two equal weights met at the cut of sentence 0: the lower id stayed
        row = wts[0].copy()
        row[list(unused)] = 0
        tie = np.flatnonzero(row == np.sort(row)[-max_terms])
        assert len(tie) == 2 and tie[0] in got["indices"][0] and tie[1] not in got["indices"][0]


@CASES
def test_weights_match_float64_on_the_devices_hidden_states_and_end_to_end(shape, compute, gpu):
    cfg, _, _, mask, hd, x, emb = _problem(shape)
    run = _run(shape, compute)
    assert not run["walks"]  # the device's hidden states come from the same per-op kernels
    _check_weights("weights_on_device_hidden", shape, compute, run["hidden"].astype(np.float64), 1e-4)
    _check_weights("end_to_end", shape, compute, x, SO.transform_bound(x, hd, cfg["layer_norm_eps"], 1e-4) + 1e-4)
    assert np.abs(run["first"]["dense"] - emb)[mask.any(axis=1)].max() <= 2e-5


@CASES
def test_repeatability_and_non_interference(shape, compute, gpu):
    run = _run(shape, compute)
    assert run["first"]["dense"].tobytes() == run["dense_plain"].tobytes()  # the same per-op kernels (no shape here walks): the same bits
    assert sorted(run["first"]) == sorted(run["second"]) == ["count", "dense", "indices", "values", "weights"]
    assert all(run["first"][k].tobytes() == run["second"][k].tobytes() for k in run["first"]) and run["same_plain"]  # (plain forwards around: unchanged)


def test_chunked_sentences_give_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("MVDB_SPLADE_BUF_KIB", "1")  # 256 words: one sentence of 150 weights per chunk
    enc = _encoder("edge")
    got, flag = _device(enc, "edge", 0)
    assert flag == 0 and all(got[k].tobytes() == v.tobytes() for k, v in _run("edge", 0)["first"].items())
    enc.close()


def test_nonfinite_logits_raise_the_overflow_word(gpu):
    hd, clean = _problem("v301")[4], _run("v301", 0)["first"]
    enc = _encoder("v301", dict(hd, dec_b=np.where(np.arange(301) == 300, np.float32("nan"), hd["dec_b"])))  # the last column of the partial tile
    got, flag = _device(enc, "v301", 0)
    assert flag == 1 and np.isnan(got["weights"][:, 300]).all() and 300 not in got["indices"]
    assert got["weights"][:, :300].tobytes() == clean["weights"][:, :300].tobytes() and got["dense"].tobytes() == clean["dense"].tobytes()
    enc.set_mlm_head(SO.state_dict(_problem("v301")[0], hd))  # the head back in place: the word is cleared by the next forward
    got, flag = _device(enc, "v301", 0)
    assert flag == 0 and got["weights"].tobytes() == clean["weights"].tobytes()
    enc.close()


def test_argument_errors_enqueue_nothing(gpu):
    import torch
    from minivectordb_amd import _native
    cfg, _, ids, mask, hd = _problem("edge")[:5]
    ids_d, mask_d, (B, S), enc = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(mask).to("cuda:0"), ids.shape, _encoder("edge", None)
    shapes = {"dense": (B, cfg["hidden_size"]), "weights": (B, cfg["vocab_size"]), "count": (B,), "indices": (B, 1024), "values": (B, 1024)}
    bufs = {k: torch.full(s, 77, dtype=torch.int32 if k in ("count", "indices") else torch.float32, device="cuda:0") for k, s in shapes.items()}

    def call(max_terms, without=()):  # -> (return code, message, every buffer still holds the sentinel)
        p = {k: ctypes.c_void_p(0 if k in without else t.data_ptr()) for k, t in bufs.items()}
        rc = _native.lib().mvdb_encoder_forward_splade_device(
            enc._h, ctypes.c_void_p(ids_d.data_ptr()), ctypes.c_void_p(mask_d.data_ptr()), B, S, 0, p["dense"], max_terms, p["weights"],
            p["count"], p["indices"], p["values"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, _native.last_error(), all(bool((t == 77).all()) for t in bufs.values())

    assert call(16)[0::2] == (_native.ERR_ARG, True) and "MLM head" in _native.last_error()  # no head set
    with pytest.raises(ValueError, match="MLM head"):
        enc.forward_splade_device(ids_d, mask_d)
    enc.set_mlm_head(SO.state_dict(cfg, hd))
    for bad in (0, 1025):  # max_terms outside [1, 1024]
        assert call(bad)[0::2] == (_native.ERR_ARG, True) and "max_terms" in _native.last_error()
    assert call(16, without=("count",))[0::2] == (_native.ERR_ARG, True) and "go together" in _native.last_error()  # a NULL count with lists
    assert call(16)[0::2] == (0, False)
    enc.close()
