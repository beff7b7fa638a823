"""GPU parity of the HIP encoder (mvdb_encoder_* through the C-ABI) with transformers' own model:
committed golden outputs + the float64 restatement.  Tolerance: 2e-5 on the unit-norm embeddings,
1e-4 on hidden states (values up to ~6), fp32 everywhere."""
import numpy as np
import pytest

from encoder_cases import load_cases
from oracle import encoder as E

pytestmark = pytest.mark.gpu
CASES = load_cases()


def _model(cfg, weights):
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    sd = {k: torch.from_numpy(v) for k, v in weights.items()}
    return GpuEncoder(cfg, sd, device=0)


@pytest.mark.parametrize("compute", [0, 2], ids=["fp32", "fp16x3"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_encoder_matches_transformers_golden(i, compute, gpu):
    """Both parity modes against transformers' own outputs, same tolerances: the exact fp32 matrix cores (compute = 0)
    and the split-precision fp16 x 3 GEMMs the drop-in uses by default (compute = 2: measured 6e-7 on the embeddings,
    8e-6 on hidden states of magnitude ~6 — the same as the exact mode)."""
    import torch
    c = CASES[i]
    cfg = E.make_config(c["name"])
    w = E.make_weights(cfg, c["wseed"])
    enc = _model(cfg, w)
    assert enc.default_compute == 2
    enc.default_compute = compute
    emb = enc.forward(c["ids"], c["mask"])
    np.testing.assert_allclose(emb, c["emb"], atol=2e-5, rtol=0)
    dev = torch.device("cuda", 0)
    out, hidden = enc.forward_device(torch.from_numpy(c["ids"]).to(dev), torch.from_numpy(c["mask"]).to(dev),
                                     want_hidden=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), emb, atol=0, rtol=0)  # host and device entry points agree
    hidden = hidden.cpu().numpy()
    m = c["mask"].astype(bool)
    if c["hidden_valid"] is not None:
        np.testing.assert_allclose(hidden[m], c["hidden_valid"], atol=1e-4, rtol=0)
    assert not hidden[~m].any()
    enc.close()
    if c["cls_emb"] is not None:
        # bge-m3 dense path (minivectordb/embedding_model.py:73-79): CLS pooling of the same XLM-R encoder, pinned
        # by transformers' XLMRobertaModel last_hidden_state[:, 0] (normalised as FlagEmbedding does)
        from minivectordb_amd.embedding_model import GpuEncoder
        encc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0, pooling="cls")
        np.testing.assert_allclose(encc.forward(c["ids"], c["mask"], compute=compute), c["cls_emb"], atol=2e-5, rtol=0)
        encc.close()


@pytest.mark.parametrize("switches", [{"MVDB_GEMM_LN_FUSED": "2"}, {"MVDB_GEMM_LN_FUSED": "0"},
                                      {"MVDB_ATTENTION_IMG": "0", "MVDB_GEMM_LN_FUSED": "0"}],
                         ids=["ln-fused-always", "ln-kernel", "fp32-qkv-attention"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_split_precision_kernel_variants_match_golden(i, switches, gpu, monkeypatch):
    """The default picks by batch size between (a) the N = H GEMMs with bias + residual + LayerNorm fused into their epilogue
    (gemm_x3_ln_kernel: row-owning workgroups, 32 / 64 / 128 rows by batch size) and (b) the 2D-tiled GEMM + ln_kernel; and
    attention runs on the (hi | lo) Q / K / V images of the QKV epilogue (attention_x3i_kernel: LDS-DMA'd tiles, transposed
    LDS reads) with the fp32-qkv kernel as the A/B reference.  Every variant, forced on every golden case (widths the
    fused kernel has no instantiation for — H = 64, 96, 1024 — fall back to (b) by themselves)."""
    import torch
    for k, v in switches.items():
        monkeypatch.setenv(k, v)  # read when the encoder is created
    c = CASES[i]
    cfg = E.make_config(c["name"])
    enc = _model(cfg, E.make_weights(cfg, c["wseed"]))
    emb = enc.forward(c["ids"], c["mask"], compute=2)
    np.testing.assert_allclose(emb, c["emb"], atol=2e-5, rtol=0)
    if c["hidden_valid"] is not None:
        dev = torch.device("cuda", 0)
        _, hidden = enc.forward_device(torch.from_numpy(c["ids"]).to(dev), torch.from_numpy(c["mask"]).to(dev), compute=2,
                                       want_hidden=True)
        torch.cuda.synchronize()
        np.testing.assert_allclose(hidden.cpu().numpy()[c["mask"].astype(bool)], c["hidden_valid"], atol=1e-4, rtol=0)
    enc.close()


@pytest.mark.parametrize("env", [{"MVDB_GEMM_X3_BIG": "1"}, {"MVDB_GEMM_X3_BIG": "1", "MVDB_GEMM_X3_PERSIST": "0"},
                                 {"MVDB_GEMM_X3_SPREAD": "0", "MVDB_GEMM_X3_SPREAD_SMALL": "0", "MVDB_GEMM_LN_SPREAD": "0"},
                                 {"MVDB_GEMM_X3_SPLITK": "0"}, {"MVDB_GEMM_X3_SPLITK_PARTS": "3", "MVDB_GEMM_X3_SPLITK_WIDE": "0"}],
                         ids=["persistent-256-row-tiles-forced", "one-tile-per-workgroup-256-row-tiles-forced", "dma-burst",
                              "ffn2-unsplit-at-small-batches", "three-split-k-planes-as-in-round-5"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_gemm_tile_forms_match_golden_in_a_fresh_process(i, env, gpu, monkeypatch):
    """The tile-form switches of the split-precision GEMMs are read when an encoder is created (once per process until the
    launchers got one switch table: this test then ran a child pytest per switch set; it keeps its name): a fresh encoder
    in THIS process runs every split-mode golden case with (a) the persistent 256-row kernel FORCED onto batches it would never
    be chosen for (fewer tiles than CUs, a last row band of a few rows), (b) its one-tile-per-workgroup predecessor, (c) the
    LDS-DMA instructions issued as one burst per K-step instead of between the MFMAs, (d) FFN2 unsplit at small batches (round
    4: by default it runs split over K there — which every golden case of the other tests exercises), (e) round 5's split-K
    rule (three planes, QKV / FFN1 of the wide shapes unsplit) beside round 6's (as many planes as leave each four K-steps: the
    other tests).  The assertions of test_encoder_matches_transformers_golden, at its tolerances."""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the encoder is created
    c = CASES[i]
    cfg = E.make_config(c["name"])
    w = E.make_weights(cfg, c["wseed"])
    enc = _model(cfg, w)
    emb = enc.forward(c["ids"], c["mask"], compute=2)
    np.testing.assert_allclose(emb, c["emb"], atol=2e-5, rtol=0)
    dev = torch.device("cuda", 0)
    out, hidden = enc.forward_device(torch.from_numpy(c["ids"]).to(dev), torch.from_numpy(c["mask"]).to(dev), compute=2,
                                     want_hidden=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), emb, atol=0, rtol=0)  # host and device entry points agree
    hidden = hidden.cpu().numpy()
    m = c["mask"].astype(bool)
    if c["hidden_valid"] is not None:
        np.testing.assert_allclose(hidden[m], c["hidden_valid"], atol=1e-4, rtol=0)
    assert not hidden[~m].any()
    enc.close()
    if c["cls_emb"] is not None:
        from minivectordb_amd.embedding_model import GpuEncoder
        encc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0, pooling="cls")
        np.testing.assert_allclose(encc.forward(c["ids"], c["mask"], compute=2), c["cls_emb"], atol=2e-5, rtol=0)
        encc.close()


def test_batch_composition_does_not_change_a_row(gpu, monkeypatch):
    """A sentence's embedding is bit-for-bit the same whatever else is in the batch and wherever its rows fall in a tile
    (the reference semantics are B = 1) — among batches served by the same GEMM form (here: 160 .. 320 token slots, all split over
    K into the same number of planes; across the form boundaries — where the plane count changes: 640 / 832 / 1,344 / ... token
    slots on this shape, x3_splitk_parts — and at 32,768 slots the K sums associate differently, <= 1.2e-7).  Round 3 found hipcc contracting `a * b + c` INTO the fp16 conversion of the
    (hi | lo) split (v_fma_mixlo_f16) on one epilogue path and not on another: the inputs of the split are opaque now."""
    for fused in ("2", "0"):
        monkeypatch.setenv("MVDB_GEMM_LN_FUSED", fused)
        cfg = E.make_config("e5-small-dims")
        enc = _model(cfg, E.make_weights(cfg, 21))
        ids, mask = E.make_inputs(cfg, 8, 40, 22)
        ref = enc.forward(ids, mask)
        for nb in (4, 5, 7):
            assert np.array_equal(enc.forward(ids[:nb], mask[:nb]), ref[:nb]), (fused, nb)
        # batches of <= 64 token slots run the layer-walking launch (exact fp32, its own summation order): another form
        # boundary, rounding-level agreement — and bit-for-bit agreement among themselves (tests/test_encoder_walk_gpu.py)
        assert enc.walks(1, 40) and not enc.walks(2, 40)
        one = enc.forward(ids[:1], mask[:1])
        np.testing.assert_allclose(one, ref[:1], atol=5e-7, rtol=0)
        three = enc.forward(ids[:3], mask[:3])      # (120 slots: the per-op kernels, another plane count than 160+ slots)
        np.testing.assert_allclose(three, ref[:3], atol=5e-7, rtol=0)
        enc.close()


def test_exact_mode_second_lane_workspace_grows(gpu):
    """The exact mode runs big batches as two halves on two streams; the second half's workspace has its own capacity
    (round-2 advisor finding: after forward(256, 256) a forward(129, 508) fits the first lane's 65536-token capacity but
    its second half needs 65 * 508 = 33020 token slots > the 32768 the second lane was sized for)."""
    cfg = E.make_config("tiny")
    w = E.make_weights(cfg, 3)
    cfg = dict(cfg, max_position_embeddings=512)
    w["embeddings.position_embeddings.weight"] = np.random.RandomState(5).standard_normal((512, cfg["hidden_size"])).astype(np.float32) * 0.5
    enc = _model(cfg, w)
    ids1, mask1 = E.make_inputs(cfg, 256, 256, 1)
    enc.forward(ids1, mask1, compute=0)
    ids2, mask2 = E.make_inputs(cfg, 129, 508, 2)
    got = enc.forward(ids2, mask2, compute=0)       # split: lanes of 64 and 65 sentences
    enc2 = _model(cfg, w)                            # fresh workspace, sized for this call
    want = enc2.forward(ids2, mask2, compute=0)
    assert np.array_equal(got, want)
    for b in (0, 64, 128):                           # and a row equals its own single-sentence forward
        n = int(mask2[b].sum())
        np.testing.assert_allclose(got[b], enc.forward(ids2[b:b + 1, :n], mask2[b:b + 1, :n], compute=0)[0], atol=2e-6, rtol=0)
    enc.close()
    enc2.close()


def test_encoder_matches_float64_and_live_transformers(gpu):
    cfg = E.make_config("e5-small-dims")
    w = E.make_weights(cfg, 21)
    ids, mask = E.make_inputs(cfg, 8, 40, 22)
    enc = _model(cfg, w)
    emb = enc.forward(ids, mask)
    _, e64 = E.numpy_forward(cfg, w, ids, mask)
    np.testing.assert_allclose(emb, e64, atol=2e-5, rtol=0)
    _, ehf = E.hf_forward(cfg, w, ids, mask)  # transformers is part of the image on the GPU box too
    np.testing.assert_allclose(emb, ehf, atol=2e-5, rtol=0)
    # a batched row equals the B = 1 forward of the same sentence (reference semantics are B = 1)
    for b in (1, 5):
        n = int(mask[b].sum())
        e1 = enc.forward(ids[b:b + 1, :n], mask[b:b + 1, :n])
        np.testing.assert_allclose(emb[b], e1[0], atol=2e-6, rtol=0)
    # repeated calls replay the captured hipGraph: identical bits; a new shape captures a new graph
    assert np.array_equal(enc.forward(ids, mask), emb)
    assert np.array_equal(enc.forward(ids[:4], mask[:4]), emb[:4])
    assert np.array_equal(enc.forward(ids, mask), emb)
    # arbitrary (non-prefix) masks are honoured too
    mask2 = mask.copy()
    mask2[:, 3] = 0
    _, e64b = E.numpy_forward(cfg, w, ids, mask2)
    np.testing.assert_allclose(enc.forward(ids, mask2), e64b, atol=2e-5, rtol=0)
    enc.close()


def test_embedding_model_api(gpu):
    """EmbeddingModel drop-in with injected weights + a stand-in tokenizer (no HF files offline)."""
    import torch
    from minivectordb_amd import AlternativeModel, EmbeddingModel

    cfg = E.make_config("e5-small-dims")
    w = E.make_weights(cfg, 10)

    class Tok:
        def __call__(self, texts, max_length=512, padding=True, truncation=True, return_tensors="np"):
            rows = [[(ord(ch) % 900) + 50 for ch in t][:max_length] for t in texts]
            S = max(len(r) for r in rows)
            ids = np.zeros((len(rows), S), np.int64)
            mask = np.zeros((len(rows), S), np.int64)
            for i, r in enumerate(rows):
                ids[i, :len(r)] = r
                mask[i, :len(r)] = 1
            return {"input_ids": ids, "attention_mask": mask}

    m = EmbeddingModel(use_quantized_onnx_model=False, alternative_model=AlternativeModel.small,
                       state_dict={k: torch.from_numpy(v) for k, v in w.items()}, config=cfg, tokenizer=Tok())
    e = m.extract_embeddings("i like dogs")
    assert isinstance(e, list) and len(e) == 384 and abs(np.linalg.norm(e) - 1.0) < 1e-5
    ids, mask = m._tokenize(["i like dogs"])
    assert ids.shape[1] == len("passage i like dogs")  # the reference's prompt prefix (no colon)
    _, want = E.numpy_forward(cfg, w, ids, mask)
    np.testing.assert_allclose(e, want[0], atol=2e-5)
    batch = m.extract_embeddings_batch(["i like dogs", "a much longer sentence about vector databases", "x"])
    np.testing.assert_allclose(batch[0], e, atol=2e-6)
    with pytest.raises(NotImplementedError):
        EmbeddingModel()  # quantised ONNX default: blob absent from the reference tree
    # bge-m3 (the reference's default alternative): XLM-R position ids + CLS pooling + normalise;
    # no prompt prefix (embedding_model.py:74-78 passes the raw text)
    xcfg = E.make_config("xlmr-tiny")
    xw = E.make_weights(xcfg, 9)

    class XTok(Tok):
        def __call__(self, texts, **kw):
            out = Tok.__call__(self, texts, **kw)
            out["input_ids"] = np.where(out["attention_mask"] == 1, out["input_ids"] % 140 + 2, 1)
            return out

    mb = EmbeddingModel(use_quantized_onnx_model=False, state_dict={k: torch.from_numpy(v) for k, v in xw.items()},
                        config=xcfg, tokenizer=XTok())
    assert mb.alternative_model == AlternativeModel.bgem3
    eb = mb.extract_embeddings("hello world")
    assert isinstance(eb, list) and len(eb) == 128
    tb = XTok()(["hello world"])
    hb, _ = E.numpy_forward(xcfg, xw, tb["input_ids"].astype(np.int32), tb["attention_mask"].astype(np.int32))
    cls = hb[0, 0] / np.linalg.norm(hb[0, 0])
    np.testing.assert_allclose(eb, cls, atol=2e-5)
    m2 = EmbeddingModel(use_quantized_onnx_model=False, e5_model_size="small",
                        state_dict={k: torch.from_numpy(v) for k, v in w.items()}, config=cfg, tokenizer=Tok())
    assert m2.alternative_model == AlternativeModel.small


def test_split_mode_recomputes_exactly_when_an_activation_leaves_fp16_range(gpu):
    """Activations enter the split-precision GEMMs as fp16 pieces.  With an FFN weight blown up by 1e6 the GELU outputs
    pass 65504, the split-precision forward turns non-finite, and the host path returns the exact-fp32 mode's result."""
    cfg = E.make_config("tiny")
    w = E.make_weights(cfg, 3)
    w = {k: v.copy() for k, v in w.items()}
    w["encoder.layer.0.intermediate.dense.weight"] *= np.float32(1e6)
    ids, mask = E.make_inputs(cfg, 15, 9, 4)   # 135 token slots: the per-op kernels (<= 128 slots run the exact-fp32 walking launch in both modes)
    enc = _model(cfg, w)
    assert not enc.walks(15, 9)
    import torch
    dev = torch.device("cuda", 0)
    ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    raw, _ = enc.forward_device(ids_d, mask_d, compute=2)
    assert not torch.isfinite(raw).all()                    # the device path reports what the kernels produced ...
    torch.cuda.synchronize()
    assert int(enc.overflow_flag().item()) == 1              # ... and raises the device-side flag (no embedding is read back for it)
    e2 = enc.forward(ids, mask, compute=2)
    e0 = enc.forward(ids, mask, compute=0)
    assert np.isfinite(e0).all() and np.array_equal(e2, e0)
    torch.cuda.synchronize()
    assert int(enc.overflow_flag().item()) == 0              # cleared by the next forward (the exact one)
    fixed, _ = enc.forward_device(ids_d, mask_d, compute=2, rerun_on_overflow=True)
    torch.cuda.synchronize()
    assert np.array_equal(fixed.cpu().numpy(), e0)
    # a sentence of padding only pools 0 / 0 = NaN (the reference's average_pool): not an overflow
    mask2 = mask.copy()
    mask2[1] = 0
    w_ok = E.make_weights(cfg, 3)
    enc2 = _model(cfg, w_ok)
    out2, _ = enc2.forward_device(torch.from_numpy(ids).to(dev), torch.from_numpy(mask2).to(dev), compute=2)
    torch.cuda.synchronize()
    assert torch.isnan(out2[1]).all() and int(enc2.overflow_flag().item()) == 0
    enc2.close()
    enc.close()


def test_removed_bf16_mode_is_refused(gpu):
    """compute = 1 (one bf16 product per GEMM, ~1e-3 on the embeddings) existed until round 3; the split-precision mode is
    faster and fp32-equivalent, so the mode is gone and asking for it must fail loudly, not compute something else."""
    cfg = E.make_config("tiny")
    enc = _model(cfg, E.make_weights(cfg, 1))
    ids, mask = E.make_inputs(cfg, 2, 8, 3)
    with pytest.raises(ValueError, match="compute mode 1"):
        enc.forward(ids, mask, compute=1)
    enc.close()
