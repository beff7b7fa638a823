"""The numpy restatement of BGE-M3's heads (tests/m3_oracle.py) against the same heads written with torch ops — the way the
model's own inference code writes them: relu(Linear), a scatter-max into [B, S, vocab] reduced over the sequence with the
unused columns zeroed, F.normalize — and the loader of the two head files.  No GPU."""
import numpy as np
import pytest

import m3_oracle as M
from oracle import encoder as E


def _hidden(B, S, H, seed):
    return (np.random.RandomState(seed).standard_normal((B, S, H)) * 1.5).astype(np.float32)


def _torch_heads(ids, mask, x, heads, vocab, unused=M.UNUSED):
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(x).double()
    m = torch.from_numpy(mask)
    tw = torch.relu(xt @ torch.from_numpy(heads["sparse_w"]).double() + float(heads["sparse_b"])) * m
    B, S = ids.shape
    plane = torch.zeros(B, S, vocab, dtype=torch.float64)
    plane = torch.scatter(plane, -1, torch.from_numpy(ids).long().unsqueeze(-1), tw.unsqueeze(-1))
    lex = plane.max(dim=1).values
    lex[:, list(unused)] = 0.0
    u = xt @ torch.from_numpy(heads["colbert_w"]).double().T + torch.from_numpy(heads["colbert_b"]).double()
    col = F.normalize(u[:, 1:], dim=-1) * m[:, 1:, None]
    return tw.numpy(), lex.numpy(), col.numpy()


@pytest.mark.parametrize("case", ["edge", "ragged"])
def test_restatement_matches_torch_ops(case):
    cfg = E.make_config("xlmr-tiny")
    vocab, H = cfg["vocab_size"], cfg["hidden_size"]
    if case == "edge":
        ids, mask = M.edge_batch(vocab)
    else:
        ids, mask = E.make_inputs(cfg, 12, 16, 3)
        ids[:, 0] = 0
    B, S = ids.shape
    x = _hidden(B, S, H, 17)
    heads = M.make_heads(H, 64, 23)
    tw_t, lex_t, col_t = _torch_heads(ids, mask, x, heads, vocab)

    tw = M.token_weights(x, mask, heads["sparse_w"], heads["sparse_b"])
    np.testing.assert_allclose(tw, tw_t, rtol=0, atol=1e-12)
    assert not tw[mask == 0].any()
    lex = M.lexical_weights(ids, mask, x, heads["sparse_w"], heads["sparse_b"])
    vecs = M.colbert_vecs(x, mask, heads["colbert_w"], heads["colbert_b"])
    lens = mask.sum(axis=1)
    for b in range(B):
        want = {int(i): lex_t[b, i] for i in np.nonzero(lex_t[b])[0]}
        assert sorted(lex[b]) == sorted(want) and list(lex[b]) == sorted(lex[b])  # the same ids, emitted ascending
        for i, v in want.items():
            assert abs(lex[b][i] - v) <= 1e-12
        assert not set(lex[b]) & set(M.UNUSED)
        n = max(int(lens[b]) - 1, 0)
        assert vecs[b].shape == (n, 64)
        np.testing.assert_allclose(vecs[b], col_t[b, :n], rtol=0, atol=1e-12)
        assert not col_t[b, n:].any()
        if n:
            np.testing.assert_allclose(np.linalg.norm(vecs[b], axis=1), 1.0, rtol=0, atol=1e-12)
    if case == "edge":
        assert lex[1] == {} and vecs[1].shape[0] == 0             # length 1: CLS alone
        assert sum(int(i) == 9 for i in ids[0]) == 3 and (9 in lex[0]) == (tw[0][ids[0] == 9].max() > 0)
        assert lex[0].get(9, 0.0) == tw[0][ids[0] == 9].max()       # the maximum of the three, whatever the neighbours


def test_dedupe_drops_nan_zero_and_unused_keeps_inf():
    ids = np.array([[0, 7, 7, 5, 6, 8, 2, 4]], dtype=np.int32)
    mask = np.array([[1, 1, 1, 1, 1, 1, 1, 0]], dtype=np.int32)
    tw = np.array([[3.0, 0.5, 0.25, np.nan, 0.0, np.inf, 9.0, 1.0]], dtype=np.float32)
    (keys, vals), = M.dedupe(ids, mask, tw)
    assert keys == [7, 8] and vals[0] == np.float32(0.5) and vals[1] == np.inf


def test_load_m3_heads_round_trip(tmp_path):
    import torch
    from minivectordb_amd.embedding_model import load_m3_heads
    assert load_m3_heads(str(tmp_path)) == (None, None)
    heads = M.make_heads(128, 64, 3)
    sparse, colbert = M.state_dicts(heads)
    torch.save(sparse, tmp_path / "sparse_linear.pt")
    got_s, got_c = load_m3_heads(str(tmp_path))
    assert got_c is None and torch.equal(got_s["weight"], sparse["weight"]) and torch.equal(got_s["bias"], sparse["bias"])
    torch.save(colbert, tmp_path / "colbert_linear.pt")
    got_s, got_c = load_m3_heads(str(tmp_path))
    assert got_s["weight"].shape == (1, 128) and got_c["weight"].shape == (64, 128)
    assert torch.equal(got_c["weight"], colbert["weight"]) and torch.equal(got_c["bias"], colbert["bias"])


def test_multi_extraction_without_heads_says_what_is_missing():
    from minivectordb_amd.embedding_model import EmbeddingModel
    em = EmbeddingModel.__new__(EmbeddingModel)  # (no device here: the check comes before anything touches the model)
    em.has_heads, em.tokenizer, em.model = False, None, None
    for call in (lambda: em.extract_embeddings_multi("a"), lambda: em.extract_embeddings_multi_batch(["a", "b"])):
        with pytest.raises(RuntimeError) as err:
            call()
        for word in ("sparse_linear.pt", "colbert_linear.pt", "sparse_linear=", "colbert_linear=", "model_path"):
            assert word in str(err.value)


def test_new_entry_points_are_exported():
    from minivectordb_amd import _native
    for name in ("mvdb_encoder_set_heads", "mvdb_encoder_forward_multi_device"):
        assert name in _native.PROTOTYPES and hasattr(_native.lib(), name)
    assert _native.lib().mvdb_abi_version() == 1
