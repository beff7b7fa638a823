"""tests/splade_oracle.py against transformers' own masked-language-model heads (fp32, CPU, seeded weights): pins the formula and
the weight names GpuEncoder.set_mlm_head accepts.  And the pruning restatement on hand-made rows."""
import numpy as np
import pytest

import splade_oracle as SO
from oracle import encoder as E


@pytest.mark.parametrize("name,tied", [("tiny", True), ("xlmr-tiny", True), ("tiny", False)])
def test_oracle_logits_match_transformers(name, tied):
    import torch
    import transformers
    cfg = E.make_config(name)
    w, hd, (ids, mask) = E.make_weights(cfg, 7), SO.make_head(cfg, 5, tied=tied), E.make_inputs(cfg, 3, 12, 11)
    bert = cfg["model_type"] == "bert"
    C, M = (transformers.BertConfig, transformers.BertForMaskedLM) if bert else (transformers.XLMRobertaConfig, transformers.XLMRobertaForMaskedLM)
    conf = C(**{k: v for k, v in cfg.items() if k != "model_type"}, tie_word_embeddings=tied)
    conf._attn_implementation = "eager"
    model = M(conf)
    sd = {("bert." if bert else "roberta.") + k: torch.from_numpy(v.copy()) for k, v in w.items()}
    sd.update(SO.state_dict(cfg, hd))
    bias = SO.NAMES[cfg["model_type"]][5]
    sd[bias.replace("bias", "decoder.bias")] = sd[bias]  # (the decoder's bias is the head's bias parameter)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k or "token_type_ids" in k or (tied and k.endswith("decoder.weight")) for k in missing), missing
    model.tie_weights()
    model.eval()
    with torch.no_grad():
        got = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).logits.numpy()
    x, _ = E.numpy_forward(cfg, w, ids, mask)
    want = SO.logits(x, w, hd, cfg["layer_norm_eps"])[1]
    assert got.shape == want.shape == (3, 12, cfg["vocab_size"]) and np.abs(got - want)[mask == 1].max() <= 1e-4


def test_pruning_restatement_on_rows_with_ties():
    row = np.array([0.0, 2.0, 1.0, 1.0, -3.0, 1.0, 5.0, np.nan, 1.0], dtype=np.float32)
    assert SO.prune(row, 10) == ([1, 2, 3, 5, 6, 8], [2.0, 1.0, 1.0, 1.0, 5.0, 1.0])  # everything > 0; NaN and <= 0 dropped
    assert SO.prune(row, 3) == ([1, 2, 6], [2.0, 1.0, 5.0])      # the cut falls inside the ties: the lowest id of them
    assert SO.prune(row, 3, unused=(2, 6)) == ([1, 3, 5], [2.0, 1.0, 1.0])  # unused ids never count
    assert SO.prune(np.zeros(4, np.float32), 2) == ([], [])
    z = np.array([[[1.0, -1.0], [3.0, -2.0], [9.0, 9.0]], [[5.0, 5.0]] * 3])
    assert np.array_equal(SO.weights(z, np.array([[1, 1, 0], [0, 0, 0]])), [[np.log1p(3.0), 0.0], [0.0, 0.0]])
