"""The round trip the heads exist for: one multi-output forward per document feeds the dense store, the sparse vectors and a
ColBERT row store; the document's own outputs, used as the question, find it again through the hybrid and the MaxSim search."""
import numpy as np
import pytest

import m3_oracle as M
import sparse_oracle
from oracle import encoder as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def documents(gpu):
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    cfg = E.make_config("xlmr-tiny")  # d = 128
    w = E.make_weights(cfg, 7)
    rs = np.random.RandomState(31)
    lens = [9, 12, 7, 11, 14, 10]
    S = max(lens)
    ids = np.full((6, S), cfg["pad_token_id"], dtype=np.int32)
    for b, n in enumerate(lens):
        ids[b, :n] = rs.randint(4, cfg["vocab_size"], size=n)
        ids[b, 0], ids[b, n - 1] = 0, 2
        ids[b, 3] = ids[b, 5]  # a repeated token in every document
    mask = (np.arange(S)[None, :] < np.asarray(lens)[:, None]).astype(np.int32)
    enc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0, pooling="cls")
    enc.set_heads(*M.state_dicts(M.make_heads(cfg["hidden_size"], cfg["hidden_size"], 164)))
    out = enc.forward_multi(ids, mask)
    enc.close()
    assert all(len(d) >= 2 for d in out["lexical_weights"])
    return lens, out


def test_hybrid_search_finds_the_document_by_its_own_outputs(documents, tmp_path):
    from minivectordb_amd import VectorDatabase
    lens, out = documents
    db = VectorDatabase(storage_file=str(tmp_path / "dense.pkl"))
    for i in range(6):
        db.store_embedding(i, out["dense"][i], {"doc": i})
        db.set_sparse_vector(i, out["lexical_weights"][i])
    ids, scores, _ = db.find_most_similar_hybrid(out["dense"][3], out["lexical_weights"][3], k=3)
    assert ids[0] == 3
    # the sparse part: the float32 chain ((0 + w1 w1) + w2 w2) + ... over the document's ids in ascending order
    lex = out["lexical_weights"][3]
    keys = sorted(lex)
    vals = np.asarray([lex[k] for k in keys], dtype=np.float32)
    T, matched = sparse_oracle.scores([0, len(keys)], keys, vals, keys, vals)
    assert matched[0] == len(keys)
    sids, sscores, _ = db.find_most_similar_sparse(lex, k=3)
    assert sids[0] == 3 and np.float32(sscores[0]).tobytes() == T[0].tobytes()
    # S = cosine (1 for the document itself, unit-norm vectors: 2e-5) + the sparse part, one fp32 rounding of the sum
    assert abs(float(scores[0]) - (1.0 + float(T[0]))) <= 2e-5 + 2.0 ** -23 * (1.0 + float(T[0]))


def test_maxsim_search_finds_the_document_by_its_own_colbert_vectors(documents, tmp_path):
    from minivectordb_amd import VectorDatabase
    lens, out = documents
    db = VectorDatabase(storage_file=str(tmp_path / "colbert.pkl"))
    uid = 0
    for i, vecs in enumerate(out["colbert_vecs"]):
        assert vecs.shape == (lens[i] - 1, 128)
        np.testing.assert_allclose(np.linalg.norm(vecs, axis=1), 1.0, rtol=0, atol=2e-5)
        for v in vecs:
            db.store_embedding(uid, v, {"doc": i})
            uid += 1
    question = out["colbert_vecs"][3]
    T = question.shape[0]
    ids, scores, metas = db.find_most_similar_maxsim(question, group_by="doc", k=3)
    assert metas[0][0]["doc"] == 3 and all(m["doc"] == 3 for m in metas[0])
    assert abs(float(scores[0]) - T) <= T * 2e-5
    assert float(scores[1]) < float(scores[0])
