"""Token ids -> forward_splade -> set_sparse_vector -> find_most_similar_sparse, against the numpy ranking of the same dicts."""
import numpy as np
import pytest

import sparse_oracle
import splade_oracle as SO
from oracle import encoder as E

pytestmark = pytest.mark.gpu


def test_sparse_search_ranks_splade_vectors_as_numpy_does(gpu, tmp_path):
    import torch
    from minivectordb_amd import VectorDatabase
    from minivectordb_amd.embedding_model import GpuEncoder
    cfg = E.make_config("xlmr-tiny")
    w, (ids, mask) = E.make_weights(cfg, 7), E.make_inputs(cfg, 40, 16, 31)
    enc = GpuEncoder(cfg, {k: torch.from_numpy(v) for k, v in w.items()}, device=0)
    enc.set_mlm_head(SO.state_dict(cfg, SO.make_head(cfg, 5)), unused_token_ids=(0, 1, 2, 3))
    dense = enc.forward(ids, mask)
    docs = enc.forward_splade(ids[:36], mask[:36], max_terms=24)
    queries = enc.forward_splade(ids[36:], mask[36:], max_terms=8)
    enc.close()
    assert all(len(d) == 24 and list(d) == sorted(d) for d in docs) and all(len(q) == 8 for q in queries)
    db = VectorDatabase(storage_file=str(tmp_path / "splade.pkl"))
    for i, d in enumerate(docs):
        db.store_embedding(i, dense[i], {"doc": i})
        db.set_sparse_vector(i, d)
    indptr, indices = np.cumsum([0] + [len(d) for d in docs]), [k for d in docs for k in d]
    values = np.asarray([v for d in docs for v in d.values()], dtype=np.float32)
    for q in queries:
        T, matched = sparse_oracle.scores(indptr, indices, values, list(q), np.asarray(list(q.values()), dtype=np.float32))
        D, I = sparse_oracle.sparse_topk(T, matched, np.arange(len(docs)), 5)
        got_ids, got_scores, _ = db.find_most_similar_sparse(q, k=5)
        assert list(got_ids) == I[I >= 0].tolist()
        assert np.asarray(got_scores, dtype=np.float32).tobytes() == D[I >= 0].tobytes()
