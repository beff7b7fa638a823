"""BGE-M3's two extra heads in float64 numpy, and the per-sentence dedupe in plain Python.  TEST INFRASTRUCTURE ONLY.

The arbiter of include/mvdb.h's "BGE-M3's heads" contract (the model's own inference path: a Linear(H, 1) + ReLU per token, the
maximum per token id with the special tokens left out; a Linear(H, C) per token behind the CLS slot, L2-normalised).
x: last hidden states [B,S,H]; mask: prefix masks [B,S]; ids [B,S].
"""
import numpy as np

UNUSED = (0, 1, 2, 3)  # BGE-M3: cls, pad, eos, unk


def make_heads(H, C, seed):
    """The seeded head weights every test uses (float32): sparse_w ~ N(0, 1/sqrt(H)), sparse_b = 0.05,
    colbert_w ~ N(0, 1.5/sqrt(H)), colbert_b ~ 0.1 N(0, 1)."""
    rs = np.random.RandomState(seed)
    return {"sparse_w": (rs.standard_normal(H) / np.sqrt(H)).astype(np.float32),
            "sparse_b": np.float32(0.05),
            "colbert_w": (rs.standard_normal((C, H)) * (1.5 / np.sqrt(H))).astype(np.float32),
            "colbert_b": (0.1 * rs.standard_normal(C)).astype(np.float32)}


def state_dicts(heads):
    """(sparse_linear, colbert_linear) as the state dicts GpuEncoder.set_heads takes."""
    import torch
    sparse = {"weight": torch.from_numpy(np.asarray(heads["sparse_w"], dtype=np.float32).reshape(1, -1).copy()),
              "bias": torch.from_numpy(np.asarray([heads["sparse_b"]], dtype=np.float32))}
    colbert = {"weight": torch.from_numpy(heads["colbert_w"].copy()), "bias": torch.from_numpy(heads["colbert_b"].copy())}
    return sparse, colbert


def edge_batch(vocab, seed=5):
    """ids, mask [3,19] with lengths 19, 1, 7: every sentence starts with id 0 (CLS) and ends with id 2 (EOS) where its length
    allows; ids 2 and 3 planted mid-sentence; id 9 three times in sentence 0 with different neighbours."""
    rs = np.random.RandomState(seed)
    S, lens = 19, (19, 1, 7)
    ids = rs.randint(4, vocab, size=(3, S)).astype(np.int32)
    mask = (np.arange(S)[None, :] < np.asarray(lens)[:, None]).astype(np.int32)
    ids[:, 0] = 0
    for b, n in enumerate(lens):
        if n >= 2:
            ids[b, n - 1] = 2
    ids[0, 5], ids[0, 11] = 2, 3
    ids[0, 3] = ids[0, 8] = ids[0, 14] = 9
    ids[2, 2], ids[2, 4] = 3, ids[2, 1]  # an unused id and one repeat in the short sentence
    ids = np.where(mask == 1, ids, 1).astype(np.int32)
    return ids, mask


def token_weights(x, mask, sparse_w, sparse_b):
    """tw[b,t] = max(0, sparse_w . x[b,t] + sparse_b) for valid slots (NaN stays NaN), 0 for masked ones; float64 [B,S]."""
    x = np.asarray(x, dtype=np.float64)
    pre = x @ np.asarray(sparse_w, dtype=np.float64) + np.float64(sparse_b)
    with np.errstate(invalid="ignore"):
        tw = np.where(np.isnan(pre), pre, np.maximum(pre, 0.0))
    return np.where(np.asarray(mask) != 0, tw, 0.0)


def token_weight_bound(x, mask, sparse_w, sparse_b, H):
    """gamma_{H+2} (sum_i |x_i w_i| + |b|) per slot: the any-order fp32 bound of an H-term dot product plus the bias."""
    u = (H + 2) * 2.0 ** -24
    gamma = u / (1.0 - u)
    mag = np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(sparse_w, dtype=np.float64)) + abs(float(sparse_b))
    return np.where(np.asarray(mask) != 0, gamma * mag, 0.0)


def dedupe(ids, mask, tw, unused=UNUSED):
    """Per sentence: ([token ids ascending], [the largest weight of each]) over the valid slots whose id is not unused and whose
    weight is > 0 (a NaN fails the test, +inf passes).  Plain Python on the values given — bit for bit when tw is float32."""
    out = []
    for b in range(len(ids)):
        best = {}
        for t in range(len(ids[b])):
            if not mask[b][t]:
                continue
            i, w = int(ids[b][t]), tw[b][t]
            if i in unused or i < 0 or not (w > 0):
                continue
            if i not in best or w > best[i]:
                best[i] = w
        keys = sorted(best)
        out.append((keys, [best[k] for k in keys]))
    return out


def lexical_weights(ids, mask, x, sparse_w, sparse_b, unused=UNUSED):
    """[{token id: weight}] per sentence, from the hidden states."""
    tw = token_weights(x, mask, sparse_w, sparse_b)
    return [dict(zip(k, (float(v) for v in vals))) for k, vals in dedupe(ids, mask, tw, unused)]


def colbert_pre(x, colbert_w, colbert_b):
    """u[b,t,:] = colbert_w x[b,t] + colbert_b for every slot; float64 [B,S,C]."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(colbert_w, dtype=np.float64).T + np.asarray(colbert_b, dtype=np.float64)


def colbert_vecs(x, mask, colbert_w, colbert_b):
    """Per sentence the [max(len - 1, 0), C] rows u / max(|u|, 1e-12) of the slots 1 .. len - 1 (CLS dropped, EOS kept)."""
    u = colbert_pre(x, colbert_w, colbert_b)
    v = u / np.maximum(np.linalg.norm(u, axis=-1, keepdims=True), 1e-12)
    lens = np.asarray(mask).sum(axis=1)
    return [v[b, 1:max(int(lens[b]), 1)] for b in range(len(lens))]
