"""float64 restatement of SPLADE's head and of its pruning (helpers only; TEST INFRASTRUCTURE).
    t = LayerNorm(gelu(x W_t^T + b_t));  z[p, v] = t[p] . E[v] + b_v;  w[b, v] = max over b's valid tokens of log(1 + relu(z))
pruning: the max_terms largest weights > 0 whose id is not unused, equal weights to the lower id, by ascending id."""
import numpy as np
from scipy.special import erf

KEYS = ("tw", "tb", "g", "b", "dec_w", "dec_b")
NAMES = {"bert": ("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
                  "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias",
                  "cls.predictions.decoder.weight", "cls.predictions.bias"),
         "xlm-roberta": ("lm_head.dense.weight", "lm_head.dense.bias", "lm_head.layer_norm.weight", "lm_head.layer_norm.bias",
                         "lm_head.decoder.weight", "lm_head.bias")}


def make_head(cfg, seed, tied=True):
    """Seeded MLM head (float32): tw, tb, g, b, dec_b, and dec_w when the decoder is not tied to the word embeddings."""
    rs = np.random.RandomState(seed)
    H, V = cfg["hidden_size"], cfg["vocab_size"]
    hd = {"tw": rs.standard_normal((H, H)) * (1.5 / np.sqrt(H)), "tb": 0.1 * rs.standard_normal(H),
          "g": 1.0 + 0.2 * rs.standard_normal(H), "b": 0.1 * rs.standard_normal(H), "dec_b": 0.3 * rs.standard_normal(V)}
    if not tied:
        hd["dec_w"] = rs.standard_normal((V, H)) * 0.5
    return {k: v.astype(np.float32) for k, v in hd.items()}


def state_dict(cfg, hd):
    """The head under transformers' own names (a tied decoder weight is left out)."""
    import torch
    return {n: torch.from_numpy(hd[k].copy()) for n, k in zip(NAMES[cfg["model_type"]], KEYS) if k in hd}


def decoder(weights, hd):  # [V, H]: its own, or tied to the word embeddings
    return (hd["dec_w"] if "dec_w" in hd else weights["embeddings.word_embeddings.weight"]).astype(np.float64)


def _normalised(x, hd, eps):
    h = x.astype(np.float64) @ hd["tw"].astype(np.float64).T + hd["tb"].astype(np.float64)
    h = 0.5 * h * (1.0 + erf(h / np.sqrt(2.0)))
    mu = h.mean(-1, keepdims=True)
    sigma = np.sqrt(((h - mu) ** 2).mean(-1, keepdims=True) + eps)
    return (h - mu) / sigma, sigma


def logits(x, weights, hd, eps):  # [..., H] hidden states -> (t [..., H], z [..., V])
    t = _normalised(x, hd, eps)[0] * hd["g"].astype(np.float64) + hd["b"].astype(np.float64)
    return t, t @ decoder(weights, hd).T + hd["dec_b"].astype(np.float64)


def weights(z, mask):
    """[B, S, V] logits -> [B, V]; padding never wins, a sentence without tokens has no weight."""
    return np.where(mask[..., None] == 1, np.log1p(np.maximum(z, 0.0)), 0.0).max(axis=1)


def logit_bound(t, E, hd, eps_t):
    """|dz| <= sum_i eps_t[i] |E_vi| + (2^-21 + gamma_H) sum_i |t_i E_vi| + 8 ulps of (sum_i |t_i E_vi| + |b_v| + 1) for the scale,
    the bias add and log1pf: [..., V].  eps_t: a scalar, or the per-element bound of t (t's shape)."""
    u, H = 2.0 ** -24, t.shape[-1]
    mag = np.abs(t) @ np.abs(E).T
    return (np.broadcast_to(eps_t, t.shape) @ np.abs(E).T + (2.0 ** -21 + H * u / (1.0 - H * u)) * mag
            + 8 * u * (mag + np.abs(hd["dec_b"].astype(np.float64)) + 1.0))


def transform_bound(x, hd, eps, eps_x):
    """Bound of t when x moves by at most eps_x per element: gelu' <= 1.13, so |dh_j| <= 1.13 eps_x |W_t[j]|_1; LayerNorm's Jacobian is
    (g_i / sigma)(delta_ij - 1 / H - n_i n_j / H), n the normalised row (mean |n| <= 1): |dt_i| <= (|g_i| / sigma)(2 + |n_i|) |dh|_inf; 1 % more."""
    n, sigma = _normalised(x, hd, eps)
    dh = 1.13 * eps_x * np.abs(hd["tw"].astype(np.float64)).sum(axis=1).max()
    return 1.01 * np.abs(hd["g"].astype(np.float64)) / sigma * (2.0 + np.abs(n)) * dh


def prune(row, max_terms, unused=()):
    ok = np.asarray(row) > 0  # one sentence's [V] weights -> (ids ascending, values); NaN fails > 0
    ok[[u for u in unused if 0 <= u < len(row)]] = False
    ids = sorted(sorted(np.flatnonzero(ok).tolist(), key=lambda i: (-float(row[i]), i))[:max_terms])
    return ids, [row[i] for i in ids]
