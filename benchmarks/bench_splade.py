#!/usr/bin/env python3
"""SPLADE vectors from one call (GpuEncoder.forward_splade_device) against the dense-only forward and against what a user
wrote before the head ran inside the encoder.  Two shapes: BERT-base dimensions (H 768, 12 layers, V = 30,522) and the
multilingual-e5-small shape with the XLM-R vocabulary (H 384, 12 layers, V = 250,002); random weights, a tied decoder.  Batches
of 1 x 32, 256 x 32 and 256 x 512 token slots, ragged lengths in [S / 4, S] (seeded), max_terms = 256, the encoder's default
arithmetic (split-precision).

Per cell, in ONE process, the variants alternate round by round (MVDB_BENCH_ROUNDS, default 5; each round runs a variant for
about MVDB_BENCH_WINDOW_S = 0.25 s, at least twice) and every timing is a host clock around calls that end in a stream wait:
  a      forward_device, dense only (the graph-cached forward; up to 64 token slots the one layer-walking launch)
  b      forward_splade_device: dense + count / indices / values, all left on the device
  c_dev  before: forward_device(want_hidden=True) — the padded [B,S,H] hidden states —, then the head in torch (fp32): transform,
         the [tokens, V] logits in chunks of sentences that keep them under 1 GiB, log1p(relu), masked max, top-k
One JSON line per cell, printed and appended to profiles/splade_bench.jsonl (MVDB_BENCH_OUT moves it).
MVDB_BENCH_MODELS="bert-base,e5-small-xlmr", MVDB_BENCH_CELLS="1x32,256x32,256x512"."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivectordb_amd.embedding_model import GpuEncoder  # noqa: E402
from oracle.encoder import weight_names  # noqa: E402

MAX_TERMS = 256
MODELS = {
    "bert-base": {"model_type": "bert", "vocab_size": 30522, "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12,
                  "intermediate_size": 3072, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
                  "pad_token_id": 0},
    "e5-small-xlmr": {"model_type": "bert", "vocab_size": 250002, "hidden_size": 384, "num_hidden_layers": 12, "num_attention_heads": 12,
                      "intermediate_size": 1536, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
                      "pad_token_id": 0},
}


def make_encoder(name):
    cfg = dict(MODELS[name], hidden_act="gelu")
    g = torch.Generator(device="cpu").manual_seed(0)
    H, F, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    sd = {}
    for n in weight_names(cfg):
        if n == "embeddings.word_embeddings.weight":
            shape = (V, H)
        elif n == "embeddings.position_embeddings.weight":
            shape = (cfg["max_position_embeddings"], H)
        elif n == "embeddings.token_type_embeddings.weight":
            shape = (cfg["type_vocab_size"], H)
        elif n.endswith("intermediate.dense.weight"):
            shape = (F, H)
        elif n.endswith("intermediate.dense.bias"):
            shape = (F,)
        elif n.endswith("output.dense.weight") and "attention" not in n:
            shape = (H, F)
        elif n.endswith(".weight") and "LayerNorm" not in n:
            shape = (H, H)
        else:
            shape = (H,)
        t = torch.randn(shape, generator=g) * 0.05
        sd[n] = t + 1.0 if "LayerNorm.weight" in n else t
    enc = GpuEncoder(cfg, sd, device=0)
    # a decoder bias of -1.5 leaves a few per cent of the vocabulary positive per sentence, as a trained SPLADE model does
    head = {"cls.predictions.transform.dense.weight": torch.randn((H, H), generator=g) * (1.5 / H ** 0.5),
            "cls.predictions.transform.dense.bias": torch.randn((H,), generator=g) * 0.1,
            "cls.predictions.transform.LayerNorm.weight": torch.ones(H), "cls.predictions.transform.LayerNorm.bias": torch.zeros(H),
            "cls.predictions.bias": torch.full((V,), -1.5)}
    enc.set_mlm_head(head)
    dev = enc.device
    return cfg, enc, {k: v.to(dev) for k, v in head.items()}, sd["embeddings.word_embeddings.weight"].to(dev)


def cell(name, cfg, enc, head, E, B, S, rounds, window):
    dev = enc.device
    H, V = cfg["hidden_size"], cfg["vocab_size"]
    rs = np.random.RandomState(1000 * B + S)
    lens = np.maximum(rs.randint(S // 4, S + 1, size=B), 2)
    mask_h = (np.arange(S)[None, :] < lens[:, None]).astype(np.int32)
    ids_h = np.where(mask_h == 1, rs.randint(4, V, size=(B, S)), cfg["pad_token_id"]).astype(np.int32)
    ids, mask = torch.from_numpy(ids_h).to(dev), torch.from_numpy(mask_h).to(dev)
    sync = torch.cuda.current_stream().synchronize
    tw, tb = head["cls.predictions.transform.dense.weight"], head["cls.predictions.transform.dense.bias"]
    g, b, db = head["cls.predictions.transform.LayerNorm.weight"], head["cls.predictions.transform.LayerNorm.bias"], head["cls.predictions.bias"]
    per = max(1, (1 << 28) // (S * V))  # sentences per chunk: [per, S, V] fp32 logits under 1 GiB

    def before_device():
        dense, hidden = enc.forward_device(ids, mask, want_hidden=True)
        t = torch.nn.functional.layer_norm(torch.nn.functional.gelu(hidden @ tw.T + tb), (H,), g, b, cfg["layer_norm_eps"])
        rows = []
        for b0 in range(0, B, per):
            z = torch.log1p(torch.relu(t[b0:b0 + per] @ E.T + db)) * mask[b0:b0 + per, :, None]
            rows.append(z.max(dim=1).values)
        val, idx = torch.topk(torch.cat(rows), MAX_TERMS, dim=1)
        return dense, val, idx

    variants = {"a": lambda: enc.forward_device(ids, mask), "b": lambda: enc.forward_splade_device(ids, mask, max_terms=MAX_TERMS),
                "c_dev": before_device}
    for f in variants.values():  # every shape warm: workspace, weight images, graphs, torch's own kernels
        f()
        f()
    sync()
    reps = {}
    for k, f in variants.items():
        t0 = time.perf_counter()
        f()
        sync()
        reps[k] = max(2, int(window / max(time.perf_counter() - t0, 1e-6)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            t0 = time.perf_counter()
            for _ in range(reps[k]):
                f()
            sync()
            times[k].append((time.perf_counter() - t0) / reps[k] * 1e3)
    rec = {"model": name, "B": B, "S": S, "tokens": int(lens.sum()), "H": H, "V": V, "max_terms": MAX_TERMS, "compute": enc.default_compute,
           "dense_walks": enc.walks(B, S), "rounds": rounds, "reps": reps,
           "ms_median": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "ms_min": {k: round(min(v), 4) for k, v in times.items()},
           "logit_bytes_never_written": int(lens.sum()) * V * 4}
    m = rec["ms_median"]
    rec["b_minus_a_ms"] = round(m["b"] - m["a"], 4)
    rec["b_over_c_dev"] = round(m["b"] / m["c_dev"], 4)
    rec["head_tflops_fp32_equivalent"] = round(2.0 * int(lens.sum()) * V * H / max(m["b"] - m["a"], 1e-6) / 1e9, 2)
    return rec


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a real stream: the encoder replays hipGraphs on it
    rounds = int(os.environ.get("MVDB_BENCH_ROUNDS", "5"))
    window = float(os.environ.get("MVDB_BENCH_WINDOW_S", "0.25"))
    out = os.environ.get("MVDB_BENCH_OUT", os.path.join(ROOT, "profiles", "splade_bench.jsonl"))
    for name in os.environ.get("MVDB_BENCH_MODELS", "bert-base,e5-small-xlmr").split(","):
        cfg, enc, head, E = make_encoder(name)
        for c in os.environ.get("MVDB_BENCH_CELLS", "1x32,256x32,256x512").split(","):
            B, S = (int(v) for v in c.split("x"))
            rec = cell(name, cfg, enc, head, E, B, S, rounds, window)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")
        enc.close()


if __name__ == "__main__":
    main()
