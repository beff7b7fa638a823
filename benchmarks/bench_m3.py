#!/usr/bin/env python3
"""BGE-M3's three outputs from one forward (GpuEncoder.forward_multi*) against the dense-only forward and against what a user
wrote before the heads ran inside the encoder.  Two encoder shapes (multilingual-e5-small: H 384, 12 layers; XLM-R large =
bge-m3: H 1024, 24 layers; random weights, a 32,000-word vocabulary — the table's height does not enter the time), B = 1 / 256,
S = 32 / 512, ragged lengths in [S / 4, S] (seeded), colbert_dim = H, the encoder's default arithmetic (split-precision).

Per cell, in ONE process, the variants alternate round by round (MVDB_BENCH_ROUNDS, default 5; each round runs a variant for
about MVDB_BENCH_WINDOW_S = 0.25 s, at least twice) and every timing is a host clock around calls that end in a stream wait:
  a       forward_device, dense only (the graph-cached forward; up to 64 token slots the one layer-walking launch)
  b       forward_multi_device: dense + token weights + lexical weights + ColBERT vectors, all left on the device
  b_host  forward_multi: the same, trimmed results brought to the host (dicts, per-sentence arrays)
  c_dev   before: forward_device(want_hidden=True) — the padded [B,S,H] hidden states —, then the two heads as torch ops
  c_host  c_dev, then token weights and padded ColBERT rows copied to the host and the per-sentence dedupe in numpy
  b_graph (B = 1, S = 32 only) b captured into a torch.cuda.graph by the caller and replayed: what a graph saves b's plain launches
`bytes_to_host` is computed from the shapes: what each form brings across the bus.  One JSON line per cell, printed and appended
to profiles/m3_bench.jsonl (MVDB_BENCH_OUT moves it).  MVDB_BENCH_MODELS="e5-small,xlmr-large", MVDB_BENCH_B="1,256",
MVDB_BENCH_S="32,512"."""
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

UNUSED = (0, 1, 2, 3)
MODELS = {
    "e5-small": {"model_type": "bert", "hidden_size": 384, "num_hidden_layers": 12, "num_attention_heads": 12,
                 "intermediate_size": 1536, "max_position_embeddings": 512, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
                 "pad_token_id": 0},
    "xlmr-large": {"model_type": "xlm-roberta", "hidden_size": 1024, "num_hidden_layers": 24, "num_attention_heads": 16,
                   "intermediate_size": 4096, "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
                   "pad_token_id": 1},
}


def make_encoder(name):
    cfg = dict(MODELS[name], vocab_size=32000, hidden_act="gelu")
    g = torch.Generator(device="cpu").manual_seed(0)
    H, F = cfg["hidden_size"], cfg["intermediate_size"]
    sd = {}
    for n in weight_names(cfg):
        if n == "embeddings.word_embeddings.weight":
            shape = (cfg["vocab_size"], H)
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
    enc = GpuEncoder(cfg, sd, device=0, pooling="cls" if cfg["model_type"] != "bert" else "mean")
    heads = {"sparse": {"weight": torch.randn((1, H), generator=g) / H ** 0.5, "bias": torch.tensor([0.05])},
             "colbert": {"weight": torch.randn((H, H), generator=g) * (1.5 / H ** 0.5), "bias": torch.randn((H,), generator=g) * 0.1}}
    enc.set_heads(heads["sparse"], heads["colbert"])
    dev = enc.device
    return cfg, enc, {k: {kk: v.to(dev) for kk, v in d.items()} for k, d in heads.items()}


def host_dedupe(ids, mask, tw):
    out = []
    for b in range(ids.shape[0]):
        keep = (mask[b] != 0) & (tw[b] > 0) & ~np.isin(ids[b], UNUSED)
        uniq, inv = np.unique(ids[b][keep], return_inverse=True)
        best = np.zeros(len(uniq), dtype=np.float32)
        np.maximum.at(best, inv, tw[b][keep])
        out.append(dict(zip(uniq.tolist(), best.tolist())))
    return out


def cell(name, cfg, enc, heads, B, S, rounds, window):
    dev = enc.device
    H = cfg["hidden_size"]
    rs = np.random.RandomState(1000 * B + S)
    lens = np.maximum(rs.randint(S // 4, S + 1, size=B), 2)
    mask_h = (np.arange(S)[None, :] < lens[:, None]).astype(np.int32)
    ids_h = np.where(mask_h == 1, rs.randint(4, cfg["vocab_size"], size=(B, S)), cfg["pad_token_id"]).astype(np.int32)
    ids_h[:, 0] = 0
    ids, mask = torch.from_numpy(ids_h).to(dev), torch.from_numpy(mask_h).to(dev)
    sw, sb = heads["sparse"]["weight"].reshape(H), heads["sparse"]["bias"]
    cw, cb = heads["colbert"]["weight"], heads["colbert"]["bias"]
    sync = torch.cuda.current_stream().synchronize

    def before_device():
        dense, hidden = enc.forward_device(ids, mask, want_hidden=True)
        tw = torch.relu(hidden @ sw + sb) * mask
        col = torch.nn.functional.normalize(hidden[:, 1:] @ cw.T + cb, dim=-1) * mask[:, 1:, None]
        return dense, tw, col

    def before_host():
        dense, tw, col = before_device()
        dense, tw, col = dense.cpu().numpy(), tw.cpu().numpy(), col.cpu().numpy()
        return dense, host_dedupe(ids_h, mask_h, tw), [col[b, :lens[b] - 1] for b in range(B)]

    variants = {"a": lambda: enc.forward_device(ids, mask), "b": lambda: enc.forward_multi_device(ids, mask),
                "b_host": lambda: enc.forward_multi(ids_h, mask_h), "c_dev": before_device, "c_host": before_host}
    for f in variants.values():  # every shape warm: workspace, weight images, graphs, torch's own kernels
        f()
        f()
    sync()
    if B == 1 and S == 32:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=torch.cuda.current_stream(), capture_error_mode="thread_local"):
            held = enc.forward_multi_device(ids, mask)  # noqa: F841  (the graph's outputs)
        variants["b_graph"] = graph.replay
        graph.replay()
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
    valid_rows = int((lens - 1).sum())
    small = B * H * 4
    lex = B * S * 4
    rec = {"model": name, "B": B, "S": S, "tokens": int(lens.sum()), "H": H, "colbert_dim": H, "compute": enc.default_compute,
           "dense_walks": enc.walks(B, S), "rounds": rounds, "reps": reps,
           "ms_median": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "ms_min": {k: round(min(v), 4) for k, v in times.items()},
           "bytes_to_host": {"a": small, "b_host": small + 3 * lex + 8 * B + 4 * B + valid_rows * H * 4,
                             "c_host": small + lex + B * (S - 1) * H * 4},
           "device_bytes_written_for_outputs": {"b": small + 3 * lex + 8 * B + B * (S - 1) * H * 4,
                                                "c_dev": small + B * S * H * 4 + lex + B * (S - 1) * H * 4}}
    m = rec["ms_median"]
    rec["b_minus_a_ms"] = round(m["b"] - m["a"], 4)
    rec["b_over_c_dev"] = round(m["b"] / m["c_dev"], 4)
    rec["b_host_over_c_host"] = round(m["b_host"] / m["c_host"], 4)
    return rec


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a real stream: the encoder replays hipGraphs on it
    rounds = int(os.environ.get("MVDB_BENCH_ROUNDS", "5"))
    window = float(os.environ.get("MVDB_BENCH_WINDOW_S", "0.25"))
    out = os.environ.get("MVDB_BENCH_OUT", os.path.join(ROOT, "profiles", "m3_bench.jsonl"))
    for name in os.environ.get("MVDB_BENCH_MODELS", "e5-small,xlmr-large").split(","):
        cfg, enc, heads = make_encoder(name)
        for B in [int(v) for v in os.environ.get("MVDB_BENCH_B", "1,256").split(",")]:
            for S in [int(v) for v in os.environ.get("MVDB_BENCH_S", "32,512").split(",")]:
                rec = cell(name, cfg, enc, heads, B, S, rounds, window)
                line = json.dumps(rec)
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
        enc.close()


if __name__ == "__main__":
    main()
