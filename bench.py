#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X flat-search hot path.

metric (BASELINE.json): queries/sec + p50 latency, brute-force IP kNN, 10M x 512 fp32, k = 10.

A "step" is ONE query (nq = 1, the reference API: minivectordb/vector_database.py:473-497) = one
pass of the scan over this rank's resident corpus shard, followed — when N > 1 — by the RCCL
all-gather of the per-shard top-k and the k-way merge.  Weak scaling: every rank holds its own
`--rows` x `--dim` shard (10M x 512 = 20.48 GB), generated on the device, so the searched corpus is
N x 10M rows (BASELINE config 4 at N = 8: 80M x 512).  `value` is the user-visible rate: queries
per second answered over the WHOLE N x rows corpus (every query is scanned by all ranks jointly, so
it does not grow with N — the corpus does); `corpus_rows_per_s` and `roofline.achieved` carry the
aggregate scan rate (rows/s and GB/s summed over ranks, against N x the HBM peak), with the
per-rank kernel times beside them.

Inputs are resident in HBM when the timed region starts (corpus and all W+K queries are generated
on the device beforehand, from fixed seeds: the same arguments give the same inputs); results stay on the device.
--dump-outputs DIR writes the (D, I) of the last timed step as DIR/D.npy and DIR/I.npy.

A plain run sets up, warms up, times the K steps and prints the line (headline, p50 latency, the roofline of the timed
launches).  --full adds everything else, all measured OUTSIDE the headline's timed region: at N = 1 the PCIe-inclusive
host API rate (`host_api_qps`, never `value`), the opt-in fp16-shadow single-query rate, the package power under the
step, the CPU oracle's rate over the whole corpus (`cpu_baseline`; --no-cpu-baseline skips it) and three more blocks
(BASELINE config 5; --no-encoder skips them):
  "certified_passes_on_unfriendly_data": the batch passes (and the opt-in single-query shadow route) on an all-positive and on a
             clustered 10M x 512 corpus, where certification can fail — with the re-run rate;
  "encoder": the e5-small-shaped encoder forward (256 sentences, S = 32 and 512) in the drop-in's default arithmetic
             (split-precision fp16 x 3 on the 16-bit matrix cores) and in the exact fp32-MFMA mode, each with its MFMA
             roofline, next to `cpu_baseline` = transformers' own BertModel (what the reference runs,
             minivectordb/embedding_model.py:62-71) + average_pool + F.normalize on this box's host cores; the
             one-sentence-per-call latencies; "large": the bge-m3 / e5-large shape;
  "config5": encoder forward -> 256 queries -> kNN over a resident 10M x 384 corpus, end to end on the device.

Launch: python bench.py [--gpus 1] [--full]       or, for N > 1 (one rank per GPU):
        python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
               --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL) — before any HIP init
os.environ.setdefault("NCCL_DEBUG", "WARN")  # RCCL's own warnings reach the log of a failed multi-GPU bring-up


def _rccl_version():
    try:
        import torch
        return ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:  # noqa: BLE001
        return None

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)


def baseline_metric():
    """The metric string exactly as BASELINE.json spells it."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except Exception:
        return "queries/sec + p50 latency, brute-force IP kNN, 10M\u00d7512 fp32, k=10"


def pmc_traffic(n, d, nq=1, scan_name=None, launched=""):
    """HBM bytes per scan launch from the committed rocprofv3 PMC passes (profiles/*_pmc_summary.json,
    separate --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, FETCH_SIZE doubled per the
    guide's gfx950 correction).  Counters cannot be collected from inside the timed process, so this
    is the figure of the profiled run of the same workload — accepted only when the profile's kernel is the very
    instantiation this run launched (`launched`, from mvdb_prof_symbol: template arguments included); the newest such
    profile wins and is named, with the commit it was taken at, in `source`.  None when no profile matches."""
    import glob
    squeeze = lambda t: t.replace(" ", "")  # noqa: E731
    if not launched:
        return {"bytes": None, "source": "refused: the library did not report the launched kernel"}
    best, refused = None, None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")))
    files.sort(key=lambda f: f"nq{nq}_" in os.path.basename(f))  # the pass profiled at this nq wins
    batch = "h16" in launched
    elem = 2.0 if launched.startswith("flat_scan_h16_kernel") else 4.0  # the h16 pass streams the fp16 shadow of the rows
    for f in files:
        try:
            recs = json.load(open(f))
        except Exception:
            continue
        for rec in recs:
            if not isinstance(rec, dict) or "kernel" not in rec or rec.get("launches_fetch_pass", 0) <= 0:
                continue
            if launched.split("<")[0] not in rec["kernel"]:
                continue
            t = rec["hbm_traffic_bytes_per_launch_avg"]
            # a corpus pass of the split-precision kernels is up to four main launches (phases): the profile
            # holds the average over those launches, like `algorithmic_bytes_per_launch`
            if not any(abs(t * per_pass / (n * d * elem) - 1.0) < 0.25 for per_pass in ((1, 2, 3, 4) if batch else (1,))):
                continue   # another workload size
            if squeeze(launched) not in squeeze(rec["kernel"]):
                refused = f"refused: {os.path.basename(f)} profiled {rec['kernel']}, this run launched {launched}"
                continue
            best = {"bytes": int(t), "source": {"file": os.path.basename(f), "kernel": rec["kernel"],
                                                "git_head": rec.get("git_head")}}
    return best or {"bytes": None, "source": refused or f"no committed PMC profile of {launched} at this size"}


def cpu_baseline(native, idx, d, k, queries_host, full_rows, budget_s=24.0):
    """Time the CPU oracle (oracle/flat_oracle.c, a port of faiss' nq = 1 sequential scan) on the WHOLE resident corpus:
    every row is fetched to the host in 1M-row blocks (10M x 512 = 20.5 GB of host memory, placed next to the threads that
    scan it) and a bounded number of queries is timed over all of it — one thread (what faiss uses at nq = 1), then the same
    port with the rows partitioned over OpenMP threads at a few thread counts, keeping the best.  Nothing is extrapolated."""
    import numpy as np
    from oracle import flat
    avail = max(1, min(flat.max_threads(), len(os.sched_getaffinity(0))))
    n = int(full_rows)
    # a host with less free memory than 1.3 x the corpus times a bounded sample instead (the first rows that fit in half of
    # what is free) and scales the rate by rows / sample — labelled as such; the GPU box's hosts hold the whole 20.5 GB
    scaled = 1.0
    try:
        with open("/proc/meminfo") as f:
            free = next(int(l.split()[1]) * 1024 for l in f if l.startswith("MemAvailable:"))
        if free < 1.3 * n * d * 4:
            n = max(1, min(n, int(free * 0.5 / (d * 4))))
            scaled = n / float(full_rows)
    except (OSError, StopIteration, ValueError):
        pass
    t0 = time.perf_counter()
    x = np.empty((n, d), dtype=np.float32)   # untouched pages
    block = 1_000_000
    buf = np.empty((min(block, n), d), dtype=np.float32)
    for b in range(0, n, block):
        m = min(block, n - b)
        idx.get_rows(b, m, out=buf[:m])
        flat.first_touch_copy_block(x, buf[:m], avail, b)
    del buf
    fetch_s = time.perf_counter() - t0
    flat.flat_search(x, queries_host[0], k, nthreads=avail)  # warm (page tables, thread pool)
    nq = 0
    t0 = time.perf_counter()
    while True:
        flat.flat_search(x, queries_host[nq % len(queries_host)], k, nthreads=1)
        nq += 1
        if time.perf_counter() - t0 > budget_s / 3 or nq >= 64:
            break
    t1 = time.perf_counter() - t0
    # past the host's memory bandwidth more threads only add contention: a few counts, keep the best
    best, tried = (0.0, 1), {}
    for cores in sorted({min(avail, c) for c in (8, 16, 32, 64, 96, avail)}):
        flat.flat_search(x, queries_host[0], k, nthreads=cores)  # warm
        nq_mt = 0
        t0 = time.perf_counter()
        while True:
            flat.flat_search(x, queries_host[nq_mt % len(queries_host)], k, nthreads=cores)
            nq_mt += 1
            if time.perf_counter() - t0 > budget_s / 9 or nq_mt >= 64:
                break
        rate = nq_mt / (time.perf_counter() - t0)
        tried[str(cores)] = round(rate, 3)
        if rate > best[0]:
            best = (rate, cores)
    del x
    return {
        "value": round(nq / t1 * scaled, 4),
        "unit": "queries/s",
        "cores": 1,
        "kind": "port",
        "sample": (f"{n} of {full_rows} rows x {d} fp32 (" + ("the whole corpus" if scaled == 1.0 else "the host's free memory holds no more")
                   + f", fetched from the device in {fetch_s:.1f} s), {nq} queries, 1 thread (faiss uses one thread at nq=1); "
                   + ("nothing scaled" if scaled == 1.0 else f"rates scaled by {scaled:.4f} = sample / corpus rows")),
        "multithread_value": round(best[0] * scaled, 4),
        "multithread_cores": best[1],
        "multithread_tried_qps": tried,
        "host_cores_available": avail,
        "gb_per_s_1thread": round(n * d * 4 * nq / t1 / 1e9, 2),
        "gb_per_s_multithread": round(n * d * 4 * best[0] / 1e9, 2),
    }


MFMA_PEAK_TF = {"fp16x3": 2500.0, "fp32": 157.3}   # dense peaks, /opt/skills/guides/MI355X_MICROARCH.md
E5_SMALL = {"model_type": "bert", "vocab_size": 250037, "hidden_size": 384, "num_hidden_layers": 12,
            "num_attention_heads": 12, "intermediate_size": 1536, "max_position_embeddings": 512, "type_vocab_size": 2,
            "layer_norm_eps": 1e-12, "hidden_act": "gelu", "pad_token_id": 0}


def _hwmon_of(dev_index):
    """The hwmon directory of HIP device `dev_index` (matched by PCI address), or None."""
    import glob
    cards = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
    if not cards:
        return None
    want = None
    try:
        import torch
        pr = torch.cuda.get_device_properties(dev_index)
        want = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
    except Exception:  # noqa: BLE001
        pass
    for h in cards:
        addr = os.path.basename(os.path.realpath(os.path.join(h, "..", "..")))
        if want and addr.lower() == want:
            return h
    return cards[0] if len(cards) == 1 else None


def _read_int(path):
    try:
        with open(path) as f:
            return int(f.read().strip())
    except Exception:  # noqa: BLE001
        return None


def power_probe(step, what, sync, seconds=1.5, dev_index=0):
    """Package power and shader clock under a sustained load (informational; round 4: the fp16x3 encoder forward at 256 x 512
    tokens and the 128- / 256-query scan passes run AT the 1400 W package cap with the shader clock pulled to 1.4 - 2.0 GHz —
    the bound neither the HBM nor the MFMA roofline shows).  `step` is enqueued back to back; after `seconds` of load the
    device's hwmon files (power1_input = PPT in microwatts, freq1_input = sclk in Hz, power1_cap) are read four times 0.15 s
    apart while the load keeps running — no child process.  Where the hwmon directory cannot be matched to the device (and
    no profiler is preloaded: a child process of a GPU process must not exec under one) `rocm-smi` is sampled once."""
    import re
    import shutil
    import subprocess
    hw = _hwmon_of(dev_index)
    profiled = any("rocprof" in v.lower() for k, v in os.environ.items() if k == "LD_PRELOAD" or k.startswith("ROCP"))
    smi = None if hw or profiled else (shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi")
    if not hw and not (smi and os.path.exists(smi)):
        return None
    try:
        t0, proc, n, samples, next_at = time.perf_counter(), None, 0, [], seconds
        while True:
            step()
            n += 1
            if n % 4 == 0:
                sync()  # bound the launch queue
            el = time.perf_counter() - t0
            if hw and el >= next_at:
                samples.append((_read_int(os.path.join(hw, "power1_input")), _read_int(os.path.join(hw, "freq1_input"))))
                next_at = el + 0.15
                if len(samples) >= 4:
                    break
            if not hw and proc is None and el >= seconds:
                proc = subprocess.Popen([smi, "--showpower", "--showclocks", "--showmaxpower"], stdout=subprocess.PIPE,
                                        stderr=subprocess.DEVNULL, text=True)
            if (proc is not None and proc.poll() is not None) or el > 20.0:
                break
        sync()
        if hw:
            pw = [p for p, _ in samples if p]
            ck = [c for _, c in samples if c]
            if not pw:
                return None
            cap = _read_int(os.path.join(hw, "power1_cap"))
            pw_w, pc = float(np_median(pw)) / 1e6, cap / 1e6 if cap else None
            return {"load": what, "package_w": round(pw_w, 1), "cap_w": pc, "at_cap": bool(pc and pw_w >= 0.985 * pc),
                    "sclk_mhz": int(np_median(ck) / 1e6) if ck else None, "steps_under_load": n,
                    "source": "hwmon power1_input / freq1_input, median of %d reads after %.1f s of back-to-back steps" % (len(pw), seconds)}
        text = proc.communicate(timeout=20)[0] if proc is not None else ""
        w = re.search(r"Current Socket Graphics Package Power \(W\): ([\d.]+)", text)
        cap = re.search(r"Max Graphics Package Power \(W\): ([\d.]+)", text)
        clk = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", text)
        if not w:
            return None
        pw, pc = float(w.group(1)), float(cap.group(1)) if cap else None
        return {"load": what, "package_w": pw, "cap_w": pc, "at_cap": bool(pc and pw >= 0.985 * pc),
                "sclk_mhz": int(clk.group(1)) if clk else None, "steps_under_load": n,
                "source": "rocm-smi, one sample after %.1f s of back-to-back steps" % seconds}
    except Exception as e:  # noqa: BLE001 - informational only
        return {"error": f"{type(e).__name__}: {e}"}


def np_median(v):
    v = sorted(v)
    m = len(v) // 2
    return v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])


def encoder_flops(lens, cfg):
    """Algorithmic FLOPs of one forward: the four GEMMs per layer + the two attention products."""
    H, F, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    gemm = float(sum(lens)) * L * (4 * 2 * H * H + 2 * 2 * H * F)
    attn = float(sum(L * 4 * int(n) * int(n) * H for n in lens))
    return gemm + attn


XLMR_LARGE = {"model_type": "xlm-roberta", "vocab_size": 30000, "hidden_size": 1024, "num_hidden_layers": 24,
              "num_attention_heads": 16, "intermediate_size": 4096, "max_position_embeddings": 514, "type_vocab_size": 1,
              "layer_norm_eps": 1e-5, "hidden_act": "gelu", "pad_token_id": 1}


def seeded_state_dict(cfg, dev, seed=0):
    """Seeded random weights of a BERT / XLM-R encoder, keyed like an HF state_dict, generated on the device (no checkpoint
    offline; building transformers' own 560M-parameter module on the host just to time the GPU forward would take longer than
    the measurement).  Scales keep the activations in a trained model's range."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    H, F, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]

    def rn(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * scale + shift

    sd = {"embeddings.word_embeddings.weight": rn(cfg["vocab_size"], H, scale=0.5),
          "embeddings.position_embeddings.weight": rn(cfg["max_position_embeddings"], H, scale=0.5),
          "embeddings.token_type_embeddings.weight": rn(cfg["type_vocab_size"], H, scale=0.5),
          "embeddings.LayerNorm.weight": rn(H, scale=0.2, shift=1.0), "embeddings.LayerNorm.bias": rn(H, scale=0.1)}
    for i in range(L):
        pre = f"encoder.layer.{i}."
        for part in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            sd[pre + part + ".weight"] = rn(H, H, scale=1.5 / H ** 0.5)
            sd[pre + part + ".bias"] = rn(H, scale=0.1)
        sd[pre + "intermediate.dense.weight"] = rn(F, H, scale=1.5 / H ** 0.5)
        sd[pre + "intermediate.dense.bias"] = rn(F, scale=0.1)
        sd[pre + "output.dense.weight"] = rn(H, F, scale=1.0 / F ** 0.5)
        sd[pre + "output.dense.bias"] = rn(H, scale=0.1)
        for ln in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[pre + ln + ".weight"] = rn(H, scale=0.2, shift=1.0)
            sd[pre + ln + ".bias"] = rn(H, scale=0.1)
    return sd


def one_sentence_latency(enc, vocab, lengths=(8, 16, 32, 64, 128, 256, 512), calls=200):
    """ONE sentence per call — the reference's only shape (extract_embeddings(text): minivectordb/embedding_model.py:62-71):
    host token ids in, host embedding out (GpuEncoder.forward: ids and embedding through one host-mapped buffer, the forward,
    one stream wait), up to the 512 tokens the reference truncates at (embedding_model.py:64,77)."""
    import numpy as np
    rs = np.random.RandomState(1)
    rows = []
    for S in lengths:
        ids = rs.randint(5, vocab, size=(1, S)).astype(np.int32)
        mask = np.ones((1, S), np.int32)
        for _ in range(5):
            enc.forward(ids, mask)
        lat = []
        for _ in range(calls):
            t0 = time.perf_counter()
            enc.forward(ids, mask)
            lat.append(time.perf_counter() - t0)
        rows.append({"tokens": S, "p50_ms": round(float(np.median(lat)) * 1e3, 4), "p99_ms": round(float(np.percentile(lat, 99)) * 1e3, 4),
                     "one_launch_walks_the_layers": bool(enc.walks(1, S))})
    return rows


def large_encoder_block(dev):
    """The reference's DEFAULT alternative model is bge-m3 (minivectordb/embedding_model.py:17, :59-60) — XLM-R-large widths (H 1024,
    24 layers, 16 heads of 64, FFN 4096), CLS pooling; e5-large is the same encoder with mean pooling.  256 x 32 tokens, one
    256 x 512 sample and the one-sentence-per-call latencies, seeded weights (vocabulary cut to 30,000 rows: the table is only gathered)."""
    import numpy as np
    import torch
    from minivectordb_amd.embedding_model import GpuEncoder
    enc = GpuEncoder(XLMR_LARGE, seeded_state_dict(XLMR_LARGE, dev), device=dev.index or 0, pooling="cls")
    B = 256
    out = {"model": "bge-m3 / multilingual-e5-large architecture (XLM-R large: H 1024, 24 layers, 16 heads, FFN 4096), CLS pooling, "
                    "seeded weights, vocabulary cut to 30,000", "sentences": B, "shapes": []}
    for S, reps in ((32, 8), (512, 2)):
        rs = np.random.RandomState(S)
        ids = torch.from_numpy(rs.randint(5, 30000, size=(B, S)).astype(np.int32)).to(dev)
        mask = torch.ones((B, S), dtype=torch.int32, device=dev)
        flops = encoder_flops(np.full(B, S), XLMR_LARGE)
        rec = {"S": S, "ragged": False, "tokens": B * S}
        for mode, compute, products in (("fp16x3", 2, 3),) + ((("fp32", 0, 1),) if S == 32 else ()):
            for _ in range(2):
                enc.forward_device(ids, mask, compute=compute)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.forward_device(ids, mask, compute=compute)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            tf = products * flops / dt / 1e12
            rec[mode] = {"ms": round(dt * 1e3, 3), "sentences_per_s": round(B / dt, 1),
                         "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": MFMA_PEAK_TF[mode], "unit": "TFLOP/s",
                                      "frac": round(tf / MFMA_PEAK_TF[mode], 4), "mfma_products_per_algorithmic_product": products,
                                      "algorithmic_tflop_per_forward": round(flops / 1e12, 4)}}
        out["shapes"].append(rec)
    out["one_sentence_per_call"] = one_sentence_latency(enc, 30000)
    enc.close()
    return out


def encoder_and_config5(native, dev, k, no_cpu):
    """BASELINE config 5 where the driver sees it: encoder forward (256 sentences) alone, its CPU baseline, and encoder ->
    256-query kNN over 10M x 384 end to end.  Weights are seeded random tensors of the e5-small architecture (no
    checkpoint offline); the SAME weights run on the CPU through transformers' BertModel."""
    import numpy as np
    import torch
    from transformers import BertConfig, BertModel
    from minivectordb_amd.embedding_model import GpuEncoder

    torch.manual_seed(0)
    hf = BertModel(BertConfig(**{kk: v for kk, v in E5_SMALL.items() if kk != "model_type"}), add_pooling_layer=False).eval()
    with torch.no_grad():  # HF's init: 0.02-sigma weights, zero biases, unit LayerNorm — make every term count
        for name, p in hf.named_parameters():
            if name.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
            elif "LayerNorm.weight" in name:
                p.add_(0.2 * torch.randn_like(p))
            elif "dense.weight" in name or "self." in name:
                p.mul_(2.5)
    enc = GpuEncoder(hf.config, hf.state_dict(), device=dev.index or 0)
    B, H = 256, E5_SMALL["hidden_size"]
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # a real stream: the encoder replays its captured hipGraph on it
    stream = torch.cuda.current_stream().cuda_stream
    out = {"model": "multilingual-e5-small architecture (BERT, H 384, 12 layers, 12 heads, FFN 1536), seeded weights",
           "sentences": B, "shapes": []}
    inputs = {}
    for S in (32, 512):
        rs = np.random.RandomState(S)
        ids = rs.randint(5, 250000, size=(B, S)).astype(np.int32)
        for ragged in (False, True):
            lens = rs.randint(max(1, S // 4), S + 1, size=B) if ragged else np.full(B, S)
            mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int32)
            ids_d, mask_d = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
            inputs[(S, ragged)] = (ids, mask, ids_d, mask_d, lens)
            flops = encoder_flops(lens, E5_SMALL)
            rec = {"S": S, "ragged": bool(ragged), "tokens": int(lens.sum())}
            for mode, compute, products in (("fp16x3", 2, 3), ("fp32", 0, 1)):
                for _ in range(3):
                    enc.forward_device(ids_d, mask_d, compute=compute)
                torch.cuda.synchronize()
                reps = 20 if S == 32 else 5
                t0 = time.perf_counter()
                for _ in range(reps):
                    enc.forward_device(ids_d, mask_d, compute=compute)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / reps
                tf = products * flops / dt / 1e12   # matrix-core products actually issued
                rec[mode] = {"ms": round(dt * 1e3, 3), "sentences_per_s": round(B / dt, 1),
                             "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": MFMA_PEAK_TF[mode],
                                          "unit": "TFLOP/s", "frac": round(tf / MFMA_PEAK_TF[mode], 4),
                                          "mfma_products_per_algorithmic_product": products,
                                          "algorithmic_tflop_per_forward": round(flops / 1e12, 4)}}
            if not ragged:
                rec["power"] = power_probe(lambda: enc.forward_device(ids_d, mask_d, compute=2),
                                           f"fp16x3 forward, 256 x {S} tokens, back to back", torch.cuda.synchronize)
            out["shapes"].append(rec)
    out["default_mode"] = "fp16x3 (split-precision: a.w ~ al.wh + ah.wl + ah.wh in fp16 pieces, fp32 accumulate)"
    # one sentence per call, the reference's only shape: <= 64 token slots run as ONE launch that walks the layers (exact fp32)
    out["one_sentence_per_call"] = one_sentence_latency(enc, 250000)

    # (before the CPU baseline: its 100+ busy host threads starve the launching thread afterwards — a 20-launch search took
    # 11 ms instead of 2.8 when measured behind it)
    # ---- config 5 end to end: encoder -> 256 queries -> kNN over 10M x 384, nothing leaves the device -----------------
    n5 = 10_000_000
    idx5 = native.FlatIndex(H, device=dev.index or 0)
    idx5.reserve(n5)
    idx5.add_synthetic(n5, 1234, normalize=True)
    D = torch.empty((B, k), dtype=torch.float32, device=dev)
    I = torch.empty((B, k), dtype=torch.int64, device=dev)
    c5 = {"workload": f"256 sentences -> e5-small-shaped encoder -> 256 x {H} queries -> IP kNN, k = {k}, over {n5} x {H} fp32",
          "shapes": []}
    for S in (32, 512):
        _, _, ids_d, mask_d, lens = inputs[(S, True)]

        def step():
            emb, _ = enc.forward_device(ids_d, mask_d)
            idx5.search_device(emb.data_ptr(), B, k, D.data_ptr(), I.data_ptr(), stream=stream)

        for _ in range(2):
            step()
        torch.cuda.synchronize()
        reruns0 = native.split_rerun_count()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            enc.forward_device(ids_d, mask_d)
        torch.cuda.synchronize()
        t_enc = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        t_all = (time.perf_counter() - t0) / reps
        # the same chain as ONE hipGraph (the search never synchronises: tests/test_config5_gpu.py checks the replay bit for
        # bit): no host launches between the encoder's graph and the search's ~25 kernels
        t_graph = None
        try:
            g = torch.cuda.CUDAGraph()
            emb_g = torch.empty((B, H), dtype=torch.float32, device=dev)
            with torch.cuda.graph(g, stream=torch.cuda.current_stream(), capture_error_mode="thread_local"):
                e_, _ = enc.forward_device(ids_d, mask_d)
                emb_g.copy_(e_)
                idx5.search_device(emb_g.data_ptr(), B, k, D.data_ptr(), I.data_ptr(), stream=stream)
            g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                g.replay()
            torch.cuda.synchronize()
            t_graph = (time.perf_counter() - t0) / reps
            del g
        except Exception as e:  # noqa: BLE001 - a capture problem must not cost the bench line
            print(f"[bench] config 5 graph capture skipped: {e}", file=sys.stderr)
        uncertified = (native.split_rerun_count() - reruns0) / reps
        knn_power = None
        if S == 32:
            emb_fix = enc.forward_device(ids_d, mask_d)[0].clone()
            knn_power = power_probe(lambda: idx5.search_device(emb_fix.data_ptr(), B, k, D.data_ptr(), I.data_ptr(), stream=stream),
                                    f"256-query kNN over {n5} x {H}, back to back", torch.cuda.synchronize)
        passes = -(-B // max(native.half_max_queries(H), 128))
        # the batch's nomination pass streams the index' fp16 shadow where it keeps one (2 B per element: its algorithmic bytes)
        shadow5 = int(native.lib().mvdb_index_shadow_rows(idx5.handle)) >= n5
        knn_gbs = passes * n5 * H * (2 if shadow5 else 4) / max(t_all - t_enc, 1e-9) / 1e9
        c5["shapes"].append({"S": S, "ragged": True, "tokens": int(lens.sum()), "encoder_ms": round(t_enc * 1e3, 3),
                             "knn_ms": round((t_all - t_enc) * 1e3, 3), "end_to_end_ms": round(t_all * 1e3, 3),
                             "end_to_end_one_graph_ms": None if t_graph is None else round(t_graph * 1e3, 3),
                             "sentences_per_s": round(B / t_all, 1), "knn_corpus_passes": passes,
                             # query chunks that held a query the certified pass could not certify (re-run exactly, on the device)
                             "uncertified_chunks_per_search": uncertified,
                             "knn_power": knn_power,
                             "knn_roofline": {"bound": "hbm", "achieved": round(knn_gbs, 1), "peak": HBM_PEAK_GBS,
                                              "unit": "GB/s", "frac": round(knn_gbs / HBM_PEAK_GBS, 4),
                                              "operand": "fp16 shadow (2 B per element)" if shadow5 else "fp32 corpus (4 B per element)",
                                              "note": "whole kNN leg (seed launch, 3 main launches, merges, certification) "
                                                      "against ONE pass over the operand"}})
    idx5.close()
    # ---- CPU baseline: the reference's own forward (transformers BertModel + average_pool + F.normalize) ------------
    if not no_cpu:
        import torch.nn.functional as F
        threads = torch.get_num_threads()

        def cpu_forward(ids, mask):
            with torch.no_grad():
                bi, bm = torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(mask.astype(np.int64))
                o = hf(input_ids=bi, attention_mask=bm).last_hidden_state
                o = o.masked_fill(~bm[..., None].bool(), 0.0)
                return F.normalize(o.sum(dim=1) / bm.sum(dim=1)[..., None], p=2, dim=1).numpy()

        cpu = {"kind": "reference", "cores": threads, "unit": "sentences/s",
               "what": "transformers BertModel (the library the reference calls) + average_pool + F.normalize, torch CPU"}
        ids, mask, ids_d, mask_d, lens = inputs[(32, True)]
        cpu_forward(ids[:32], mask[:32])  # warm the thread pool
        t0 = time.perf_counter()
        ref = cpu_forward(ids, mask)
        t32 = time.perf_counter() - t0
        got, _ = enc.forward_device(ids_d, mask_d)
        torch.cuda.synchronize()
        cpu["S32_ragged"] = {"ms_per_256_sentences": round(t32 * 1e3, 1), "value": round(B / t32, 1),
                             "sample": "the whole 256-sentence batch, once"}
        cpu["max_abs_diff_gpu_vs_cpu_embedding"] = float(np.abs(got.cpu().numpy() - ref).max())
        ids, mask, _, _, lens = inputs[(512, True)]
        nb = 16  # bounded sample: 16 of the 256 sentences
        t0 = time.perf_counter()
        cpu_forward(ids[:nb], mask[:nb])
        t512 = time.perf_counter() - t0
        frac = float(lens[:nb].sum()) / float(lens.sum())
        cpu["S512_ragged"] = {"ms_per_256_sentences": round(t512 / frac * 1e3, 1), "value": round(B * frac / t512, 1),
                              "sample": f"first {nb} of 256 sentences ({frac:.3f} of the tokens), time scaled by tokens"}
        cpu["value"] = cpu["S32_ragged"]["value"]
        out["cpu_baseline"] = cpu
    else:
        out["cpu_baseline"] = None

    enc.close()
    try:
        out["large"] = large_encoder_block(dev)
    except Exception as e:  # noqa: BLE001
        out["large"] = {"error": f"{type(e).__name__}: {e}"}
    return out, c5


def certified_passes_on_unfriendly_data(native, dev, k, n=10_000_000, d=512, nq=256):
    """Every throughput figure of the certified batch passes above is on the zero-mean stream, where certification always
    succeeds.  The same passes on the two unfriendly families of the generator (oracle/flat_oracle.c synth_value): rows like
    the reference's own test vectors (numpy.random.rand, tests/test_sharded_multithreaded_operations.py:22: a narrow cone) and a
    clustered corpus (4,096 centres + 6 % noise, exact and near duplicates: thousands of rows within 1e-3 of a query's best).
    Per corpus: 256 queries of the same family, 256 / 32 per call and the opt-in single-query route over the fp16 shadow, with
    the exact single-query scan beside them; `uncertified_chunks_per_call` = chunks of a call that held a query the
    certificate refused (answered exactly, on the device: by the rescue pass over the shadow, or by an exact fp32 pass)."""
    import numpy as np
    import torch
    # (clustered at 10M rows: ~19 noise-free / near-duplicate rows per centre outscore the centre's other 2,400 rows by 2e-3, so
    #  k = 10 certifies; at 1M rows there are ~2 of them per centre and every query's 10th and 64th best are within 1e-3: the
    #  regime where certification always fails — measured at that size, with the zero-mean stream of the same size beside it)
    fam = {"zero_mean": (0, n), "all_positive": (1 << 56, n), "clustered": (2 << 56, n),
           "zero_mean_1M": (0, 1_000_000), "clustered_1M": (2 << 56, 1_000_000)}
    out = {"workload": f"rows x {d} fp32, IP, k = {k}, {nq} queries drawn from the corpus' own family", "corpora": {}}
    stream = torch.cuda.current_stream().cuda_stream
    for name, (bits, n) in fam.items():
        idx = native.FlatIndex(d, device=dev.index or 0)
        idx.reserve(n)
        idx.add_synthetic(n, 1234 | bits, normalize=True)
        q = torch.empty((nq, d), dtype=torch.float32, device=dev)
        native.check(native.lib().mvdb_synth_fill_device(q.data_ptr(), nq, d, 5678 | bits, 0, 1, dev.index or 0, stream))
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        rec = {"rows": n}

        def run(per_call, count):
            for a in range(0, count, per_call):
                m = min(per_call, count - a)
                idx.search_device(q[a:a + m].data_ptr(), m, k, D[a:a + m].data_ptr(), I[a:a + m].data_ptr(), stream=stream)

        def timed(per_call, count, reps):
            run(per_call, count)   # first call: shadow, workspaces
            torch.cuda.synchronize()
            before = native.split_rerun_count()
            t0 = time.perf_counter()
            for _ in range(reps):
                run(per_call, count)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps
            calls = (count + per_call - 1) // per_call
            return {"queries_per_s": round(count / dt, 1), "ms_per_call": round(dt / calls * 1e3, 4),
                    "uncertified_chunks_per_call": round((native.split_rerun_count() - before) / reps / calls, 3)}

        rec["exact_single_query_scan"] = timed(1, 32, 2)
        exact_ids = I[:32].cpu().numpy().copy()
        rec["256_per_call"] = timed(256, nq, 3)
        same256 = bool(np.array_equal(I[:32].cpu().numpy(), exact_ids))
        # where a refused call spends its device time: the certified pass, the RESCUE pass (refused queries once more over the
        # shadow, every row above their floor re-scored: exact), the gated exact fp32 passes behind it (launches that return at
        # their gate included, ~7 us each)
        native.prof_enable(True)
        try:
            fams = ("ip_scan_half", "ip_scan_half_seed", "ip_scan_rescue", "ip_scan_rerun")
            for f in fams:
                native.prof_read(f)
            run(256, nq)
            torch.cuda.synchronize()
            t = {f: native.prof_read(f) for f in fams}
        finally:
            native.prof_enable(False)
        rec["256_per_call"]["device_ms_by_tier"] = {
            "certified_pass": round(t["ip_scan_half"][1] + t["ip_scan_half_seed"][1], 3),
            "rescue_pass": round(t["ip_scan_rescue"][1], 3), "exact_rerun_passes": round(t["ip_scan_rerun"][1], 3),
            "launches": {"rescue": t["ip_scan_rescue"][0], "exact_rerun": t["ip_scan_rerun"][0]}}
        rec["32_per_call"] = timed(32, nq, 2)
        idx.set_option("shadow_single_query", 1)
        rec["single_query_over_fp16_shadow_opt_in"] = timed(1, 32, 2)
        same1 = bool(np.array_equal(I[:32].cpu().numpy(), exact_ids))
        idx.set_option("shadow_single_query", 0)
        # (raw equality with the exact single-query scan; on the clustered corpora rows within 2e-6 of each other may swap between
        #  two exact kernels' summation orders — tests/test_fullsize_gpu.py adjudicates every such difference in float64)
        rec["ids_equal_exact_scan_first_32_queries"] = {"256_per_call": same256, "single_query_over_fp16_shadow": same1}
        out["corpora"][name] = rec
        idx.close()
    return out


DUMP_LIMIT_BYTES = 60 << 20   # under 64 MB with the .npy headers


def dump_outputs(out_dir, arrays):
    """DIR/<name>.npy per array: floating results as float32, integer ids as float64 (exact below 2**53).  Past
    DUMP_LIMIT_BYTES in all, the same fixed, seeded sample of rows is kept of every array (its row numbers in DIR/rows.npy)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {name: np.asarray(a, dtype=np.float32 if np.issubdtype(np.asarray(a).dtype, np.floating) else np.float64)
              for name, a in arrays.items()}
    rows = next(iter(arrays.values())).shape[0]
    per_row = sum(a.nbytes for a in arrays.values()) / max(rows, 1) + 8
    if per_row * rows > DUMP_LIMIT_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(rows, int(DUMP_LIMIT_BYTES // per_row), replace=False))
        arrays = {name: a[keep] for name, a in arrays.items()}
        arrays["rows"] = keep.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows per GPU")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1, help="queries per step (1 = the reference API shape; >1 = one "
                    "multi-query MFMA pass per step)")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline (host API rate, "
                    "opt-in shadow route, power, CPU baseline, unfriendly corpora, encoder / config-5 blocks)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-encoder", action="store_true", help="with --full: skip the unfriendly-corpora / encoder / "
                    "config-5 blocks")
    ap.add_argument("--dump", default=None, help="rank 0 writes the merged (D, I) of the first 16 timed steps to this "
                    ".npz (tests/test_config4_gpu.py compares them with a single-index search)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="rank 0 writes the (D, I) the last timed step "
                    "returned as DIR/D.npy (float32) and DIR/I.npy (float64), at most 64 MB in all")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and world == 1:
        raise SystemExit("for --gpus N > 1 launch through torch.distributed.run (one rank per GPU)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # test hook: MVDB_BENCH_SHARE_GPU=1 + MVDB_BENCH_BACKEND=gloo runs the N > 1 code path with every rank
    # on GPU 0 of a one-GPU box (RCCL refuses two ranks on one device); never used for reported numbers
    share_gpu = os.environ.get("MVDB_BENCH_SHARE_GPU") == "1"
    backend = os.environ.get("MVDB_BENCH_BACKEND", "nccl")
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from minivectordb_amd import _native as native
    from minivectordb_amd.distributed import ShardedSearcher

    n, d, k, nq = args.rows, args.dim, args.k, args.nq
    W, K = args.warmup, args.steps
    # dominant kernel by batch size: GEMV scan (nq = 1), 16/32-query MFMA pass, 128-query GEMM-tiled scan
    scan_names = ("ip_scan", "ip_scan_mfma", "ip_scan_gemm", "ip_scan_half")
    idx = native.FlatIndex(d, device=local_rank)
    idx.reserve(n)
    idx.add_synthetic(n, 1234, first_row=rank * n, normalize=True)

    # all queries on the device up front (same on every rank), normalised
    nqs = (W + K) * nq
    queries = torch.empty((nqs, d), dtype=torch.float32, device=dev)
    native.check(native.lib().mvdb_synth_fill_device(queries.data_ptr(), nqs, d, 5678, 0, 1, local_rank,
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()

    # A scaling run should measure the in-library RCCL route (ncclAllGather issued from libmvdb.so).  That route has never
    # run with more than one rank (the build boxes have one GPU), so its first N-GPU run must end in a number or in ONE
    # parseable line, never in a traceback or a silent hang:
    #   * the bring-up raises (every rank together: Collective agrees on the outcome by a MIN all-reduce)  ->  the run falls
    #     back, LOUDLY, to torch.distributed's all-gather (RCCL as well) and the line carries `native_route_error` next to
    #     `collective`; MVDB_BENCH_REQUIRE_NATIVE=1 turns the fallback off (one JSON error line, exit 3);
    #   * the bring-up or the warm-up HANGS  ->  a watchdog prints the JSON error line and ends the process after
    #     MVDB_BENCH_BRINGUP_TIMEOUT_S (default 300 s; torchrun then ends the other ranks).
    want_native = world > 1 and backend == "nccl" and not share_gpu and os.environ.get("MVDB_COLLECTIVE") != "torch"

    def error_line(msg):
        return json.dumps({"error": msg, "collective": "ncclAllGather (mvdb_allgather_topk, libmvdb.so)",
                           "rank": rank, "n_gpus": world, "rccl": _rccl_version(),
                           "hint": "MVDB_COLLECTIVE=torch benches torch.distributed's all-gather instead; "
                                   "NCCL_DEBUG=INFO shows RCCL's own bring-up log"})

    watchdog = None
    if world > 1:
        import threading
        limit = float(os.environ.get("MVDB_BENCH_BRINGUP_TIMEOUT_S", "300"))

        def bail():
            stream = sys.stdout if rank == 0 else sys.stderr
            print(error_line(f"rank {rank}: the exchange bring-up / warm-up did not finish within {limit:.0f} s"), file=stream,
                  flush=True)
            os._exit(3)

        watchdog = threading.Timer(limit, bail)
        watchdog.daemon = True
        watchdog.start()

    native_route_error = None
    searcher = None
    inject = world > 1 and os.environ.get("MVDB_BENCH_TEST_NATIVE_FAILURE") == "1"   # test hook: the failure path on a box without N GPUs
    if want_native or inject:
        try:
            if inject:
                raise RuntimeError("injected by MVDB_BENCH_TEST_NATIVE_FAILURE (test hook)")
            searcher = ShardedSearcher(idx, k, rank=rank, world=world, rows_per_rank=n, device=dev, collective="native")
            if not searcher.collective.startswith("ncclAllGather"):
                raise RuntimeError(f"the exchange came up as {searcher.collective!r}")
        except Exception as e:  # noqa: BLE001 - every failure of the bring-up ends the same way
            native_route_error = f"{type(e).__name__}: {e}"
            searcher = None
            print(f"[bench] rank {rank}: {error_line(native_route_error)}", file=sys.stderr, flush=True)
            if os.environ.get("MVDB_BENCH_REQUIRE_NATIVE") == "1":
                if rank == 0:
                    print(error_line(native_route_error), flush=True)
                try:
                    dist.destroy_process_group()
                except Exception:  # noqa: BLE001
                    pass
                raise SystemExit(3)
    if searcher is None:
        searcher = ShardedSearcher(idx, k, rank=rank, world=world, rows_per_rank=n, device=dev,
                                   collective="torch" if native_route_error is not None else None)

    def barrier():
        if world > 1:
            dist.barrier()

    for i in range(W):
        searcher.search_device(queries[i * nq:(i + 1) * nq])
    torch.cuda.synchronize()
    barrier()
    if watchdog is not None:
        watchdog.cancel()   # every rank got through the bring-up and the warm-up exchanges
    for name in scan_names:
        native.prof_read(name)  # drop warm-up launches
    native.prof_enable(True)
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(W, W + K):
        last = searcher.search_device(queries[i * nq:(i + 1) * nq])
    torch.cuda.synchronize()
    barrier()
    dt = time.perf_counter() - t0
    native.prof_enable(False)
    if args.dump_outputs and rank == 0:
        # (the result buffers are reused by the next search of this nq: copy them out before anything else runs)
        dump_outputs(args.dump_outputs, {"D": last[0].cpu().numpy(), "I": last[1].cpu().numpy()})
    # dominant kernel by batch size: GEMV scan (nq = 1), fp32-MFMA pass, the certified pass over the fp16 shadow, the
    # GEMM-tiled exact scan — whichever took the most time in the timed region
    prof = {name: native.prof_read(name) for name in scan_names}
    scan_name = max(prof, key=lambda name: prof[name][1])
    launches, scan_ms = prof[scan_name]

    rank_ms = [scan_ms / max(launches, 1)]  # this rank's mean launch duration of the dominant kernel
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        g = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(g, torch.tensor(rank_ms, dtype=torch.float64, device=dev))
        rank_ms = [float(v.item()) for v in g]

    if args.dump:
        got = []
        for i in range(W, W + min(K, 16)):
            D_, I_ = searcher.search_device(queries[i * nq:(i + 1) * nq])
            got.append((D_.cpu().numpy().copy(), I_.cpu().numpy().copy()))
        if rank == 0:
            np.savez(args.dump, D=np.stack([g[0] for g in got]), I=np.stack([g[1] for g in got]),
                     first_query=W * nq, nq=nq, rows_per_rank=n, world=world)

    # p50 latency: per-query wall (enqueue -> result on device), outside the timed region
    lat = []
    for i in range(W, W + min(K, 100)):
        torch.cuda.synchronize()
        a = time.perf_counter()
        searcher.search_device(queries[i * nq:(i + 1) * nq])
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - a) * 1e3)
    p50 = float(np.median(lat))

    out = None
    if rank == 0:
        bytes_per_launch = n * d * 4  # algorithmic: every stored row of this rank's shard once
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        chunk = 128  # queries per corpus pass of the batch passes
        if scan_name == "ip_scan_half":
            # fp16 nomination pass: the seed launch (ip_scan_half_seed) covers the first 32-row tile of every CU
            chunk = native.half_max_queries(d)
            # round 4: where the index keeps an fp16 shadow of its rows the main launches stream THAT — 2 bytes per element
            # are the pass's algorithmic bytes (the fp32 matrix is read by the seed launch and the re-scores only)
            shadow = native.prof_symbol(scan_name).startswith("flat_scan_h16_kernel")
            bytes_per_launch = (n - min((n + 31) // 32, cus) * 32) * d * (2 if shadow else 4)
        passes = K * ((nq + chunk - 1) // chunk)
        if scan_name == "ip_scan_half":
            # one corpus pass = the seed launch + up to four main launches of growing size (phases, admission floors
            # refreshed in between): the per-launch figures below are averages over those launches
            bytes_per_launch = bytes_per_launch * passes / max(launches, 1)
        avg_ms = scan_ms / max(launches, 1)
        # aggregate over ranks: every rank streams its own shard once per launch
        achieved = sum(bytes_per_launch / (ms * 1e-3) / 1e9 for ms in rank_ms if ms > 0) if launches else 0.0
        out = {
            "metric": baseline_metric(),
            "value": round(K * nq / dt, 3),
            "unit": "queries/s",
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": round(dt / K * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32 (fp16 single-product nomination, f32 re-score + certificate)" if scan_name == "ip_scan_half" else "f32",
            "data": "synthetic",
            "config": {
                "workload": (f"{world * n} x {d} fp32 corpus ({n} rows resident per GPU), IP, k={k}, "
                             f"nq={nq} per step"),
                "rows_per_gpu": n, "dim": d, "k": k, "nq": nq,
                "parallelism": f"row-sharded x{world}" + (", RCCL all-gather of per-shard top-k" if world > 1 else ""),
            },
            "p50_latency_ms": round(p50, 4),
            "corpus_rows": world * n,
            "corpus_rows_per_s": round(world * n * K * nq / dt, 1),
            "shard_passes_per_s": round(world * passes / dt, 3),
            "collective": searcher.collective,
            "native_route_error": native_route_error,   # not None: the in-library RCCL route failed, torch's all-gather ran
            "roofline": None,
        }
        if scan_name == "ip_scan_gemm":
            # compute-bound regime: fp32 MFMA roofline; one launch scores min(nq, 128) queries against n rows
            per_launch = min(nq, 128)
            flops = 2.0 * n * d * per_launch
            tf = flops / (avg_ms * 1e-3) / 1e12 if launches else 0.0
            out["roofline"] = {"bound": "mfma", "achieved": round(tf, 2), "peak": 157.3, "unit": "TFLOP/s",
                               "frac": round(tf / 157.3, 4), "traffic": None, "kernel": "flat_scan_gemm_kernel",
                               "launches": launches, "avg_launch_ms": round(avg_ms, 4),
                               "algorithmic_flops_per_launch": flops}
        else:
            launched = native.prof_symbol(scan_name)
            traffic = pmc_traffic(n, d, nq, scan_name, launched)
            out["roofline"] = {
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS * world,
                "unit": "GB/s",
                "frac": round(achieved / (HBM_PEAK_GBS * world), 4),
                "traffic": traffic["bytes"],
                "traffic_source": traffic["source"],
                "traffic_note": ("HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (FETCH_SIZE x 2 per "
                                 "the guide + WRITE_SIZE) — not a counter of this run: counters cannot be collected inside the timed process"),
                "launched": launched,
                "kernel": {"ip_scan": "flat_scan_kernel", "ip_scan_mfma": "flat_scan_mfma2_kernel", "ip_scan_gemm": "flat_scan_gemm_kernel",
                           "ip_scan_half": (launched.split("<")[0] or "flat_scan_h16_kernel")}[scan_name],
                "operand": ("fp16 shadow of the corpus (2 B per element; the fp32 matrix stays resident beside it)"
                            if launched.startswith("flat_scan_h16_kernel") else "fp32 corpus (4 B per element)"),
                "launches": launches,
                "avg_launch_ms": round(avg_ms, 4),
                "algorithmic_bytes_per_launch": int(bytes_per_launch),
                "launches_per_corpus_pass": round(launches / max(passes, 1), 2),
                "queries_per_corpus_pass": min(nq, chunk),
                "per_rank_avg_launch_ms": [round(v, 4) for v in rank_ms],
                "per_rank_launch_ms_min_max": [round(min(rank_ms), 4), round(max(rank_ms), 4)],
            }
        if world == 1 and args.full:
            # PCIe-inclusive host API (numpy in, numpy out): reported, never `value`
            qh = queries[W * nq:W * nq + 64].cpu().numpy()
            for i in range(3):
                idx.search(qh[i], k)  # first calls allocate the host-path workspace
            hl = []
            for i in range(qh.shape[0]):
                a = time.perf_counter()
                idx.search(qh[i], k)
                hl.append(time.perf_counter() - a)
            if nq == 1 and native.lib().mvdb_index_shadow_rows(idx.handle) >= 0 and d in (256, 384, 512) and n >= 500_000:
                # OPT-IN, never `value`: the same single queries through the certified fp16-shadow pass
                # (MVDB_SHADOW_SINGLE_QUERY=1: nomination over an fp16 copy of the rows, exact fp32 re-score, certificate,
                # device-gated exact re-run) — same ids, same fp32 scores, about half the bytes per query
                try:
                    exact = []
                    for i in range(W, W + min(K, 16)):
                        D_, I_ = searcher.search_device(queries[i:i + 1])
                        exact.append((D_.cpu().numpy().copy(), I_.cpu().numpy().copy()))
                    idx.set_option("shadow_single_query", 1)
                    for i in range(3):
                        searcher.search_device(queries[i:i + 1])    # the first call builds the shadow
                    torch.cuda.synchronize()
                    same = all(np.array_equal(searcher.search_device(queries[i:i + 1])[1].cpu().numpy(), exact[i - W][1])
                               for i in range(W, W + min(K, 16)))
                    t0 = time.perf_counter()
                    for i in range(W, W + K):
                        searcher.search_device(queries[i:i + 1])
                    torch.cuda.synchronize()
                    dts = time.perf_counter() - t0
                    out["opt_in_single_query_over_fp16_shadow"] = {
                        "how": "mvdb_index_set_option(idx, \"shadow_single_query\", 1) / VectorDatabase(fast_single_query=True) / MVDB_SHADOW_SINGLE_QUERY=1", "queries_per_s": round(K / dts, 3), "ms_per_query": round(dts / K * 1e3, 4),
                        "ids_equal_exact_scan": bool(same), "shadow_rows": int(native.lib().mvdb_index_shadow_rows(idx.handle)),
                        "note": "not the headline: the exact fp32 scan above is; this path reads 2 B per element"}
                except Exception as e:  # noqa: BLE001
                    out["opt_in_single_query_over_fp16_shadow"] = {"error": str(e)}
                finally:
                    idx.set_option("shadow_single_query", 0)
            pq = [0]

            def one_step():
                i = W + pq[0] % K
                pq[0] += 1
                searcher.search_device(queries[i * nq:(i + 1) * nq])

            out["power"] = power_probe(one_step, f"the timed step (nq={nq}) back to back", torch.cuda.synchronize)
            out["host_api_qps"] = round(len(hl) / sum(hl), 3)
            out["host_api_p50_ms"] = round(float(np.median(hl)) * 1e3, 4)
            if not args.no_cpu_baseline and nq == 1:
                try:   # (the headline line must survive a host that cannot hold or score the corpus)
                    out["cpu_baseline"] = cpu_baseline(native, idx, d, k, qh, n)
                except Exception as e:  # noqa: BLE001
                    out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
            else:
                out["cpu_baseline"] = None
            if not args.no_encoder and nq == 1:
                searcher.close()
                idx.close()   # the headline corpus (20 GB) is no longer needed
                try:
                    out["certified_passes_on_unfriendly_data"] = certified_passes_on_unfriendly_data(native, dev, k)
                except Exception as e:  # noqa: BLE001
                    out["certified_passes_on_unfriendly_data"] = {"error": f"{type(e).__name__}: {e}"}
                try:
                    out["encoder"], out["config5"] = encoder_and_config5(native, dev, k, args.no_cpu_baseline)
                except Exception as e:  # the headline line must survive a failure of the secondary blocks
                    out["encoder"] = {"error": f"{type(e).__name__}: {e}"}
                    out["config5"] = None
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    barrier()
    searcher.close()
    idx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
