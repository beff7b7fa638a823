// probe_scan.hpp — probed search (mvdb_index_search_probe): the rows are partitioned into C member lists by their nearest
// centre (mvdb_partition), a query scans only the lists of its nprobe best centres (include/mvdb.h "PROBED SEARCH",
// DESIGN.md section 6m).  Which lists a query scans is decided on the device; the host never sees a probe.
//
//   (coarse scores)       flat_scan_kernel in score mode over the centre matrix, one grid row per query: the single-query
//                         scan's own bits, a NaN marked kNotCandidate.  Not in this file.
//   probe_plan_kernel     a workgroup per query: its C keys make_key(score, centre) ordered in LDS — through the wave lists
//                         of topk_device.hpp up to 64 probes, a bitonic sort beyond —, the best nprobe kept; their list
//                         lengths, read from the offsets, become the query's work items: (begin, end) slices of
//                         kProbeSlice positions of the member array, and an item count.  An empty list takes its probe slot
//                         and no item.
//   probe_scan_kernel     grouped_scan_kernel (grouped_scan.hpp) with the item table read from device memory: block
//                         (x, query) takes item x of the query, blocks beyond the query's item count return at once.  The
//                         per-row arithmetic is flat_scan_kernel's, restated instruction for instruction for the same
//                         (G, C, MASKED): chunk order, fmaf order, xor butterfly.  Row numbers come from the member list by
//                         one 4-byte load, tail lanes clamped to the item's last position; SEL 2 tests the row's bit of a
//                         bitmap, a row beyond the bitmap is not selected.  Keys are make_key(score, row): ties fall to the
//                         lower row whatever list the row came from.
//   probe_merge_kernel    merge_keys_seg_kernel for the item lists of a query: D, I = row + label offset.
//
// Roofline: HBM, gather.  Bytes of a call = nq x (C x ld x 4 of centres, from L2 after the first query) + rows touched x
// (ld x 4 + 4) + items x (8 + 16 k).
#pragma once
#include "assign_scan.hpp"
#include "grouped_scan.hpp"

namespace mvdb {

constexpr int kProbeMaxLists = kAssignMaxVectors;  // C of a partition: assign's guard, and what the plan holds in LDS
constexpr int kProbeSlice = 128;                   // list positions per work item: a whole number of block steps of every shape
constexpr int kProbePlanThreads = 1024;
constexpr int kProbePlanWaves = kProbePlanThreads / kWave;
constexpr int kProbePlanPer = kProbeMaxLists / kProbePlanThreads;  // probe slots a thread of the plan owns

struct ProbeItem {
    uint32_t begin, end;  // positions of the member array (end > begin), inside ONE list
};

struct ProbePlanArgs {
    const uint32_t* scores;  // [nq, C] bit patterns of the coarse scores, kNotCandidate: no candidate
    int C;
    int P;                   // C rounded up to a power of two (>= 2)
    int nprobe;              // 1 .. C
    const uint32_t* off;     // [C + 1] the lists' offsets into the member array
    int max_items;           // item slots per query: what the nprobe largest lists need
    ProbeItem* items;        // [nq, max_items]
    int* count;              // [nq] items of each query
};

__global__ __launch_bounds__(kProbePlanThreads) void probe_plan_kernel(ProbePlanArgs a) {
    __shared__ uint64_t keys[kProbeMaxLists];
    __shared__ uint32_t pre[kProbeMaxLists + 1];
    __shared__ uint32_t wsum[kProbePlanWaves];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int qi = blockIdx.x;
    const uint32_t* const sc = a.scores + (int64_t)qi * a.C;
    auto key_of = [&](int c) -> uint64_t {
        if (c >= a.C) return 0ull;
        const uint32_t bits = sc[c];
        return bits == kNotCandidate ? 0ull : make_key(__uint_as_float(bits), (uint32_t)c);
    };

    // ---- keys[0 .. nprobe): the query's probes, best first (0: no candidate left) ------------------------------------------
    if (a.nprobe <= kMaxFusedK) {  // (uniform)
        WaveTopK tk;
        tk.init(a.nprobe);
        for (int base = wave * kWave; base < a.C; base += kProbePlanThreads) tk.offer(key_of(base + lane));  // (uniform bound)
        // the waves' lists merged pairwise, four rounds (block_merge_topk would have wave 0 take the other fifteen in turn)
        for (int step = 1; step < kProbePlanWaves; step <<= 1) {
            keys[wave * kWave + lane] = tk.key;
            __syncthreads();
            if (wave % (2 * step) == 0) tk.offer(keys[(wave + step) * kWave + lane]);  // (uniform over the wave)
            __syncthreads();
        }
        if (wave == 0) keys[lane] = tk.key;  // (lanes >= nprobe hold 0)
        __syncthreads();
    } else {
        const int P = a.P;
        for (int i = tid; i < P; i += kProbePlanThreads) keys[i] = key_of(i);
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int tix = tid; tix < P / 2; tix += kProbePlanThreads) {
                    const int lo = 2 * tix - (tix & (stride - 1));
                    const int hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const uint64_t x = keys[lo], y = keys[hi];
                    if ((x < y) == desc) {
                        keys[lo] = y;
                        keys[hi] = x;
                    }
                }
                __syncthreads();
            }
        }
    }

    // ---- items per probe, their exclusive prefix sum: a thread owns kProbePlanPer consecutive probe slots -------------------
    uint32_t mine[kProbePlanPer];
    uint32_t tsum = 0;
#pragma unroll
    for (int e = 0; e < kProbePlanPer; ++e) {
        const int j = tid * kProbePlanPer + e;
        uint32_t pieces = 0;
        if (j < a.nprobe) {
            const uint64_t key = keys[j];
            if (key) {
                const uint32_t c = key_row(key);
                pieces = (a.off[c + 1] - a.off[c] + kProbeSlice - 1) / kProbeSlice;
            }
        }
        mine[e] = tsum;
        tsum += pieces;
    }
    uint32_t wtot;
    const uint32_t ex = kmeans_wave_scan(tsum, &wtot);
    if (lane == 0) wsum[wave] = wtot;
    __syncthreads();
    uint32_t wbase = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kProbePlanWaves; ++w) {
        wbase += w < wave ? wsum[w] : 0u;
        total += wsum[w];
    }
#pragma unroll
    for (int e = 0; e < kProbePlanPer; ++e) {
        const int j = tid * kProbePlanPer + e;
        if (j < a.nprobe) pre[j] = wbase + ex + mine[e];
    }
    if (tid == 0) pre[a.nprobe] = total;
    __syncthreads();

    // (the host sized max_items from the nprobe LARGEST lists: never below the total; the bound keeps every write inside the table)
    total = total < (uint32_t)a.max_items ? total : (uint32_t)a.max_items;
    if (tid == 0) a.count[qi] = (int)total;
    ProbeItem* const items = a.items + (int64_t)qi * a.max_items;
    for (uint32_t i = tid; i < total; i += kProbePlanThreads) {
        int lo = 0, hi = a.nprobe;  // the last probe slot j with pre[j] <= i: it owns item i (a slot without items owns none)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= i) lo = mid;
            else hi = mid;
        }
        const uint32_t c = key_row(keys[lo]);
        const uint32_t begin = a.off[c] + (i - pre[lo]) * kProbeSlice;
        const uint32_t end = a.off[c + 1];
        items[i] = ProbeItem{begin, end - begin < (uint32_t)kProbeSlice ? end : begin + kProbeSlice};
    }
}

struct ProbeScanArgs {
    const float* X;           // [n_phys, ld] corpus
    int64_t ld;               // row stride in floats (multiple of 4)
    int d4;                   // valid 16-B chunks per row
    const float* q;           // [nq, ld] queries (device), zero padded
    int normalize_q;          // L2-normalise the query in the prologue
    int k;                    // <= kMaxFusedK
    const uint32_t* members;  // the member lists, list after list, ascending rows inside each
    const ProbeItem* items;   // [nq, max_items]
    const int* count;         // [nq]
    int max_items;
    const uint64_t* mask;     // SEL 2: bitmap over the physical rows [0, mask_n)
    int64_t mask_n;
    uint64_t* cand;           // [nq, max_items, k] one sorted list per item
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void probe_scan_kernel(ProbeScanArgs a) {
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int qi = blockIdx.y;
    if ((int)blockIdx.x >= a.count[qi]) return;  // (uniform) beyond the query's items
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction

    // the item: block-uniform, read through the scalar cache
    const int64_t slot = (int64_t)qi * a.max_items + blockIdx.x;
    const ProbeItem it = a.items[slot];
    const uint32_t* __restrict__ rows = a.members + it.begin;
    const int64_t m = (int64_t)it.end - (int64_t)it.begin;  // > 0 by construction

    // ---- query -> registers (flat_scan_kernel's prologue, same operation order) ---------------
    f32x4 qv[C];
    bool cvalid[C];
    const float* qptr = a.q + (int64_t)qi * a.ld;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int chunk = c * G + t;
        cvalid[c] = !MASKED || chunk < a.d4;
        qv[c] = cvalid[c] ? *reinterpret_cast<const f32x4*>(qptr + chunk * 4) : f32x4{0, 0, 0, 0};
    }
    if (a.normalize_q) {
        float nr = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c)
            nr += qv[c].x * qv[c].x + qv[c].y * qv[c].y + qv[c].z * qv[c].z + qv[c].w * qv[c].w;
        nr = group_reduce_add<G>(nr);
        if (nr > 0.f) {
            const float inorm = 1.0f / sqrtf(nr);
#pragma unroll
            for (int c = 0; c < C; ++c) qv[c] *= inorm;
        }
    }

    WaveTopK tk;
    tk.init(a.k);

    const int64_t nbatches = (m + RB - 1) / RB;
    const int64_t last = m - 1;

    // physical rows of the item's batch b: one 4-byte load per row through the member list (clamped: tail lanes re-read the
    // item's last row, result discarded — never a position outside [begin, end))
    auto batch_rows = [&](int64_t b, int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            pr[u] = (int64_t)rows[r];
        }
    };
    // the U*C row loads of a batch and, SEL 2, the rows' bitmap words behind them (nothing waits here)
    auto load_batch = [&](const int64_t (&pr)[U], f32x4 (&x)[U][C], uint64_t (&word)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* p = a.X + pr[u] * a.ld + t * 4;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const f32x4* src = reinterpret_cast<const f32x4*>(p + c * G * 4);
                if (MASKED)
                    x[u][c] = cvalid[c] ? __builtin_nontemporal_load(src) : f32x4{0, 0, 0, 0};
                else
                    x[u][c] = __builtin_nontemporal_load(src);
            }
        }
        if (SEL == 2) {
#pragma unroll
            for (int u = 0; u < U; ++u) word[u] = pr[u] < a.mask_n ? a.mask[pr[u] >> 6] : 0ull;  // (a row added after the set was built: not in it)
        }
    };
    auto consume_batch = [&](int64_t b, const int64_t (&pr)[U], f32x4 (&x)[U][C], const uint64_t (&word)[U]) {
        const int64_t row0 = b * RB + g;
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                acc = fmaf(x[u][c].x, qv[c].x, acc);
                acc = fmaf(x[u][c].y, qv[c].y, acc);
                acc = fmaf(x[u][c].z, qv[c].z, acc);
                acc = fmaf(x[u][c].w, qv[c].w, acc);
            }
            s[u] = acc;
        }
#pragma unroll
        for (int mm = G / 2; mm >= 1; mm >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], mm);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            const bool sel = SEL != 2 || ((word[u] >> (pr[u] & 63)) & 1ull);
            // the key carries the ROW: ties go to the lower row number, whichever list it came from
            const bool pass = (t == 0) && (r < m) && sel && (s[u] >= tk.thr_score);
            if (__ballot(pass)) tk.offer(pass ? make_key(s[u], (uint32_t)pr[u]) : 0ull);
        }
    };

    // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
    int64_t pr[U], pn[U];
    if (wave < nbatches) batch_rows(wave, pr);
    for (int64_t b = wave; b < nbatches; b += kScanWaves) {
        f32x4 x[U][C];
        uint64_t word[U] = {};
        load_batch(pr, x, word);
        const int64_t bn = b + kScanWaves;
        batch_rows(bn < nbatches ? bn : b, pn);
        consume_batch(b, pr, x, word);
#pragma unroll
        for (int u = 0; u < U; ++u) pr[u] = pn[u];
    }

    __shared__ uint64_t sh[(kScanWaves - 1) * kWave];
    block_merge_topk(tk, sh, kScanWaves);
    if (wave == 0 && lane < a.k) a.cand[slot * a.k + lane] = tk.key;
}

// ---- last stage: merge the k-lists of each query's items and emit (D, I) -------------------------------------------------------
// grid = (nq), block = 1024.  merge_keys_seg_kernel with the item counts read from the plan; a key carries its row.
struct ProbeMergeArgs {
    const uint64_t* keys;  // [nq, max_items, k]
    const int* count;      // [nq]
    int max_items;
    int k;
    int64_t label_offset;
    float* D;    // [nq, k]
    int64_t* I;  // [nq, k]
};

__global__ __launch_bounds__(kMergeThreads) void probe_merge_kernel(ProbeMergeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const int64_t total = (int64_t)a.count[qi] * a.k;
    const uint64_t* src = a.keys + (int64_t)qi * a.max_items * a.k;
    WaveTopK tk;
    tk.init(a.k);
    for (int64_t base = (int64_t)wave * kWave * kMergeUnroll; base < total; base += (int64_t)kMergeThreads * kMergeUnroll) {
        uint64_t c[kMergeUnroll];
#pragma unroll
        for (int j = 0; j < kMergeUnroll; ++j) {
            const int64_t i = base + j * kWave + lane;
            c[j] = i < total ? src[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kMergeUnroll; ++j) tk.offer(c[j]);
    }
    __shared__ uint64_t sh[(kMergeWaves - 1) * kWave];
    block_merge_topk(tk, sh, kMergeWaves);
    if (wave == 0 && lane < a.k) {
        const uint64_t key = tk.key;
        a.D[(int64_t)qi * a.k + lane] = key ? key_score(key) : -3.402823466e+38f;  // faiss convention for missing results
        a.I[(int64_t)qi * a.k + lane] = key ? (int64_t)key_row(key) + a.label_offset : -1;
    }
}

// labels[rows[i]] = the label of word best[rows[i]] (assign's running best; 0: no candidate -> -1)
__global__ __launch_bounds__(256) void probe_relabel_kernel(const int64_t* __restrict__ rows, int64_t m, const uint64_t* __restrict__ best,
                                                             int32_t* __restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = rows[i];
        const uint64_t key = best[r];
        labels[r] = key ? (int32_t)key_row(key) : -1;
    }
}

}  // namespace mvdb
