// distinct_select.hpp — distinct search (mvdb_index_search_distinct): the best row of each GROUP of stored rows, the k best
// groups (include/mvdb.h "DISTINCT SEARCH").  A grouping is one int32 code per stored row.
//
// Tier 1, distinct_collapse_kernel.  Behind the plain search of fetch_k candidates: one workgroup per query looks the
// candidates' codes up, marks the first occurrence of each code, writes the first k firsts in order and pads.  No row of the
// matrix is read.  A group absent from the candidates has no row above their last score, so when the candidates hold k
// groups (or are the whole ranking) this is the exact answer; else the kernel raises need[query].
//
// Tier 2, for the queries whose need word is set — the launches are always enqueued, a block whose query does not need them
// returns at once (the pattern of RangeScanArgs::gate_count):
//   distinct_clear_kernel     zeroes the query's slot of the table, n_groups 64-bit words;
//   group_best_scan_kernel    one pass over the selected rows.  The per-row arithmetic is range_scan_kernel's (range_scan.hpp),
//                             restated instruction for instruction for the inner product and the same (G, C, MASKED): lane t of
//                             the row's G lanes takes chunks t, t + G, ..., C x 4 fmaf in chunk order, then the G/2 ... 1 xor
//                             butterfly, the same fused query normalisation — a score is bit for bit the single-query scan's.
//                             Instead of appending, lane t == 0 offers make_key(score, position) to table[slot][code] with an
//                             atomicMax.  The word is read with a plain load first (issued with the batch's row loads; not at
//                             all where the lane offered to the same group last and remembers what the atomic returned) and
//                             the atomic skipped when the key is not larger: within a call a word only grows, so a stale
//                             view costs a spare atomic, never a wrong answer.  An integer maximum does not depend on the order of arrival: the table is deterministic.
//                             A key orders by (score, then LOWER position): ties go to the lower row, or list position.
//                             NaN scores are never offered.
//   distinct_topk_kernel      the k largest non-zero words of the slot (per-wave sorted lists of topk_device.hpp, merged per
//                             block: k <= 64), written over tier 1's output of that query.
//
// Bytes, tier 2, per needed query: n * ld * 4 (the rows) + 4 n (the codes; + 8 n of a row list, + n / 8 of a bitmap) +
// 16 n_groups (the slot cleared, then read once).
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

constexpr int kDistinctMaxFetch = 1024;
constexpr int kDistinctThreads = 1024;  // most threads of a collapse block (one per candidate), and the top-k block
constexpr int kDistinctWaves = kDistinctThreads / kWave;
static_assert(kDistinctMaxFetch <= kDistinctThreads, "the collapse gives every candidate a thread");

struct DistinctCollapseArgs {
    const float* candD;     // [nq, fetch_k] the plain search's scores, best first
    const int64_t* candI;   // [nq, fetch_k] its row numbers (label_offset 0), -1 = missing
    const int32_t* codes;   // [n] group code of every stored row
    int fetch_k, k;
    int covers;             // fetch_k >= the selected rows: the candidates are the whole ranking (known on the host)
    int64_t label_offset;
    float* D;               // [nq, k]
    int64_t* I;             // [nq, k]
    int32_t* G;             // [nq, k] or NULL
    int* need;              // [nq]: 1 = tier 1 is not the answer
    unsigned int* ticket;   // one word of the call's workspace, zero between launches: the last block publishes the counter
    unsigned int* ctr;      // NULL, or the index's device word: queries tier 2 has answered (a running total)
    volatile unsigned int* host;  // its host-mapped mirror
};

// blockDim.x: fetch_k rounded up to whole waves
__global__ __launch_bounds__(kDistinctThreads) void distinct_collapse_kernel(DistinctCollapseArgs a) {
    __shared__ int32_t code[kDistinctMaxFetch];
    __shared__ int wfirst[kDistinctWaves];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int nwaves = (int)blockDim.x >> 6;
    const int F = a.fetch_k;
    const int64_t qi = blockIdx.x;

    int64_t row = -1;
    float score = 0.f;
    int32_t c = -1;
    if (tid < F) {
        row = a.candI[qi * F + tid];
        score = a.candD[qi * F + tid];
        if (row >= 0) c = a.codes[row];
        code[tid] = c;
    }
    const int nvalid = __syncthreads_count(row >= 0);
    // first occurrence: no earlier valid candidate carries my code (every lane of a wave reads the same word: a broadcast)
    bool first = row >= 0;
    if (first) {
        for (int i = 0; i < tid; ++i) {
            if (code[i] == c) {
                first = false;
                break;
            }
        }
    }
    const uint64_t fm = __ballot(first);
    if (lane == 0) wfirst[wave] = __popcll(fm);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int n = wfirst[w];
        before += w < wave ? n : 0;
        total += n;
    }
    const int rank = before + __popcll(fm & ((1ull << lane) - 1ull));
    float* D = a.D + qi * a.k;
    int64_t* I = a.I + qi * a.k;
    int32_t* G = a.G ? a.G + qi * a.k : nullptr;
    if (first && rank < a.k) {
        D[rank] = score;
        I[rank] = row + a.label_offset;
        if (G) G[rank] = c;
    }
    for (int t = total + tid; t < a.k; t += (int)blockDim.x) {  // fewer groups than k: the tail is missing
        D[t] = -3.402823466e+38f;
        I[t] = -1;
        if (G) G[t] = -1;
    }
    if (tid == 0) {
        const int need = (total >= a.k || nvalid < F || a.covers) ? 0 : 1;
        a.need[qi] = need;
        if (a.ctr) {
            if (need) atomicAdd(a.ctr, 1u);
            __threadfence();
            if (atomicAdd(a.ticket, 1u) == gridDim.x - 1) {  // every block of the launch has counted
                *a.ticket = 0u;
                a.host[0] = atomicAdd(a.ctr, 0u);
            }
        }
    }
}

// ---- tier 2 ------------------------------------------------------------------------------------------------------------------
// blockIdx.y: the slot; zeroes the slot's words if its query needs tier 2
__global__ __launch_bounds__(256) void distinct_clear_kernel(uint64_t* __restrict__ table, int64_t n_groups, const int* __restrict__ need) {
    if (need[blockIdx.y] == 0) return;
    uint64_t* t = table + (int64_t)blockIdx.y * n_groups;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_groups; i += (int64_t)gridDim.x * blockDim.x) t[i] = 0ull;
}

struct GroupBestArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [slots, ld] the sub-tile's queries (device), zero padded
    int normalize_q;       // L2-normalise the query in the prologue
    const int* need;       // [slots]: a slot whose word is clear is not scanned
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    const int32_t* codes;  // [n_phys] group code of every stored row
    uint64_t* table;       // [slots, n_groups] best key of every group: make_key(score, position), 0 = none
    int64_t n_groups;
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void group_best_scan_kernel(GroupBestArgs a) {
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int qi = blockIdx.y;
    if (a.need[qi] == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction

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

    uint64_t* const tab = a.table + (int64_t)qi * a.n_groups;
    int32_t lcode = -1;   // the group this lane offered to last, and what it knows of that group's word: a value the word
    uint64_t lbest = 0;   // has held (it only grows) — stale at worst, like a plain load
    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t last = a.n - 1;

    auto batch_rows = [&](int64_t b, int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;  // clamp: tail lanes re-read the last row, result discarded
            pr[u] = SUBSET ? a.rows[r] : r;
        }
    };
    // The rows' codes first — one 4-byte word per row, the G lanes of a row read the same word —, then the rows, then the
    // table words of those codes: loads return in order, so the codes are back while the rows are still in flight and the
    // table words travel behind the rows instead of behind the arithmetic.  A word read here is one batch staler than one
    // read at the offer; it can only be smaller than the truth.
    auto load_batch = [&](const int64_t (&pr)[U], f32x4 (&x)[U][C], int32_t (&cd)[U], uint64_t (&wv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) cd[u] = a.codes[pr[u]];
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
        // (only the lane that offers reads, and not where the row's group is the one this lane offered to last: its view of
        //  that word, lbest, is kept in a register.  When one group holds most rows every wave would otherwise read ONE
        //  line at every batch — 10M x 512 under one group: 4.35 ms of requests to one L2 channel against a 2.9 ms scan)
#pragma unroll
        for (int u = 0; u < U; ++u) wv[u] = (t == 0 && cd[u] != lcode) ? tab[cd[u]] : lbest;
    };
    auto batch_bits = [&](int64_t b, bool (&sel)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            sel[u] = (a.mask[r >> 6] >> (r & 63)) & 1ull;
        }
    };
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C], const int32_t (&cd)[U], const uint64_t (&wv)[U], const bool (&sel)[U]) {
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
        for (int m = G / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], m);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            // a NaN fails s == s; the key carries the position (row number, or position in the row list)
            const bool pass = (t == 0) && (r < a.n) && (SEL != 2 || sel[u]) && (s[u] == s[u]);
            if (pass) {
                const uint64_t key = make_key(s[u], (uint32_t)r);
                uint64_t seen = cd[u] == lcode ? lbest : wv[u];  // (an earlier row of this batch may have offered to the same group)
                if (key > seen) {
                    const uint64_t old = atomicMax((unsigned long long*)(tab + cd[u]), (unsigned long long)key);
                    seen = old > key ? old : key;
                }
                lcode = cd[u];
                lbest = seen;
            }
        }
    };

    bool all_rows[U];
#pragma unroll
    for (int u = 0; u < U; ++u) all_rows[u] = true;
    if (SEL == 2) {
        bool sel[U], seln[U];
        if (gw < nbatches) batch_bits(gw, sel);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            int32_t cd[U];
            uint64_t wv[U];
            batch_rows(b, pr);
            load_batch(pr, x, cd, wv);
            const int64_t bn = b + nwaves_total;
            batch_bits(bn < nbatches ? bn : b, seln);  // behind the row loads: never waited for by its own batch
            consume_batch(b, x, cd, wv, sel);
#pragma unroll
            for (int u = 0; u < U; ++u) sel[u] = seln[u];
        }
    } else if (SUBSET) {
        // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
        int64_t pr[U], pn[U];
        if (gw < nbatches) batch_rows(gw, pr);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int32_t cd[U];
            uint64_t wv[U];
            load_batch(pr, x, cd, wv);
            const int64_t bn = b + nwaves_total;
            batch_rows(bn < nbatches ? bn : b, pn);
            consume_batch(b, x, cd, wv, all_rows);
#pragma unroll
            for (int u = 0; u < U; ++u) pr[u] = pn[u];
        }
    } else {
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            int32_t cd[U];
            uint64_t wv[U];
            batch_rows(b, pr);
            load_batch(pr, x, cd, wv);
            consume_batch(b, x, cd, wv, all_rows);
        }
    }
}

struct DistinctTopkArgs {
    const uint64_t* table;  // [slots, n_groups]
    int64_t n_groups;
    const int* need;        // [slots]
    const int64_t* rows;    // NULL, or the row list the keys' positions index
    const int32_t* codes;
    int k;
    int64_t label_offset;
    float* D;               // [slots, k] the sub-tile's part of the call's output
    int64_t* I;
    int32_t* G;             // or NULL
};

// blockIdx.x: the slot.  Non-zero words are distinct keys (distinct positions).
__global__ __launch_bounds__(kDistinctThreads) void distinct_topk_kernel(DistinctTopkArgs a) {
    __shared__ uint64_t merge[(kDistinctWaves - 1) * kWave];
    const int qi = blockIdx.x;
    if (a.need[qi] == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t* tab = a.table + (int64_t)qi * a.n_groups;
    WaveTopK tk;
    tk.init(a.k);
    // (the bound is uniform over the wave: offer is wave-cooperative)
    for (int64_t base = (int64_t)(threadIdx.x - lane); base < a.n_groups; base += kDistinctThreads) {
        const int64_t i = base + lane;
        tk.offer(i < a.n_groups ? tab[i] : 0ull);
    }
    block_merge_topk(tk, merge, kDistinctWaves);
    if (threadIdx.x < a.k) {  // wave 0 (k <= 64): lane i holds the i-th best group
        const int64_t o = (int64_t)qi * a.k + threadIdx.x;
        if (tk.key) {
            const int64_t p = (int64_t)key_row(tk.key);
            const int64_t row = a.rows ? a.rows[p] : p;
            a.D[o] = key_score(tk.key);
            a.I[o] = row + a.label_offset;
            if (a.G) a.G[o] = a.codes[row];
        } else {
            a.D[o] = -3.402823466e+38f;
            a.I[o] = -1;
            if (a.G) a.G[o] = -1;
        }
    }
}

}  // namespace mvdb
