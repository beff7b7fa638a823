// grouped_scan.hpp — the gathered scan for a batch of queries in which EVERY QUERY HAS ITS OWN ROW LIST
// (mvdb_index_search_grouped): one launch over "work items", one segmented merge.
//
// An item is (query qi, positions [begin, end) of that query's row list).  One 256-thread block takes one item; block ->
// item is blockIdx.x, nothing is searched on the device.  The host cuts the lists into items (mvdb.hip, plan_grouped_items)
// so that a short list is one item and a long list is many: one 5M-row filter beside 63 small ones does not serialise
// the launch.
//
// Roofline: HBM, gather.  Algorithmic bytes per launch = sum over the queries of m_i * (ld * 4 + 8): every listed row
// once, plus its 8-byte id.
//
// The per-row arithmetic is flat_scan_kernel's (scan_kernels.hpp), restated instruction for instruction for the same
// (G, C, MASKED, METRIC): lane t of the row's G lanes takes chunks t, t + G, ..., C x 4 fmaf in chunk order, then the
// G/2 ... 1 xor butterfly, negation for L2.  The score of a (query, row) pair is a function of that shape alone — not of the
// grid, of U, or of the rows that share the launch — and selection is by 64-bit (score, position in the list) keys, so a
// query's result is bit for bit what the single-query row-list scan returns for it (tests/test_grouped_gpu.py).
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

struct GroupedQuery {
    const int64_t* rows;  // the query's row list (device), NULL iff m == 0
    int64_t m;            // its length; < 0: the query is not part of the grouped launch (no items, its result row is left alone)
    int first_item;       // the query's items are [first_item, next query's first_item)
    int pad_;
};
struct GroupedItem {
    int q;                // query of the call
    uint32_t begin, end;  // positions of the query's list (end > begin)
    uint32_t pad_;
};

struct GroupedScanArgs {
    const float* X;   // [n_phys, ld] corpus
    int64_t ld;       // row stride in floats (multiple of 4)
    int d4;           // valid 16-B chunks per row
    const float* q;   // [nq, ld] queries (device), zero padded
    int normalize_q;  // L2-normalise the query in the prologue
    int k;            // <= kMaxFusedK
    const GroupedItem* items;     // [gridDim.x]
    const GroupedQuery* queries;  // [nq + 1] (the last entry carries first_item = number of items)
    uint64_t* cand;               // [gridDim.x, k] one sorted list per item
};

template <int G, int C, int U, int METRIC, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void grouped_scan_kernel(GroupedScanArgs a) {
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction

    // the item: block-uniform, read through the scalar cache
    const GroupedItem it = a.items[blockIdx.x];
    const int qi = it.q;
    const int64_t* __restrict__ rows = a.queries[qi].rows;
    const int64_t begin = it.begin;
    const int64_t m = (int64_t)it.end - begin;  // > 0 by construction

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

    // physical rows of the item's batch b: one 8-byte load per row through the list (clamped: tail lanes re-read the item's
    // last row, result discarded — never a position outside [begin, end))
    auto batch_rows = [&](int64_t b, int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            pr[u] = rows[begin + r];
        }
    };
    auto load_batch = [&](const int64_t (&pr)[U], f32x4 (&x)[U][C]) {
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
    };
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C]) {
        const int64_t row0 = b * RB + g;
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (METRIC == 0) {
                    acc = fmaf(x[u][c].x, qv[c].x, acc);
                    acc = fmaf(x[u][c].y, qv[c].y, acc);
                    acc = fmaf(x[u][c].z, qv[c].z, acc);
                    acc = fmaf(x[u][c].w, qv[c].w, acc);
                } else {
                    const f32x4 df = qv[c] - x[u][c];
                    acc = fmaf(df.x, df.x, acc);
                    acc = fmaf(df.y, df.y, acc);
                    acc = fmaf(df.z, df.z, acc);
                    acc = fmaf(df.w, df.w, acc);
                }
            }
            s[u] = acc;
        }
#pragma unroll
        for (int mm = G / 2; mm >= 1; mm >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], mm);
        }
        if (METRIC != 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = -s[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            // the key carries the position in the QUERY's list (ties: lowest position first, as the single-query scan)
            const bool pass = (t == 0) && (r < m) && (s[u] >= tk.thr_score);
            if (__ballot(pass)) tk.offer(pass ? make_key(s[u], (uint32_t)(begin + r)) : 0ull);
        }
    };

    // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
    int64_t pr[U], pn[U];
    if (wave < nbatches) batch_rows(wave, pr);
    for (int64_t b = wave; b < nbatches; b += kScanWaves) {
        f32x4 x[U][C];
        load_batch(pr, x);
        const int64_t bn = b + kScanWaves;
        batch_rows(bn < nbatches ? bn : b, pn);
        consume_batch(b, x);
#pragma unroll
        for (int u = 0; u < U; ++u) pr[u] = pn[u];
    }

    __shared__ uint64_t sh[(kScanWaves - 1) * kWave];
    block_merge_topk(tk, sh, kScanWaves);
    if (wave == 0 && lane < a.k) a.cand[(int64_t)blockIdx.x * a.k + lane] = tk.key;
}

// ---- second stage: merge the k-lists of each query's items and emit (D, I) ---------------------------------------------
// grid = (nq), block = 1024.  merge_keys_kernel for a variable number of lists per query; labels are mapped here:
// I = rows_qi[position] + label_offset.  A query without items (an empty list) gets a fully missing row.
struct MergeSegArgs {
    const uint64_t* keys;         // [items, k]
    const GroupedQuery* queries;  // [nq + 1]
    int k;
    int metric;
    int64_t label_offset;
    float* D;    // [nq, k]
    int64_t* I;  // [nq, k]
};

__global__ __launch_bounds__(kMergeThreads) void merge_keys_seg_kernel(MergeSegArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const GroupedQuery gq = a.queries[qi];
    if (gq.m < 0) return;  // not a query of the grouped launch (its set is a bitmap or NULL: answered by its own scan)
    const int item0 = gq.first_item;
    const int64_t total = (int64_t)(a.queries[qi + 1].first_item - item0) * a.k;
    const uint64_t* src = a.keys + (int64_t)item0 * a.k;
    WaveTopK tk;
    tk.init(a.k);
    for (int64_t base = (int64_t)wave * kWave * kMergeUnroll; base < total;
         base += (int64_t)kMergeThreads * kMergeUnroll) {
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
        float d;
        int64_t id;
        if (key) {
            const float s = key_score(key);
            d = a.metric == 0 ? s : -s;
            id = gq.rows[key_row(key)] + a.label_offset;  // key != 0 only for positions < m of a non-empty list
        } else {  // faiss convention for missing results
            d = a.metric == 0 ? -3.402823466e+38f : 3.402823466e+38f;
            id = -1;
        }
        a.D[(int64_t)qi * a.k + lane] = d;
        a.I[(int64_t)qi * a.k + lane] = id;
    }
}

}  // namespace mvdb
