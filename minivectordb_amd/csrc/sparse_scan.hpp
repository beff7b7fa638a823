// sparse_scan.hpp — sparse vectors: every stored row holds a sparse vector beside its embedding, and a sparse query is scored
// against ALL of them in one CSR pass (include/mvdb.h "SPARSE VECTORS AND HYBRID SEARCH").  The score of row r is
//   acc = +0.0; for the row's entries in stored order whose index is in the query: acc = acc + (q[index] * value)
// every operation rounded on its own; matched[r] counts the entries used.  No reference counterpart (its
// hybrid_rerank_results takes a sparse cosine of the k rows a dense search has already returned).
//
// Layout.  The non-zeros of all rows, row after row, as 8-byte (index, value) entries — one 16-byte load brings two — behind
// them two padding entries whose index no query can hold; indptr [n + 1] as the caller's; and the TILE TABLE the host cut at
// creation: tile t covers the rows [tile_row[t], tile_row[t + 1]) and the entries [tile_ent[t], tile_ent[t + 1]), at most
// kSparseTileRows rows and kSparseSpan entries — a longer row has a tile of its own.  Work is balanced by non-zeros, and no
// launch waits for a device-side scan.
//
// One launch, sparse_scan_kernel<MODE, SEL>:
//   The query lives in LDS as an open-addressed table of kSparseSlots (index, value) slots, filled once per block: the home
//   slot of an index is ((index mod slots) * kSparseHashMul) mod slots — a bijection of the low bits, so a run of consecutive
//   indices (the head of a Zipf vocabulary) lands slots apart and linear probing stays short, while indices congruent modulo
//   the slot count share a home.  At most 1,024 query terms in 2,048 slots: a probe always ends at an empty slot.
//   A block takes tiles in a grid-stride loop.  Phase 1: the lanes stream the tile's entries, 16 bytes per lane and load, four
//   loads in flight per lane; each entry probes the table and leaves q[index] * value — or +0.0 — in the staging buffer and a
//   matched byte beside it.  Phase 2: one lane per row walks the row's staged products in order: acc = acc + p.  acc is never
//   -0.0 (it starts as +0.0, and a sum of two fp32 numbers is -0.0 only if both are), so adding the +0.0 of a skipped entry is
//   the same bits as skipping it.  A row longer than the span is staged chunk by chunk, its lane carrying acc across them.
//   MODE 0 writes T[r] = weight * acc (one more rounded multiply; weight 1 is the identity) and matched[r]; MODE 1 offers
//   (acc, r) of every selected row with matched >= 1 and acc == acc to the wave's sorted list (topk_device.hpp) and leaves one
//   list per block for merge_keys_kernel.  SEL 0: every row; SEL 2: a bitmap over the physical rows (a row list is turned into
//   one first, rows_to_mask_kernel) — an unselected row is never offered, the tile walk is the same.
// No floating-point atomics, no scratch.  LDS per block: table 16 KiB + products 16 KiB + matched bytes 4 KiB (+ 1.5 KiB of
// list merge space in MODE 1): four blocks per CU.
// Bytes: 8 per non-zero + 8 per row (indptr) (+ 4 or 8 per row written in MODE 0).
#pragma once
#include "topk_device.hpp"

namespace mvdb {

constexpr int kSparseThreads = 256;
constexpr int kSparseWaves = kSparseThreads / kWave;
constexpr int kSparseSpan = 4096;                  // most entries of a tile (a longer row: alone, in chunks)
constexpr int kSparseTileRows = kSparseThreads;    // most rows of a tile: one lane per row in phase 2
constexpr int kSparseSlots = 2048;                 // slots of the query table (a power of two)
constexpr int kSparseMaxQuery = 1024;              // most terms of a query: the table is never more than half full
constexpr int kSparseStage = kSparseSpan + 2;      // staged entries per chunk: a tile that starts at an odd entry is read from the even one before it
constexpr int kSparseBlocksPerCu = 4;
constexpr uint32_t kSparseHashMul = 1265u;         // odd, ~ slots / golden ratio
constexpr uint32_t kSparseEmpty = 0xFFFFFFFFu;     // index of an empty slot
constexpr uint32_t kSparsePadIndex = 0x7FFFFFFFu;  // index of the padding entries: dim <= 2^31 - 1, so no row or query holds it

struct SparseEntry {
    uint32_t index;
    uint32_t value;  // the fp32 bits
};
static_assert(sizeof(SparseEntry) == 8, "two entries per 16-byte load");

struct SparseScanArgs {
    const SparseEntry* entries;  // [nnz + 2], 16-byte aligned
    const int64_t* indptr;       // [n + 1]
    const int64_t* tile_row;     // [ntiles + 1]
    const int64_t* tile_ent;     // [ntiles + 1]
    int64_t ntiles;
    const int64_t* q_indptr;     // [nq + 1] (device): query y holds the terms [q_indptr[y], q_indptr[y + 1])
    const SparseEntry* q_terms;  // (index, value) of every query term
    float weight;                // MODE 0: T = weight * acc
    float* T;                    // MODE 0: [n]
    int32_t* matched;            // MODE 0: [n] or NULL
    const uint64_t* mask;        // SEL 2: bitmap over the rows [0, mask_rows)
    int64_t mask_rows;
    int k;                       // MODE 1: <= kMaxFusedK
    uint64_t* cand;              // MODE 1: [nq, gridDim.x, k] sorted block lists
};

__device__ __forceinline__ uint32_t sparse_home(uint32_t index) { return ((index & (kSparseSlots - 1)) * kSparseHashMul) & (kSparseSlots - 1); }

// the contract's two operations, never contracted (boost_scan.hpp: why the pragma and not the intrinsics)
__device__ __forceinline__ float sparse_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float sparse_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// rows[i] -> bit rows[i] of mask (zeroed by the caller); a row outside [0, n) is skipped
__global__ __launch_bounds__(256) void rows_to_mask_kernel(const int64_t* rows, int64_t m, int64_t n, unsigned long long* mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t r = rows[i];
    if (r < 0 || r >= n) return;
    atomicOr(mask + (r >> 6), 1ull << (r & 63));
}

template <int MODE, int SEL>
__global__ __launch_bounds__(kSparseThreads) void sparse_scan_kernel(SparseScanArgs a) {
    __shared__ SparseEntry tab[kSparseSlots];
    __shared__ float prod[kSparseStage];
    __shared__ unsigned char hit[kSparseStage];
    const int tid = threadIdx.x;
    const int qi = blockIdx.y;

    // ---- the query -> LDS table ----------------------------------------------------------------
    for (int i = tid; i < kSparseSlots; i += kSparseThreads) tab[i] = SparseEntry{kSparseEmpty, 0u};
    __syncthreads();
    {
        const int64_t q0 = a.q_indptr[qi];
        const int m = (int)(a.q_indptr[qi + 1] - q0);
        for (int i = tid; i < m && i < kSparseMaxQuery; i += kSparseThreads) {
            const SparseEntry e = a.q_terms[q0 + i];
            uint32_t slot = sparse_home(e.index);
            while (atomicCAS(&tab[slot].index, kSparseEmpty, e.index) != kSparseEmpty) slot = (slot + 1) & (kSparseSlots - 1);
            tab[slot].value = e.value;
        }
    }
    __syncthreads();

    // one entry: its product (or +0.0) and matched byte into staging slot i
    auto stage = [&](int i, uint32_t index, uint32_t value) {
        uint32_t slot = sparse_home(index);
        float p = 0.f;
        unsigned char h = 0;
        for (;;) {
            const SparseEntry e = tab[slot];
            if (e.index == index) {
                p = sparse_mul(__uint_as_float(e.value), __uint_as_float(value));
                h = 1;
                break;
            }
            if (e.index == kSparseEmpty) break;
            slot = (slot + 1) & (kSparseSlots - 1);
        }
        prod[i] = p;
        hit[i] = h;
    };

    WaveTopK tk;
    if (MODE == 1) tk.init(a.k);

    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t r0 = a.tile_row[t];
        const int nrows = (int)(a.tile_row[t + 1] - r0);
        const int64_t e0 = a.tile_ent[t], e1 = a.tile_ent[t + 1];
        const int64_t r = r0 + tid;
        const bool mine = tid < nrows;
        int64_t rb = 0, re = 0;
        bool selected = mine;
        if (mine) {
            rb = a.indptr[r];
            re = a.indptr[r + 1];
            if (SEL == 2) selected = r < a.mask_rows && ((a.mask[r >> 6] >> (r & 63)) & 1ull);
        }
        float acc = 0.f;
        int cnt = 0;
        for (int64_t c = e0 & ~(int64_t)1; c < e1; c += kSparseStage) {
            // ---- phase 1: stream the chunk's entries, two per lane and load ----------------------
            const int64_t left = e1 - c;
            const int pairs = (int)((left < kSparseStage ? left + 1 : (int64_t)kSparseStage) >> 1);
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4* src = reinterpret_cast<const u32x4*>(a.entries + c);
            for (int p0 = tid; p0 < pairs; p0 += 4 * kSparseThreads) {
                u32x4 w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int p = p0 + j * kSparseThreads;
                    if (p < pairs) w[j] = __builtin_nontemporal_load(src + p);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int p = p0 + j * kSparseThreads;
                    if (p < pairs) {
                        stage(2 * p, w[j].x, w[j].y);
                        stage(2 * p + 1, w[j].z, w[j].w);
                    }
                }
            }
            __syncthreads();
            // ---- phase 2: one lane per row, its products in stored order --------------------------
            if (mine) {
                const int lo = (int)((rb > c ? rb : c) - c);
                const int64_t cend = c + kSparseStage;
                const int hi = (int)((re < cend ? re : cend) - c);
                for (int i = lo; i < hi; ++i) {
                    acc = sparse_add(acc, prod[i]);
                    cnt += hit[i];
                }
            }
            __syncthreads();
        }
        if (MODE == 0) {
            if (mine) {
                a.T[r] = sparse_mul(a.weight, acc);
                if (a.matched) a.matched[r] = cnt;
            }
        } else {
            // the gate: selected, matched, and a score that is no NaN (a NaN fails the comparison)
            const bool pass = selected && cnt >= 1 && acc >= tk.thr_score;
            if (__ballot(pass)) tk.offer(pass ? make_key(acc, (uint32_t)r) : 0ull);
        }
    }

    if (MODE == 1) {
        __shared__ uint64_t sh[(kSparseWaves - 1) * kWave];
        block_merge_topk(tk, sh, kSparseWaves);
        if ((tid >> 6) == 0 && tid < a.k) a.cand[((int64_t)qi * gridDim.x + blockIdx.x) * a.k + tid] = tk.key;
    }
}

}  // namespace mvdb
