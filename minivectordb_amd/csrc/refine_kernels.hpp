// refine_kernels.hpp — kernels of the refine store (refine.hip; contract in include/mvdb.h "REFINE STORE").
//
// The store keeps every row as IEEE binary16, [n, d] with d a multiple of 8: a row is d / 8 chunks of 16 bytes.  A re-rank
// scores (query, candidate row) pairs — every row read meets exactly one query, a gathered GEMV, so there is nothing for the
// matrix cores to share — and keeps the k best per query.
//
//   refine_convert_kernel     fp32 rows -> binary16 rows (v_cvt_f16_f32: round to nearest even), one 16-byte store per thread;
//                             with a row list it scatters (set_rows).
//   refine_move_kernel        listed rows -> consecutive rows, one 16-byte chunk per thread (removal gathers the survivors).
//   refine_rerank_kernel<K>   one block per (query, slice of its list): one key per list slot, 0 where the slot names no row.
//   refine_merge_kernel       one block per query: the slots' keys -> the k best distinct ones -> D, I.
//
// The score of a pair.  Lane l of a wave owns chunks l, 64 + l, 128 + l, ... of the row (d < 512: lanes past d / 8 own none;
// d > 512: several passes, the last one part-filled — both by predicating the load, rows are never padded).  It folds its
// chunks, ascending, dimension by dimension into ONE fp32 accumulator with fmaf(q_i, float(x_i), acc) — v_fma_mix_f32 reads
// the binary16 operand as it is — and the 64 lane sums meet in a butterfly: xor 32, 16, 8, 4, 2, 1.  The order is a function of
// d alone, so a pair's score has the same bits whatever the call's nq, m, k, the slot or the slice.
#pragma once
#include <float.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kRefineMaxDim = 4096;
constexpr int kRefineMaxList = 1024;
constexpr int kRefineThreads = 256;
constexpr int kRefineWaves = kRefineThreads / kWave;
// Candidate rows a wave keeps in flight: their loads are independent 16-byte gathers, issued together.  A first guess, not swept.
constexpr int kRefineRows = 4;
constexpr int kRefineSlots = kRefineWaves * kRefineRows;  // list slots one block takes per round

typedef _Float16 rf_f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t rf_u32x4 __attribute__((ext_vector_type(4)));

// ---- rows in, rows moved -----------------------------------------------------------------------------------------------------
// x [n, d] fp32 -> row j of dst (rows == nullptr) or row rows[j] (distinct and in range: checked on the host).  Thread i takes
// chunk i of x: eight floats in, one 16-byte store out.  Overflow rounds to +-inf, subnormals are kept, NaN stays NaN.
__global__ __launch_bounds__(256) void refine_convert_kernel(const float* __restrict__ x, int64_t n, int chunks,
                                                             const int64_t* __restrict__ rows, rf_u32x4* __restrict__ dst) {
    const int64_t total = n * chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = ((const float4*)x)[2 * i], b = ((const float4*)x)[2 * i + 1];
        const rf_f16x8 h = {(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w,
                            (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
        const int64_t j = i / chunks;
        const int64_t r = rows ? rows[j] : j;
        dst[r * chunks + (i - j * chunks)] = (rf_u32x4)h;
    }
}

// row from[j] of src -> row j of dst
__global__ __launch_bounds__(256) void refine_move_kernel(const rf_u32x4* __restrict__ src, const int64_t* __restrict__ from,
                                                          int64_t m, int chunks, rf_u32x4* __restrict__ dst) {
    const int64_t total = m * chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = i / chunks;
        dst[i] = src[from[j] * chunks + (i - j * chunks)];
    }
}

// ---- re-rank -----------------------------------------------------------------------------------------------------------------
struct RefineRerankArgs {
    const uint16_t* rows;   // [n, d] binary16
    int64_t n;
    int d;
    const float* q;         // [nq, d]
    const void* list;       // [nq, m]: int64 row numbers, or (KEYS) top-k keys of a scan — 0: none, else key_row names the row
    int m;
    int per_block;          // list slots per block: a multiple of kRefineSlots
    uint64_t* scored;       // [nq, m]: make_key(S, row) per slot, 0 where the slot is no candidate
};

// grid (slices, nq).  The query goes into LDS as fp32 once per block; a wave then takes kRefineRows slots per round.  A slot's
// row number is checked BEFORE anything is formed from it: a value outside [0, n) — the -1 of a short list, a stale or foreign
// id — turns the slot's loads off and its key into 0.
template <bool KEYS>
__global__ __launch_bounds__(kRefineThreads) void refine_rerank_kernel(RefineRerankArgs a) {
    __shared__ float4 qsh[kRefineMaxDim / 4];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.y;
    const int chunks = a.d >> 3;
    const float4* qsrc = (const float4*)(a.q + (int64_t)qi * a.d);
    for (int i = threadIdx.x; i < 2 * chunks; i += kRefineThreads) qsh[i] = qsrc[i];
    __syncthreads();

    const int s0 = blockIdx.x * a.per_block;
    const int s1 = min(a.m, s0 + a.per_block);
    const int64_t base = (int64_t)qi * a.m;
    for (int g = s0 + wave * kRefineRows; g < s1; g += kRefineSlots) {  // (wave-uniform)
        bool ok[kRefineRows];
        uint32_t id[kRefineRows];
        const rf_u32x4* row[kRefineRows];
        float acc[kRefineRows];
#pragma unroll
        for (int r = 0; r < kRefineRows; ++r) {
            int64_t c = -1;
            if (g + r < s1) {
                if (KEYS) {
                    const uint64_t key = ((const uint64_t*)a.list)[base + g + r];
                    c = key ? (int64_t)key_row(key) : -1;
                } else {
                    c = ((const int64_t*)a.list)[base + g + r];
                }
            }
            ok[r] = c >= 0 && c < a.n;
            id[r] = ok[r] ? (uint32_t)c : 0u;
            row[r] = (const rf_u32x4*)(a.rows + (int64_t)id[r] * a.d);
            acc[r] = 0.0f;
        }
#pragma unroll 2
        for (int c0 = 0; c0 < chunks; c0 += kWave) {
            const int c = c0 + lane;
            const bool on = c < chunks;
            const rf_u32x4 z = {0u, 0u, 0u, 0u};
            rf_u32x4 x[kRefineRows];
#pragma unroll
            for (int r = 0; r < kRefineRows; ++r) x[r] = (on && ok[r]) ? __builtin_nontemporal_load(row[r] + c) : z;
            const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4 qa = on ? qsh[2 * c] : z4, qb = on ? qsh[2 * c + 1] : z4;
            const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
            for (int r = 0; r < kRefineRows; ++r) {
                const rf_f16x8 h = (rf_f16x8)x[r];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r] = fmaf(qv[j], (float)h[j], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kRefineRows; ++r) {
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) acc[r] += __shfl_xor(acc[r], off, kWave);
            if (lane == r && g + r < s1) a.scored[base + g + r] = (ok[r] && acc[r] == acc[r]) ? make_key(acc[r], id[r]) : 0ull;
        }
    }
}

// WaveTopK::offer for lists that may name a row twice: a pair's score is a function of the pair, so the second mention makes
// the very key the first one made, and a key the list already holds is dropped.  (One the list has let go lies below its
// threshold and never comes back.)
__device__ __forceinline__ void refine_offer_distinct(WaveTopK& tk, uint64_t cand) {
    uint64_t todo = __ballot(cand > tk.thr);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t kn = readlane_u64(cand, src);
        if (__ballot(tk.key == kn) != 0ull) continue;
        tk.insert_uniform(kn);
    }
}

// One block per query.  Wave w reads every slot and offers the keys of rows with row % 4 == w, so equal keys always meet in
// one wave's list and block_merge_topk folds lists that share none.  Missing slots: I = -1, D = -FLT_MAX.
__global__ __launch_bounds__(kRefineThreads) void refine_merge_kernel(const uint64_t* __restrict__ scored, int m, int k,
                                                                      float* __restrict__ D, int64_t* __restrict__ I) {
    __shared__ uint64_t sh[(kRefineWaves - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const uint64_t* src = scored + (int64_t)qi * m;
    WaveTopK tk;
    tk.init(k);
    for (int i0 = 0; i0 < m; i0 += kWave) {
        const uint64_t key = i0 + lane < m ? src[i0 + lane] : 0ull;
        refine_offer_distinct(tk, (key_row(key) & (kRefineWaves - 1)) == (uint32_t)wave ? key : 0ull);
    }
    block_merge_topk(tk, sh, kRefineWaves);
    if (wave == 0 && lane < k) {
        const int64_t o = (int64_t)qi * k + lane;
        D[o] = tk.key ? key_score(tk.key) : -FLT_MAX;
        I[o] = tk.key ? (int64_t)key_row(tk.key) : -1;
    }
}

}  // namespace mvdb
