// pq_kernels.hpp — kernels of the product-quantised index (pq.hip; contract in include/mvdb.h "product-quantised index" and
// INTEGRATION.md 3v).
//
// A row is M code bytes — 1 to 16 chunks of 16 —, byte m naming one of 256 centroids of sub-space m (dsub = d / M floats).  A
// query becomes a table u[m][c] of 16-bit integers plus (step, bias); the score of a row is the INTEGER S = sum_m u[m][code[m]]
// <= 256 * 65535 < 2^24, so -(float)S is exact and topk_device.hpp's key orders candidates "smaller S first, then the lower
// row": WaveTopK and block_merge_topk serve as they stand, and every form returns the same bits.
//
//   pq_lut_kernel     queries -> tables, ONE launch per call: blocks over (slab of sub-spaces, query) form t[m][c] in fp32 and
//                     the per-m extremes; the last block of a query to finish derives (step, bias) and quantises.
//   pq_scan_kernel    the ADC scan: the pass's interleaved table in LDS for the whole launch, G lanes per row, 16-byte
//                     non-temporal row loads, ONE LDS read per code byte for 1, 2 or 4 queries.
//   pq_merge_kernel   the blocks' partial lists -> S (int32), D (fp32), I (int64 rows).
//   pq_encode_kernel  fp32 rows -> codes (add, and the assign step of training).
//   pq_update_kernel  Lloyd's update, one block per centroid, fp64 in a fixed order.
#pragma once
#include <float.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kPqThreads = 256;         // lut, merge, encode, update: thread c <-> centroid c, or thread r <-> tile row r
constexpr int kPqScanMaxThreads = 1024; // the scan's block: 4, 8 or 16 waves, by what the table leaves of the LDS
constexpr int kPqCentroids = 256;
constexpr int kPqMaxM = 256;
constexpr int kPqScanU = 4;             // row batches in flight per wave (a first guess, as the binary scan's)
constexpr int32_t kPqNoScore = 0x7FFFFFFF;

// sub-spaces per block of the table launch: 16 * dsub floats of the query, at most 32
__host__ __device__ constexpr int pq_lut_slab(int dsub) { return dsub <= 2 ? 16 : 32 / dsub; }

typedef int pq_i32x4 __attribute__((ext_vector_type(4)));

// the binary index's device for an integer distance: the key's score is -(float)S, exact below 2^24
__device__ __forceinline__ uint64_t pq_key(int s, uint32_t row) { return make_key(-(float)s, row); }
__device__ __forceinline__ int32_t pq_key_score(uint64_t key) { return (int32_t)(-key_score(key)); }

// ---- the query table -------------------------------------------------------------------------------------------------------
struct PqLutArgs {
    const float* q;     // [nq, d]
    const float* cb;    // [M, 256, dsub]
    int d, M, dsub, lg_dsub, metric, nq;
    int NQ;             // queries of a pass: the table is lut[pass][m][c][NQ], the query fastest
    int nslab;          // M / pq_lut_slab(dsub) = gridDim.x
    float* t;           // [nq, M, 256] fp32 entries on their way to the quantiser
    float* lo;          // [nq, M] min_c t
    float* hi;          // [nq, M] max_c t
    int* bad;           // [nq, nslab] a non-finite entry seen
    int* ticket;        // [nq] blocks of the query that have finished; zero between launches
    uint16_t* lut;
    float* step;        // [nq]
    float* bias;        // [nq]
    int* valid;         // [nq] 0: the table holds a non-finite value, the query returns padding
};

__device__ __forceinline__ float pq_wave_min(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ float pq_wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// grid (nslab, nq), 256 threads.  Per sub-space of the slab the codebook cb[m] goes through LDS — coalesced in, row stride
// dsub | 1 words so that thread c reads centroid c off the other threads' banks —, thread c forms t[m][c] against the query's
// sub-vector (an LDS broadcast) and the block reduces min and max.  Then the blocks of a query take a ticket: the last one sees
// every t, lo and hi of the query (fence, atomic, fence) and does the second step — span over m, step, bias in ascending m,
// the quantising sweep into the interleaved table — and leaves the ticket at zero for the next launch.
__global__ __launch_bounds__(kPqThreads) void pq_lut_kernel(PqLutArgs a) {
    __shared__ float cbs[kPqCentroids * 33];
    __shared__ float qs[32];
    __shared__ float red[2][16][kPqThreads / kWave];
    __shared__ float fin[kPqThreads / kWave];
    __shared__ float sbias;
    __shared__ int slast;
    const int c = threadIdx.x, lane = c & (kWave - 1), wave = c >> 6;
    const int slab = blockIdx.x, qi = blockIdx.y;
    const int MS = pq_lut_slab(a.dsub);
    const int m0 = slab * MS;
    const int ls = a.dsub | 1;
    const bool ip = a.metric == MVDB_METRIC_IP;
    if (c < MS * a.dsub) qs[c] = a.q[(int64_t)qi * a.d + m0 * a.dsub + c];
    int bad = 0;
    for (int mi = 0; mi < MS; ++mi) {
        const int m = m0 + mi;
        __syncthreads();
        const float* src = a.cb + (int64_t)m * kPqCentroids * a.dsub;
        for (int i = c; i < kPqCentroids * a.dsub; i += kPqThreads) cbs[(i >> a.lg_dsub) * ls + (i & (a.dsub - 1))] = src[i];
        __syncthreads();
        float acc = 0.f;
        for (int j = 0; j < a.dsub; ++j) {
            const float x = cbs[c * ls + j], qv = qs[mi * a.dsub + j];
            const float diff = qv - x;
            acc = ip ? fmaf(qv, x, acc) : fmaf(diff, diff, acc);
        }
        const float t = ip ? -acc : acc;
        bad |= !(fabsf(t) <= FLT_MAX);
        a.t[((int64_t)qi * a.M + m) * kPqCentroids + c] = t;
        const float mn = pq_wave_min(t), mx = pq_wave_max(t);
        if (lane == 0) {
            red[0][mi][wave] = mn;
            red[1][mi][wave] = mx;
        }
    }
    bad = __syncthreads_or(bad);
    if (c < MS) {
        a.lo[(int64_t)qi * a.M + m0 + c] = fminf(fminf(red[0][c][0], red[0][c][1]), fminf(red[0][c][2], red[0][c][3]));
        a.hi[(int64_t)qi * a.M + m0 + c] = fmaxf(fmaxf(red[1][c][0], red[1][c][1]), fmaxf(red[1][c][2], red[1][c][3]));
    }
    if (c == 0) a.bad[(int64_t)qi * a.nslab + slab] = bad;
    __threadfence();
    __syncthreads();
    if (c == 0) slast = atomicAdd(&a.ticket[qi], 1) == a.nslab - 1;
    __syncthreads();
    if (!slast) return;
    __threadfence();

    // the last block of query qi: lo[m] -> cbs[m], span = max_m (hi - lo), bias = sum_m lo (ascending m)
    const float l = c < a.M ? a.lo[(int64_t)qi * a.M + c] : 0.f;
    float sp = c < a.M ? a.hi[(int64_t)qi * a.M + c] - l : 0.f;
    cbs[c] = l;
    int anybad = c < a.nslab ? a.bad[(int64_t)qi * a.nslab + c] : 0;
    sp = pq_wave_max(sp);
    if (lane == 0) fin[wave] = sp;
    __syncthreads();
    const float span = fmaxf(fmaxf(fin[0], fin[1]), fmaxf(fin[2], fin[3]));
    anybad = __syncthreads_or(anybad | !(span <= FLT_MAX));
    if (c == 0) {
        float b = 0.f;
        for (int m = 0; m < a.M; ++m) b += cbs[m];
        sbias = b;
    }
    __syncthreads();
    const float step = span == 0.f ? 1.f : span / 65535.f;
    if (c == 0) {
        a.step[qi] = step;
        a.bias[qi] = sbias;
        a.valid[qi] = !anybad && fabsf(sbias) <= FLT_MAX;
        a.ticket[qi] = 0;
    }
    const int pass = qi / a.NQ, ql = qi - pass * a.NQ;
    uint16_t* out = a.lut + (int64_t)pass * a.M * kPqCentroids * a.NQ + ql;
    const float* tq = a.t + (int64_t)qi * a.M * kPqCentroids;
    for (int i = c; i < a.M * kPqCentroids; i += kPqThreads) {
        const float u = fminf(65535.f, rintf((tq[i] - cbs[i >> 8]) / step));
        out[(int64_t)i * a.NQ] = anybad ? (uint16_t)0 : (uint16_t)u;
    }
}

// ---- the scan --------------------------------------------------------------------------------------------------------------
struct PqScanArgs {
    const uint8_t* codes;   // [n, M]
    int nchunk;             // M / 16
    int M;
    int64_t n;
    const uint64_t* mask;   // nullptr: every row; else bit r & 63 of word r >> 6 set = row r selected
    const uint16_t* lut;    // [gridDim.y][M][256][NQ]
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k] keys
};

__host__ __device__ constexpr size_t pq_table_bytes(int M, int NQ) { return (size_t)NQ * M * kPqCentroids * sizeof(uint16_t); }
__host__ __device__ constexpr size_t pq_scan_lds_bytes(int M, int NQ, int nwaves) {
    return pq_table_bytes(M, NQ) + (size_t)(nwaves > 1 ? nwaves - 1 : 1) * kWave * sizeof(uint64_t);
}

__device__ __forceinline__ uint4 pq_load16(const uint8_t* p) {
    const pq_i32x4 v = __builtin_nontemporal_load((const pq_i32x4*)p);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
}

template <int CTRL>
__device__ __forceinline__ int pq_dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// The sum over the G <= 16 lanes of a row, left in every one of them — the binary scan's steps inside a DPP row of 16 lanes:
// xor 1 and xor 2 as quad permutations; once the quads (the halves) are uniform, the mirror of the half row (the row) reads
// the other quad (half).
template <int G>
__device__ __forceinline__ int pq_group_sum(int s) {
    if (G >= 2) s = pq_dpp_add<0xB1>(s);    // quad_perm [1, 0, 3, 2]
    if (G >= 4) s = pq_dpp_add<0x4E>(s);    // quad_perm [2, 3, 0, 1]
    if (G >= 8) s = pq_dpp_add<0x141>(s);   // row_half_mirror
    if (G >= 16) s = pq_dpp_add<0x140>(s);  // row_mirror
    return s;
}

// ONE LDS read per code byte: the NQ 16-bit entries of (m, c) lie side by side — ds_read_u16, ds_read_b32 or ds_read_b64
template <int NQ>
__device__ __forceinline__ void pq_lookup(const unsigned char* p, uint32_t (&acc)[NQ]) {
    if constexpr (NQ == 1) {
        acc[0] += *(const uint16_t*)p;
    } else if constexpr (NQ == 2) {
        const uint32_t x = *(const uint32_t*)p;
        acc[0] += x & 0xFFFFu;
        acc[1] += x >> 16;
    } else {
        const uint2 x = *(const uint2*)p;
        acc[0] += x.x & 0xFFFFu;
        acc[1] += x.x >> 16;
        acc[2] += x.y & 0xFFFFu;
        acc[3] += x.y >> 16;
    }
}

// blockDim.x = 64 * (4 | 8 | 16); blockIdx.y: the pass, queries [NQ blockIdx.y, NQ blockIdx.y + NQ).  The binary scan's lane
// layout: G lanes per row, lane t of the group holds the row's 16-byte chunk t — sub-spaces [16 t, 16 t + 16) — and lanes with
// t >= nchunk load nothing (3 chunks of 4: M = 48); a wave takes tiles of U * 64 / G consecutive rows with U loads in flight,
// the grid strides over the tiles.  Entry (m, c) of the pass's table is at byte (m * 256 + c) * 2 NQ of the LDS; the lane's
// 16 t * 256 * 2 NQ is folded into its base pointer and j * 256 * 2 NQ into the read's offset field.
template <int G, int U, int NQ>
__global__ __launch_bounds__(kPqScanMaxThreads) void pq_scan_kernel(PqScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_lds[];
    constexpr int R = kWave / G;
    constexpr uint32_t kEntry = 2 * NQ;
    const int NW = blockDim.x >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane & (G - 1);
    const int grp = lane / G;
    const int q0 = blockIdx.y * NQ;
    const bool live = t < a.nchunk;
    const int64_t rb = a.M;

    const uint32_t tab16 = (uint32_t)(pq_table_bytes(a.M, NQ) / 16);
    const uint4* src = (const uint4*)(a.lut + (int64_t)blockIdx.y * a.M * kPqCentroids * NQ);
    for (uint32_t i = threadIdx.x; i < tab16; i += blockDim.x) ((uint4*)pq_lds)[i] = src[i];
    uint64_t* sh = (uint64_t*)(pq_lds + (size_t)tab16 * 16);
    __syncthreads();
    const unsigned char* tab = pq_lds + (live ? t : 0) * (16 * kPqCentroids * kEntry);

    WaveTopK tk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) tk[q].init(a.k);

    const int64_t stride = (int64_t)gridDim.x * NW * (R * U);
    for (int64_t base = ((int64_t)blockIdx.x * NW + wave) * (R * U); base < a.n; base += stride) {
        uint4 v[U];
        uint64_t mw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool in = row < a.n;
            v[u] = (live && in) ? pq_load16(a.codes + row * rb + t * 16) : make_uint4(0, 0, 0, 0);
            mw[u] = !in ? 0ull : (a.mask ? a.mask[row >> 6] : ~0ull);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool lead = t == 0 && ((mw[u] >> (row & 63)) & 1ull);
            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t acc[NQ] = {};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t byte = (w[j >> 2] >> (8 * (j & 3))) & 255u;
                pq_lookup<NQ>(tab + (j * kPqCentroids + byte) * kEntry, acc);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int s = pq_group_sum<G>(live ? (int)acc[q] : 0);
                tk[q].offer(lead && q0 + q < a.nq ? pq_key(s, (uint32_t)row) : 0ull);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        block_merge_topk(tk[q], sh, NW);
        if (wave == 0 && q0 + q < a.nq && lane < a.k)
            a.cand[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * a.k + lane] = tk[q].key;
        __syncthreads();
    }
}

// ---- merge and housekeeping ------------------------------------------------------------------------------------------------
// L2: D = (float)(bias + step * S) in fp64, ascending; IP: that value negated — an estimate of q.x —, descending
__device__ __forceinline__ float pq_distance(int32_t s, float step, float bias, int metric) {
    const double v = (double)bias + (double)step * (double)s;
    return (float)(metric == MVDB_METRIC_IP ? -v : v);
}
__device__ __forceinline__ float pq_missing(int metric) { return metric == MVDB_METRIC_IP ? -FLT_MAX : FLT_MAX; }

// One block per query: the nlists partial lists -> sorted top-k; missing slots (and every slot of a query whose table is not
// finite) I = -1, S = INT32_MAX, D = +-FLT_MAX.
__global__ __launch_bounds__(kPqThreads) void pq_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k, int metric,
                                                              const float* __restrict__ step, const float* __restrict__ bias,
                                                              const int* __restrict__ valid, float* __restrict__ D,
                                                              int64_t* __restrict__ I, int32_t* __restrict__ S) {
    constexpr int NW = kPqThreads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const uint64_t* src = cand + (int64_t)qi * nlists * k;
    WaveTopK tk;
    tk.init(k);
    const int64_t total = (int64_t)nlists * k;
    for (int64_t i0 = (int64_t)wave * kWave; i0 < total; i0 += (int64_t)NW * kWave) {
        const int64_t i = i0 + lane;
        tk.offer(i < total ? src[i] : 0ull);
    }
    block_merge_topk(tk, sh, NW);
    if (wave == 0 && lane < k) {
        const int64_t o = (int64_t)qi * k + lane;
        const bool hit = tk.key != 0ull && valid[qi];
        const int32_t s = hit ? pq_key_score(tk.key) : kPqNoScore;
        D[o] = hit ? pq_distance(s, step[qi], bias[qi], metric) : pq_missing(metric);
        I[o] = hit ? (int64_t)key_row(tk.key) : -1;
        if (S) S[o] = s;
    }
}

__global__ void pq_fill_missing_kernel(float* D, int64_t* I, int32_t* S, int64_t total, int metric) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = pq_missing(metric);
        I[i] = -1;
        if (S) S[i] = kPqNoScore;
    }
}

// removal: dst row j <- src row keep[j], out of place, one 16-byte chunk per thread
__global__ __launch_bounds__(256) void pq_gather_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ keep,
                                                        int64_t m, int nchunk, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    ((uint4*)dst)[j * nchunk + ch] = ((const uint4*)src)[keep[j] * nchunk + ch];
}

__global__ void pq_zero_kernel(int* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---- encoding --------------------------------------------------------------------------------------------------------------
// A block takes a tile of 256 rows, thread r row r of the tile.  Per sub-space m the 256 centroids of cb[m] are staged in LDS
// (256 * DSUB floats, at most 32 KiB) and every thread walks them at the SAME address — a broadcast, no bank conflicts — against
// its own sub-vector in registers: sum_j (x_j - cb_j)^2 by fused multiply-adds in ascending j, the running minimum kept with <
// (ties to the lower c; a distance that is NaN never enters, so an all-NaN sub-vector keeps code 0).  Sixteen codes are
// gathered in four registers and leave as ONE 16-byte store.
template <int DSUB>
__global__ __launch_bounds__(kPqThreads) void pq_encode_kernel(const float* __restrict__ x, int64_t n, int M,
                                                               const float* __restrict__ cb, uint8_t* __restrict__ codes) {
    __shared__ __attribute__((aligned(16))) float cbs[kPqCentroids * DSUB];
    const int64_t row = (int64_t)blockIdx.x * kPqThreads + threadIdx.x;
    const bool in = row < n;
    const float* xr = x + (in ? row : 0) * ((int64_t)M * DSUB);
    uint4 w = make_uint4(0, 0, 0, 0);
    for (int m = 0; m < M; ++m) {
        __syncthreads();
        const float* src = cb + (int64_t)m * kPqCentroids * DSUB;
        for (int i = threadIdx.x; i < kPqCentroids * DSUB; i += kPqThreads) cbs[i] = src[i];
        __syncthreads();
        float xs[DSUB];
#pragma unroll
        for (int j = 0; j < DSUB; ++j) xs[j] = xr[m * DSUB + j];
        float best = INFINITY;
        uint32_t bc = 0;
        for (int c = 0; c < kPqCentroids; ++c) {
            float dist = 0.f;
#pragma unroll
            for (int j = 0; j < DSUB; ++j) {
                const float diff = xs[j] - cbs[c * DSUB + j];
                dist = fmaf(diff, diff, dist);
            }
            if (dist < best) {
                best = dist;
                bc = (uint32_t)c;
            }
        }
        const uint32_t placed = bc << (8 * (m & 3));
        const int word = (m >> 2) & 3;
        w.x |= word == 0 ? placed : 0u;
        w.y |= word == 1 ? placed : 0u;
        w.z |= word == 2 ? placed : 0u;
        w.w |= word == 3 ? placed : 0u;
        if ((m & 15) == 15) {
            if (in) *(uint4*)(codes + row * M + (m - 15)) = w;
            w = make_uint4(0, 0, 0, 0);
        }
    }
}

// ---- training: Lloyd's update ----------------------------------------------------------------------------------------------
// One block per (m, c) = (blockIdx.x >> 8, blockIdx.x & 255).  Thread t walks rows [t slice, t slice + slice) of the sample's
// code column m and adds the sub-vectors of the rows coded c in fp64, in row order; the 256 partials meet in LDS and thread j
// < DSUB adds component j in thread order, divides by the count in fp64 and rounds to fp32.  A centroid without members keeps
// its value.  The order is fixed and there are no floating-point atomics: the rule mvdb_index_kmeans follows.
template <int DSUB>
__global__ __launch_bounds__(kPqThreads) void pq_update_kernel(const float* __restrict__ x, const uint8_t* __restrict__ codes,
                                                               int64_t n, int M, float* __restrict__ cb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pq_upd_lds[];
    double* part = (double*)pq_upd_lds;                 // [256][DSUB]
    int* counts = (int*)(part + kPqThreads * DSUB);     // [256]
    const int m = blockIdx.x >> 8;
    const uint32_t c = blockIdx.x & 255;
    const int t = threadIdx.x;
    const int64_t slice = (n + kPqThreads - 1) / kPqThreads;
    const int64_t i0 = (int64_t)t * slice, i1 = i0 + slice < n ? i0 + slice : n;
    const int64_t d = (int64_t)M * DSUB;
    double acc[DSUB];
#pragma unroll
    for (int j = 0; j < DSUB; ++j) acc[j] = 0.0;
    int cnt = 0;
    for (int64_t i = i0; i < i1; ++i) {
        if (codes[i * M + m] != c) continue;
        const float* p = x + i * d + m * DSUB;
#pragma unroll
        for (int j = 0; j < DSUB; ++j) acc[j] += (double)p[j];
        ++cnt;
    }
#pragma unroll
    for (int j = 0; j < DSUB; ++j) part[t * DSUB + j] = acc[j];
    counts[t] = cnt;
    __syncthreads();
    if (t < DSUB) {
        double s = 0.0;
        int64_t total = 0;
        for (int tt = 0; tt < kPqThreads; ++tt) {
            s += part[tt * DSUB + t];
            total += counts[tt];
        }
        if (total > 0) cb[((int64_t)m * kPqCentroids + c) * DSUB + t] = (float)(s / (double)total);
    }
}

}  // namespace mvdb
