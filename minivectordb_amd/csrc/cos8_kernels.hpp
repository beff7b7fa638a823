// cos8_kernels.hpp — kernels of the int8 cosine index (cos8.hip; contract in include/mvdb.h and INTEGRATION.md).
//
// A row is `stride` bytes of int8 codes (d rounded up to 16 bytes, zero padded) plus its int32 a2 = sum code^2.  The
// scan reads each row as 16-byte chunks: a GROUP of G lanes (G = the power of two >= chunks per row, at most 64) takes
// one row, lane t of the group chunk t (+ 64 c for c < NCH when a row has more than 64 chunks), so a wave covers 64 / G
// rows per step.  The query chunks a lane needs sit in its registers for the whole scan — Q queries per corpus pass.
// Products are v_dot4c_i32_i8 (exact int32), summed over the group by xor shuffles: the sum does not depend on the
// order, so every batch shape returns what a single query returns.
//
// The exact distance costs an fp64 division and square root; it is computed only for a (query, row) pair whose fp32
// estimate lies within 1e-5 of the query's current k-th distance (the estimate's error is below 1e-6), or where a zero
// makes the estimate meaningless.  Top-k keys are topk_device.hpp's with score = -distance: negation is exact and the
// key order puts ties on the lower row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kCos8Threads = 256;
constexpr int kCos8MaxChunks = 256;  // d <= 4096

// The quantisation rule, once.  x points at one fp32 row of length d; writes `stride` code bytes (padding zero) and
// returns a2.  fp64 IEEE arithmetic throughout (this file must not be built with fast-math).
__device__ __forceinline__ int32_t cos8_quantize_row(const float* __restrict__ x, int d, int stride,
                                                     int8_t* __restrict__ out) {
    double mag2 = 0.0;
    for (int i = 0; i < d; ++i) {
        const double v = (double)x[i];
        mag2 += v * v;  // the square of an fp32 value is exact in fp64: one rounding per step, index order
    }
    const double mag = sqrt(mag2);
    const bool zero = !(mag > 0.0) || !isfinite(mag);
    int32_t a2 = 0;
    uint32_t* w = (uint32_t*)out;  // stride is a multiple of 16: whole words
    for (int j = 0; j < stride; j += 4) {
        uint32_t word = 0;
        for (int b = 0; b < 4; ++b) {
            const int i = j + b;
            int c = 0;
            if (i < d && !zero) {
                const float p = x[i] * 127.0f;
                double t = trunc((double)p / mag);
                t = fmin(127.0, fmax(-127.0, t));  // NaN-free here (mag finite and > 0, p finite or +-inf)
                c = (int)t;
            }
            a2 += c * c;
            word |= ((uint32_t)(uint8_t)(int8_t)c) << (8 * b);
        }
        w[j >> 2] = word;
    }
    return a2;
}

// one thread per row (the fp64 magnitude is a sequential sum)
__global__ __launch_bounds__(256) void cos8_quantize_kernel(const float* __restrict__ x, int64_t n, int d, int stride,
                                                            int8_t* __restrict__ codes, int32_t* __restrict__ a2) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    a2[r] = cos8_quantize_row(x + r * d, d, stride, codes + r * stride);
}

// set_rows: staged row i -> the stored row rows[i] (distinct rows: checked on the host).  The same rule, the same thread per row.
__global__ __launch_bounds__(256) void cos8_quantize_list_kernel(const float* __restrict__ x, const int64_t* __restrict__ rows,
                                                                 int64_t m, int d, int stride, int8_t* __restrict__ codes,
                                                                 int32_t* __restrict__ a2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t r = rows[i];
    a2[r] = cos8_quantize_row(x + i * d, d, stride, codes + r * stride);
}

// The distance, once.
__device__ __forceinline__ float cos8_distance(int32_t ab, int32_t a2, int32_t b2) {
    if (a2 == 0 && b2 == 0) return 0.0f;
    if (a2 == 0 || b2 == 0 || ab == 0) return 1.0f;
    return (float)(1.0 - (double)ab / sqrt((double)a2 * (double)b2));
}

struct Cos8ScanArgs {
    const int8_t* codes;
    const int32_t* a2;
    int stride;             // bytes per row
    int nchunk;             // stride / 16
    int64_t n;              // rows scanned: ntotal, or the length of `rows`
    const int64_t* rows;    // F == 1: sorted row list (positions -> rows)
    const uint64_t* mask;   // F == 2: bit set = row excluded
    const int8_t* qcodes;   // [nq, stride]
    const int32_t* qb2;     // [nq]
    int nq;
    int k;
    int64_t per_block;      // positions per block
    uint64_t* cand;         // top-k mode: [nq][gridDim.x][k] keys
    float* scores;          // scores mode: [nq][n], -distance (-inf: not selected)
};

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int4 cos8_load16(const int8_t* p) {
    const i32x4 v = __builtin_nontemporal_load((const i32x4*)p);
    return make_int4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ int cos8_dot16(int4 a, int4 b, int acc) {
    acc = __builtin_amdgcn_sdot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_sdot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_sdot4(a.z, b.z, acc, false);
    return __builtin_amdgcn_sdot4(a.w, b.w, acc, false);
}

// G lanes per row, NCH chunks per lane, Q queries per pass (blockIdx.y), F: 0 every row, 1 row list, 2 exclusion
// bitmap; SCORES: write every distance instead of keeping top-k lists.
template <int G, int NCH, int Q, int F, bool SCORES>
__global__ __launch_bounds__(kCos8Threads) void cos8_scan_kernel(Cos8ScanArgs a) {
    constexpr int R = kWave / G;  // rows per wave step
    constexpr int NW = kCos8Threads / kWave;
    __shared__ uint64_t sh[SCORES ? 1 : (NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane & (G - 1);
    const int grp = lane / G;
    const int q0 = blockIdx.y * Q;

    int4 qv[Q][NCH];
    int32_t b2[Q];
    float rb[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const bool live = q0 + q < a.nq;
        b2[q] = live ? a.qb2[q0 + q] : 0;
        rb[q] = b2[q] ? rsqrtf((float)b2[q]) : 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = t + c * G;
            qv[q][c] = (live && ch < a.nchunk) ? *(const int4*)(a.qcodes + (int64_t)(q0 + q) * a.stride + ch * 16)
                                               : make_int4(0, 0, 0, 0);
        }
    }
    WaveTopK tk[SCORES ? 1 : Q];
    if (!SCORES) {
#pragma unroll
        for (int q = 0; q < Q; ++q) tk[q].init(a.k);
    }

    const int64_t beg = (int64_t)blockIdx.x * a.per_block;
    const int64_t end = beg + a.per_block < a.n ? beg + a.per_block : a.n;
    for (int64_t base = beg + (int64_t)wave * R; base < end; base += (int64_t)NW * R) {
        const int64_t p = base + grp;
        bool valid = p < end;
        int64_t row = p;
        if (F == 1 && valid) row = a.rows[p];
        if (F == 2 && valid) valid = !((a.mask[row >> 6] >> (row & 63)) & 1ull);
        int acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0;
        if (valid) {
            const int8_t* src = a.codes + row * a.stride;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int ch = t + c * G;
                if (ch < a.nchunk) {
                    const int4 v = cos8_load16(src + ch * 16);
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc[q] = cos8_dot16(v, qv[q][c], acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off, kWave);
        }
        const bool lead = t == 0 && valid;
        const int32_t ar = lead ? a.a2[row] : 0;
        const float rar = ar ? rsqrtf((float)ar) : 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (SCORES) {
                if (t == 0 && p < end && q0 + q < a.nq)
                    a.scores[(int64_t)(q0 + q) * a.n + p] = valid ? -cos8_distance(acc[q], ar, b2[q]) : -INFINITY;
            } else {
                uint64_t cand = 0;
                if (lead && q0 + q < a.nq) {
                    bool pass = tk[q].thr == 0 || ar == 0 || b2[q] == 0 || acc[q] == 0;
                    if (!pass) {
                        const float est = 1.0f - (float)acc[q] * rar * rb[q];
                        pass = -est >= tk[q].thr_score - 1e-5f;
                    }
                    if (pass) {
                        const uint64_t key = make_key(-cos8_distance(acc[q], ar, b2[q]), (uint32_t)row);
                        cand = key > tk[q].thr ? key : 0;
                    }
                }
                tk[q].offer(cand);
            }
        }
    }
    if (!SCORES) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            block_merge_topk(tk[q], sh, NW);
            if (wave == 0 && q0 + q < a.nq && lane < a.k)
                a.cand[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * a.k + lane] = tk[q].key;
            __syncthreads();
        }
    }
}

// ---- batch pass on the matrix cores: 32 queries per corpus pass ------------------------------------------------------
// v_mfma_i32_32x32x32_i8: A = 32 rows x 32 code bytes, B = 32 code bytes x 32 queries, C = 32 x 32 exact int32 sums.  Lane l
// supplies row / query (l & 31) and the 16 bytes at offset 16 (l >> 5) of each 32-byte K step for BOTH operands, so whatever
// order the unit sums the K elements in, A and B are paired element for element (an integer sum is order-free).  C lane l,
// element j: query (l & 31), row 8 (j >> 2) + 4 (l >> 5) + (j & 3).  Each wave keeps one sorted k-list per query in LDS;
// a lane holds the k-th key of ITS query's list as its gate, so the 16 candidates of a lane are tested in parallel and only
// candidates that beat the gate reach the wave-cooperative list insert.  d <= 1024 (the queries sit in LDS), k <= 64.
constexpr int kCos8MfmaQ = 32;
typedef int i32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int cos8_mfma_lds_stride(int stride) { return stride + 16; }  // zero pad: conflict-free reads

__device__ __forceinline__ i32x4 cos8_i4(int4 v) {
    i32x4 r;
    r.x = v.x;
    r.y = v.y;
    r.z = v.z;
    r.w = v.w;
    return r;
}

// F: 0 every row, 2 exclusion bitmap.  Dynamic LDS: 32 query rows of cos8_mfma_lds_stride(stride) bytes, then
// 4 waves x 32 queries x k keys.
template <int F>
__global__ __launch_bounds__(kCos8Threads) void cos8_mfma_kernel(Cos8ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cos8_lds[];
    constexpr int NW = kCos8Threads / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int qn = lane & 31;  // this lane's query (B column, C column)
    const int q0 = blockIdx.y * kCos8MfmaQ;
    const int ls = cos8_mfma_lds_stride(a.stride);
    int8_t* qsh = (int8_t*)cos8_lds;
    uint64_t* lists = (uint64_t*)(cos8_lds + kCos8MfmaQ * ls);
    const int k = a.k;

    // stage the pass's queries (zero rows past nq, zero pad) and clear the lists
    for (int i = threadIdx.x; i < kCos8MfmaQ * (ls / 16); i += kCos8Threads) {
        const int qq = i / (ls / 16), c = i - qq * (ls / 16);
        int4 v = make_int4(0, 0, 0, 0);
        if (q0 + qq < a.nq && c < a.nchunk) v = *(const int4*)(a.qcodes + (int64_t)(q0 + qq) * a.stride + c * 16);
        *(int4*)(qsh + qq * ls + c * 16) = v;
    }
    for (int i = threadIdx.x; i < NW * kCos8MfmaQ * k; i += kCos8Threads) lists[i] = 0ull;
    __syncthreads();

    const bool qlive = q0 + qn < a.nq;
    const int32_t b2 = qlive ? a.qb2[q0 + qn] : 0;
    const float rb = b2 ? rsqrtf((float)b2) : 0.0f;
    uint64_t gate = 0;                // k-th key of this lane's query list (0: not full)
    float gate_score = -INFINITY;
    uint64_t* mylists = lists + (int64_t)wave * kCos8MfmaQ * k;
    const int nsteps = (a.stride + 31) / 32;

    const int64_t beg = (int64_t)blockIdx.x * a.per_block;
    const int64_t end = beg + a.per_block < a.n ? beg + a.per_block : a.n;
    for (int64_t r0 = beg + (int64_t)wave * 32; r0 < end; r0 += (int64_t)NW * 32) {
        const int64_t ra = r0 + qn;                 // the row this lane feeds into A
        const bool va = ra < end;
        const int8_t* src = a.codes + (va ? ra : 0) * a.stride;
        i32x16 acc = {};
        for (int s0 = 0; s0 < nsteps; s0 += 8) {
            i32x4 av[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int off = (s0 + u) * 32 + half * 16;
                av[u] = (va && s0 + u < nsteps && off < a.stride) ? cos8_i4(cos8_load16(src + off)) : i32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (s0 + u < nsteps) {
                    const int off = (s0 + u) * 32 + half * 16;
                    const i32x4 bv = *(const i32x4*)(qsh + qn * ls + off);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[u], bv, acc, 0, 0, 0);
                }
            }
        }
        // per-row facts, held by lanes 0..31 (row r0 + lane) and fetched by the lanes that need them
        int32_t ar_l = 0;
        int sel_l = 0;
        if (lane < 32 && va) {
            ar_l = a.a2[ra];
            sel_l = F == 2 ? !((a.mask[ra >> 6] >> (ra & 63)) & 1ull) : 1;
        }
        uint64_t cand[16];
        bool pass[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int m = 8 * (j >> 2) + 4 * half + (j & 3);
            const int32_t ar = __shfl(ar_l, m, kWave);
            const int sel = __shfl(sel_l, m, kWave);
            const int32_t ab = acc[j];
            bool p = qlive && sel;
            if (p && gate != 0 && ar != 0 && b2 != 0 && ab != 0) {
                const float est = 1.0f - (float)ab * rsqrtf((float)ar) * rb;
                p = -est >= gate_score - 1e-5f;
            }
            cand[j] = 0;
            if (p) {
                const uint64_t key = make_key(-cos8_distance(ab, ar, b2), (uint32_t)(r0 + m));
                p = key > gate;
                cand[j] = key;
            }
            pass[j] = p;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint64_t mask = __ballot(pass[j]);
            while (mask) {
                const int srcl = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const uint64_t key = readlane_u64(cand[j], srcl);
                const int q = srcl & 31;
                const uint64_t kth = lds_list_insert(mylists + q * k, k, key, lane);
                if (qn == q) {
                    gate = kth;
                    gate_score = kth ? key_score(kth) : -INFINITY;
                }
            }
        }
    }
    __syncthreads();
    // fold the waves' lists per query and write this block's partial list
    for (int q = wave; q < kCos8MfmaQ; q += NW) {
        WaveTopK tk;
        tk.init(k);
        for (int w = 0; w < NW; ++w) tk.offer(lane < k ? lists[((int64_t)w * kCos8MfmaQ + q) * k + lane] : 0ull);
        if (q0 + q < a.nq && lane < k) a.cand[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * k + lane] = tk.key;
    }
}

// One block per query: the nlists partial lists -> sorted top-k, D = distance, I = row + label_offset.
__global__ __launch_bounds__(kCos8Threads) void cos8_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k,
                                                                  int64_t label_offset, float* __restrict__ D,
                                                                  int64_t* __restrict__ I) {
    constexpr int NW = kCos8Threads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint64_t* src = cand + (int64_t)blockIdx.x * nlists * k;
    WaveTopK tk;
    tk.init(k);
    const int64_t total = (int64_t)nlists * k;
    for (int64_t i0 = (int64_t)wave * kWave; i0 < total; i0 += (int64_t)NW * kWave) {
        const int64_t i = i0 + lane;
        tk.offer(i < total ? src[i] : 0ull);
    }
    block_merge_topk(tk, sh, NW);
    if (wave == 0 && lane < k) {
        const int64_t o = (int64_t)blockIdx.x * k + lane;
        if (tk.key) {
            D[o] = -key_score(tk.key);
            I[o] = label_offset + (int64_t)key_row(tk.key);
        } else {
            D[o] = 3.402823466e+38f;
            I[o] = -1;
        }
    }
}

__global__ void cos8_fill_missing_kernel(float* D, int64_t* I, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = 3.402823466e+38f;
        I[i] = -1;
    }
}

// large k over a row list: the select labelled positions (+ label_offset); map them to rows (+ label_offset)
__global__ void cos8_map_positions_kernel(int64_t* I, int64_t total, const int64_t* __restrict__ rows,
                                          int64_t label_offset) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && I[i] >= 0) I[i] = rows[I[i] - label_offset] + label_offset;
}

// removal: dst row j <- src row keep[j] (codes and a2), out of place
__global__ __launch_bounds__(256) void cos8_gather_kernel(const int8_t* __restrict__ src, const int32_t* __restrict__ a2s,
                                                          const int64_t* __restrict__ keep, int64_t m, int nchunk,
                                                          int8_t* __restrict__ dst, int32_t* __restrict__ a2d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    const int64_t from = keep[j];
    ((int4*)dst)[j * nchunk + ch] = ((const int4*)src)[from * nchunk + ch];
    if (ch == 0) a2d[j] = a2s[from];
}

}  // namespace mvdb
