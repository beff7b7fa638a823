// sq4_kernels.hpp — kernels of the 4-bit scalar-quantised index (sq4.hip; contract in include/mvdb.h "4-bit scalar-quantised
// index" and INTEGRATION.md 3w).
//
// A row is d / 2 bytes, 1 to 128 chunks of 16: byte j holds the code of dimension 2 j in its low nibble and that of 2 j + 1 in
// its high nibble.  The query is quantised to int8 and written DE-INTERLEAVED per chunk of 32 dimensions — 16 even-dimension
// bytes, then 16 odd-dimension bytes — so a row dword v pairs as (v & 0x0F0F0F0F) with the even half and ((v >> 4) & 0x0F0F0F0F)
// with the odd half, and nibbles become int8 operands in three VALU operations per dword.  The score S = sum q8[i] code[i] is an
// exact int32, |S| <= 127 * 15 * 4096 < 2^24, so (float)S is exact, the key is topk_device.hpp's make_key((float)S, row) — larger
// S first, then the lower row — and WaveTopK, lds_list_insert and block_merge_topk serve as they stand.
//
//   sq4_encode_kernel  fp32 rows -> nibble rows: one wave per row, 8 dimensions -> one dword per lane.
//   sq4_query_kernel   fp32 queries -> int8 queries (de-interleaved), step, bias, valid: one block per query.
//   sq4_scan_kernel    1, 2 or 4 queries per pass on the VALU: G lanes per row, 16-byte loads, v_dot4_i32_i8.
//   sq4_mfma_kernel    32 or 64 queries per row read on the int8 matrix cores: nibbles expanded in registers.
//   sq4_merge_kernel   the blocks' partial lists -> S (int32), I (int64 rows), D (fp32 estimate of q . x).
//   sq4_minmax_kernel  per-dimension min and max over the finite values of a sample, two stages, no atomics.
#pragma once
#include <float.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kSq4Threads = 256;           // encode, query, scan, merge, minmax
constexpr int kSq4MaxChunks = 128;         // d <= 4096
constexpr int kSq4MaxDim = 32 * kSq4MaxChunks;
constexpr int kSq4MfmaMaxDim = 2048;       // the matrix-core form: 64 queries of 2048 + 16 bytes are 129 KiB of LDS (with k = 64
                                           // the lists no longer fit beside them: 32 queries per row read, sq4.hip sq4_mfma_block)
constexpr int kSq4MfmaMaxThreads = 512;    // its block: 1, 2, 4 or 8 waves, by what the lists leave of the LDS
constexpr int kSq4MinmaxCols = 64;         // columns per block of the first min/max stage; 4 row lanes beside them
constexpr int32_t kSq4NoScore = INT32_MIN;
constexpr uint32_t kSq4Nibbles = 0x0F0F0F0Fu;

typedef int sq4_i32x4 __attribute__((ext_vector_type(4)));
typedef int sq4_i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint64_t sq4_key(int s, uint32_t row) { return make_key((float)s, row); }
__device__ __forceinline__ int32_t sq4_key_score(uint64_t key) { return (int32_t)key_score(key); }

__device__ __forceinline__ uint4 sq4_load16(const uint8_t* p) {
    const sq4_i32x4 v = __builtin_nontemporal_load((const sq4_i32x4*)p);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
}

__device__ __forceinline__ bool sq4_nonfinite(float f) { return (__float_as_uint(f) & 0x7F800000u) == 0x7F800000u; }

// ---- encoding --------------------------------------------------------------------------------------------------------------
// u = (x - lo) * inv: one fp32 subtract, one fp32 multiply (nothing to contract).  15 from 15 up, 0 unless u > 0 (NaN, -inf and
// negatives), else rintf: ties to even.
__device__ __forceinline__ uint32_t sq4_code(float x, float lo, float inv) {
    const float u = (x - lo) * inv;
    return u >= 15.0f ? 15u : !(u > 0.0f) ? 0u : (uint32_t)(int)rintf(u);
}

// One wave per row.  Of each slab of 512 dimensions lane l takes [8 l, 8 l + 8): two 16-byte loads of x, lo and inv each, eight
// codes, ONE dword — nibble m of it is dimension 8 l + m, which is the row's byte order — so a wave stores 256 consecutive
// bytes per slab.  rows == nullptr: staged row i -> row i of out (add); else -> row rows[i] of out (set_rows: distinct rows,
// checked on the host).
__global__ __launch_bounds__(kSq4Threads) void sq4_encode_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                 const float* __restrict__ lo, const float* __restrict__ inv,
                                                                 const int64_t* __restrict__ rows, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * (kSq4Threads / kWave) + (threadIdx.x >> 6);
    if (i >= n) return;  // (wave-uniform)
    const float* src = x + i * d;
    const int64_t r = rows ? rows[i] : i;
    uint32_t* dst = (uint32_t*)(out + r * (d >> 1));
    for (int base = lane * 8; base < d; base += 8 * kWave) {
        const float4 xa = *(const float4*)(src + base), xb = *(const float4*)(src + base + 4);
        const float4 la = *(const float4*)(lo + base), lb = *(const float4*)(lo + base + 4);
        const float4 ia = *(const float4*)(inv + base), ib = *(const float4*)(inv + base + 4);
        uint32_t w = sq4_code(xa.x, la.x, ia.x) | sq4_code(xa.y, la.y, ia.y) << 4;
        w |= sq4_code(xa.z, la.z, ia.z) << 8 | sq4_code(xa.w, la.w, ia.w) << 12;
        w |= sq4_code(xb.x, lb.x, ib.x) << 16 | sq4_code(xb.y, lb.y, ib.y) << 20;
        w |= sq4_code(xb.z, lb.z, ib.z) << 24 | sq4_code(xb.w, lb.w, ib.w) << 28;
        dst[base >> 3] = w;
    }
}

// ---- the query -------------------------------------------------------------------------------------------------------------
struct Sq4QueryArgs {
    const float* q;    // [nq, d]
    const float* lo;   // [d]
    const float* s;    // [d] (hi - lo) / 15
    int d;
    int8_t* q8;        // [nq, d] de-interleaved per 32 dimensions
    double* step;      // [nq]
    double* bias;      // [nq]
    int* valid;        // [nq] 0: a non-finite component of q or of w
};

// where dimension i of a query sits: chunk i / 32, the even dimensions of the chunk first
__host__ __device__ constexpr int sq4_query_slot(int i) { return (i & ~31) + ((i & 1) << 4) + ((i & 31) >> 1); }

// One block per query.  w = q * s in fp32, amax = max |w| (block reduce; a maximum has no order), q8 = rint(w * (127 / amax)) in
// fp64, step = amax / 127.  The products q[i] * lo[i] are exact in fp64 (24 x 24 bits); they wait in LDS and thread 0 adds them
// in ascending i: the bits of a plain loop, fused or not.
__global__ __launch_bounds__(kSq4Threads) void sq4_query_kernel(Sq4QueryArgs a) {
    constexpr int NW = kSq4Threads / kWave;
    __shared__ double prod[kSq4MaxDim];
    __shared__ float wave_max[NW];
    __shared__ int wave_bad[NW];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const float* q = a.q + (int64_t)qi * a.d;
    float amax = 0.0f;
    bool bad = false;
    for (int i = threadIdx.x; i < a.d; i += kSq4Threads) {
        const float qv = q[i];
        const float w = qv * a.s[i];
        bad |= sq4_nonfinite(qv) || sq4_nonfinite(w);
        amax = fmaxf(amax, fabsf(w));
        prod[i] = (double)qv * (double)a.lo[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, kWave));
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        wave_max[wave] = amax;
        wave_bad[wave] = any_bad;
    }
    __syncthreads();
    amax = 0.0f;
    int nbad = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        amax = fmaxf(amax, wave_max[w]);
        nbad |= wave_bad[w];
    }
    const bool quantise = !nbad && amax > 0.0f;
    const double scale = quantise ? 127.0 / (double)amax : 0.0;
    int8_t* dst = a.q8 + (int64_t)qi * a.d;
    for (int i = threadIdx.x; i < a.d; i += kSq4Threads) {
        const float w = q[i] * a.s[i];
        dst[sq4_query_slot(i)] = quantise ? (int8_t)(int)rint((double)w * scale) : (int8_t)0;
    }
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (int i = 0; i < a.d; ++i) b += prod[i];
        a.step[qi] = (double)amax / 127.0;
        a.bias[qi] = b;
        a.valid[qi] = !nbad;
    }
}

// ---- VALU form -------------------------------------------------------------------------------------------------------------
struct Sq4ScanArgs {
    const uint8_t* rows;    // [n, 16 nchunk]
    int nchunk;             // 16-byte chunks per row = d / 32
    int64_t n;
    const uint64_t* mask;   // nullptr: every row; else bit r & 63 of word r >> 6 set = row r selected
    const int8_t* q8;       // [nq, 32 nchunk] de-interleaved
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k] keys
};

template <int CTRL>
__device__ __forceinline__ int sq4_dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// The sum over the G lanes of a row, left in every one of them (bits_kernels.hpp: bits_group_sum, with the step across the two
// halves of the wave for G = 64).
template <int G>
__device__ __forceinline__ int sq4_group_sum(int h) {
    if (G >= 2) h = sq4_dpp_add<0xB1>(h);    // quad_perm [1, 0, 3, 2]
    if (G >= 4) h = sq4_dpp_add<0x4E>(h);    // quad_perm [2, 3, 0, 1]
    if (G >= 8) h = sq4_dpp_add<0x141>(h);   // row_half_mirror
    if (G >= 16) h = sq4_dpp_add<0x140>(h);  // row_mirror
    if (G >= 32) h += __shfl_xor(h, 16, kWave);
    if (G >= 64) h += __shfl_xor(h, 32, kWave);
    return h;
}

// one row dword against the even and the odd query dword that belong to it: two expansions, two v_dot4_i32_i8
__device__ __forceinline__ int sq4_dot8(uint32_t e, uint32_t o, uint32_t qe, uint32_t qo, int acc) {
    acc = __builtin_amdgcn_sdot4((int)e, (int)qe, acc, false);
    return __builtin_amdgcn_sdot4((int)o, (int)qo, acc, false);
}

// G lanes per row: lane t of the group holds chunk t (and chunk t + 64 when NCH = 2: rows of more than 64 chunks); lanes whose
// chunk is past the row load nothing.  U batches of 64 / G rows in flight per wave, NQ queries per pass (blockIdx.y).  A wave
// takes tiles of U * 64 / G consecutive rows, the grid strides over the tiles.  The 8 query dwords per query and chunk stay in
// the lane's registers for the launch.
template <int G, int NCH, int U, int NQ>
__global__ __launch_bounds__(kSq4Threads) void sq4_scan_kernel(Sq4ScanArgs a) {
    constexpr int R = kWave / G;
    constexpr int NW = kSq4Threads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane & (G - 1);
    const int grp = lane / G;
    const int q0 = blockIdx.y * NQ;
    const int64_t rb = (int64_t)a.nchunk * 16;

    bool live[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) live[c] = t + kWave * c < a.nchunk;
    uint4 qe[NQ][NCH], qo[NQ][NCH];
    WaveTopK tk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const bool on = live[c] && q0 + q < a.nq;
            const uint4* src = (const uint4*)(a.q8 + (int64_t)(on ? q0 + q : 0) * rb * 2 + (on ? t + kWave * c : 0) * 32);
            qe[q][c] = on ? src[0] : make_uint4(0, 0, 0, 0);
            qo[q][c] = on ? src[1] : make_uint4(0, 0, 0, 0);
        }
        tk[q].init(a.k);
    }

    const int64_t stride = (int64_t)gridDim.x * NW * (R * U);
    for (int64_t base = ((int64_t)blockIdx.x * NW + wave) * (R * U); base < a.n; base += stride) {
        uint4 v[U][NCH];
        uint64_t mw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool in = row < a.n;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                v[u][c] = (live[c] && in) ? sq4_load16(a.rows + row * rb + (t + kWave * c) * 16) : make_uint4(0, 0, 0, 0);
            mw[u] = !in ? 0ull : (a.mask ? a.mask[row >> 6] : ~0ull);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool lead = t == 0 && ((mw[u] >> (row & 63)) & 1ull);
            uint4 e[NCH], o[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                e[c] = make_uint4(v[u][c].x & kSq4Nibbles, v[u][c].y & kSq4Nibbles, v[u][c].z & kSq4Nibbles, v[u][c].w & kSq4Nibbles);
                o[c] = make_uint4((v[u][c].x >> 4) & kSq4Nibbles, (v[u][c].y >> 4) & kSq4Nibbles, (v[u][c].z >> 4) & kSq4Nibbles,
                                  (v[u][c].w >> 4) & kSq4Nibbles);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                int s = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    s = sq4_dot8(e[c].x, o[c].x, qe[q][c].x, qo[q][c].x, s);
                    s = sq4_dot8(e[c].y, o[c].y, qe[q][c].y, qo[q][c].y, s);
                    s = sq4_dot8(e[c].z, o[c].z, qe[q][c].z, qo[q][c].z, s);
                    s = sq4_dot8(e[c].w, o[c].w, qe[q][c].w, qo[q][c].w, s);
                }
                s = sq4_group_sum<G>(s);
                tk[q].offer(lead && q0 + q < a.nq ? sq4_key(s, (uint32_t)row) : 0ull);
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

// ---- matrix-core form ------------------------------------------------------------------------------------------------------
// v_mfma_i32_32x32x32_i8 fed as cos8_kernels.hpp and bits_kernels.hpp feed it: A = 32 rows x 32 bytes, B = 32 bytes x 32
// queries, C exact int32.  Lane l supplies row / query (l & 31) and the 16 bytes of half (l >> 5) of each K step for BOTH
// operands, so A and B pair element for element whatever the order inside the step.  C lane l, element j: query (l & 31), row
// 8 (j >> 2) + 4 (l >> 5) + (j & 3).
//
// A K step is 64 dimensions = 2 row chunks: half h of the lanes loads chunk 2 s + h — 16 bytes, HBM to registers —, expands it
// into the even operand (v & 0x0F0F0F0F, the 16 even dimensions of the chunk) and the odd operand ((v >> 4) & 0x0F0F0F0F): 12
// VALU operations for two MFMAs, and the pair is used again for each of the QB blocks of 32 queries, so at QB = 2 one row read
// and one expansion serve 64 queries.  A row of an odd chunk count leaves half 1 of the last step at zero.  Row nibbles never
// touch LDS.  The slab's queries sit in LDS as the query kernel wrote them, query q at q * (d + 16) (the pad keeps the 16-byte
// reads of neighbouring queries off each other's banks): the operands of chunk c are its bytes [32 c, 32 c + 16) and
// [32 c + 16, 32 c + 32).  Behind the queries: one sorted k-list per wave and query, gated by the k-th key each lane keeps.
__host__ __device__ constexpr int sq4_mfma_lds_stride(int d) { return d + 16; }
__host__ __device__ constexpr size_t sq4_mfma_lds_bytes(int d, int k, int qb, int nwaves) {
    return (size_t)32 * qb * sq4_mfma_lds_stride(d) + (size_t)nwaves * 32 * qb * k * sizeof(uint64_t);
}

struct Sq4MfmaArgs {
    const uint8_t* rows;
    int nchunk;
    int d;
    int64_t n;
    const uint64_t* mask;
    const int8_t* q8;
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k]
};

// blockDim.x = 64 * (1 | 2 | 4 | 8); a wave takes tiles of 32 rows, the grid strides over them; blockIdx.y: the slab of 32 QB queries.
template <int QB>
__global__ __launch_bounds__(kSq4MfmaMaxThreads) void sq4_mfma_kernel(Sq4MfmaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sq4_lds[];
    constexpr int NQS = 32 * QB;
    const int NW = blockDim.x >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int qn = lane & 31;
    const int q0 = blockIdx.y * NQS;
    const int ls = sq4_mfma_lds_stride(a.d);
    const int rb = a.nchunk * 16;
    const int k = a.k;
    unsigned char* qsh = sq4_lds;
    uint64_t* lists = (uint64_t*)(sq4_lds + NQS * ls);

    // the slab's queries (past nq: zeros, never offered) and empty lists
    const int per = a.d >> 4;
    for (int i = threadIdx.x; i < NQS * per; i += blockDim.x) {
        const int qq = i / per, p = i - qq * per;
        sq4_i32x4 v = {0, 0, 0, 0};
        if (q0 + qq < a.nq) v = *(const sq4_i32x4*)(a.q8 + (int64_t)(q0 + qq) * a.d + p * 16);
        *(sq4_i32x4*)(qsh + qq * ls + p * 16) = v;
    }
    for (int i = threadIdx.x; i < NW * NQS * k; i += blockDim.x) lists[i] = 0ull;
    __syncthreads();

    bool qlive[QB];
    uint64_t gate[QB];  // the k-th key of this lane's query list (0: not full)
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        qlive[b] = q0 + 32 * b + qn < a.nq;
        gate[b] = 0ull;
    }
    uint64_t* mylists = lists + (int64_t)wave * NQS * k;
    const unsigned char* qrow = qsh + qn * ls;
    const int nstep = (a.nchunk + 1) >> 1;

    const int64_t stride = (int64_t)gridDim.x * NW * 32;
    for (int64_t r0 = ((int64_t)blockIdx.x * NW + wave) * 32; r0 < a.n; r0 += stride) {
        const int64_t ra = r0 + qn;  // the row this lane feeds into A
        const bool va = ra < a.n;
        const uint8_t* src = a.rows + (va ? ra : 0) * rb;
        sq4_i32x16 acc[QB];
#pragma unroll
        for (int b = 0; b < QB; ++b) acc[b] = sq4_i32x16{};
        for (int s0 = 0; s0 < nstep; s0 += 4) {
            uint4 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = 2 * (s0 + u) + half;
                w[u] = (va && c < a.nchunk) ? sq4_load16(src + c * 16) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (s0 + u < nstep) {  // (wave-uniform)
                    const int c = min(2 * (s0 + u) + half, a.nchunk - 1);  // (past the row: A is zero, any query bytes do)
                    const unsigned char* qp = qrow + c * 32;
                    const sq4_i32x4 e = {(int)(w[u].x & kSq4Nibbles), (int)(w[u].y & kSq4Nibbles), (int)(w[u].z & kSq4Nibbles),
                                         (int)(w[u].w & kSq4Nibbles)};
                    const sq4_i32x4 o = {(int)((w[u].x >> 4) & kSq4Nibbles), (int)((w[u].y >> 4) & kSq4Nibbles),
                                         (int)((w[u].z >> 4) & kSq4Nibbles), (int)((w[u].w >> 4) & kSq4Nibbles)};
#pragma unroll
                    for (int b = 0; b < QB; ++b) {
                        const unsigned char* qb = qp + b * 32 * ls;
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(e, *(const sq4_i32x4*)(qb), acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(o, *(const sq4_i32x4*)(qb + 16), acc[b], 0, 0, 0);
                    }
                }
            }
        }
        // which rows of the tile are selected: lanes 0..31 look (row r0 + lane), the others fetch
        int sel_l = 0;
        if (lane < 32 && va) sel_l = a.mask ? (int)((a.mask[ra >> 6] >> (ra & 63)) & 1ull) : 1;
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            uint64_t cand[16];
            bool pass[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = 8 * (j >> 2) + 4 * half + (j & 3);
                const int sel = __shfl(sel_l, m, kWave);
                cand[j] = sq4_key(acc[b][j], (uint32_t)(r0 + m));
                pass[j] = qlive[b] && sel && cand[j] > gate[b];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                uint64_t todo = __ballot(pass[j]);
                while (todo) {
                    const int srcl = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const uint64_t key = readlane_u64(cand[j], srcl);
                    const int q = srcl & 31;
                    const uint64_t kth = lds_list_insert(mylists + (32 * b + q) * k, k, key, lane);
                    if (qn == q) gate[b] = kth;
                }
            }
        }
    }
    __syncthreads();
    // fold the waves' lists per query and write this block's partial list
    for (int q = wave; q < NQS; q += NW) {
        WaveTopK tk;
        tk.init(k);
        for (int w = 0; w < NW; ++w) tk.offer(lane < k ? lists[((int64_t)w * NQS + q) * k + lane] : 0ull);
        if (q0 + q < a.nq && lane < k) a.cand[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * k + lane] = tk.key;
    }
}

// ---- merge and housekeeping ------------------------------------------------------------------------------------------------
// D = (float)(bias + step * S) in fp64, the product rounded before the sum (numpy's two operations)
__device__ __forceinline__ float sq4_estimate(int32_t s, double step, double bias) {
#pragma clang fp contract(off)
    const double p = step * (double)s;
    return (float)(bias + p);
}

// One block per query: the nlists partial lists -> sorted top-k; missing slots (and every slot of a query that is not valid)
// I = -1, S = INT32_MIN, D = -FLT_MAX.
__global__ __launch_bounds__(kSq4Threads) void sq4_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k,
                                                                const double* __restrict__ step, const double* __restrict__ bias,
                                                                const int* __restrict__ valid, float* __restrict__ D,
                                                                int64_t* __restrict__ I, int32_t* __restrict__ S) {
    constexpr int NW = kSq4Threads / kWave;
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
        const int32_t s = hit ? sq4_key_score(tk.key) : kSq4NoScore;
        D[o] = hit ? sq4_estimate(s, step[qi], bias[qi]) : -FLT_MAX;
        I[o] = hit ? (int64_t)key_row(tk.key) : -1;
        if (S) S[o] = s;
    }
}

__global__ void sq4_fill_missing_kernel(float* D, int64_t* I, int32_t* S, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = -FLT_MAX;
        I[i] = -1;
        if (S) S[i] = kSq4NoScore;
    }
}

// removal: dst row j <- src row keep[j], out of place, one 16-byte chunk per thread
__global__ __launch_bounds__(256) void sq4_gather_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ keep,
                                                         int64_t m, int nchunk, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    ((uint4*)dst)[j * nchunk + ch] = ((const uint4*)src)[keep[j] * nchunk + ch];
}

// set_rows_codes: staged row j -> stored row rows[j] (distinct rows: checked on the host)
__global__ __launch_bounds__(256) void sq4_scatter_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ rows,
                                                          int64_t m, int nchunk, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    ((uint4*)dst)[rows[j] * nchunk + ch] = ((const uint4*)src)[j * nchunk + ch];
}

// ---- training: per-dimension min and max over the finite values ------------------------------------------------------------
// Values are compared through f2ord, the order-preserving image of topk_device.hpp (-0 below +0), so the extremes are the same
// bits in whatever order the rows are met.  Stage 1 (final == 0): grid (d / 64 rounded up, slabs); a block is 64 columns x 4 row
// lanes, thread (c, l) walks rows l, l + 4, ... of its slab down its column — a wave reads 64 consecutive floats — and writes
// partial (4 slab + l).  Stage 2 (final == 1, one slab, x = stage 1's images): the same walk over the partials; a column without
// a finite value gets lo = hi = 0.
__global__ __launch_bounds__(kSq4Threads) void sq4_minmax_kernel(const void* __restrict__ x, int64_t n, int d, int64_t slab_rows,
                                                                 int final, uint32_t* __restrict__ plo, uint32_t* __restrict__ phi,
                                                                 float* __restrict__ lo, float* __restrict__ hi) {
    const int col = blockIdx.x * kSq4MinmaxCols + (threadIdx.x & (kSq4MinmaxCols - 1));
    const int l = threadIdx.x / kSq4MinmaxCols;
    constexpr int L = kSq4Threads / kSq4MinmaxCols;
    if (col >= d) return;
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;  // (no finite value seen: mn > mx)
    if (!final) {
        const float* xf = (const float*)x;
        const int64_t r1 = min(n, ((int64_t)blockIdx.y + 1) * slab_rows);
        for (int64_t r = (int64_t)blockIdx.y * slab_rows + l; r < r1; r += L) {
            const float v = xf[r * d + col];
            if (!sq4_nonfinite(v)) {
                mn = min(mn, f2ord(v));
                mx = max(mx, f2ord(v));
            }
        }
        const int64_t p = (int64_t)blockIdx.y * L + l;
        plo[p * d + col] = mn;
        phi[p * d + col] = mx;
    } else if (l == 0) {
        for (int64_t p = 0; p < n; ++p) {
            mn = min(mn, plo[p * d + col]);
            mx = max(mx, phi[p * d + col]);
        }
        lo[col] = mn <= mx ? ord2f(mn) : 0.0f;
        hi[col] = mn <= mx ? ord2f(mx) : 0.0f;
    }
}

}  // namespace mvdb
