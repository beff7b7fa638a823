// bits_kernels.hpp — kernels of the binary index (bits.hip; contract in include/mvdb.h "binary index" and INTEGRATION.md 3u).
//
// A row is d_bits / 8 opaque bytes: 1 to 32 chunks of 16.  The distance is the Hamming distance H = popcount(row ^ query),
// an integer, so every form returns the same bits.  A candidate is topk_device.hpp's key with score -(float)H — exact, H <= 4096
// — so the key order is "smaller H first, then the lower row" and WaveTopK, the gate, lds_list_insert and block_merge_topk serve
// as they stand.
//
//   bits_pack_kernel   fp32 rows -> packed rows: one ballot per 64 dimensions, one 8-byte vector store per lane.
//   bits_scan_kernel   1 to 8 queries per pass on the VALU: G lanes per row, 16-byte loads, U batches in flight, nothing in LDS.
//   bits_mfma_kernel   32 queries per row read on the int8 matrix cores: bits expanded to +1 / -1 bytes in registers,
//                      q.x = d - 2 H from v_mfma_i32_32x32x32_i8.
//   bits_merge_kernel  the blocks' partial lists -> D (int32 H, ascending), I (int64 rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kBitsThreads = 256;          // scan, merge
constexpr int kBitsMaxChunks = 32;         // d_bits <= 4096
constexpr int kBitsMfmaQ = 32;             // queries per slab of the matrix-core form (grid.y)
constexpr int kBitsMfmaMaxThreads = 512;   // its block: 1, 2, 4 or 8 waves, by what the lists leave of the LDS
constexpr int32_t kBitsNoDistance = 0x7FFFFFFF;

typedef int bits_i32x4 __attribute__((ext_vector_type(4)));
typedef int bits_i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned bits_u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t bits_key(int h, uint32_t row) { return make_key(-(float)h, row); }
__device__ __forceinline__ int32_t bits_key_distance(uint64_t key) { return (int32_t)(-key_score(key)); }

// ---- sign packing ------------------------------------------------------------------------------------------------------
// One wave per row.  Segment s of the row is its dimensions [64 s, 64 s + 64): lane l tests x[64 s + l] > 0 (false for NaN and
// for -0) and the ballot holds dimension 64 s + l in bit l.  numpy.packbits wants dimension 8 j in bit 7 of byte j: reversing the
// 64 bits puts dimension l at bit 63 - l — byte 7 - l / 8, bit 7 - l % 8 — and swapping the 8 bytes puts the byte right.  Lane s
// keeps word s, so after d_bits / 64 <= 64 segments the row leaves in ONE 8-byte store per lane.  rows == nullptr: staged row
// i -> stored row row0 + i (add); else -> stored row rows[i] (set_rows: distinct rows, checked on the host).
__global__ __launch_bounds__(kBitsThreads) void bits_pack_kernel(const float* __restrict__ x, int64_t n, int d_bits,
                                                                 const int64_t* __restrict__ rows, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * (kBitsThreads / kWave) + (threadIdx.x >> 6);
    if (i >= n) return;  // (wave-uniform)
    const float* src = x + i * d_bits;
    const int nseg = d_bits >> 6;
    uint64_t mine = 0;
    for (int s = 0; s < nseg; ++s) {
        // x > 0 on the bit pattern — [0x00000001, 0x7F800000]: denormals count whatever the kernel's denormal mode is
        const bool positive = __float_as_uint(src[s * 64 + lane]) - 1u < 0x7F800000u;
        const uint64_t word = __builtin_bswap64(__brevll(__ballot(positive)));
        if (lane == s) mine = word;
    }
    const int64_t r = rows ? rows[i] : i;
    if (lane < nseg) ((uint64_t*)(out + r * (d_bits >> 3)))[lane] = mine;
}

// ---- VALU form ---------------------------------------------------------------------------------------------------------
struct BitsScanArgs {
    const uint8_t* rows;    // [n, 16 nchunk]
    int nchunk;             // 16-byte chunks per row
    int d_bits;
    int64_t n;
    const uint64_t* mask;   // nullptr: every row; else bit r & 63 of word r >> 6 set = row r selected
    const uint8_t* q;       // packed queries [nq, 16 nchunk]
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k] keys
};

__device__ __forceinline__ uint4 bits_load16(const uint8_t* p) {
    const bits_i32x4 v = __builtin_nontemporal_load((const bits_i32x4*)p);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
}

// v_bcnt_u32_b32 adds its second operand: four of them per chunk and query
__device__ __forceinline__ int bits_hamming16(uint4 a, uint4 b) {
    int h = __builtin_popcount(a.x ^ b.x);
    h += __builtin_popcount(a.y ^ b.y);
    h += __builtin_popcount(a.z ^ b.z);
    return h + __builtin_popcount(a.w ^ b.w);
}

template <int CTRL>
__device__ __forceinline__ int bits_dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// The sum over the G lanes of a row, left in every one of them: log2(G) steps.  Inside a DPP row of 16 lanes the partner comes
// through the DPP operand: xor 1 and xor 2 as quad permutations; once the quads (the halves) are uniform, the mirror of the half
// row (the row) reads the other quad (half) — what xor 4 (xor 8) would.  Only the step across two rows, G = 32, is a shuffle.
template <int G>
__device__ __forceinline__ int bits_group_sum(int h) {
    if (G >= 2) h = bits_dpp_add<0xB1>(h);    // quad_perm [1, 0, 3, 2]
    if (G >= 4) h = bits_dpp_add<0x4E>(h);    // quad_perm [2, 3, 0, 1]
    if (G >= 8) h = bits_dpp_add<0x141>(h);   // row_half_mirror
    if (G >= 16) h = bits_dpp_add<0x140>(h);  // row_mirror
    if (G >= 32) h += __shfl_xor(h, 16, kWave);
    return h;
}

// G lanes per row (lane t of the group holds chunk t; lanes with t >= nchunk load nothing: 3, 6, 12 or 24 chunks of 4, 8, 16, 32),
// U batches of 64 / G rows in flight per wave, NQ queries per pass (blockIdx.y).  A wave takes tiles of U * 64 / G consecutive
// rows, the grid strides over the tiles.  The NQ query chunks of a lane stay in its registers.
template <int G, int U, int NQ>
__global__ __launch_bounds__(kBitsThreads) void bits_scan_kernel(BitsScanArgs a) {
    constexpr int R = kWave / G;
    constexpr int NW = kBitsThreads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane & (G - 1);
    const int grp = lane / G;
    const int q0 = blockIdx.y * NQ;
    const bool live = t < a.nchunk;
    const int64_t rb = (int64_t)a.nchunk * 16;

    uint4 qv[NQ];
    WaveTopK tk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        qv[q] = (live && q0 + q < a.nq) ? *(const uint4*)(a.q + (int64_t)(q0 + q) * rb + t * 16) : make_uint4(0, 0, 0, 0);
        tk[q].init(a.k);
    }

    const int64_t stride = (int64_t)gridDim.x * NW * (R * U);
    for (int64_t base = ((int64_t)blockIdx.x * NW + wave) * (R * U); base < a.n; base += stride) {
        uint4 v[U];
        uint64_t mw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool in = row < a.n;
            v[u] = (live && in) ? bits_load16(a.rows + row * rb + t * 16) : make_uint4(0, 0, 0, 0);
            mw[u] = !in ? 0ull : (a.mask ? a.mask[row >> 6] : ~0ull);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool lead = t == 0 && ((mw[u] >> (row & 63)) & 1ull);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int h = bits_group_sum<G>(bits_hamming16(v[u], qv[q]));
                tk[q].offer(lead && q0 + q < a.nq ? bits_key(h, (uint32_t)row) : 0ull);
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

// ---- matrix-core form --------------------------------------------------------------------------------------------------
// v_mfma_i32_32x32x32_i8 (cos8_kernels.hpp feeds it the same way): A = 32 rows x 32 bytes, B = 32 bytes x 32 queries, C exact
// int32.  Lane l supplies row / query (l & 31) and the 16 bytes of half (l >> 5) of each 32-byte K step for BOTH operands, so A and
// B are paired element for element whatever the order inside the unit.  C lane l, element j: query (l & 31), row
// 8 (j >> 2) + 4 (l >> 5) + (j & 3).
//
// A K element is one BIT, expanded to a byte: +1 for a 0 bit, -1 for a 1 bit, so a.b = (equal bits) - (differing bits) = d - 2 H.
// Four bits x make one dword: x | x << 7 | x << 14 | x << 21 puts bit i at 8 i (the twelve other copies land between), the mask
// 0x01010101 keeps the four 0 / 1 bytes m, and m * 0xFE + 0x01010101 turns each into 0xFF or 0x01 — no byte exceeds 0xFF, nothing
// carries.  16 bits -> one operand of 16 bytes.
//
// Per 16-byte chunk c of a row, half h of the lanes takes its bytes [8 h, 8 h + 8): one 8-byte load, four operands (byte pairs
// j = 0..3), four MFMAs.  The queries are expanded ONCE, in the prologue, into LDS in the order the lanes read them: operand
// (c, j, h) of query q at q * ls + ((4 c + j) * 2 + h) * 16, ls = d_bits + 16 (the pad keeps the 16-byte reads off each other's
// banks, as cos8_mfma_lds_stride).  Row bits never touch LDS.  Behind the queries: one sorted k-list per wave and query.
__host__ __device__ constexpr int bits_mfma_lds_stride(int d_bits) { return d_bits + 16; }
__host__ __device__ constexpr size_t bits_mfma_lds_bytes(int d_bits, int k, int nwaves) {
    return (size_t)kBitsMfmaQ * bits_mfma_lds_stride(d_bits) + (size_t)nwaves * kBitsMfmaQ * k * sizeof(uint64_t);
}

__device__ __forceinline__ uint32_t bits_expand4(uint32_t x) {  // x < 16
    uint32_t y = x | (x << 7);
    y |= y << 14;
    return (y & 0x01010101u) * 0xFEu + 0x01010101u;
}
__device__ __forceinline__ bits_i32x4 bits_expand16(uint32_t v) {  // the low 16 bits of v
    bits_i32x4 r;
    r.x = (int)bits_expand4(v & 15u);
    r.y = (int)bits_expand4((v >> 4) & 15u);
    r.z = (int)bits_expand4((v >> 8) & 15u);
    r.w = (int)bits_expand4((v >> 12) & 15u);
    return r;
}

struct BitsMfmaArgs {
    const uint8_t* rows;
    int nchunk;
    int d_bits;
    int64_t n;
    const uint64_t* mask;
    const uint8_t* q;
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k]
};

// blockDim.x = 64 * (1 | 2 | 4 | 8); a wave takes tiles of 32 rows, the grid strides over them; blockIdx.y: the slab of 32 queries.
__global__ __launch_bounds__(kBitsMfmaMaxThreads) void bits_mfma_kernel(BitsMfmaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bits_lds[];
    const int NW = blockDim.x >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int qn = lane & 31;
    const int q0 = blockIdx.y * kBitsMfmaQ;
    const int ls = bits_mfma_lds_stride(a.d_bits);
    const int rb = a.nchunk * 16;
    const int k = a.k;
    unsigned char* qsh = bits_lds;
    uint64_t* lists = (uint64_t*)(bits_lds + kBitsMfmaQ * ls);

    // expand the slab's queries (rows past nq: all zero bits, never offered) and clear the lists
    const int npair = rb >> 1;
    for (int i = threadIdx.x; i < kBitsMfmaQ * npair; i += blockDim.x) {
        const int qq = i / npair, p = i - qq * npair;
        const uint32_t v = q0 + qq < a.nq ? *(const uint16_t*)(a.q + (int64_t)(q0 + qq) * rb + 2 * p) : 0u;
        const int c = p >> 3, h = (p >> 2) & 1, j = p & 3;
        *(bits_i32x4*)(qsh + qq * ls + ((4 * c + j) * 2 + h) * 16) = bits_expand16(v);
    }
    for (int i = threadIdx.x; i < NW * kBitsMfmaQ * k; i += blockDim.x) lists[i] = 0ull;
    __syncthreads();

    const bool qlive = q0 + qn < a.nq;
    uint64_t gate = 0;  // the k-th key of this lane's query list (0: not full)
    uint64_t* mylists = lists + (int64_t)wave * kBitsMfmaQ * k;
    const unsigned char* qrow = qsh + qn * ls + half * 16;

    const int64_t stride = (int64_t)gridDim.x * NW * 32;
    for (int64_t r0 = ((int64_t)blockIdx.x * NW + wave) * 32; r0 < a.n; r0 += stride) {
        const int64_t ra = r0 + qn;  // the row this lane feeds into A
        const bool va = ra < a.n;
        const uint8_t* src = a.rows + (va ? ra : 0) * rb + half * 8;
        bits_i32x16 acc = {};
        for (int c0 = 0; c0 < a.nchunk; c0 += 4) {
            bits_u32x2 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                w[u] = (va && c0 + u < a.nchunk) ? __builtin_nontemporal_load((const bits_u32x2*)(src + (c0 + u) * 16))
                                                 : bits_u32x2{0u, 0u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u < a.nchunk) {
                    const unsigned char* qb = qrow + (c0 + u) * 128;
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bits_expand16(w[u].x), *(const bits_i32x4*)(qb), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bits_expand16(w[u].x >> 16), *(const bits_i32x4*)(qb + 32), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bits_expand16(w[u].y), *(const bits_i32x4*)(qb + 64), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(bits_expand16(w[u].y >> 16), *(const bits_i32x4*)(qb + 96), acc, 0, 0, 0);
                }
            }
        }
        // which rows of the tile are selected: lanes 0..31 look (row r0 + lane), the others fetch
        int sel_l = 0;
        if (lane < 32 && va) sel_l = a.mask ? (int)((a.mask[ra >> 6] >> (ra & 63)) & 1ull) : 1;
        uint64_t cand[16];
        bool pass[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int m = 8 * (j >> 2) + 4 * half + (j & 3);
            const int sel = __shfl(sel_l, m, kWave);
            cand[j] = bits_key((a.d_bits - acc[j]) >> 1, (uint32_t)(r0 + m));
            pass[j] = qlive && sel && cand[j] > gate;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint64_t todo = __ballot(pass[j]);
            while (todo) {
                const int srcl = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint64_t key = readlane_u64(cand[j], srcl);
                const int q = srcl & 31;
                const uint64_t kth = lds_list_insert(mylists + q * k, k, key, lane);
                if (qn == q) gate = kth;
            }
        }
    }
    __syncthreads();
    // fold the waves' lists per query and write this block's partial list
    for (int q = wave; q < kBitsMfmaQ; q += NW) {
        WaveTopK tk;
        tk.init(k);
        for (int w = 0; w < NW; ++w) tk.offer(lane < k ? lists[((int64_t)w * kBitsMfmaQ + q) * k + lane] : 0ull);
        if (q0 + q < a.nq && lane < k) a.cand[((int64_t)(q0 + q) * gridDim.x + blockIdx.x) * k + lane] = tk.key;
    }
}

// ---- merge and housekeeping --------------------------------------------------------------------------------------------
// One block per query: the nlists partial lists -> sorted top-k; missing slots I = -1, D = INT32_MAX.
__global__ __launch_bounds__(kBitsThreads) void bits_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k,
                                                                  int32_t* __restrict__ D, int64_t* __restrict__ I) {
    constexpr int NW = kBitsThreads / kWave;
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
        D[o] = tk.key ? bits_key_distance(tk.key) : kBitsNoDistance;
        I[o] = tk.key ? (int64_t)key_row(tk.key) : -1;
    }
}

__global__ void bits_fill_missing_kernel(int32_t* D, int64_t* I, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = kBitsNoDistance;
        I[i] = -1;
    }
}

// removal: dst row j <- src row keep[j], out of place, one 16-byte chunk per thread
__global__ __launch_bounds__(256) void bits_gather_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ keep,
                                                          int64_t m, int nchunk, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    ((uint4*)dst)[j * nchunk + ch] = ((const uint4*)src)[keep[j] * nchunk + ch];
}

// set_rows with packed input: staged row j -> stored row rows[j] (distinct rows: checked on the host)
__global__ __launch_bounds__(256) void bits_scatter_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ rows,
                                                           int64_t m, int nchunk, uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * nchunk) return;
    const int64_t j = i / nchunk;
    const int ch = (int)(i - j * nchunk);
    ((uint4*)dst)[rows[j] * nchunk + ch] = ((const uint4*)src)[j * nchunk + ch];
}

}  // namespace mvdb
