// mx_kernels.hpp — kernels of the MX index (mx.hip; contract in include/mvdb.h "MX INDEX" and INTEGRATION.md 3y).
//
// Rows are OCP microscaling blocks: 32 elements (E2M1 nibbles: MXFP4, or E4M3 bytes: MXFP8) under one E8M0 scale byte.  They are
// scored by v_mfma_scale_f32_16x16x128_f8f6f4, which multiplies FP4 / FP8 operands directly and applies one E8M0 scale per lane
// and operand.  In a 16x16x128 step lane l supplies row (A) or query (B) l & 15; with g = l >> 4, an FP4 operand's four registers
// are K [32 g, 32 g + 32) — one 16-byte chunk of the row as it is stored — and an FP8 operand's eight are K [16 g, 16 g + 16)
// and K [64 + 16 g, 64 + 16 g + 16): the step's chunks g and 4 + g.
// The lane's scale byte belongs to K block g, [32 g, 32 g + 32), whatever the element format — so FP8 elements and their scale
// come from different lanes' loads, which costs nothing: both are plain loads.  A row goes from HBM into the A operand with no
// LDS and no VALU work.  The result: lane l holds rows 4 (l >> 4) + i, i = 0..3, of column l & 15.
//
// Device layout.  codes[n, d * FMT / 8] as the host gives them.  Scales TRANSPOSED per row: [n, 4, S4] bytes, S4 = d / 128
// rounded up to 4 — the scale of MX block 4 t + b (K step t, K block b) sits at byte b * S4 + t — so the scales a lane needs for
// K steps 4 g .. 4 g + 3 are ONE dword and the instruction's opsel picks the byte.  The MXFP8 queries have the same two layouts.
//
//   mx_encode_kernel<FMT>      fp32 rows -> codes + scales: one wave per row, a lane quad per MX block; also the queries.
//   mx_scan_kernel<FMT,QB,REG> 16 QB queries per row read; REG: the B operands stay in registers (d <= 1024, <= 16 queries).
//   mx_merge_kernel            the blocks' partial lists -> D (fp32 scores), I (int64 rows).
//   mx_merge_keys_kernel       refined search: one segment's partial lists -> its best keys, left as keys for the re-rank.
//   mx_move_kernel             codes and scales of listed rows, together: removal (gather) and set_rows_codes (scatter).
#pragma once
#include <float.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kMxThreads = 256;        // encode, merge
constexpr int kMxMaxDim = 4096;
constexpr int kMxMaxThreads = 512;     // the scan's block: 1, 2, 4 or 8 waves
constexpr int kMxRegSteps = 8;         // the register form holds the B operands of up to 8 K steps (d <= 1024)

typedef int mx_i32x4 __attribute__((ext_vector_type(4)));
typedef int mx_i32x8 __attribute__((ext_vector_type(8)));
typedef float mx_f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int mx_s4(int d) { return ((d >> 7) + 3) & ~3; }
__host__ __device__ constexpr int mx_row_bytes(int d, int fmt) { return d * fmt / 8; }
// where the scale of MX block `blk` sits in a transposed scale row
__host__ __device__ constexpr int mx_scale_slot(int blk, int s4) { return (blk & 3) * s4 + (blk >> 2); }

// ---- encoding --------------------------------------------------------------------------------------------------------------
// The element grids.  E2M1: 1 sign, 2 exponent (bias 1), 1 mantissa bit; largest 6, 2^emax = 4.  E4M3: 1, 4 (bias 7), 3; largest
// 448 (0x7E; 0x7F is NaN and never written), 2^emax = 256.
template <int FMT>
struct MxGrid;
template <>
struct MxGrid<4> {
    static constexpr int M = 1, BIAS = 1, EMAX = 2, SIGN = 0x8;
    static constexpr float MAXV = 6.0f, MIN_NORMAL = 1.0f, INV_SUB = 2.0f;
};
template <>
struct MxGrid<8> {
    static constexpr int M = 3, BIAS = 7, EMAX = 8, SIGN = 0x80;
    static constexpr float MAXV = 448.0f, MIN_NORMAL = 0.015625f, INV_SUB = 512.0f;
};

// |x| of a finite x as its bits (an order-preserving image), 0 for NaN and inf: the block maximum ignores them
__device__ __forceinline__ uint32_t mx_finite_abs(float x) {
    const uint32_t a = __float_as_uint(x) & 0x7FFFFFFFu;
    return a >= 0x7F800000u ? 0u : a;
}

// e = floor(log2(amax)) - emax clamped to [-127, 127], 0 for amax == 0; amax comes as its bits.  A subnormal amax has exponent
// field 0: -127 - emax, which the clamp brings to -127 as it brings the true logarithm.
template <int FMT>
__device__ __forceinline__ int mx_exponent(uint32_t amax_bits) {
    if (amax_bits == 0u) return 0;
    const int e = (int)(amax_bits >> 23) - 127 - MxGrid<FMT>::EMAX;
    return e < -127 ? -127 : e;  // (e <= 127 - emax)
}

// u = x * 2^-e (v_ldexp_f32: exact), clamped to the largest element, rounded to the nearest grid value, ties to the even code.
// Below the smallest normal the codes are the integers u / step, so rintf rounds them; above, the code is the float's bits cut to
// M mantissa bits with the usual add-half-minus-one-plus-lsb, and the carry walks into the exponent by itself.  NaN: code 0.
template <int FMT>
__device__ __forceinline__ uint32_t mx_code(float x, int e) {
    using G = MxGrid<FMT>;
    if (x != x) return 0u;
    const uint32_t sign = (__float_as_uint(x) >> 31) ? (uint32_t)G::SIGN : 0u;
    const float a = fminf(fabsf(ldexpf(x, -e)), G::MAXV);
    uint32_t code;
    if (a < G::MIN_NORMAL) {
        code = (uint32_t)(int)rintf(a * G::INV_SUB);
    } else {
        constexpr int SH = 23 - G::M;
        const uint32_t b = __float_as_uint(a);
        code = ((b + ((1u << (SH - 1)) - 1u) + ((b >> SH) & 1u)) >> SH) - ((uint32_t)(127 - G::BIAS) << G::M);
    }
    return sign | code;
}

template <int CTRL>
__device__ __forceinline__ uint32_t mx_dpp_max(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
    return v > o ? v : o;
}

struct MxEncodeArgs {
    const float* x;        // [n, d]
    int64_t n;
    int d;
    const int64_t* rows;   // nullptr: staged row i -> row i of the outputs; else -> row rows[i] (distinct, checked on the host)
    uint8_t* codes;        // [., d FMT / 8]
    uint8_t* scales;       // [., 4, S4]
    int* valid;            // nullptr, or [n]: 0 where the row has a non-finite component (queries)
};

// One wave per row.  Of each slab of 512 dimensions lane l takes [8 l, 8 l + 8), so a lane quad owns an MX block: the block's
// amax is two quad_perm steps, the exponent comes from its bits, and a lane writes its 8 codes as one dword (FP4: nibble m is
// dimension 8 l + m, the row's byte order) or as 8 bytes (FP8) — a quad's stores are one or two whole 16-byte chunks — and the
// quad's first lane the scale byte into the transposed plane.
template <int FMT>
__global__ __launch_bounds__(kMxThreads) void mx_encode_kernel(MxEncodeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * (kMxThreads / kWave) + (threadIdx.x >> 6);
    if (i >= a.n) return;  // (wave-uniform)
    const float* src = a.x + i * a.d;
    const int64_t r = a.rows ? a.rows[i] : i;
    const int s4 = mx_s4(a.d);
    uint8_t* crow = a.codes + r * mx_row_bytes(a.d, FMT);
    uint8_t* srow = a.scales + r * 4 * s4;
    bool bad = false;
    for (int base = lane * 8; base < a.d; base += 8 * kWave) {
        const float4 xa = *(const float4*)(src + base), xb = *(const float4*)(src + base + 4);
        const float v[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        uint32_t amax = 0u;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const uint32_t f = mx_finite_abs(v[m]);
            bad |= (__float_as_uint(v[m]) & 0x7F800000u) == 0x7F800000u;
            amax = f > amax ? f : amax;
        }
        amax = mx_dpp_max<0xB1>(amax);  // quad_perm [1, 0, 3, 2]
        amax = mx_dpp_max<0x4E>(amax);  // quad_perm [2, 3, 0, 1]
        const int e = mx_exponent<FMT>(amax);
        if (FMT == 4) {
            uint32_t w = 0u;
#pragma unroll
            for (int m = 0; m < 8; ++m) w |= mx_code<4>(v[m], e) << (4 * m);
            *(uint32_t*)(crow + (base >> 1)) = w;
        } else {
            uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                w0 |= mx_code<8>(v[m], e) << (8 * m);
                w1 |= mx_code<8>(v[m + 4], e) << (8 * m);
            }
            *(uint2*)(crow + base) = make_uint2(w0, w1);
        }
        if ((lane & 3) == 0) srow[mx_scale_slot(base >> 5, s4)] = (uint8_t)(e + 127);
    }
    // the pad of the scale plane (S4 > d / 128) is never read by a scan; it is cleared so a stored row is a function of its values
    const int nstep = a.d >> 7;
    for (int p = lane; p < 4 * (s4 - nstep); p += kWave) srow[(p / (s4 - nstep)) * s4 + nstep + p % (s4 - nstep)] = 0;
    if (a.valid) {
        const bool any_bad = __ballot(bad) != 0ull;
        if (lane == 0) a.valid[i] = !any_bad;
    }
}

// ---- scan ------------------------------------------------------------------------------------------------------------------
// LDS of a block: [REG ? nothing : 16 QB queries at stride d + 16, then their scale planes], then one sorted k-list per wave and
// query.  (The 16-byte pad keeps the 16-byte reads of neighbouring queries off each other's banks: a first guess, not swept.)
__host__ __device__ constexpr int mx_lds_stride(int d) { return d + 16; }
__host__ __device__ constexpr size_t mx_lds_query_bytes(int d, int qb) {
    return (size_t)16 * qb * (mx_lds_stride(d) + 4 * mx_s4(d));
}
__host__ __device__ constexpr size_t mx_lds_bytes(int d, int k, int qb, int nwaves, bool reg) {
    return (reg ? 0 : mx_lds_query_bytes(d, qb)) + (size_t)nwaves * 16 * qb * k * sizeof(uint64_t);
}

struct MxScanArgs {
    const uint8_t* codes;    // [n, d FMT / 8]
    const uint8_t* scales;   // [n, 4, S4]
    int d;
    int64_t n;
    const uint64_t* mask;    // nullptr: every row; else bit r & 63 of word r >> 6 set = row r selected
    const uint8_t* q8;       // [nq, d] E4M3
    const uint8_t* qs;       // [nq, 4, S4]
    int nq;
    int k;
    uint64_t* cand;          // [nq][gridDim.x][k] keys
    int64_t base = 0;        // added to a row's number in its key: the rows are a segment that starts there (refined search)
};

template <int N>
__device__ __forceinline__ void mx_load_chunks(const uint8_t* p, bool on, mx_i32x8& v) {
    const mx_i32x4 z = {0, 0, 0, 0};
    const mx_i32x4 lo = on ? __builtin_nontemporal_load((const mx_i32x4*)p) : z;
    const mx_i32x4 hi = (on && N == 2) ? __builtin_nontemporal_load((const mx_i32x4*)(p + 64)) : z;
    v = mx_i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

// one K step: A in format FMT, B E4M3, byte OP of each scale dword
template <int FMT, int OP>
__device__ __forceinline__ mx_f32x4 mx_mfma(mx_i32x8 a, mx_i32x8 b, mx_f32x4 c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FMT == 4 ? 4 : 0, 0, OP, sa, OP, sb);
}

// blockDim.x = 64 * (1 | 2 | 4 | 8).  A wave takes groups of T tiles of 16 rows — T = 4 (FP4) or 2 (FP8): 64 bytes per lane and
// K-step quartet in flight either way —, the grid strides over the groups; blockIdx.y: the slab of 16 QB queries.  Per quartet of
// K steps a lane loads, for each tile, its row's four blocks and ONE scale dword; each B operand is fetched once (registers or
// LDS) and used for the T tiles.  Every (row, query) has one fp32 accumulator, K ascending: the same instruction and order
// whatever QB, REG or the tile a row falls into, so a query's scores do not depend on its batch.
template <int FMT, int QB, bool REG>
__global__ __launch_bounds__(kMxMaxThreads) void mx_scan_kernel(MxScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_lds[];
    constexpr int NQS = 16 * QB;
    constexpr int T = FMT == 4 ? 4 : 2;
    constexpr int CH = FMT == 4 ? 1 : 2;       // 16-byte chunks per MX block
    static_assert(!REG || QB == 1, "the register form holds one group of 16 queries");
    const int NW = blockDim.x >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int col = lane & 15;                 // row of the tile (A), query of the group (B and C)
    const int kb = lane >> 4;                  // K block of the step (A and B), row quartet (C)
    const int q0 = blockIdx.y * NQS;
    const int d = a.d, k = a.k;
    const int nstep = d >> 7;
    const int s4 = mx_s4(d);
    const int rb = mx_row_bytes(d, FMT);
    const int ls = mx_lds_stride(d);
    unsigned char* qsh = mx_lds;
    unsigned char* ssh = mx_lds + (REG ? 0 : NQS * ls);
    uint64_t* lists = (uint64_t*)(mx_lds + (REG ? 0 : mx_lds_query_bytes(d, QB)));

    // the slab's queries (past nq: zero codes and scales, never offered) and empty lists
    mx_i32x8 bq[REG ? kMxRegSteps : 1];
    int bs[REG ? kMxRegSteps / 4 : 1];
    if (REG) {
        const bool on = q0 + col < a.nq;
        const uint8_t* qp = a.q8 + (int64_t)(on ? q0 + col : 0) * d + 16 * kb;
        const uint8_t* sp = a.qs + ((int64_t)(on ? q0 + col : 0) * 4 + kb) * s4;
#pragma unroll
        for (int t = 0; t < (REG ? kMxRegSteps : 1); ++t) {
            const mx_i32x4 z = {0, 0, 0, 0};
            const bool live = on && t < nstep;
            const mx_i32x4 lo = live ? *(const mx_i32x4*)(qp + 128 * t) : z;
            const mx_i32x4 hi = live ? *(const mx_i32x4*)(qp + 128 * t + 64) : z;
            bq[t] = mx_i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        }
#pragma unroll
        for (int g = 0; g < (REG ? kMxRegSteps / 4 : 1); ++g) bs[g] = (on && 4 * g < nstep) ? *(const int*)(sp + 4 * g) : 0;
    } else {
        const int per = d >> 4;
        for (int i = threadIdx.x; i < NQS * per; i += blockDim.x) {
            const int qq = i / per, p = i - qq * per;
            mx_i32x4 v = {0, 0, 0, 0};
            if (q0 + qq < a.nq) v = *(const mx_i32x4*)(a.q8 + (int64_t)(q0 + qq) * d + p * 16);
            *(mx_i32x4*)(qsh + qq * ls + p * 16) = v;
        }
        for (int i = threadIdx.x; i < NQS * s4; i += blockDim.x) {  // (4 S4 bytes per query = S4 dwords)
            const int qq = i / s4;
            ((int*)ssh)[i] = q0 + qq < a.nq ? ((const int*)a.qs)[(int64_t)q0 * s4 + i] : 0;
        }
    }
    for (int i = threadIdx.x; i < NW * NQS * k; i += blockDim.x) lists[i] = 0ull;
    __syncthreads();

    bool qlive[QB];
    uint64_t gate[QB];  // the k-th key of this lane's query list (0: not full)
#pragma unroll
    for (int g = 0; g < QB; ++g) {
        qlive[g] = q0 + 16 * g + col < a.nq;
        gate[g] = 0ull;
    }
    uint64_t* mylists = lists + (int64_t)wave * NQS * k;

    const int64_t stride = (int64_t)gridDim.x * NW * (16 * T);
    for (int64_t r0 = ((int64_t)blockIdx.x * NW + wave) * (16 * T); r0 < a.n; r0 += stride) {
        bool va[T];
        const uint8_t* crow[T];
        const uint8_t* srow[T];
        mx_f32x4 acc[T][QB];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int64_t ra = r0 + 16 * t + col;  // the row this lane feeds into A
            va[t] = ra < a.n;
            crow[t] = a.codes + (va[t] ? ra : 0) * rb + 16 * kb;
            srow[t] = a.scales + ((va[t] ? ra : 0) * 4 + kb) * s4;
#pragma unroll
            for (int g = 0; g < QB; ++g) acc[t][g] = mx_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int s0 = 0; s0 < (REG ? kMxRegSteps : kMxMaxDim / 128); s0 += 4) {
            if (s0 >= nstep) break;  // (wave-uniform)
            mx_i32x8 w[T][4];
            int sa[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int u = 0; u < 4; ++u) mx_load_chunks<CH>(crow[t] + (s0 + u) * (64 * CH), va[t] && s0 + u < nstep, w[t][u]);
                sa[t] = va[t] ? *(const int*)(srow[t] + s0) : 0;
            }
#define MVDB_MX_STEP(U)                                                                                              \
    if (s0 + U < nstep) {                                                                                            \
        _Pragma("unroll") for (int g = 0; g < QB; ++g) {                                                             \
            mx_i32x8 b;                                                                                              \
            int sb;                                                                                                  \
            if (REG) {                                                                                               \
                b = bq[REG ? s0 + U : 0];                                                                            \
                sb = bs[REG ? s0 / 4 : 0];                                                                           \
            } else {                                                                                                 \
                const unsigned char* qp = qsh + (16 * g + col) * ls + 128 * (s0 + U) + 16 * kb;                      \
                const mx_i32x4 lo = *(const mx_i32x4*)qp, hi = *(const mx_i32x4*)(qp + 64);                          \
                b = mx_i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};                                        \
                sb = *(const int*)(ssh + ((16 * g + col) * 4 + kb) * s4 + s0);                                       \
            }                                                                                                        \
            _Pragma("unroll") for (int t = 0; t < T; ++t) acc[t][g] = mx_mfma<FMT, U>(w[t][U], b, acc[t][g], sa[t], sb); \
        }                                                                                                            \
    }
            MVDB_MX_STEP(0)
            MVDB_MX_STEP(1)
            MVDB_MX_STEP(2)
            MVDB_MX_STEP(3)
#undef MVDB_MX_STEP
        }
        // offers: lanes 0..15 look their tile row up in the bitmap, a lane's four results fetch the bits of their rows
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int64_t rt = r0 + 16 * t;
            if (rt >= a.n) break;  // (wave-uniform)
            int sel_l = 0;
            if (lane < 16 && va[t]) sel_l = a.mask ? (int)((a.mask[(rt + lane) >> 6] >> ((rt + lane) & 63)) & 1ull) : 1;
#pragma unroll
            for (int g = 0; g < QB; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = 4 * kb + j;
                    const int sel = __shfl(sel_l, m, kWave);
                    const float s = acc[t][g][j];
                    const uint64_t key = make_key(s, (uint32_t)(a.base + rt + m));
                    uint64_t todo = __ballot(qlive[g] && sel && s == s && key > gate[g]);
                    while (todo) {
                        const int srcl = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        const uint64_t kn = readlane_u64(key, srcl);
                        const int q = srcl & 15;
                        const uint64_t kth = lds_list_insert(mylists + (16 * g + q) * k, k, kn, lane);
                        if (col == q) gate[g] = kth;
                    }
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
// One block per query: the nlists partial lists -> sorted top-k; missing slots (and every slot of a query that is not valid)
// I = -1, D = -FLT_MAX.
__global__ __launch_bounds__(kMxThreads) void mx_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k,
                                                              const int* __restrict__ valid, float* __restrict__ D,
                                                              int64_t* __restrict__ I) {
    constexpr int NW = kMxThreads / kWave;
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
        D[o] = hit ? key_score(tk.key) : -FLT_MAX;
        I[o] = hit ? (int64_t)key_row(tk.key) : -1;
    }
}

// The refined search's merge, one block per query: the nlists partial lists of ONE segment -> its f best keys, left as keys in
// slots [seg f, seg f + f) of the query's candidate list keys[nq, nseg f] for the re-rank to read (refine_kernels.hpp).  An
// empty segment (nlists == 0) and a query that is not valid leave zeros: no candidates.
__global__ __launch_bounds__(kMxThreads) void mx_merge_keys_kernel(const uint64_t* __restrict__ cand, int nlists, int f,
                                                                   const int* __restrict__ valid, int seg, int nseg,
                                                                   uint64_t* __restrict__ keys) {
    constexpr int NW = kMxThreads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const uint64_t* src = cand + (int64_t)qi * nlists * f;
    WaveTopK tk;
    tk.init(f);
    const int64_t total = (int64_t)nlists * f;
    for (int64_t i0 = (int64_t)wave * kWave; i0 < total; i0 += (int64_t)NW * kWave) {
        const int64_t i = i0 + lane;
        tk.offer(i < total ? src[i] : 0ull);
    }
    block_merge_topk(tk, sh, NW);
    if (wave == 0 && lane < f) keys[((int64_t)qi * nseg + seg) * f + lane] = valid[qi] ? tk.key : 0ull;
}

__global__ void mx_fill_missing_kernel(float* D, int64_t* I, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

// Row j of the source -> row j of the destination, codes and scales together, one 16-byte chunk per thread (a scale row, 4 S4
// bytes, is whole chunks too).  from != nullptr: the source row is from[j] (removal gathers survivors); to != nullptr: the
// destination row is to[j] (set_rows_codes scatters; distinct rows, checked on the host).
__global__ __launch_bounds__(256) void mx_move_kernel(const uint8_t* __restrict__ src_codes, const uint8_t* __restrict__ src_scales,
                                                      const int64_t* __restrict__ from, const int64_t* __restrict__ to, int64_t m,
                                                      int cchunk, int schunk, uint8_t* __restrict__ dst_codes,
                                                      uint8_t* __restrict__ dst_scales) {
    const int per = cchunk + schunk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * per) return;
    const int64_t j = i / per;
    const int ch = (int)(i - j * per);
    const int64_t rs = from ? from[j] : j, rd = to ? to[j] : j;
    if (ch < cchunk) ((uint4*)dst_codes)[rd * cchunk + ch] = ((const uint4*)src_codes)[rs * cchunk + ch];
    else ((uint4*)dst_scales)[rd * schunk + ch - cchunk] = ((const uint4*)src_scales)[rs * schunk + ch - cchunk];
}

}  // namespace mvdb
