// rabitq_kernels.hpp — kernels of the RaBitQ index (rabitq.hip; contract in include/mvdb.h "RaBitQ index" and INTEGRATION.md 3x).
//
// A row is the sign bits of its centred, rotated image — d / 8 bytes in numpy.packbits order, 1 to 32 chunks of 16 — and three
// numbers beside them: f = |r|^2 / |r|_1, g = <x - c, c> and B = 2 popcount(code) - d.  A query is rotated the same way and cut
// to 4 bits per dimension, u in [0, 15], with lo, delta, qc = <q, c> and U = sum u.  T = sum u[i] code[i] is an exact integer —
// on the VALU sum_p 2^p popcount(code & plane_p), on the matrix cores an int8 product of 0 / 1 bytes with u — and the score
//     S = fl(fl(f * fl(fl(delta * (2 T - U)) + fl(lo * B))) + fl(g + qc))
// is four unfused fp32 operations on exact integers, so every form and batch size returns the same bits.  The key is
// topk_device.hpp's make_key(S, row): WaveTopK, lds_list_insert and block_merge_topk serve as they stand; a NaN score fails the
// `s == s` gate in front of every make_key.
//
//   rbq_rotate         R rounds of sign flips + a Walsh-Hadamard butterfly over a power-of-two window, one wave per vector.
//   rbq_encode_kernel  fp32 rows -> code, (f, g), B: one wave per row.
//   rbq_query_kernel   fp32 queries -> 4 bit planes, the u bytes in the matrix-core order, (lo, delta, qc, U): one wave per query.
//   rbq_scan_kernel    1, 2 or 4 queries per pass on the VALU: G lanes per row, 16-byte loads, AND + v_bcnt against 4 planes.
//   rbq_mfma_kernel    32 or 64 queries per row read on the int8 matrix cores: row bits expanded to 0 / 1 bytes in registers.
//   rbq_merge_kernel   the blocks' partial lists -> D (fp32 S), I (int64 rows).
#pragma once
#include <float.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_device.hpp"

namespace mvdb {

constexpr int kRbqThreads = 256;          // encode, scan, merge
constexpr int kRbqMaxChunks = 32;         // d <= 4096
constexpr int kRbqMaxRounds = 4;
constexpr int kRbqMfmaMaxThreads = 512;   // the matrix-core block: 1, 2, 4 or 8 waves, by what the lists leave of the LDS

typedef int rbq_i32x4 __attribute__((ext_vector_type(4)));
typedef int rbq_i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned rbq_u32x2 __attribute__((ext_vector_type(2)));

// ---- the rotation ----------------------------------------------------------------------------------------------------------
// The vector lives in a wave-private strip of LDS, element e at w[e], and lane l owns the elements e = 64 j + l: it alone reads
// and writes them, so the strip is per-lane storage with a run-time index and needs no barrier.  Both windows start at a
// multiple of 64 ([0, P) and [d - P, d); d and P are multiples of 128), so window element i sits in lane i & 63, register
// i >> 6 of the NR = P / 64 a lane loads: the stages h = 1 .. 32 cross lanes, the stages h = 64 .. P / 2 pair registers of one
// lane, and the order h = 1, 2, 4, ... of the contract is the order below.  One LDS round trip per ROUND (the elements outside
// the window have to wait somewhere, and a register file indexed by the window offset would cost a kernel per width); the
// butterfly itself never leaves the registers.
struct RbqRotation {
    const uint8_t* signs;   // [R, d / 8] numpy.packbits order, a set bit negates
    int R;
    float scale;            // the fp32 nearest 1 / sqrt(P)
};

template <int CTRL>
__device__ __forceinline__ float rbq_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// pair (i, i + h) -> (a + b, a - b): the lane whose bit h is clear holds a
template <int H>
__device__ __forceinline__ float rbq_lane_stage(float v, int lane) {
    float p;
    if (H == 1) p = rbq_dpp<0xB1>(v);        // quad_perm [1, 0, 3, 2]
    else if (H == 2) p = rbq_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    else if (H == 8) p = rbq_dpp<0x128>(v);  // row_ror:8 — lane ^ 8 inside a row of 16
    else p = __shfl_xor(v, H, kWave);
    return (lane & H) ? p - v : v + p;
}

template <int NR>
__device__ __forceinline__ void rbq_rotate(float* w, int d, RbqRotation rot, int lane) {
    const int nreg = d >> 6;
    const int rb = d >> 3;
    for (int r = 0; r < rot.R; ++r) {
        const uint8_t* sg = rot.signs + r * rb;
        for (int j = 0; j < nreg; ++j) {
            const int e = j * kWave + lane;
            if ((sg[e >> 3] >> (7 - (e & 7))) & 1) w[e] = -w[e];
        }
        float* win = w + ((r & 1) ? d - NR * kWave : 0) + lane;
        float v[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            float t = win[j * kWave];
            t = rbq_lane_stage<1>(t, lane);
            t = rbq_lane_stage<2>(t, lane);
            t = rbq_lane_stage<4>(t, lane);
            t = rbq_lane_stage<8>(t, lane);
            t = rbq_lane_stage<16>(t, lane);
            v[j] = rbq_lane_stage<32>(t, lane);
        }
#pragma unroll
        for (int s = 1; s < NR; s <<= 1) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if (!(j & s)) {
                    const float a = v[j], b = v[j | s];
                    v[j] = a + b;
                    v[j | s] = a - b;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) win[j * kWave] = v[j] * rot.scale;
    }
}

__device__ __forceinline__ double rbq_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// 64 predicates, lane l = dimension 64 s + l -> the 8 bytes of numpy.packbits (bits_kernels.hpp: bits_pack_kernel)
__device__ __forceinline__ uint64_t rbq_pack64(bool bit) { return __builtin_bswap64(__brevll(__ballot(bit))); }

// ---- encoding --------------------------------------------------------------------------------------------------------------
struct RbqEncodeArgs {
    const float* x;         // [n, d]
    int64_t n;
    int d;
    const float* c;         // [d] the centroid
    RbqRotation rot;
    const int64_t* rows;    // nullptr: staged row i -> stored row i of the outputs; else -> stored row rows[i] (distinct rows)
    uint8_t* codes;         // [.., d / 8]
    float2* fg;
    int32_t* B;
};

// One wave per row, blockDim.x / 64 rows per block, d floats of dynamic LDS per wave.  The sums of f and g are fp64 sums of
// products that are exact in fp64 (24 x 24 bits), rounded to fp32 once.
template <int NR>
__global__ __launch_bounds__(kRbqThreads) void rbq_encode_kernel(RbqEncodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rbq_strip[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * (kRbqThreads / kWave) + wave;
    if (i >= a.n) return;  // (wave-uniform)
    float* w = rbq_strip + wave * a.d;
    const float* src = a.x + i * a.d;
    const int nreg = a.d >> 6;
    double gs = 0.0;
    for (int j = 0; j < nreg; ++j) {
        const int e = j * kWave + lane;
        const float cv = a.c[e];
        const float r = src[e] - cv;
        w[e] = r;
        gs += (double)r * (double)cv;
    }
    rbq_rotate<NR>(w, a.d, a.rot, lane);
    double n1 = 0.0, n2 = 0.0;
    uint64_t mine = 0;
    int ones = 0;
    for (int j = 0; j < nreg; ++j) {
        const float r = w[j * kWave + lane];
        n2 += (double)r * (double)r;
        n1 += fabs((double)r);
        // r > 0 on the bit pattern — [0x00000001, 0x7F800000]: denormals count, NaN and -0 do not
        const uint64_t word = rbq_pack64(__float_as_uint(r) - 1u < 0x7F800000u);
        ones += __popcll(word);
        if (lane == j) mine = word;
    }
    gs = rbq_wave_sum(gs);
    n1 = rbq_wave_sum(n1);
    n2 = rbq_wave_sum(n2);
    const int64_t r = a.rows ? a.rows[i] : i;
    if (lane < nreg) ((uint64_t*)(a.codes + r * (a.d >> 3)))[lane] = mine;
    if (lane == 0) {
        a.fg[r] = make_float2(n1 == 0.0 ? 0.0f : (float)(n2 / n1), (float)gs);
        a.B[r] = 2 * ones - a.d;
    }
}

// add_codes: B = 2 popcount(code) - d for rows that arrive encoded, one thread per row
__global__ __launch_bounds__(256) void rbq_popcount_kernel(const uint8_t* __restrict__ codes, int64_t n, int nchunk, int d,
                                                           int32_t* __restrict__ B) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* src = (const uint4*)codes + i * nchunk;
    int ones = 0;
    for (int c = 0; c < nchunk; ++c) {
        const uint4 v = src[c];
        ones += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    B[i] = 2 * ones - d;
}

// ---- the query -------------------------------------------------------------------------------------------------------------
// Where dimension i of a query's u bytes sits: the order in which the lanes of the matrix-core form read them.  Byte b = i / 8
// of a code row belongs to chunk c = b / 16, half h = (b / 8) & 1, byte pair j = (b / 2) & 3; the pair is read as a
// little-endian 16-bit value, whose bit t — byte t / 8 of the pair, bit t & 7, which packbits gives dimension 7 - (t & 7) of that
// byte — is expanded into operand byte t.  Operand (c, j, h) is bytes [((4 c + j) * 2 + h) * 16, + 16).
__host__ __device__ constexpr int rbq_query_slot(int i) {
    const int b = i >> 3;
    return (((b >> 4) * 4 + ((b >> 1) & 3)) * 2 + ((b >> 3) & 1)) * 16 + ((b & 1) << 3) + 7 - (i & 7);
}

struct RbqQueryArgs {
    const float* q;         // [nq, d]
    int d;
    const float* c;
    RbqRotation rot;
    uint8_t* planes;        // [nq, 4, d / 8]: plane p holds bit p of every u, packed like a code
    uint8_t* u;             // [nq, d] in rbq_query_slot order
    float4* params;         // [nq]: lo, delta, qc, (float)U
};

// One block of one wave per query.  u = clamp(rintf((q' - lo) * inv), 0, 15): one subtract, one multiply, both fp32.
template <int NR>
__global__ __launch_bounds__(kWave) void rbq_query_kernel(RbqQueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rbq_strip[];
    const int lane = threadIdx.x;
    const int qi = blockIdx.x;
    const float* src = a.q + (int64_t)qi * a.d;
    float* w = rbq_strip;
    const int nreg = a.d >> 6;
    double qc = 0.0;
    for (int j = 0; j < nreg; ++j) {
        const int e = j * kWave + lane;
        const float qv = src[e], cv = a.c[e];
        w[e] = qv - cv;
        qc += (double)qv * (double)cv;
    }
    rbq_rotate<NR>(w, a.d, a.rot, lane);
    float lo = INFINITY, hi = -INFINITY;
    for (int j = 0; j < nreg; ++j) {
        lo = fminf(lo, w[j * kWave + lane]);
        hi = fmaxf(hi, w[j * kWave + lane]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, kWave));
        hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
    }
    const float span = hi - lo;
    const bool ok = span > 0.0f;
    const float delta = ok ? __fdiv_rn(span, 15.0f) : 0.0f;
    const float inv = ok ? __fdiv_rn(15.0f, span) : 0.0f;
    uint64_t mine[4] = {0, 0, 0, 0};
    int usum = 0;
    uint8_t* udst = a.u + (int64_t)qi * a.d;
    for (int j = 0; j < nreg; ++j) {
        const int e = j * kWave + lane;
        const float t = rintf((w[e] - lo) * inv);
        const int ui = t >= 15.0f ? 15 : !(t > 0.0f) ? 0 : (int)t;
        usum += ui;
        udst[rbq_query_slot(e)] = (uint8_t)ui;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint64_t word = rbq_pack64((ui >> p) & 1);
            if (lane == j) mine[p] = word;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) usum += __shfl_xor(usum, off, kWave);
    qc = rbq_wave_sum(qc);
    if (lane < nreg) {
#pragma unroll
        for (int p = 0; p < 4; ++p) ((uint64_t*)(a.planes + ((int64_t)qi * 4 + p) * (a.d >> 3)))[lane] = mine[p];
    }
    if (lane == 0) a.params[qi] = make_float4(lo, delta, (float)qc, (float)usum);
}

// ---- the score -------------------------------------------------------------------------------------------------------------
// prm = (lo, delta, qc, (float)U); every integer is below 2^24, so the conversions are exact
__device__ __forceinline__ float rbq_score(int T, float4 prm, float f, float g, int B) {
#pragma clang fp contract(off)
    const float A = (float)(2 * T - (int)prm.w);
    const float da = prm.y * A;
    const float lb = prm.x * (float)B;
    const float e = da + lb;
    const float fe = f * e;
    const float gq = g + prm.z;
    return fe + gq;
}

// a NaN score has no place in the key order (topk_device.hpp): it is no candidate
__device__ __forceinline__ uint64_t rbq_key(float s, uint32_t row) { return s == s ? make_key(s, row) : 0ull; }

// ---- VALU form -------------------------------------------------------------------------------------------------------------
struct RbqScanArgs {
    const uint8_t* codes;   // [n, 16 nchunk]
    const float2* fg;       // [n]
    const int32_t* B;       // [n]
    int nchunk;             // 16-byte chunks per row = d / 128
    int64_t n;
    const uint64_t* mask;   // nullptr: every row; else bit r & 63 of word r >> 6 set = row r selected
    const uint8_t* planes;  // [nq, 4, 16 nchunk]
    const float4* params;   // [nq]
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k] keys
};

__device__ __forceinline__ uint4 rbq_load16(const uint8_t* p) {
    const rbq_i32x4 v = __builtin_nontemporal_load((const rbq_i32x4*)p);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
}

// popcount(row & plane) over one chunk, added to acc: four ANDs, four accumulating v_bcnt_u32_b32
__device__ __forceinline__ int rbq_and_count(uint4 a, uint4 b, int acc) {
    acc += __builtin_popcount(a.x & b.x);
    acc += __builtin_popcount(a.y & b.y);
    acc += __builtin_popcount(a.z & b.z);
    return acc + __builtin_popcount(a.w & b.w);
}

template <int CTRL>
__device__ __forceinline__ int rbq_dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// the sum over the G lanes of a row, left in every one of them (bits_kernels.hpp: bits_group_sum)
template <int G>
__device__ __forceinline__ int rbq_group_sum(int h) {
    if (G >= 2) h = rbq_dpp_add<0xB1>(h);    // quad_perm [1, 0, 3, 2]
    if (G >= 4) h = rbq_dpp_add<0x4E>(h);    // quad_perm [2, 3, 0, 1]
    if (G >= 8) h = rbq_dpp_add<0x141>(h);   // row_half_mirror
    if (G >= 16) h = rbq_dpp_add<0x140>(h);  // row_mirror
    if (G >= 32) h += __shfl_xor(h, 16, kWave);
    return h;
}

// G lanes per row (lane t of the group holds chunk t; lanes with t >= nchunk load nothing), U batches of 64 / G rows in flight
// per wave, NQ queries per pass (blockIdx.y).  A wave takes tiles of U * 64 / G consecutive rows, the grid strides over the
// tiles.  A lane keeps the 4 planes x 4 dwords of its chunk per query in registers; the lane sums are weighted BEFORE the DPP
// ladder (T = T0 + 2 T1 + 4 T2 + 8 T3 is linear), so a row costs one ladder per query.
template <int G, int U, int NQ>
__global__ __launch_bounds__(kRbqThreads) void rbq_scan_kernel(RbqScanArgs a) {
    constexpr int R = kWave / G;
    constexpr int NW = kRbqThreads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane & (G - 1);
    const int grp = lane / G;
    const int q0 = blockIdx.y * NQ;
    const bool live = t < a.nchunk;
    const int64_t rb = (int64_t)a.nchunk * 16;

    uint4 pl[NQ][4];
    float4 prm[NQ];
    WaveTopK tk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const bool on = q0 + q < a.nq;
#pragma unroll
        for (int p = 0; p < 4; ++p)
            pl[q][p] = (live && on) ? *(const uint4*)(a.planes + ((int64_t)(q0 + q) * 4 + p) * rb + t * 16) : make_uint4(0, 0, 0, 0);
        prm[q] = on ? a.params[q0 + q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        tk[q].init(a.k);
    }

    const int64_t stride = (int64_t)gridDim.x * NW * (R * U);
    for (int64_t base = ((int64_t)blockIdx.x * NW + wave) * (R * U); base < a.n; base += stride) {
        uint4 v[U];
        uint64_t mw[U];
        float2 fg[U];
        int Bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool in = row < a.n;
            v[u] = (live && in) ? rbq_load16(a.codes + row * rb + t * 16) : make_uint4(0, 0, 0, 0);
            mw[u] = !in ? 0ull : (a.mask ? a.mask[row >> 6] : ~0ull);
            fg[u] = in ? a.fg[row] : make_float2(0.0f, 0.0f);
            Bv[u] = in ? a.B[row] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * R + grp;
            const bool lead = t == 0 && ((mw[u] >> (row & 63)) & 1ull);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int t0 = rbq_and_count(v[u], pl[q][0], 0), t1 = rbq_and_count(v[u], pl[q][1], 0);
                const int t2 = rbq_and_count(v[u], pl[q][2], 0), t3 = rbq_and_count(v[u], pl[q][3], 0);
                const int T = rbq_group_sum<G>(t0 + 2 * t1 + 4 * t2 + 8 * t3);
                const float s = rbq_score(T, prm[q], fg[u].x, fg[u].y, Bv[u]);
                tk[q].offer(lead && q0 + q < a.nq ? rbq_key(s, (uint32_t)row) : 0ull);
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
// v_mfma_i32_32x32x32_i8 fed as bits_kernels.hpp feeds it: A = 32 rows x 32 bytes, B = 32 bytes x 32 queries, C exact int32.
// Lane l supplies row / query (l & 31) and the 16 bytes of half (l >> 5) of each K step for BOTH operands.  C lane l, element j:
// query (l & 31), row 8 (j >> 2) + 4 (l >> 5) + (j & 3).
//
// A K element is one dimension: the row's bit as a 0 / 1 byte against the query's u byte, so C = T.  Four bits x make one
// dword: x | x << 7 | x << 14 | x << 21 puts bit i at 8 i and the mask 0x01010101 keeps the four bytes.  Per 16-byte chunk c of
// a row, half h of the lanes takes its bytes [8 h, 8 h + 8): one 8-byte load, four operands (byte pairs j = 0 .. 3), four MFMAs
// per block of 32 queries — at QB = 2 one row read and one expansion serve 64 queries.  The slab's u bytes sit in LDS as the
// query kernel wrote them (rbq_query_slot), query q at q * (d + 16): the pad keeps the 16-byte reads of neighbouring queries off
// each other's banks.  Row bits never touch LDS.  Behind the queries: one sorted k-list per wave and query.
__host__ __device__ constexpr int rbq_mfma_lds_stride(int d) { return d + 16; }
__host__ __device__ constexpr size_t rbq_mfma_lds_bytes(int d, int k, int qb, int nwaves) {
    return (size_t)32 * qb * rbq_mfma_lds_stride(d) + (size_t)nwaves * 32 * qb * k * sizeof(uint64_t);
}

__device__ __forceinline__ uint32_t rbq_expand4(uint32_t x) {  // x < 16
    uint32_t y = x | (x << 7);
    y |= y << 14;
    return y & 0x01010101u;
}
__device__ __forceinline__ rbq_i32x4 rbq_expand16(uint32_t v) {  // the low 16 bits of v
    rbq_i32x4 r;
    r.x = (int)rbq_expand4(v & 15u);
    r.y = (int)rbq_expand4((v >> 4) & 15u);
    r.z = (int)rbq_expand4((v >> 8) & 15u);
    r.w = (int)rbq_expand4((v >> 12) & 15u);
    return r;
}

struct RbqMfmaArgs {
    const uint8_t* codes;
    const float2* fg;
    const int32_t* B;
    int nchunk;
    int d;
    int64_t n;
    const uint64_t* mask;
    const uint8_t* u;       // [nq, d] in rbq_query_slot order
    const float4* params;
    int nq;
    int k;
    uint64_t* cand;         // [nq][gridDim.x][k]
};

// blockDim.x = 64 * (1 | 2 | 4 | 8); a wave takes tiles of 32 rows, the grid strides over them; blockIdx.y: the slab of 32 QB queries.
template <int QB>
__global__ __launch_bounds__(kRbqMfmaMaxThreads) void rbq_mfma_kernel(RbqMfmaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rbq_lds[];
    constexpr int NQS = 32 * QB;
    const int NW = blockDim.x >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int qn = lane & 31;
    const int q0 = blockIdx.y * NQS;
    const int ls = rbq_mfma_lds_stride(a.d);
    const int rb = a.nchunk * 16;
    const int k = a.k;
    unsigned char* qsh = rbq_lds;
    uint64_t* lists = (uint64_t*)(rbq_lds + NQS * ls);

    // the slab's queries (past nq: zeros, never offered) and empty lists
    const int per = a.d >> 4;
    for (int i = threadIdx.x; i < NQS * per; i += blockDim.x) {
        const int qq = i / per, p = i - qq * per;
        rbq_i32x4 v = {0, 0, 0, 0};
        if (q0 + qq < a.nq) v = *(const rbq_i32x4*)(a.u + (int64_t)(q0 + qq) * a.d + p * 16);
        *(rbq_i32x4*)(qsh + qq * ls + p * 16) = v;
    }
    for (int i = threadIdx.x; i < NW * NQS * k; i += blockDim.x) lists[i] = 0ull;
    __syncthreads();

    bool qlive[QB];
    uint64_t gate[QB];  // the k-th key of this lane's query list (0: not full)
    float4 prm[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        qlive[b] = q0 + 32 * b + qn < a.nq;
        gate[b] = 0ull;
        prm[b] = qlive[b] ? a.params[q0 + 32 * b + qn] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    uint64_t* mylists = lists + (int64_t)wave * NQS * k;
    const unsigned char* qrow = qsh + qn * ls + half * 16;

    const int64_t stride = (int64_t)gridDim.x * NW * 32;
    for (int64_t r0 = ((int64_t)blockIdx.x * NW + wave) * 32; r0 < a.n; r0 += stride) {
        const int64_t ra = r0 + qn;  // the row this lane feeds into A
        const bool va = ra < a.n;
        const uint8_t* src = a.codes + (va ? ra : 0) * rb + half * 8;
        rbq_i32x16 acc[QB];
#pragma unroll
        for (int b = 0; b < QB; ++b) acc[b] = rbq_i32x16{};
        for (int c0 = 0; c0 < a.nchunk; c0 += 4) {
            rbq_u32x2 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                w[u] = (va && c0 + u < a.nchunk) ? __builtin_nontemporal_load((const rbq_u32x2*)(src + (c0 + u) * 16))
                                                 : rbq_u32x2{0u, 0u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u < a.nchunk) {  // (wave-uniform)
                    const rbq_i32x4 x0 = rbq_expand16(w[u].x), x1 = rbq_expand16(w[u].x >> 16);
                    const rbq_i32x4 x2 = rbq_expand16(w[u].y), x3 = rbq_expand16(w[u].y >> 16);
#pragma unroll
                    for (int b = 0; b < QB; ++b) {
                        const unsigned char* qb = qrow + b * 32 * ls + (c0 + u) * 128;
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x0, *(const rbq_i32x4*)(qb), acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x1, *(const rbq_i32x4*)(qb + 32), acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x2, *(const rbq_i32x4*)(qb + 64), acc[b], 0, 0, 0);
                        acc[b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x3, *(const rbq_i32x4*)(qb + 96), acc[b], 0, 0, 0);
                    }
                }
            }
        }
        // lanes 0..31 fetch row r0 + lane's selection bit and factors, the others receive them
        int sel_l = 0, B_l = 0;
        float2 fg_l = make_float2(0.0f, 0.0f);
        if (lane < 32 && va) {
            sel_l = a.mask ? (int)((a.mask[ra >> 6] >> (ra & 63)) & 1ull) : 1;
            fg_l = a.fg[ra];
            B_l = a.B[ra];
        }
        int sel[16], Bv[16];
        float f[16], g[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int m = 8 * (j >> 2) + 4 * half + (j & 3);
            sel[j] = __shfl(sel_l, m, kWave);
            f[j] = __shfl(fg_l.x, m, kWave);
            g[j] = __shfl(fg_l.y, m, kWave);
            Bv[j] = __shfl(B_l, m, kWave);
        }
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            uint64_t cand[16];
            bool pass[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = 8 * (j >> 2) + 4 * half + (j & 3);
                cand[j] = rbq_key(rbq_score(acc[b][j], prm[b], f[j], g[j], Bv[j]), (uint32_t)(r0 + m));
                pass[j] = qlive[b] && sel[j] && cand[j] > gate[b];
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
// One block per query: the nlists partial lists -> sorted top-k; D is the key's score, missing slots I = -1, D = -FLT_MAX.
__global__ __launch_bounds__(kRbqThreads) void rbq_merge_kernel(const uint64_t* __restrict__ cand, int nlists, int k,
                                                                float* __restrict__ D, int64_t* __restrict__ I) {
    constexpr int NW = kRbqThreads / kWave;
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
        D[o] = tk.key ? key_score(tk.key) : -FLT_MAX;
        I[o] = tk.key ? (int64_t)key_row(tk.key) : -1;
    }
}

__global__ void rbq_fill_missing_kernel(float* D, int64_t* I, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

// Rows on the move, code and factors together: row (to ? to[j] : j) of the destination <- row (from ? from[j] : j) of the source.
// One 16-byte chunk per thread, and one thread per row for (f, g) and B.  Removal gathers (from = the survivors) into a staging
// copy, set_rows with encoded input scatters (to = the row list: distinct rows, checked on the host).
struct RbqStore {
    uint8_t* codes;
    float2* fg;
    int32_t* B;
};
__global__ __launch_bounds__(256) void rbq_move_kernel(RbqStore src, const int64_t* __restrict__ from, const int64_t* __restrict__ to,
                                                       int64_t m, int nchunk, RbqStore dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = nchunk + 1;
    if (i >= m * per) return;
    const int64_t j = i / per;
    const int ch = (int)(i - j * per);
    const int64_t s = from ? from[j] : j, t = to ? to[j] : j;
    if (ch < nchunk) {
        ((uint4*)dst.codes)[t * nchunk + ch] = ((const uint4*)src.codes)[s * nchunk + ch];
    } else {
        dst.fg[t] = src.fg[s];
        dst.B[t] = src.B[s];
    }
}

}  // namespace mvdb
