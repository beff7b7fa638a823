// mmr_select.hpp — the selection stage of MMR search (mvdb_index_search_mmr): k diverse rows picked greedily from the
// fetch_k candidates a plain search has just written (include/mvdb.h "MMR SEARCH").
//
// One workgroup per query, no communication between workgroups: the only waits are __syncthreads.  Step 0 takes candidate
// position 0; step t >= 1 takes the unpicked valid position j that maximises
//     obj[j] = lambda * rel[j] - (1 - lambda) * max over the picked p of s(p, j),
// ties to the lower position, a NaN objective ranking as -inf.  maxsim[j] is carried from step to step, so a step only
// forms s(last pick, j): k - 1 passes over the candidates, the last pick needs none.
//
// s(p, j), the inner product of two stored rows at the matrix' stride (the zero padding behind d adds nothing): lane l of
// the wave that owns j takes the 16-byte chunks l, l + 64, ... in ascending order, four fmaf per chunk in element order,
// then the 32 ... 1 xor butterfly.  That order is a function of the row stride alone — not of j, of the step, of the query
// or of the form — so exact duplicate rows score bit-identically and a call is reproducible.
//
// Wave w owns the positions w, w + W, ...: at most 64 of them (fetch_k <= 1024 = 64 W), so "picked" is one 64-bit
// register per wave, and maxsim[j] is only ever touched by the wave that owns j.
//
// Two forms (mvdb.hip: mmr_form_rule decides on the host, from the row stride, fetch_k and the device's LDS alone):
//   FORM 0  the candidate rows are gathered into LDS once; every step reads LDS.          HBM/L2: fetch_k * ld * 4 bytes
//   FORM 1  only the row picked last is kept in LDS; every step reads the candidates' rows from the matrix, through L2:
//           (k - 1) * fetch_k * ld * 4 bytes per query, at most fetch_k * ld * 4 of them distinct (2 MiB at 1024 x 512).
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

constexpr int kMmrThreads = 1024;
constexpr int kMmrWaves = kMmrThreads / kWave;
constexpr int kMmrMaxFetch = 1024;
constexpr int kMmrUnroll = 4;                       // candidates a wave has in flight (FORM 1: their loads overlap)
constexpr size_t kMmrStaticLds = 512;               // the two-deep per-wave argmax slots below, as the code object reports them
static_assert(kMmrMaxFetch <= 64 * kMmrWaves, "a wave's picked positions must fit one 64-bit register");
static_assert(kMmrMaxFetch <= kMmrThreads, "one __syncthreads_count counts the valid candidates");
static_assert(64 % kMmrUnroll == 0, "a wave's 64 position slots are walked in whole groups");

// dynamic LDS of a launch: the row tile (FORM 0: every candidate; FORM 1: the row picked last), then per candidate its
// row number (8), rel (4) and maxsim (4)
inline size_t mmr_lds_bytes(int form, int fetch_k, int64_t ld) {
    return (size_t)(form == 0 ? fetch_k : 1) * (size_t)ld * sizeof(float) + (size_t)fetch_k * 16;
}

struct MmrArgs {
    const float* X;         // [n, ld] corpus
    int64_t ld;             // row stride in floats (multiple of 4)
    const float* candD;     // [nq, fetch_k] stage 1: scores (rel), best first
    const int64_t* candI;   // [nq, fetch_k] stage 1: row numbers (label_offset 0), -1 = missing
    int fetch_k, k;
    float lambda, mu;       // mu = 1 - lambda, rounded once on the host
    int64_t label_offset;
    float* D;               // [nq, k]
    int64_t* I;             // [nq, k]
};

template <int FORM>
__global__ __launch_bounds__(kMmrThreads) void mmr_select_kernel(MmrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mmr_lds[];
    __shared__ float wobj[2][kMmrWaves];
    __shared__ int wpos[2][kMmrWaves];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int F = a.fetch_k;
    const int c4 = (int)(a.ld >> 2);  // 16-byte chunks per row
    f32x4* tile = reinterpret_cast<f32x4*>(mmr_lds);
    int64_t* crow = reinterpret_cast<int64_t*>(mmr_lds + (size_t)(FORM == 0 ? F : 1) * (size_t)a.ld * sizeof(float));
    float* rel = reinterpret_cast<float*>(crow + F);
    float* maxsim = rel + F;
    const float* cD = a.candD + (int64_t)blockIdx.x * F;
    const int64_t* cI = a.candI + (int64_t)blockIdx.x * F;
    float* D = a.D + (int64_t)blockIdx.x * a.k;
    int64_t* I = a.I + (int64_t)blockIdx.x * a.k;

    bool valid = false;
    if (tid < F) {
        const int64_t r = cI[tid];
        crow[tid] = r;
        rel[tid] = cD[tid];
        maxsim[tid] = -INFINITY;
        valid = r >= 0;
    }
    const int nvalid = __syncthreads_count(valid);
    const int npick = crow[0] >= 0 ? min(a.k, nvalid) : 0;
    for (int t = npick + tid; t < a.k; t += kMmrThreads) {  // fewer valid candidates than k: the tail is missing
        D[t] = -3.402823466e+38f;
        I[t] = -1;
    }
    if (npick == 0) return;
    if (tid == 0) {
        D[0] = rel[0];
        I[0] = crow[0] + a.label_offset;
    }
    if (npick == 1) return;

    if (FORM == 0) {  // the candidates' rows, once
        const int total = F * c4;
        for (int e = tid; e < total; e += kMmrThreads) {
            const int j = e / c4;
            const int64_t r = crow[j];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r >= 0) v = reinterpret_cast<const f32x4*>(a.X + r * a.ld)[e - j * c4];
            tile[e] = v;
        }
        __syncthreads();
    }

    unsigned long long mine = wave == 0 ? 1ull : 0ull;  // bit i: position wave + i * W has been picked
    int last = 0;
    for (int t = 1; t < npick; ++t) {
        const f32x4* lastrow = tile;
        if (FORM == 0) {
            lastrow = tile + (size_t)last * c4;
        } else {
            const f32x4* src = reinterpret_cast<const f32x4*>(a.X + crow[last] * a.ld);
            for (int c = tid; c < c4; c += kMmrThreads) tile[c] = src[c];
            __syncthreads();
        }
        float best = -INFINITY;
        int bpos = 0x7fffffff;
        for (int i0 = 0; i0 * kMmrWaves + wave < F; i0 += kMmrUnroll) {
            const f32x4* row[kMmrUnroll];
            bool live[kMmrUnroll];
            float acc[kMmrUnroll];
#pragma unroll
            for (int u = 0; u < kMmrUnroll; ++u) {
                const int j = (i0 + u) * kMmrWaves + wave;
                live[u] = j < F && !((mine >> (i0 + u)) & 1ull) && crow[j] >= 0;
                // (a slot that is not live reads the row picked last again and its sum is dropped)
                if (FORM == 0) row[u] = live[u] ? tile + (size_t)j * c4 : lastrow;
                else row[u] = reinterpret_cast<const f32x4*>(a.X + crow[live[u] ? j : last] * a.ld);
                acc[u] = 0.f;
            }
            for (int c = lane; c < c4; c += kWave) {
                const f32x4 p = lastrow[c];
                f32x4 v[kMmrUnroll];
#pragma unroll
                for (int u = 0; u < kMmrUnroll; ++u) v[u] = row[u][c];
#pragma unroll
                for (int u = 0; u < kMmrUnroll; ++u) {
                    acc[u] = fmaf(v[u].x, p.x, acc[u]);
                    acc[u] = fmaf(v[u].y, p.y, acc[u]);
                    acc[u] = fmaf(v[u].z, p.z, acc[u]);
                    acc[u] = fmaf(v[u].w, p.w, acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kMmrUnroll; ++u) {
#pragma unroll
                for (int off = kWave / 2; off >= 1; off >>= 1) acc[u] += __shfl_xor(acc[u], off);
                if (!live[u]) continue;
                const int j = (i0 + u) * kMmrWaves + wave;
                const float s = acc[u];
                float ms = maxsim[j];
                ms = (s != s || ms != ms) ? NAN : fmaxf(ms, s);  // a NaN similarity stays
                if (lane == 0) maxsim[j] = ms;
                float obj = __fsub_rn(__fmul_rn(a.lambda, rel[j]), __fmul_rn(a.mu, ms));
                if (!(obj == obj)) obj = -INFINITY;
                if (obj > best || bpos == 0x7fffffff) {  // j ascends within the wave: an equal objective keeps the lower position
                    best = obj;
                    bpos = j;
                }
            }
        }
        const int slot = t & 1;  // two-deep: the next step's writes cannot overtake this step's reads
        if (lane == 0) {
            wobj[slot][wave] = best;
            wpos[slot][wave] = bpos;
        }
        __syncthreads();
        float gbest = wobj[slot][0];
        int gpos = wpos[slot][0];
#pragma unroll
        for (int w = 1; w < kMmrWaves; ++w) {
            const float o = wobj[slot][w];
            const int p = wpos[slot][w];
            if (o > gbest || (o == gbest && p < gpos)) {
                gbest = o;
                gpos = p;
            }
        }
        // npick <= the valid candidates: some wave had a live position, so gpos is one
        last = gpos;
        if ((gpos & (kMmrWaves - 1)) == wave) mine |= 1ull << (gpos / kMmrWaves);
        if (tid == 0) {
            D[t] = rel[gpos];
            I[t] = crow[gpos] + a.label_offset;
        }
    }
}

}  // namespace mvdb
