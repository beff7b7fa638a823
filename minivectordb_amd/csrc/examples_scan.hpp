// examples_scan.hpp — search by examples (mvdb_index_search_examples): the question is P positive and N negative vectors, a
// row scores by its nearest positive unless a negative is at least as near (include/mvdb.h "SEARCH BY EXAMPLES", DESIGN.md
// section 6n).
//
//   examples_clear_kernel   zeroes the running pair of every stored row: one 64-bit word per PHYSICAL row, the high half the order
//                           image (f2ord) of the best positive score so far, the low half that of the best negative score; 0 in
//                           a half = no offer yet (the image of every non-NaN score is above 0).
//   examples_scan_kernel    one pass over the selected rows for Vp <= 32 consecutive vectors of the concatenated [P + N, d]
//                           matrix.  It is assign_scan_kernel (assign_scan.hpp) with the bookkeeping changed: the same
//                           (G, C, U, SEL, MASKED) forms from the one shape table, the same prologue (maxsim_load_vector), the
//                           same load order, the same non-temporal row loads and SUBSET prefetch of the next batch's row ids,
//                           and per (row, vector) the same chunk order of fmaf and the same butterfly (maxsim_butterfly) — a
//                           score is bit for bit the single-query scan's.  Lane t follows row t % U and keeps TWO images
//                           instead of (image, vector): vector v of the pass is a positive iff v0 + v < P (a pass may straddle
//                           the boundary), its score goes to the maximum of its side; a NaN never offers.  Lanes t < U then
//                           merge both halves into their row's word with a plain read / max / write: the group owns the row for
//                           the pass, passes follow each other on the stream, and a row listed twice is written twice with the
//                           same value.  No atomics, no score tile, no LDS beyond the vectors, no workgroup waits for another.
//                           A maximum does not depend on how the vectors are cut into passes.
//   examples_skip_kernel    zeroes the words of the skip rows (rows outside [0, n) are ignored): they are never results.
//   examples_topk_kernel    strides over the n words; S = bp if bp > bn else -(bn * bn) — the fp32 `>`, one fp32 multiply and
//                           a negation; a zero high half is no key, a zero low half is bn = -inf —; every block keeps its k
//                           best make_key(S, row) as a sorted list (equal S: the lower row).
//   examples_emit_kernel    one block merges the block lists and writes D, I (+ label_offset) and the padding.
//
// Bytes of a call: passes x (n * ld * 4 + 8 n; + 8 n of a row list, + n / 8 of a bitmap) + 16 n (the words cleared and read
// once by the selection) — under 1 % of a pass at d = 512.
#pragma once
#include "assign_scan.hpp"

namespace mvdb {

constexpr int kExamplesMaxVectors = 256;  // P + N of one call
constexpr int kExamplesMaxSkip = 1024;    // skip rows of one call
constexpr int kExamplesLists = 256;       // most block lists of examples_topk_kernel

// THE rule of the vectors per pass: MaxSim's (knob: index option examples_vectors_per_pass, 0 = none)
inline int examples_vectors_per_pass(int V, int64_t ld, int knob) { return maxsim_tokens_per_pass(V, ld, knob); }

__global__ __launch_bounds__(256) void examples_clear_kernel(uint64_t* __restrict__ best, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) best[i] = 0ull;
}

struct ExamplesScanArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [Vp, ld] the pass's vectors (device), zero padded
    int Vp;                // vectors of this pass
    int v0;                // number, in the call, of the pass's first vector
    int P;                 // vector j of the CALL is a positive iff j < P
    int normalize_q;       // L2-normalise every vector in the prologue
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    uint64_t* best;        // [n_phys] running pair of every physical row: f2ord(bp) << 32 | f2ord(bn), 0 in a half = none
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kMaxsimThreads) void examples_scan_kernel(ExamplesScanArgs a) {
    extern __shared__ __align__(16) unsigned char examples_lds[];
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int Vp = a.Vp;
    // vectors [0, npos) of the pass are positives, the rest negatives
    const int npos = a.P - a.v0 < 0 ? 0 : (a.P - a.v0 < Vp ? a.P - a.v0 : Vp);
    float* const qs = reinterpret_cast<float*>(examples_lds);  // [Vp, ld]

    bool cvalid[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cvalid[c] = !MASKED || c * G + t < a.d4;

    // ---- the vectors -> LDS (maxsim_scan_kernel's prologue) -------------------------------------------------------------------
    {
        constexpr int kGroups = kMaxsimThreads / G;
        const int gi = threadIdx.x / G;
        for (int v0 = 0; v0 < Vp; v0 += kGroups) {  // (uniform over the block: the reduction runs with every lane on)
            const int v = v0 + gi;
            const bool live = v < Vp;
            f32x4 qv[C];
            maxsim_load_vector<G, C>(a.q + (int64_t)(live ? v : 0) * a.ld, t, cvalid, a.normalize_q, qv);
            if (live) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (cvalid[c]) *reinterpret_cast<f32x4*>(qs + (int64_t)v * a.ld + (c * G + t) * 4) = qv[c];
            }
        }
    }
    __syncthreads();

    const int64_t nwaves_total = (int64_t)gridDim.x * kMaxsimWaves;
    const int64_t gw = (int64_t)blockIdx.x * kMaxsimWaves + wave;
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t last = a.n - 1;

    auto batch_rows = [&](int64_t b, int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;  // clamp: tail lanes re-read the last row, result discarded
            pr[u] = SUBSET ? a.rows[r] : r;
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
        // After the butterfly every lane of a row's group holds the score of each of the U rows in flight: lane t follows ONE of
        // them, row t % U, so the bookkeeping below runs once per vector, not U times.
        const int mu = t % U;
        uint32_t op = 0u;  // image of that row's best positive score of the pass (0: none — every non-NaN image is above it)
        uint32_t on = 0u;  // ... and of its best negative score
        for (int v = 0; v < Vp; ++v) {
            const float* qp = qs + (int64_t)v * a.ld + t * 4;
            f32x4 qv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) qv[c] = cvalid[c] ? *reinterpret_cast<const f32x4*>(qp + c * G * 4) : f32x4{0, 0, 0, 0};
            float s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    acc = fmaf(x[u][c].x, qv[c].x, acc);
                    acc = fmaf(x[u][c].y, qv[c].y, acc);
                    acc = fmaf(x[u][c].z, qv[c].z, acc);
                    acc = fmaf(x[u][c].w, qv[c].w, acc);
                }
                s[u] = acc;
            }
            maxsim_butterfly<G, U>(s);
            float mine = s[0];
#pragma unroll
            for (int u = 1; u < U; ++u) mine = mu == u ? s[u] : mine;
            const uint32_t o = mine == mine ? f2ord(mine) : 0u;  // a NaN fails s == s
            if (v < npos)                                         // (uniform)
                op = o > op ? o : op;
            else
                on = o > on ? o : on;
        }
        if (t < U && (op | on)) {  // lane t of the group: row t of the U
            // (its position again, by arithmetic — and its list entry / bitmap word re-read, both cached — instead of a pick
            //  out of the U registers of the batch: a register array indexed by the lane would live in scratch)
            const int64_t pos = row0 + (int64_t)mu * RPI;
            bool offered = pos < a.n;
            if (SEL == 2) offered = offered && ((a.mask[pos >> 6] >> (pos & 63)) & 1ull);
            if (offered) {
                const int64_t row = SUBSET ? a.rows[pos] : pos;
                uint64_t* const w = a.best + row;
                const uint64_t old = *w;
                const uint32_t hp = (uint32_t)(old >> 32), hn = (uint32_t)old;
                const uint64_t now = ((uint64_t)(op > hp ? op : hp) << 32) | (uint64_t)(on > hn ? on : hn);
                if (now != old) *w = now;
            }
        }
    };

    if (SUBSET) {
        // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
        int64_t pr[U], pn[U];
        if (gw < nbatches) batch_rows(gw, pr);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            load_batch(pr, x);
            const int64_t bn = b + nwaves_total;
            batch_rows(bn < nbatches ? bn : b, pn);
            consume_batch(b, x);
#pragma unroll
            for (int u = 0; u < U; ++u) pr[u] = pn[u];
        }
    } else {  // every row, or the rows of a bitmap: all are scored, the bit decides at the merge
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            batch_rows(b, pr);
            load_batch(pr, x);
            consume_batch(b, x);
        }
    }
}

// the skip rows' words back to "no offer": rows outside [0, n) are ignored (the host entry point refuses them beforehand)
__global__ __launch_bounds__(256) void examples_skip_kernel(uint64_t* __restrict__ best, int64_t n, const int64_t* __restrict__ skip, int n_skip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_skip) {
        const int64_t r = skip[i];
        if (r >= 0 && r < n) best[r] = 0ull;  // (duplicates write the same value)
    }
}

struct ExamplesTopkArgs {
    const uint64_t* best;  // [n] the rows' words
    int64_t n;
    int k;
    uint64_t* part;        // [gridDim.x, 64] the blocks' sorted lists of make_key(S, row), 0 = none
};

__global__ __launch_bounds__(kDistinctThreads) void examples_topk_kernel(ExamplesTopkArgs a) {
    __shared__ uint64_t merge[(kDistinctWaves - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    WaveTopK tk;
    tk.init(a.k);
    // (the bound is uniform over the wave: offer is wave-cooperative)
    for (int64_t base = (int64_t)blockIdx.x * kDistinctThreads + (threadIdx.x - lane); base < a.n; base += (int64_t)gridDim.x * kDistinctThreads) {
        const int64_t i = base + lane;
        uint64_t key = 0ull;
        if (i < a.n) {
            const uint64_t word = a.best[i];
            const uint32_t hp = (uint32_t)(word >> 32), hn = (uint32_t)word;
            if (hp) {  // a row no positive offered to is never a result
                const float bp = ord2f(hp);
                const float bn = hn ? ord2f(hn) : -INFINITY;
                const float sq = bn * bn;
                const float S = bp > bn ? bp : -sq;
                key = make_key(S, (uint32_t)i);
            }
        }
        tk.offer(key);
    }
    block_merge_topk(tk, merge, kDistinctWaves);
    if (threadIdx.x < kWave) a.part[(int64_t)blockIdx.x * kWave + threadIdx.x] = tk.key;  // (lanes >= k hold 0)
}

struct ExamplesEmitArgs {
    const uint64_t* part;  // [nlists, 64]
    int nlists;            // 0: an empty index or an empty set — every output is padding
    int k;
    int64_t label_offset;
    float* D;              // [k]
    int64_t* I;            // [k]
};

__global__ __launch_bounds__(kDistinctThreads) void examples_emit_kernel(ExamplesEmitArgs a) {
    __shared__ uint64_t merge[(kDistinctWaves - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    WaveTopK tk;
    tk.init(a.k);
    const int total = a.nlists * kWave;
    for (int base = (int)threadIdx.x - lane; base < total; base += kDistinctThreads) tk.offer(a.part[base + lane]);
    block_merge_topk(tk, merge, kDistinctWaves);
    if ((int)threadIdx.x < a.k) {  // wave 0 (k <= 64): lane i holds the i-th best row
        const uint64_t key = tk.key;
        a.D[threadIdx.x] = key ? key_score(key) : -3.402823466e+38f;
        a.I[threadIdx.x] = key ? (int64_t)key_row(key) + a.label_offset : -1;
    }
}

}  // namespace mvdb
