// maxsim_scan.hpp — MaxSim search (mvdb_index_search_maxsim): ONE question of T query vectors, a document (a GROUP of stored
// rows) scores the sum over the vectors of its best row for each vector (include/mvdb.h "MAXSIM SEARCH").
//
//   maxsim_clear_kernel    zeroes the table of the call: n_groups x T 64-bit words, group-major.
//   maxsim_scan_kernel     one pass over the selected rows for Tp <= 32 of the vectors.  It is group_best_scan_kernel
//                          (distinct_select.hpp) with the query side turned into a run-time loop: the same (G, C, MASKED), the
//                          same load order per row (code, then the row, nontemporal), and per (row, vector) the same chunk
//                          order of fmaf and the same G/2 ... 1 xor butterfly — a score is bit for bit the single-query
//                          scan's (the butterfly's lower steps as DPP modifiers: maxsim_butterfly_step).  The Tp vectors
//                          live in LDS, normalised once in the prologue by the scan's own prologue arithmetic (the G
//                          lanes of a group of threads own one vector at a time); a row's registers are
//                          reused across the vectors, and one 16-byte LDS read of a query chunk feeds the U rows a lane holds.
//                          The scores of a wave's batch, RB rows x Tp vectors, are parked in a per-wave LDS tile (NaN for a row
//                          that is not selected or past the end: a NaN is never offered); then the 64 lanes walk the tile, lane
//                          per (row, vector), and offer make_key(score, position) to table[code][vector] with an atomicMax
//                          behind a plain load — the Tp words of one row are consecutive, so the loads of a row are one or
//                          two cache lines however many vectors the pass carries.  Within a call a word only grows: a stale
//                          read costs a spare atomic, never a wrong answer (section 6i), and an integer maximum does not
//                          depend on the order of arrival.  No workgroup waits for another.
//   maxsim_topk_kernel     strides over the groups; a group's T words are folded IN ORDER into S = m[0] + m[1] + ... with plain
//                          fp32 adds; a zero word (no offer for that vector) or a NaN sum drops the group; every block keeps its
//                          k best make_key(S, code) — equal sums go to the lower code — as a sorted list.
//   maxsim_emit_kernel     one block merges the block lists and writes D, G and, from the winners' table words, I_tok / D_tok.
//
// Bytes of a call: passes x (n * ld * 4 + 4 n; + 8 n of a row list, + n / 8 of a bitmap) + 3 x 8 T n_groups (the table
// cleared, offered to, read once).
#pragma once
#include "code8_scan.hpp"
#include "distinct_select.hpp"

namespace mvdb {

constexpr int kMaxsimMaxTokens = 256;     // T of one call
constexpr int kMaxsimPassTokens = 32;     // most vectors of one pass, whatever the width
constexpr size_t kMaxsimQueryLds = 128u << 10;  // LDS the vectors of a pass may take (of 160 KiB; the score tiles need <= 17 KiB more)
constexpr int kMaxsimThreads = 512;
constexpr int kMaxsimWaves = kMaxsimThreads / kWave;
constexpr int kMaxsimLists = 256;         // most block lists of maxsim_topk_kernel

// THE rule of the vectors per pass, from T and the row stride alone (knob: index option maxsim_tokens_per_pass, 0 = none)
inline int maxsim_tokens_per_pass(int T, int64_t ld, int knob) {
    const int64_t fit = std::max<int64_t>(1, (int64_t)kMaxsimQueryLds / (ld * 4));
    int64_t tp = std::min<int64_t>(std::min<int64_t>(T, kMaxsimPassTokens), fit);
    if (knob > 0) tp = std::min<int64_t>(tp, knob);
    return (int)tp;
}
// dynamic LDS of a pass: the vectors, then per wave a tile of RB x Tp scores, then per wave RB codes
inline size_t maxsim_lds_bytes(int Tp, int64_t ld, int RB) {
    return 4 * ((size_t)Tp * (size_t)ld + (size_t)kMaxsimWaves * RB * ((size_t)Tp + 1));
}
// rows in flight per wave: twice the streaming scan's where the registers allow, so that a query chunk read from LDS feeds
// several rows (a score does not depend on U)
constexpr int maxsim_u(int G, int C) { return C <= 3 ? 4 : C <= 8 ? 2 : 1; }

__global__ __launch_bounds__(256) void maxsim_clear_kernel(uint64_t* __restrict__ table, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) table[i] = 0ull;
}

// an empty index or an empty set: every output is padding
__global__ void maxsim_fill_missing_kernel(float* D, int32_t* G, int64_t* I_tok, float* D_tok, int k, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) {
        D[i] = -3.402823466e+38f;
        G[i] = -1;
    }
    if (i < k * T) {
        if (I_tok) I_tok[i] = -1;
        if (D_tok) D_tok[i] = -3.402823466e+38f;
    }
}

// the lanes of ONE wave hand values to each other through LDS: LDS serves a wave's accesses in order, the fences keep the
// compiler from moving them across
__device__ __forceinline__ void maxsim_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One step of flat_scan_kernel's butterfly, s += (s of lane l ^ M), with the same two operands in every lane — the same
// bits — and, for M <= 8, without the trip through the LDS crossbar that __shfl_xor takes: the pass runs the butterfly once
// per (row, vector) and the crossbar is the unit it is bound by.  M = 8, 2, 1 are DPP operand modifiers (lane_xor,
// code8_scan.hpp).  M = 4 is row_ror:4, which hands lane l the value of lane (l +- 4) mod 16 of its row of 16: the steps run
// M = G/2 ... 1, so the step M = 8 has run and a value equals that of the lane across bit 3 — both candidates hold what
// lane l ^ 4 holds.
template <int M>
__device__ __forceinline__ float maxsim_butterfly_step(float s) {
    if constexpr (M == 4)
        return s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x124, 0xF, 0xF, false));  // row_ror:4
    else if constexpr (M == 1 || M == 2 || M == 8)
        return s + __int_as_float(lane_xor<M>(__float_as_int(s)));
    else
        return s + __shfl_xor(s, M);
}
template <int G, int U, int M = G / 2>
__device__ __forceinline__ void maxsim_butterfly(float (&s)[U]) {
    static_assert(G >= 16, "the step M = 4 relies on the step M = 8 before it");
    if constexpr (M >= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = maxsim_butterfly_step<M>(s[u]);  // (the U butterflies are independent: step by step)
        maxsim_butterfly<G, U, M / 2>(s);
    }
}

// One query vector into the registers of the G lanes that own it (lane t of the group: chunks c * G + t), normalised or not:
// flat_scan_kernel's prologue, the same operation order.  Every lane of the wave runs it (the reduction needs them all on).
// Shared by the MaxSim pass and the assignment pass (assign_scan.hpp), which also writes k-means' centres with it.
template <int G, int C>
__device__ __forceinline__ void maxsim_load_vector(const float* qptr, int t, const bool (&cvalid)[C], int normalize, f32x4 (&qv)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int chunk = c * G + t;
        qv[c] = cvalid[c] ? *reinterpret_cast<const f32x4*>(qptr + chunk * 4) : f32x4{0, 0, 0, 0};
    }
    if (normalize) {
        float nr = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c)
            nr += qv[c].x * qv[c].x + qv[c].y * qv[c].y + qv[c].z * qv[c].z + qv[c].w * qv[c].w;
        nr = group_reduce_add<G>(nr);
        if (nr > 0.f) {
            const float inorm = 1.0f / sqrtf(nr);
#pragma unroll
            for (int c = 0; c < C; ++c) qv[c] *= inorm;
        }
    }
}

struct MaxsimScanArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [Tp, ld] the pass's query vectors (device), zero padded
    int Tp;                // vectors of this pass
    int normalize_q;       // L2-normalise every vector in the prologue
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    const int32_t* codes;  // [n_phys] group code of every stored row
    uint64_t* table;       // the word of (group 0, first vector of the pass); group g, vector v of the pass: table[g * T + v]
    int T;                 // words per group
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kMaxsimThreads) void maxsim_scan_kernel(MaxsimScanArgs a) {
    extern __shared__ __align__(16) unsigned char maxsim_lds[];
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int Tp = a.Tp;
    float* const qs = reinterpret_cast<float*>(maxsim_lds);                     // [Tp, ld]
    float* const sc = qs + (int64_t)Tp * a.ld + (int64_t)wave * RB * Tp;        // this wave's [RB, Tp] scores
    int32_t* const cs = reinterpret_cast<int32_t*>(qs + (int64_t)Tp * a.ld + (int64_t)kMaxsimWaves * RB * Tp) + wave * RB;

    bool cvalid[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cvalid[c] = !MASKED || c * G + t < a.d4;

    // ---- the vectors -> LDS (flat_scan_kernel's prologue, same operation order, a group of G lanes per vector) ----------------
    {
        constexpr int kGroups = kMaxsimThreads / G;
        const int gi = threadIdx.x / G;
        for (int v0 = 0; v0 < Tp; v0 += kGroups) {  // (uniform over the block: the reduction below runs with every lane on)
            const int v = v0 + gi;
            const bool live = v < Tp;
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
    // the rows' codes first — one 4-byte word per row —, then the rows (group_best_scan_kernel's order)
    auto load_batch = [&](const int64_t (&pr)[U], f32x4 (&x)[U][C], int32_t (&cd)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) cd[u] = a.codes[pr[u]];
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
    auto batch_bits = [&](int64_t b, bool (&sel)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            sel[u] = (a.mask[r >> 6] >> (r & 63)) & 1ull;
        }
    };
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C], const int32_t (&cd)[U], const bool (&sel)[U]) {
        const int64_t row0 = b * RB + g;
        bool offered[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            offered[u] = (row0 + (int64_t)u * RPI < a.n) && (SEL != 2 || sel[u]);
            if (t == 0) cs[u * RPI + g] = cd[u];
        }
        for (int v = 0; v < Tp; ++v) {
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
            if (t == 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) sc[(u * RPI + g) * Tp + v] = offered[u] ? s[u] : __builtin_nanf("");
            }
        }
        maxsim_wave_sync();
        // lane per (row of the batch, vector): entry p = j * Tp + v, position b * RB + j; a NaN fails s == s
        const int64_t pos0 = b * RB;
        for (int p = lane; p < RB * Tp; p += kWave) {
            const int j = p / Tp;
            const int v = p - j * Tp;
            const float s = sc[p];
            if (s == s) {
                const uint64_t key = make_key(s, (uint32_t)(pos0 + j));
                uint64_t* const w = a.table + (int64_t)cs[j] * a.T + v;
                if (key > *w) atomicMax((unsigned long long*)w, (unsigned long long)key);
            }
        }
        maxsim_wave_sync();
    };

    bool all_rows[U];
#pragma unroll
    for (int u = 0; u < U; ++u) all_rows[u] = true;
    if (SEL == 2) {
        bool sel[U], seln[U];
        if (gw < nbatches) batch_bits(gw, sel);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            int32_t cd[U];
            batch_rows(b, pr);
            load_batch(pr, x, cd);
            const int64_t bn = b + nwaves_total;
            batch_bits(bn < nbatches ? bn : b, seln);  // behind the row loads: never waited for by its own batch
            consume_batch(b, x, cd, sel);
#pragma unroll
            for (int u = 0; u < U; ++u) sel[u] = seln[u];
        }
    } else if (SUBSET) {
        // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
        int64_t pr[U], pn[U];
        if (gw < nbatches) batch_rows(gw, pr);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int32_t cd[U];
            load_batch(pr, x, cd);
            const int64_t bn = b + nwaves_total;
            batch_rows(bn < nbatches ? bn : b, pn);
            consume_batch(b, x, cd, all_rows);
#pragma unroll
            for (int u = 0; u < U; ++u) pr[u] = pn[u];
        }
    } else {
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            int32_t cd[U];
            batch_rows(b, pr);
            load_batch(pr, x, cd);
            consume_batch(b, x, cd, all_rows);
        }
    }
}

struct MaxsimTopkArgs {
    const uint64_t* table;  // [n_groups, T]
    int64_t n_groups;
    int T, k;
    uint64_t* part;         // [gridDim.x, 64] the blocks' sorted lists of make_key(S, code), 0 = none
};

__global__ __launch_bounds__(kDistinctThreads) void maxsim_topk_kernel(MaxsimTopkArgs a) {
    __shared__ uint64_t merge[(kDistinctWaves - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    WaveTopK tk;
    tk.init(a.k);
    // (the bound is uniform over the wave: offer is wave-cooperative)
    for (int64_t base = (int64_t)blockIdx.x * kDistinctThreads + (threadIdx.x - lane); base < a.n_groups;
         base += (int64_t)gridDim.x * kDistinctThreads) {
        const int64_t i = base + lane;
        uint64_t key = 0ull;
        if (i < a.n_groups) {
            const uint64_t* w = a.table + i * a.T;
            uint64_t word = w[0];
            bool every = word != 0ull;
            float S = key_score(word);
            for (int t = 1; t < a.T; ++t) {  // in order, plain adds
                word = w[t];
                every = every && word != 0ull;
                S = S + key_score(word);
            }
            if (every && S == S) key = make_key(S, (uint32_t)i);
        }
        tk.offer(key);
    }
    block_merge_topk(tk, merge, kDistinctWaves);
    if (threadIdx.x < kWave) a.part[(int64_t)blockIdx.x * kWave + threadIdx.x] = tk.key;  // (lanes >= k hold 0)
}

struct MaxsimEmitArgs {
    const uint64_t* part;   // [nlists, 64]
    int nlists;
    const uint64_t* table;  // [n_groups, T]
    int T, k;
    const int64_t* rows;    // NULL, or the row list the keys' positions index
    int64_t label_offset;
    float* D;               // [k]
    int32_t* G;             // [k]
    int64_t* I_tok;         // [k, T] or NULL
    float* D_tok;           // [k, T] or NULL
};

__global__ __launch_bounds__(kDistinctThreads) void maxsim_emit_kernel(MaxsimEmitArgs a) {
    __shared__ uint64_t merge[(kDistinctWaves - 1) * kWave];
    __shared__ uint64_t win[kWave];
    const int lane = threadIdx.x & (kWave - 1);
    WaveTopK tk;
    tk.init(a.k);
    const int total = a.nlists * kWave;
    for (int base = (int)threadIdx.x - lane; base < total; base += kDistinctThreads) tk.offer(a.part[base + lane]);
    block_merge_topk(tk, merge, kDistinctWaves);
    if (threadIdx.x < kWave) win[threadIdx.x] = tk.key;  // wave 0 (k <= 64): lane i holds the i-th best group
    __syncthreads();
    if ((int)threadIdx.x < a.k) {
        const uint64_t key = win[threadIdx.x];
        a.D[threadIdx.x] = key ? key_score(key) : -3.402823466e+38f;
        a.G[threadIdx.x] = key ? (int32_t)key_row(key) : -1;
    }
    if (!a.I_tok && !a.D_tok) return;
    for (int e = threadIdx.x; e < a.k * a.T; e += kDistinctThreads) {
        const int j = e / a.T;
        const int t = e - j * a.T;
        const uint64_t key = win[j];
        int64_t row = -1;
        float s = -3.402823466e+38f;
        if (key) {
            const uint64_t word = a.table[(int64_t)key_row(key) * a.T + t];
            const int64_t p = (int64_t)key_row(word);
            row = (a.rows ? a.rows[p] : p) + a.label_offset;
            s = key_score(word);
        }
        if (a.I_tok) a.I_tok[e] = row;
        if (a.D_tok) a.D_tok[e] = s;
    }
}

}  // namespace mvdb
