// boost_scan.hpp — boosted search: a row's score is S = w_s * s + T[row] (include/mvdb.h "BOOSTED SEARCH"), s the single-query
// scan's score of the row bit for bit, T one fp32 word per stored row.  The k rows with the largest S, exact over every
// selected row, in ONE pass over the corpus.  No reference counterpart (its hybrid_rerank_results re-weights the k rows a
// dense search has already returned: a row that wins on the combined score from dense rank k + 1 is never seen).
//
// Three launches:
//   boost_combine_kernel   T[r] = w_1 t_1[r] (+ w_2 t_2[r] ...) from up to four resident term columns, element-wise, 16-byte
//                          accesses: combining into ONE column first keeps the scan at one instantiation per (shape, form)
//                          instead of one per term count.  Bytes 4 n (nterms + 1).
//   boost_scatter_kernel   T[row] += value for the sparse entries of a single query: one thread per entry, plain loads and
//                          stores — the rows are distinct (checked on the host), so no two threads meet.
//   boost_scan_kernel      flat_scan_kernel's top-k mode (scan_kernels.hpp) with one more word per row.  The lanes of a row
//                          read T[physical row] — one address per row group, as the bitmap word of SEL 2 — and that load never
//                          sits between a batch's row loads and their first use: the term words of the NEXT batch are fetched
//                          behind the current batch's row loads (SEL 0 / 2: the rows of a batch are known by arithmetic;
//                          SEL 1: the row ids run TWO batches ahead, so that the ids the term loads need have arrived before
//                          the current batch's row loads were issued).  The gate stays a ballot on S >= thr_score (NaN
//                          fails), the offer is make_key(S, physical row) in every form: equal S goes to the lower physical
//                          row, under an unsorted list too.  Then merge_keys_kernel as it stands.
// All of the arithmetic on top of s is a rounded multiply or a rounded add, never contracted (boost_chain, boost_score): plain
// numpy float32 reproduces every bit.
// Bytes of the scan: n (4 ld + 4) — 1.002 of the exact scan's at d = 512.
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

constexpr int kBoostMaxTerms = 4;

struct BoostCombineArgs {
    const float* t[kBoostMaxTerms];  // the term columns, [n] each (device)
    float w[kBoostMaxTerms];         // their weights, in call order
    int nterms;                      // 0: T = +0.0 (sparse entries only)
    int64_t n;
    float* T;                        // [n], 16-byte aligned like the columns
};

// The contract's operations are the rounded multiply and add, __fmul_rn / __fadd_rn.  This toolchain's headers define both as a
// plain `*` / `+` compiled under the default contraction mode, so a product that feeds a sum through them is fused into one
// fma all the same (seen on the device: 1 ulp off numpy in a third of the rows).  The helpers below therefore spell the
// operations out under `fp contract(off)`, which is what the intrinsics promise; nothing else in this file is compiled that way
// (the scan's normalisation prologue must contract exactly as flat_scan_kernel's does).
// one term chain element: first term T = w t, later terms T = T + (w t) — a multiply, then an add, never fused
__device__ __forceinline__ float boost_chain(float T, float w, float t, bool first) {
#pragma clang fp contract(off)
    const float p = w * t;
    const float sum = T + p;
    return first ? p : sum;
}
// S = (w_s s) + T: one multiply, then one add
__device__ __forceinline__ float boost_score(float w_s, float s, float T) {
#pragma clang fp contract(off)
    const float p = w_s * s;
    return p + T;
}
// a sparse entry: T + v
__device__ __forceinline__ float boost_add(float T, float v) {
#pragma clang fp contract(off)
    return T + v;
}

__global__ __launch_bounds__(256) void boost_combine_kernel(BoostCombineArgs a) {
    const int64_t n4 = a.n >> 2;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = tid; i < n4; i += step) {
        f32x4 v[kBoostMaxTerms];
#pragma unroll
        for (int j = 0; j < kBoostMaxTerms; ++j)
            if (j < a.nterms) v[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.t[j]) + i);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kBoostMaxTerms; ++j)
            if (j < a.nterms) {
                acc.x = boost_chain(acc.x, a.w[j], v[j].x, j == 0);
                acc.y = boost_chain(acc.y, a.w[j], v[j].y, j == 0);
                acc.z = boost_chain(acc.z, a.w[j], v[j].z, j == 0);
                acc.w = boost_chain(acc.w, a.w[j], v[j].w, j == 0);
            }
        reinterpret_cast<f32x4*>(a.T)[i] = acc;
    }
    // the up to three rows behind the last full 16 bytes
    const int64_t r = (n4 << 2) + tid;
    if (tid < 4 && r < a.n) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kBoostMaxTerms; ++j)
            if (j < a.nterms) acc = boost_chain(acc, a.w[j], a.t[j][r], j == 0);
        a.T[r] = acc;
    }
}

// T[rows[i]] += values[i]; the rows are distinct and inside [0, n) (the host has checked both; a row outside is skipped all the same)
__global__ __launch_bounds__(256) void boost_scatter_kernel(float* T, int64_t n, const int64_t* rows, const float* values, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t r = rows[i];
    if (r < 0 || r >= n) return;
    T[r] = boost_add(T[r], values[i]);
}

struct BoostScanArgs {
    const float* X;       // [n_phys, ld] corpus
    int64_t n;            // rows to score: every row, the rows of a list, or the rows a bitmap covers
    int64_t ld;           // row stride in floats (multiple of 4)
    int d4;               // valid 16-B chunks per row
    const float* q;       // [nq, ld] queries (device), zero padded
    int normalize_q;      // L2-normalise the query in the prologue
    int k;                // <= kMaxFusedK
    const int64_t* rows;  // SEL 1: physical row of logical row r
    const uint64_t* mask; // SEL 2: bitmap over the physical rows
    const float* T;       // [n_phys] the combined term column, read by PHYSICAL row
    float score_weight;   // w_s
    uint64_t* cand;       // [nq, gridDim.x, k] sorted block lists
};

// (G, C) from with_scan_shape, (SEL, MASKED) from with_scan_form, U from stream_u / gather_u: a score s has the arithmetic of
// flat_scan_kernel<G, C, ., 0, ...> — the same prologue, chunk order of fmaf and xor butterfly.
template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void boost_scan_kernel(BoostScanArgs a) {
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int qi = blockIdx.y;

    // ---- query -> registers (flat_scan_kernel's prologue) --------------------------------------
    f32x4 qv[C];
    bool cvalid[C];
    const float* qptr = a.q + (int64_t)qi * a.ld;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int chunk = c * G + t;
        cvalid[c] = !MASKED || chunk < a.d4;
        qv[c] = cvalid[c] ? *reinterpret_cast<const f32x4*>(qptr + chunk * 4) : f32x4{0, 0, 0, 0};
    }
    if (a.normalize_q) {
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

    WaveTopK tk;
    tk.init(a.k);

    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t last = a.n - 1;

    // physical rows of batch b (SUBSET: one 8-byte load per row through rows[]); tail slots are clamped to the last row
    auto batch_rows = [&](int64_t b, int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            pr[u] = SUBSET ? a.rows[r] : r;
        }
    };
    // issue the U*C loads of a batch (nothing waits here)
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
    // the term words of the given physical rows (one 4-byte load per row; the lanes of a row read the same word)
    auto batch_terms = [&](const int64_t (&pr)[U], float (&tv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) tv[u] = a.T[pr[u]];
    };
    // SEL == 2: is row r selected?
    auto batch_bits = [&](const int64_t (&pr)[U], bool (&sel)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) sel[u] = (a.mask[pr[u] >> 6] >> (pr[u] & 63)) & 1ull;
    };
    // reduce batch b, add the terms and offer its rows to the top-k list
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C], const int64_t (&pr)[U], const float (&tv)[U], const bool (&sel)[U]) {
        const int64_t row0 = b * RB + g;
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
        // the U butterflies are independent: interleave them step by step
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], m);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            const float S = boost_score(a.score_weight, s[u], tv[u]);
            // gate on the score alone (NaN fails); exact 64-bit order decided inside offer()
            const bool pass = (t == 0) && (r < a.n) && (SEL != 2 || sel[u]) && (S >= tk.thr_score);
            if (__ballot(pass)) tk.offer(pass ? make_key(S, (uint32_t)pr[u]) : 0ull);
        }
    };

    bool all_rows[U];
#pragma unroll
    for (int u = 0; u < U; ++u) all_rows[u] = true;
    if (SUBSET) {
        // ids two batches ahead, terms one: at the head of a batch its own ids and terms and the NEXT batch's ids have arrived
        // (they were issued behind the row loads of the batch before, which its reduction has waited for), so the next batch's
        // term loads go out right behind this batch's row loads without waiting for anything issued in this batch
        int64_t pr[U], pn[U], pnn[U];
        float tv[U], tn[U];
        if (gw < nbatches) {
            batch_rows(gw, pr);
            const int64_t b1 = gw + nwaves_total;
            batch_rows(b1 < nbatches ? b1 : gw, pn);
            batch_terms(pr, tv);
        }
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            load_batch(pr, x);
            batch_terms(pn, tn);
            const int64_t b2 = b + 2 * nwaves_total;
            batch_rows(b2 < nbatches ? b2 : b, pnn);
            consume_batch(b, x, pr, tv, all_rows);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pr[u] = pn[u];
                pn[u] = pnn[u];
                tv[u] = tn[u];
            }
        }
    } else {
        // rows in corpus order: the next batch's term words (and bitmap words) behind this batch's row loads
        int64_t pr[U], pn[U];
        float tv[U], tn[U];
        bool sel[U], seln[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sel[u] = seln[u] = true;
        if (gw < nbatches) {
            batch_rows(gw, pr);
            batch_terms(pr, tv);
            if (SEL == 2) batch_bits(pr, sel);
        }
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            load_batch(pr, x);
            const int64_t bn = b + nwaves_total;
            batch_rows(bn < nbatches ? bn : b, pn);
            batch_terms(pn, tn);
            if (SEL == 2) batch_bits(pn, seln);
            consume_batch(b, x, pr, tv, sel);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pr[u] = pn[u];
                tv[u] = tn[u];
                sel[u] = seln[u];
            }
        }
    }

    __shared__ uint64_t sh[(kScanWaves - 1) * kWave];
    block_merge_topk(tk, sh, kScanWaves);
    if (wave == 0 && lane < a.k) a.cand[((int64_t)qi * gridDim.x + blockIdx.x) * a.k + lane] = tk.key;
}

}  // namespace mvdb
