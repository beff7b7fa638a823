// assign_scan.hpp — assignment (mvdb_index_assign) and spherical k-means (mvdb_index_kmeans): every stored row labelled by the
// nearest of C vectors (include/mvdb.h "ASSIGN AND K-MEANS").
//
//   assign_clear_kernel      zeroes the running best of every stored row: one 64-bit word per physical row, 0 = no candidate.
//   assign_scan_kernel       one pass over the selected rows for Vp <= 32 of the vectors.  It is maxsim_scan_kernel (maxsim_scan.hpp)
//                            reduced the other way — over the vectors, per row: the same (G, C, U, SEL, MASKED) forms from the one
//                            shape table, the same prologue (maxsim_load_vector), the same load order and per (row, vector) the
//                            same chunk order of fmaf and the same butterfly (maxsim_butterfly) — a score is bit for bit the
//                            single-query scan's.  After the butterfly every lane of a row's group holds the scores of the U rows
//                            in flight; lane t follows row t % U and keeps its best (image of the score, vector) in two registers
//                            as the vectors go by: a strict "greater" on the scan's order-preserving image, so equal scores stay
//                            with the lower vector, -0.0 sits below +0.0 and a NaN is never a candidate.  No score tile, no LDS
//                            traffic beyond the vectors.  Lanes t < U then merge make_key(score, j) — j the vector's number in the
//                            CALL — into their row's word with a plain read-compare-write: the group owns the row for the pass,
//                            passes follow each other on the stream, and a row listed twice is written twice with the same
//                            value.  No atomics, no workgroup waits for another.
//   assign_emit_kernel       word -> label / score (0 -> -1 / -FLT_MAX), to the caller's arrays or packed in place for one copy back.
//   assign_normalize_kernel  the vectors normalised by that same prologue, written out: k-means' initial centres.
//
//   kmeans_changed_kernel    how many labels differ from the iteration before (an integer count).
//   kmeans_hist_kernel       the member lists are a STABLE counting sort of the rows by label: block b counts the labels of its
//   kmeans_colscan_kernel    slice of rows into hist[label][b]; a wave per label scans its column (-> where block b's members of
//   kmeans_offsets_kernel    that label start inside the label's list, and the label's count); one wave scans the counts (-> the
//   kmeans_scatter_kernel    lists' bases and the work items' bases); a wave per slice walks its rows IN ORDER, 64 at a time,
//                            ranks equal labels by lane and appends them at the slice's cursors in LDS.  A list holds its rows in
//                            ascending row number whatever the scheduling: nothing here depends on arrival order.
//   kmeans_chunksum_kernel   a workgroup per (cluster, chunk of 256 members): element-wise fp64 sum in member order, thread per
//                            element; rows are read whole, one huge cluster is many work items.
//   kmeans_finalise_kernel   a workgroup per cluster: chunk partials summed in chunk order, / count, the norm as the square root of
//                            the sequential sum of squares in element order, centre = (float)(mean / norm).
// fp64 IEEE arithmetic throughout the update, no contraction (this file must not be built with fast-math).  No floating-point
// atomics anywhere.
//
// Bytes of an assign call: passes x (n * ld * 4 + 8 n; + 8 n of a row list, + n / 8 of a bitmap) + 8 n (clear) + 8 n (emit).
#pragma once
#include "maxsim_scan.hpp"

namespace mvdb {

constexpr int kAssignMaxVectors = 4096;  // C of one call: a guard, every 32 vectors are one corpus pass
constexpr int kKmeansChunk = 256;        // members per chunk of the update
constexpr int kKmeansSlices = 2048;      // most row slices of the list build

// THE rule of the vectors per pass: MaxSim's (knob: index option assign_vectors_per_pass, 0 = none)
inline int assign_vectors_per_pass(int C, int64_t ld, int knob) { return maxsim_tokens_per_pass(C, ld, knob); }

__global__ __launch_bounds__(256) void assign_clear_kernel(uint64_t* __restrict__ best, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) best[i] = 0ull;
}

struct AssignScanArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [Vp, ld] the pass's vectors (device), zero padded
    int Vp;                // vectors of this pass
    int v0;                // number, in the call, of the pass's first vector
    int normalize_q;       // L2-normalise every vector in the prologue
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    uint64_t* best;        // [n_phys] running best of every physical row: make_key(score, vector), 0 = none
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kMaxsimThreads) void assign_scan_kernel(AssignScanArgs a) {
    extern __shared__ __align__(16) unsigned char assign_lds[];
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int Vp = a.Vp;
    float* const qs = reinterpret_cast<float*>(assign_lds);  // [Vp, ld]

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
        uint32_t bo = 0u;  // image of that row's best score so far (0: none — the image of every non-NaN score is above it)
        int bv = 0;        // ... and its vector, within the pass
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
            if (o > bo) {                                         // strictly: equal scores stay with the lower vector
                bo = o;
                bv = v;
            }
        }
        if (t < U && bo) {  // lane t of the group: row t of the U
            // (its position again, by arithmetic — and its list entry / bitmap word re-read, both cached — instead of a pick
            //  out of the U registers of the batch: a register array indexed by the lane would live in scratch)
            const int64_t pos = row0 + (int64_t)mu * RPI;
            bool offered = pos < a.n;
            if (SEL == 2) offered = offered && ((a.mask[pos >> 6] >> (pos & 63)) & 1ull);
            if (offered) {
                const int64_t row = SUBSET ? a.rows[pos] : pos;
                const uint64_t key = ((uint64_t)bo << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(a.v0 + bv));  // make_key(score, j)
                uint64_t* const w = a.best + row;
                if (key > *w) *w = key;
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

struct AssignEmitArgs {
    uint64_t* best;   // [n] the rows' words
    int64_t n;
    int32_t* labels;  // [n] or NULL
    float* scores;    // [n] or NULL
    int pack;         // also overwrite word r with (label r) | (bits of score r) << 32: what the host entry points copy back
};

__global__ __launch_bounds__(256) void assign_emit_kernel(AssignEmitArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = a.best[i];
        const int32_t lab = key ? (int32_t)key_row(key) : -1;
        const float sc = key ? key_score(key) : -3.402823466e+38f;
        if (a.labels) a.labels[i] = lab;
        if (a.scores) a.scores[i] = sc;
        if (a.pack) a.best[i] = (uint64_t)(uint32_t)lab | ((uint64_t)__float_as_uint(sc) << 32);
    }
}

// dst[v] = src[v] normalised by the scan's prologue (zero padded to ld): a group of G lanes per vector
template <int G, int C, bool MASKED>
__global__ __launch_bounds__(256) void assign_normalize_kernel(const float* __restrict__ src, float* __restrict__ dst, int nv, int64_t ld, int d4) {
    const int t = threadIdx.x % G;
    bool cvalid[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cvalid[c] = !MASKED || c * G + t < d4;
    const int v = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G);  // (uniform over a group; a wave holds whole groups)
    const bool live = v < nv;
    f32x4 qv[C];
    maxsim_load_vector<G, C>(src + (int64_t)(live ? v : 0) * ld, t, cvalid, 1, qv);
    if (live) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (cvalid[c]) *reinterpret_cast<f32x4*>(dst + (int64_t)v * ld + (c * G + t) * 4) = qv[c];
    }
}

// ---- k-means ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kmeans_changed_kernel(const int32_t* __restrict__ now, const int32_t* __restrict__ before, int64_t n,
                                                              unsigned long long* changed) {
    unsigned long long mine = 0;
    // (the bound is uniform over the wave: __ballot below runs with every lane on)
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool diff = i < n && now[i] != before[i];
        mine += (unsigned long long)__popcll(__ballot(diff));
    }
    if (lane == 0 && mine) atomicAdd(changed, mine);  // an integer sum: the order of arrival does not matter
}

// slice b of the rows: [b * per, min(n, (b + 1) * per)); hist is label-major, [C, nb]
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t per, int C, int nb,
                                                           uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t kmeans_h[];
    for (int c = threadIdx.x; c < C; c += blockDim.x) kmeans_h[c] = 0u;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const int32_t l = labels[i];
        if (l >= 0) atomicAdd(&kmeans_h[l], 1u);  // an integer count
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) hist[(int64_t)c * nb + blockIdx.x] = kmeans_h[c];
}

// exclusive prefix sum over the 64 lanes of a wave; *total: the sum (the same in every lane)
__device__ __forceinline__ uint32_t kmeans_wave_scan(uint32_t v, uint32_t* total) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    *total = __shfl(inc, kWave - 1);
    return inc - v;
}

// a wave per label: its column of hist becomes the exclusive scan over the slices; count[label] = the column's sum
__global__ __launch_bounds__(kWave) void kmeans_colscan_kernel(uint32_t* __restrict__ hist, int nb, int64_t* __restrict__ count) {
    uint32_t* const col = hist + (int64_t)blockIdx.x * nb;
    uint32_t run = 0;
    for (int b0 = 0; b0 < nb; b0 += kWave) {  // (uniform bound)
        const int b = b0 + (int)threadIdx.x;
        const uint32_t v = b < nb ? col[b] : 0u;
        uint32_t total;
        const uint32_t ex = kmeans_wave_scan(v, &total);
        if (b < nb) col[b] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) count[blockIdx.x] = (int64_t)run;
}

// one wave: base[c] = members of the labels below c (base[C]: all members), ioff[c] = chunks of the labels below c (ioff[C]: all)
__global__ __launch_bounds__(kWave) void kmeans_offsets_kernel(const int64_t* __restrict__ count, int C, uint32_t* __restrict__ base,
                                                                uint32_t* __restrict__ ioff) {
    uint32_t run_m = 0, run_i = 0;
    for (int c0 = 0; c0 < C; c0 += kWave) {
        const int c = c0 + (int)threadIdx.x;
        const uint32_t m = c < C ? (uint32_t)count[c] : 0u;
        const uint32_t it = (m + kKmeansChunk - 1) / kKmeansChunk;
        uint32_t tm, ti;
        const uint32_t em = kmeans_wave_scan(m, &tm);
        const uint32_t ei = kmeans_wave_scan(it, &ti);
        if (c < C) {
            base[c] = run_m + em;
            ioff[c] = run_i + ei;
        }
        run_m += tm;
        run_i += ti;
    }
    if (threadIdx.x == 0) {
        base[C] = run_m;
        ioff[C] = run_i;
    }
}

// a wave per slice, in row order: members[base[l] + (slice's start inside l) ...] = the slice's rows of label l, ascending
__global__ __launch_bounds__(kWave) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t per, int C, int nb,
                                                                const uint32_t* __restrict__ hist, const uint32_t* __restrict__ base,
                                                                uint32_t* __restrict__ members) {
    extern __shared__ uint32_t kmeans_cur[];
    const int lane = threadIdx.x;
    for (int c = lane; c < C; c += kWave) kmeans_cur[c] = base[c] + hist[(int64_t)c * nb + blockIdx.x];
    maxsim_wave_sync();
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    for (int64_t i0 = lo; i0 < hi; i0 += kWave) {  // (uniform bound)
        const int64_t i = i0 + lane;
        const int32_t l = i < hi ? labels[i] : -1;
        bool todo = l >= 0;
        uint64_t left = __ballot(todo);
        while (left) {  // one round per distinct label among the 64 rows: the lanes that share the first one's label
            const int first = __ffsll((long long)left) - 1;
            const int32_t lf = __shfl(l, first);
            const bool same = todo && l == lf;
            const uint64_t peers = __ballot(same);
            if (same) {
                const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
                members[kmeans_cur[lf] + rank] = (uint32_t)i;
                todo = false;
            }
            maxsim_wave_sync();  // every peer has read the cursor
            if (lane == first) kmeans_cur[lf] += (uint32_t)__popcll(peers);
            maxsim_wave_sync();
            left &= ~peers;
        }
    }
}

// binary search: the label whose items hold item i (ioff ascending, ioff[C] = items; labels without members own no item)
__device__ __forceinline__ int kmeans_item_label(const uint32_t* ioff, int C, uint32_t item) {
    int lo = 0, hi = C;  // the last c with ioff[c] <= item
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ioff[mid] <= item) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct KmeansSumArgs {
    const float* X;           // [n_phys, ld]
    int64_t ld;
    int d;
    int C;
    const uint32_t* members;  // the lists, label after label
    const uint32_t* base;     // [C + 1]
    const uint32_t* ioff;     // [C + 1]
    double* part;             // [items, d]
};

// work item = (label, chunk): thread per element, the chunk's members added one after the other, in list order
__global__ __launch_bounds__(kKmeansChunk) void kmeans_chunksum_kernel(KmeansSumArgs a) {
    __shared__ uint32_t rows[kKmeansChunk];
    const uint32_t item = blockIdx.x;
    if (item >= a.ioff[a.C]) return;  // (uniform)
    const int c = kmeans_item_label(a.ioff, a.C, item);
    const uint32_t chunk = item - a.ioff[c];
    const uint32_t begin = a.base[c] + chunk * kKmeansChunk;
    const uint32_t end = a.base[c + 1];
    const int cnt = (int)(end - begin < (uint32_t)kKmeansChunk ? end - begin : (uint32_t)kKmeansChunk);
    if ((int)threadIdx.x < cnt) rows[threadIdx.x] = a.members[begin + threadIdx.x];
    __syncthreads();
    for (int e = threadIdx.x; e < a.d; e += kKmeansChunk) {
        double acc = (double)a.X[(int64_t)rows[0] * a.ld + e];  // (the sum STARTS at the first member: 0.0 + -0.0 would lose a sign)
        for (int m = 1; m < cnt; ++m) acc += (double)a.X[(int64_t)rows[m] * a.ld + e];
        a.part[(int64_t)item * a.d + e] = acc;
    }
}

struct KmeansFinalArgs {
    double* part;           // [items, d]; the first chunk's slot of a label is reused for its mean
    const uint32_t* ioff;   // [C + 1]
    const int64_t* count;   // [C]
    float* centres;         // [C, ld]
    int64_t ld;
    int d;
};

__global__ __launch_bounds__(256) void kmeans_finalise_kernel(KmeansFinalArgs a) {
    __shared__ double norm_s;
    const int c = blockIdx.x;
    const int64_t cnt = a.count[c];
    if (cnt == 0) return;  // (uniform) no members: the centre stays
    const uint32_t i0 = a.ioff[c], i1 = a.ioff[c + 1];
    double* const mean = a.part + (int64_t)i0 * a.d;
    for (int e = threadIdx.x; e < a.d; e += blockDim.x) {
        double acc = mean[e];
        for (uint32_t i = i0 + 1; i < i1; ++i) acc += a.part[(int64_t)i * a.d + e];
        mean[e] = acc / (double)cnt;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)  // product, then sum: two roundings per step, as the contract states them
        double ss = mean[0] * mean[0];
        for (int e = 1; e < a.d; ++e) {
            const double sq = mean[e] * mean[e];
            ss = ss + sq;
        }
        norm_s = sqrt(ss);
    }
    __syncthreads();
    const double norm = norm_s;
    if (!(norm > 0.0 && norm < INFINITY)) return;  // a zero or non-finite mean: the centre stays
    for (int e = threadIdx.x; e < a.d; e += blockDim.x) a.centres[(int64_t)c * a.ld + e] = (float)(mean[e] / norm);
}

}  // namespace mvdb
