// range_scan.hpp — range search (mvdb_index_range_search): EVERY selected row whose score reaches a threshold, instead of
// the k best.  One thresholded pass over the rows appends 64-bit keys to a per-query segment, a segmented bitonic sort
// orders what was appended, an emit kernel writes (D, I).
//
// Roofline: HBM.  Algorithmic bytes per launch = n * ld * 4 (every selected row once; + 8 per row of a row list, + 1/8 per
// row of a bitmap) + 8 per passing row.
//
// The per-row arithmetic is flat_scan_kernel's (scan_kernels.hpp), restated instruction for instruction for the same
// (G, C, MASKED, METRIC) as grouped_scan_kernel does: lane t of the row's G lanes takes chunks t, t + G, ..., C x 4 fmaf in
// chunk order, then the G/2 ... 1 xor butterfly, negation for L2, the same fused query normalisation.  The score of a (query,
// row) pair is a function of that shape alone, so a returned score is bit for bit what the single-query scan returns
// (tests/test_range_gpu.py).
//
// Append path.  A query's counter is ONE 64-bit word; an atomic per passing row would serialise a dense result on that
// address.  Each wave stages passing keys in a register (lane i holds the i-th staged key) and reserves room with one
// atomicAdd per flush of up to 64 keys.  The counter keeps counting past the segment's capacity — only the store is
// suppressed — so it always ends as the true count.  The order in which waves append is not defined: the segment is sorted
// afterwards, and a segment that overflowed is reported as such, never as a partial answer.
//
// Batches.  A query may bring its own threshold (RangeScanArgs::thrs).  A batch over an inner-product index
// that keeps an fp16 shadow shares corpus passes: half_scan.hip's range_nominate_h16_kernel names candidate rows per query,
// range_rescore_kernel below scores them with this file's arithmetic and appends to the same segments, and range_scan_kernel
// runs once more, enabled per query on the device (gate_count), for the queries whose candidates overflowed.
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

struct RangeScanArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [nq, ld] queries (device), zero padded
    int normalize_q;       // L2-normalise the query in the prologue
    float thr;             // a row passes iff its key score (IP: q.x, L2: -|q-x|^2) >= thr; NaN scores fail
    const float* thrs = nullptr;  // NULL, or [nq]: query i's own threshold in place of thr (same units; a NaN entry matches nothing)
    // the fallback launch of the shared pass (mvdb.hip: range_shared_phase): query i is scanned only if its candidate counter
    // passed the capacity — every other block returns at once
    const unsigned long long* gate_count = nullptr;
    unsigned long long gate_cap = 0;
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    uint64_t* keys;        // [nq, seg] appended keys: make_key(score, position)
    int64_t seg;           // keys between consecutive queries' segments (>= cap)
    int64_t cap;           // keys a segment may hold; appends beyond are counted, not stored
    unsigned long long* counts;  // [nq] zeroed by the caller
};

// The kernel's body is range_scan_body.hpp, included as text: the range join's kernel (join_scan.hpp: join_scan_kernel) is the
// same statements with a per-query row bound switched on.  (A shared __device__ function was tried first: inlined through a
// reference it compiles to other register counts for the bitmap forms of THIS kernel, some higher.  Text does not.)
template <int G, int C, int U, int METRIC, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void range_scan_kernel(RangeScanArgs a) {
    constexpr bool BOUND = false;
    const int64_t* const bounds = nullptr;
#include "range_scan_body.hpp"
}

// ---- exact re-score of the shared pass's candidates (inner product) ---------------------------------------------------------
// The nomination launches (half_scan.hip: range_nominate_h16_kernel) left, per query, a segment of candidate ROW NUMBERS and a
// counter.  Work items are (query blockIdx.y, batch of its segment): the grid is fixed — gridDim.x blocks per query, looping
// over the batches the query's counter says there are; a query without candidates, or one whose counter passed the capacity
// (the gated range_scan_kernel answers it), costs its blocks one scalar load.  Per row this is range_scan_kernel's arithmetic
// for the same (G, C, MASKED), metric 0 — lane t of the row's G lanes takes chunks t, t + G, ..., C x 4 fmaf in chunk order,
// the G/2 ... 1 xor butterfly, the same fused query normalisation — so a score is bit for bit the single-query scan's; the
// keys carry the ROW, and go to the segments the sort and the emit kernels read through the same staged append.
struct RangeRescoreArgs {
    const float* X;
    int64_t ld;
    int d4;
    const float* q;        // [nq, ld] the fp32 queries
    int normalize_q;
    float thr;
    const float* thrs;     // NULL, or [nq]
    const uint32_t* cand;  // [nq][ccap]
    int64_t ccap;
    const unsigned long long* ccount;  // [nq]
    uint64_t* keys;
    int64_t seg;
    int64_t cap;
    unsigned long long* counts;
};

template <int G, int C, int U, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void range_rescore_kernel(RangeRescoreArgs a) {
    constexpr int RPI = kWave / G;
    constexpr int RB = RPI * U;
    const int qi = blockIdx.y;
    const unsigned long long have = a.ccount[qi];
    if (have == 0 || have > (unsigned long long)a.ccap) return;
    const int64_t m = (int64_t)have;
    const int64_t nbatches = (m + RB - 1) / RB;
    if ((int64_t)blockIdx.x * kScanWaves >= nbatches) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;
    const int g = lane / G;
    const float thr = a.thrs ? a.thrs[qi] : a.thr;
    const uint32_t* __restrict__ rows = a.cand + (int64_t)qi * a.ccap;

    // ---- query -> registers (flat_scan_kernel's prologue, same operation order) ---------------
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

    // ---- the wave's staged keys (range_scan_kernel's append path) -----------------------------------
    uint64_t stage = 0;
    int nst = 0;
    uint64_t* const seg = a.keys + (int64_t)qi * a.seg;
    unsigned long long* const ctr = a.counts + qi;
    const unsigned long long cap = (unsigned long long)a.cap;
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(ctr, (unsigned long long)nst);
        base = readlane_u64(base, 0);
        if (lane < nst && base + (unsigned long long)lane < cap) seg[base + lane] = stage;
        nst = 0;
    };
    auto append = [&](uint64_t cand) {
        uint64_t mm = __ballot(cand != 0ull);
        while (mm) {
            const int src = __ffsll((long long)mm) - 1;
            mm &= mm - 1;
            const uint64_t key = readlane_u64(cand, src);
            if (lane == nst) stage = key;
            if (++nst == kWave) flush();
        }
    };

    const int64_t last = m - 1;
    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    for (int64_t b = (int64_t)blockIdx.x * kScanWaves + wave; b < nbatches; b += nwaves_total) {
        const int64_t row0 = b * RB + g;
        uint32_t pr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;  // clamp: tail lanes re-read the segment's last candidate, result discarded
            pr[u] = rows[r];
        }
        f32x4 x[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* p = a.X + (int64_t)pr[u] * a.ld + t * 4;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const f32x4* src = reinterpret_cast<const f32x4*>(p + c * G * 4);
                if (MASKED)
                    x[u][c] = cvalid[c] ? __builtin_nontemporal_load(src) : f32x4{0, 0, 0, 0};
                else
                    x[u][c] = __builtin_nontemporal_load(src);
            }
        }
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
#pragma unroll
        for (int mm = G / 2; mm >= 1; mm >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], mm);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            const bool pass = (t == 0) && (r < m) && (s[u] >= thr);
            if (__ballot(pass)) append(pass ? make_key(s[u], pr[u]) : 0ull);
        }
    }
    if (nst) flush();
}

// ---- segmented bitonic sort (descending) of the appended keys ------------------------------------------------------------
// Query blockIdx.y owns keys[blockIdx.y * seg ...].  Its real keys are the first min(count, cap); a query that overflowed
// (count > cap) or matched nothing is skipped.  Only the leading Pc = pow2ceil(count) keys are sorted: everything behind
// them counts as zero keys (every real key is > 0), which a descending sort leaves where they are.
constexpr int kRangeSortTile = 4096;  // keys one block sorts in LDS
constexpr int kRangeSortThreads = 1024;

__device__ __forceinline__ int64_t range_sort_span(const unsigned long long* counts, int64_t cap) {
    const unsigned long long c = counts[blockIdx.y];
    if (c == 0 || c > (unsigned long long)cap) return 0;
    int64_t p = 2;
    while (p < (int64_t)c) p <<= 1;
    return p;
}

// Every (size, stride) step with stride < L, for size = size_lo ... size_hi, on the block's tile of L keys (L <= 4096, a
// power of two; tile blockIdx.x).  size_lo == 2: the first visit — the load pads with zero keys behind the count.
__global__ __launch_bounds__(kRangeSortThreads) void range_sort_lds_kernel(uint64_t* keys, int64_t seg, const unsigned long long* counts,
                                                                           int64_t cap, int L, int64_t size_lo, int64_t size_hi) {
    const int64_t Pc = range_sort_span(counts, cap);
    const int64_t base = (int64_t)blockIdx.x * L;
    if (base >= Pc || size_lo > Pc) return;
    const int Lq = (int)(Pc < L ? Pc : L);  // a short segment: sort its span only
    __shared__ uint64_t s[kRangeSortTile];
    uint64_t* k = keys + (int64_t)blockIdx.y * seg + base;
    const int64_t have = (int64_t)counts[blockIdx.y] - base;  // real keys of this tile (may exceed Lq, may be <= 0)
    for (int i = threadIdx.x; i < Lq; i += blockDim.x) s[i] = (size_lo > 2 || i < have) ? k[i] : 0ull;
    __syncthreads();
    for (int64_t size = size_lo; size <= size_hi && size <= Pc; size <<= 1) {
        int stride0 = (int)(size >> 1 < Lq / 2 ? size >> 1 : Lq / 2);
        for (int stride = stride0; stride > 0; stride >>= 1) {
            for (int tix = threadIdx.x; tix < Lq / 2; tix += blockDim.x) {
                const int lo = 2 * tix - (tix & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((base + lo) & size) == 0;
                const uint64_t x = s[lo], y = s[hi];
                if ((x < y) == desc) {
                    s[lo] = y;
                    s[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < Lq; i += blockDim.x) k[i] = s[i];
}

// One (size, stride) step in global memory (stride >= the LDS tile).
__global__ __launch_bounds__(256) void range_sort_step_kernel(uint64_t* keys, int64_t seg, const unsigned long long* counts, int64_t cap,
                                                              int64_t size, int64_t stride) {
    const int64_t Pc = range_sort_span(counts, cap);
    const int64_t tix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (size > Pc || tix >= Pc / 2) return;
    uint64_t* k = keys + (int64_t)blockIdx.y * seg;
    const int64_t lo = 2 * tix - (tix & (stride - 1));
    const int64_t hi = lo + stride;
    const bool desc = (lo & size) == 0;
    const uint64_t x = k[lo], y = k[hi];
    if ((x < y) == desc) {
        k[lo] = y;
        k[hi] = x;
    }
}

// (D, I) of query blockIdx.y: its sorted keys, best first, then missing markers; a query that overflowed gets only markers.
// rows != NULL: the keys carry positions of that row list.
__global__ void range_emit_kernel(const uint64_t* __restrict__ keys, int64_t seg, const unsigned long long* __restrict__ counts,
                                  int64_t cap, int64_t width, int metric, const int64_t* __restrict__ rows, int64_t label_offset,
                                  float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width) return;
    const unsigned long long c = counts[blockIdx.y];
    const int64_t o = (int64_t)blockIdx.y * width + i;
    if (c <= (unsigned long long)cap && (unsigned long long)i < c) {
        const uint64_t key = keys[(int64_t)blockIdx.y * seg + i];
        const float s = key_score(key);
        const int64_t p = (int64_t)key_row(key);
        D[o] = metric == 0 ? s : -s;
        I[o] = (rows ? rows[p] : p) + label_offset;
    } else {
        D[o] = metric == 0 ? -3.402823466e+38f : 3.402823466e+38f;
        I[o] = -1;
    }
}

}  // namespace mvdb
