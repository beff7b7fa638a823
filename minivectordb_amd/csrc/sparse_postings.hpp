// sparse_postings.hpp — the inverted form of a sparse store (include/mvdb.h "SPARSE POSTINGS"): posting lists by index, resident
// beside the CSR form, and a scoring launch that reads only the lists of the query's terms.  The bits are the CSR pass's: the
// indices of a stored row are strictly ascending, so "the row's entries in stored order" is "ascending index", and a
// term-at-a-time pass that takes the query's terms in ascending index order performs for every row the same chain
//   acc = +0.0; acc = acc + (q[index] * value)
// in the same order (sparse_scan.hpp adds +0.0 for the entries it skips: the same bits as skipping them).
//
// Layout.  post_ptr [dim + 1] (int64): list t is [post_ptr[t], post_ptr[t + 1]).  post [nnz + 2]: 8-byte (row, value bits)
// entries, every list in ascending row order, two padding entries behind them so a 16-byte load of the last entry stays inside
// the allocation.  It is the STABLE TRANSPOSITION of the CSR arrays — np.argsort(indices, kind="stable") applied to the
// entries — and so a pure function of them.
//
// Build (no floating-point atomics, no global atomics at all, no scratch):
//   postings_expand_kernel   one thread per entry: its row by a bounded binary search over indptr; key = index, payload (row, value)
//   an LSD radix sort of the keys, kPostRadixBits bits per pass, ceil(bits(dim - 1) / 8) passes, each pass stable:
//     postings_hist_kernel     one wave per segment of kPostSortSeg entries counts its digits in LDS (integer LDS atomics) into
//                              table[digit][segment]
//     postings_scan_*          exclusive scan of the table in place, multi-block: block sums, their scan by one block, the apply
//     postings_scatter_kernel  the wave walks its segment again in order, 64 entries a step; an entry's slot is the running
//                              offset of its digit plus its rank among the step's entries of that digit (8 ballots), so equal
//                              digits keep their order
//   postings_directory_kernel  post_ptr[t] = the first sorted position whose key is >= t: a bounded binary search per index,
//                              so the directory needs neither counts nor atomics
// The entries arrive in row order, so the stable sort by index leaves every list in ascending row order.
//
// Scoring, sparse_postings_kernel<MODE, SEL>: row-blocked, term-at-a-time, deterministic, no atomics on scores.  A workgroup
// takes row blocks [r0, r0 + kPostBlockRows) in a grid-stride loop and holds acc[kPostBlockRows] (fp32, +0.0) and a 16-bit
// matched count per row in LDS; queries are the grid's y.  The host uploads the query's terms in ascending index order with
// their lists' [begin, end) — terms whose list is empty are dropped there.  Per block: one lane per term finds by binary search
// the part of the term's list inside the block and cuts it at the waves' row quarters (every search loop is bounded by the bit
// length of the range it halves); the cuts sit in LDS.  Then every WAVE walks the terms in order over ITS quarter of the rows:
// its lanes stride the term's part (16-byte loads, two entries each) and do acc[row - r0] = acc[row - r0] + (q_t * value),
// matched++.  Rows within a term are distinct, so no two lanes touch one slot; a quarter's slots are touched by one wave only,
// whose LDS operations execute in program order, so term t + 1 never reaches a row before term t — no barrier between terms.
// MODE 0 writes T[r] = weight * acc and matched[r] for every row of the block; MODE 1 offers (acc, r) through the gate
// selected && matched >= 1 && acc == acc to the wave lists of topk_device.hpp and leaves one list per workgroup for
// merge_keys_kernel.  SEL 0: every row; SEL 2: a bitmap over the physical rows.
// LDS per workgroup: acc 8 KiB + counts 4 KiB + cuts 16 KiB (+ 1.5 KiB of list merge space in MODE 1): five fit a CU.
// Bytes: 8 per entry of the touched lists inside the block + the searches' probes + 4 (or 8) per row written in MODE 0.
#pragma once
#include "sparse_scan.hpp"

namespace mvdb {

constexpr int kPostThreads = 256;
constexpr int kPostWaves = kPostThreads / kWave;
constexpr int kPostBlockRows = 2048;                        // rows a workgroup owns at a time
constexpr int kPostWaveRows = kPostBlockRows / kPostWaves;  // ... and each of its waves
constexpr int kPostBlocksPerCu = 4;
constexpr int64_t kPostMaxDim = 1ll << 26;                  // the directory is 8 (dim + 1) bytes: 512 MiB at the cap
constexpr int kPostRadixBits = 8;
constexpr int kPostRadixDigits = 1 << kPostRadixBits;
constexpr int kPostSortSeg = 4096;                          // entries one wave ranks in LDS per pass
constexpr int kPostScanChunk = 2048;                        // table elements per block of the scan (8 per thread)
constexpr uint32_t kPostPadRow = 0xFFFFFFFFu;               // row of the padding entries: ntotal < 2^32, so no row is it

struct PostEntry {
    uint32_t row;
    uint32_t value;  // the fp32 bits
};
static_assert(sizeof(PostEntry) == 8, "two entries per 16-byte load");

// one term of an uploaded query: its list and its value
struct PostTerm {
    int64_t begin, end;  // the list [begin, end) in post
    uint32_t index;
    uint32_t value;      // the fp32 bits
};
static_assert(sizeof(PostTerm) == 24, "three 8-byte words per term");

struct PostingsArgs {
    const PostEntry* post;    // [nnz + 2], 16-byte aligned
    int64_t n;                // rows
    int64_t nblocks;          // ceil(n / kPostBlockRows)
    const int64_t* q_off;     // [nq + 1] (device): query y holds the terms [q_off[y], q_off[y + 1]), at most kSparseMaxQuery
    const PostTerm* q_terms;  // ascending index within a query, no empty list
    float weight;             // MODE 0: T = weight * acc
    float* T;                 // MODE 0: [n]
    int32_t* matched;         // MODE 0: [n] or NULL
    const uint64_t* mask;     // SEL 2: bitmap over the rows [0, mask_rows)
    int64_t mask_rows;
    int k;                    // MODE 1: <= kMaxFusedK
    uint64_t* cand;           // MODE 1: [nq, gridDim.x, k] sorted block lists
};

// halvings a binary search over `len` positions needs at most: the bit length of len
__device__ __forceinline__ int post_steps(int64_t len) { return len > 0 ? 64 - __clzll((long long)len) : 0; }

// first position in [lo, hi) whose row is >= row (hi where none is); the loop is bounded before it starts
__device__ __forceinline__ int64_t post_lower_bound(const PostEntry* post, int64_t lo, int64_t hi, int64_t row) {
    int64_t len = hi - lo;
    const int steps = post_steps(len);
    for (int s = 0; s < steps; ++s) {
        const int64_t half = len >> 1;
        const bool below = len > 0 && (int64_t)post[lo + half].row < row;
        lo = below ? lo + half + 1 : lo;
        len = below ? len - half - 1 : half;
    }
    return lo;
}

template <int MODE, int SEL>
__global__ __launch_bounds__(kPostThreads) void sparse_postings_kernel(PostingsArgs a) {
    __shared__ float acc[kPostBlockRows];
    __shared__ unsigned short cnt[kPostBlockRows];
    __shared__ int64_t cut_lo[kSparseMaxQuery];                   // first entry of the term's list inside the block
    __shared__ unsigned short cut_end[kSparseMaxQuery][kPostWaves];  // end of every wave's part, relative to cut_lo
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int qi = blockIdx.y;
    const int64_t t0 = a.q_off[qi];
    const int64_t mq = a.q_off[qi + 1] - t0;
    const int m = (int)(mq < kSparseMaxQuery ? mq : kSparseMaxQuery);
    const PostTerm* const terms = a.q_terms + t0;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

    WaveTopK tk;
    if (MODE == 1) tk.init(a.k);

    for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int64_t r0 = blk * kPostBlockRows;
        const int64_t r1 = r0 + kPostBlockRows < a.n ? r0 + kPostBlockRows : a.n;
        // ---- the wave's own slots, and the cuts: one lane per term ---------------------------------
        for (int i = lane; i < kPostWaveRows; i += kWave) {
            acc[wave * kPostWaveRows + i] = 0.f;
            cnt[wave * kPostWaveRows + i] = 0;
        }
        for (int t = tid; t < m; t += kPostThreads) {
            const PostTerm pt = terms[t];
            const int64_t lo = post_lower_bound(a.post, pt.begin, pt.end, r0);
            // rows within a list are distinct: at most kPostBlockRows entries of it lie inside the block
            const int64_t cap = lo + kPostBlockRows < pt.end ? lo + kPostBlockRows : pt.end;
            const int64_t hi = post_lower_bound(a.post, lo, cap, r1);
            int64_t c = lo;
            cut_lo[t] = lo;
#pragma unroll
            for (int w = 0; w < kPostWaves - 1; ++w) {
                c = post_lower_bound(a.post, c, hi, r0 + (int64_t)(w + 1) * kPostWaveRows);
                cut_end[t][w] = (unsigned short)(c - lo);
            }
            cut_end[t][kPostWaves - 1] = (unsigned short)(hi - lo);
        }
        __syncthreads();
        // ---- the terms in ascending index order, every wave over its quarter of the rows -----------
        for (int t = 0; t < m; ++t) {
            const int64_t lo = cut_lo[t];
            const int64_t b = lo + (wave ? (int64_t)cut_end[t][wave - 1] : 0);
            const int64_t e = lo + (int64_t)cut_end[t][wave];
            if (b < e) {
                const float qv = __uint_as_float(terms[t].value);
                for (int64_t p = (b & ~(int64_t)1) + 2 * lane; p < e; p += 2 * kWave) {
                    const u32x4 w = *reinterpret_cast<const u32x4*>(a.post + p);
                    if (p >= b) {
                        const int s = (int)((int64_t)w.x - r0);
                        acc[s] = sparse_add(acc[s], sparse_mul(qv, __uint_as_float(w.y)));
                        cnt[s] = (unsigned short)(cnt[s] + 1);
                    }
                    if (p + 1 < e) {
                        const int s = (int)((int64_t)w.z - r0);
                        acc[s] = sparse_add(acc[s], sparse_mul(qv, __uint_as_float(w.w)));
                        cnt[s] = (unsigned short)(cnt[s] + 1);
                    }
                }
            }
            // the wave's LDS operations of term t are issued before those of term t + 1
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the wave's rows out ---------------------------------------------------------------------
        for (int i = lane; i < kPostWaveRows; i += kWave) {
            const int s = wave * kPostWaveRows + i;
            const int64_t r = r0 + s;
            const bool mine = r < r1;
            const float v = acc[s];
            const int c = cnt[s];
            if (MODE == 0) {
                if (mine) {
                    a.T[r] = sparse_mul(a.weight, v);
                    if (a.matched) a.matched[r] = c;
                }
            } else {
                bool selected = mine;
                if (SEL == 2) selected = mine && r < a.mask_rows && ((a.mask[r >> 6] >> (r & 63)) & 1ull);
                // the gate: selected, matched, and a score that is no NaN (a NaN fails the comparison)
                const bool pass = selected && c >= 1 && v >= tk.thr_score;
                if (__ballot(pass)) tk.offer(pass ? make_key(v, (uint32_t)r) : 0ull);
            }
        }
        __syncthreads();  // the cuts are rewritten for the next block
    }

    if (MODE == 1) {
        __shared__ uint64_t sh[(kPostWaves - 1) * kWave];
        block_merge_topk(tk, sh, kPostWaves);
        if (wave == 0 && tid < a.k) a.cand[((int64_t)qi * gridDim.x + blockIdx.x) * a.k + tid] = tk.key;
    }
}

// ---- the build ---------------------------------------------------------------------------------------------------------

// one thread per CSR entry: its row is the last r with indptr[r] <= e; key = index, payload = (row, value)
__global__ __launch_bounds__(256) void postings_expand_kernel(const SparseEntry* entries, const int64_t* indptr, int64_t n, int64_t nnz, uint32_t* keys,
                                                              PostEntry* pay) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    // first r in [1, n] with indptr[r] > e (indptr[n] = nnz > e), bounded by the bit length of n
    int64_t lo = 1, len = n - 1;
    const int steps = post_steps(len);
    for (int s = 0; s < steps; ++s) {
        const int64_t half = len >> 1;
        const bool below = len > 0 && indptr[lo + half] <= e;
        lo = below ? lo + half + 1 : lo;
        len = below ? len - half - 1 : half;
    }
    const SparseEntry en = entries[e];
    keys[e] = en.index;
    pay[e] = PostEntry{(uint32_t)(lo - 1), en.value};
}

// table[digit * nseg + seg] = entries of segment seg whose digit (bits [shift, shift + 8) of the key) is `digit`
__global__ __launch_bounds__(kPostThreads) void postings_hist_kernel(const uint32_t* keys, int64_t nnz, int shift, int64_t nseg, int64_t* table) {
    __shared__ unsigned int hist[kPostWaves][kPostRadixDigits];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t seg = (int64_t)blockIdx.x * kPostWaves + wave;
    for (int d = lane; d < kPostRadixDigits; d += kWave) hist[wave][d] = 0u;
    __syncthreads();
    if (seg < nseg) {
        const int64_t s0 = seg * kPostSortSeg;
        const int64_t s1 = s0 + kPostSortSeg < nnz ? s0 + kPostSortSeg : nnz;
        for (int64_t i = s0 + lane; i < s1; i += kWave) atomicAdd(&hist[wave][(keys[i] >> shift) & (kPostRadixDigits - 1)], 1u);
    }
    __syncthreads();
    if (seg < nseg)
        for (int d = lane; d < kPostRadixDigits; d += kWave) table[(int64_t)d * nseg + seg] = (int64_t)hist[wave][d];
}

// exclusive scan of the block's 256 thread totals; returns the thread's offset
__device__ __forceinline__ int64_t post_block_exclusive(int64_t v, int64_t* sh, int64_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kPostThreads; off <<= 1) {
        const int64_t add = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const int64_t incl = sh[tid];
    if (total) *total = sh[kPostThreads - 1];
    __syncthreads();
    return incl - v;
}

// sums[b] = sum of x[b * chunk, (b + 1) * chunk)
__global__ __launch_bounds__(kPostThreads) void postings_scan_sums_kernel(const int64_t* x, int64_t N, int64_t* sums) {
    __shared__ int64_t sh[kPostThreads];
    const int64_t base = (int64_t)blockIdx.x * kPostScanChunk;
    int64_t v = 0;
    for (int i = threadIdx.x; i < kPostScanChunk; i += kPostThreads)
        if (base + i < N) v += x[base + i];
    int64_t total = 0;
    (void)post_block_exclusive(v, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums -> their exclusive scan, 256 at a time with a carry
__global__ __launch_bounds__(kPostThreads) void postings_scan_top_kernel(int64_t* sums, int64_t nb) {
    __shared__ int64_t sh[kPostThreads];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += kPostThreads) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < nb ? sums[i] : 0;
        int64_t total = 0;
        const int64_t ex = post_block_exclusive(v, sh, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
}

// x -> its exclusive scan in place: 8 consecutive elements per thread, the block's offset from sums
__global__ __launch_bounds__(kPostThreads) void postings_scan_apply_kernel(int64_t* x, int64_t N, const int64_t* sums) {
    __shared__ int64_t sh[kPostThreads];
    constexpr int per = kPostScanChunk / kPostThreads;
    const int64_t base = (int64_t)blockIdx.x * kPostScanChunk + (int64_t)threadIdx.x * per;
    int64_t v[per];
    int64_t mine = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        v[j] = base + j < N ? x[base + j] : 0;
        mine += v[j];
    }
    int64_t run = sums[blockIdx.x] + post_block_exclusive(mine, sh, nullptr);
#pragma unroll
    for (int j = 0; j < per; ++j) {
        if (base + j < N) x[base + j] = run;
        run += v[j];
    }
}

// the stable scatter of one pass: table holds, scanned, the first slot of (digit, segment)
__global__ __launch_bounds__(kPostThreads) void postings_scatter_kernel(const uint32_t* keys_in, const PostEntry* pay_in, uint32_t* keys_out,
                                                                        PostEntry* pay_out, int64_t nnz, int shift, int64_t nseg, const int64_t* table) {
    __shared__ int64_t off[kPostWaves][kPostRadixDigits];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t seg = (int64_t)blockIdx.x * kPostWaves + wave;
    if (seg < nseg)
        for (int d = lane; d < kPostRadixDigits; d += kWave) off[wave][d] = table[(int64_t)d * nseg + seg];
    __syncthreads();
    if (seg >= nseg) return;
    const int64_t s0 = seg * kPostSortSeg;
    const int64_t s1 = s0 + kPostSortSeg < nnz ? s0 + kPostSortSeg : nnz;
    const unsigned long long below = lane ? (~0ull >> (kWave - lane)) : 0ull;
    for (int64_t i0 = s0; i0 < s1; i0 += kWave) {   // wave-uniform trip count
        const int64_t i = i0 + lane;
        const bool valid = i < s1;
        const uint32_t key = valid ? keys_in[i] : 0u;
        const PostEntry pe = valid ? pay_in[i] : PostEntry{0u, 0u};
        const uint32_t d = (key >> shift) & (kPostRadixDigits - 1);
        // the lanes of this step that hold the same digit
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < kPostRadixBits; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long bb = __ballot(on);
            peers &= on ? bb : ~bb;
        }
        const int rank = __popcll(peers & below);
        int64_t slot = 0;
        if (valid) slot = off[wave][d];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) off[wave][d] = slot + __popcll(peers);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            keys_out[slot + rank] = key;
            pay_out[slot + rank] = pe;
        }
    }
}

// post_ptr[t] = first sorted position whose key is >= t, for t in [0, dim]
__global__ __launch_bounds__(256) void postings_directory_kernel(const uint32_t* keys, int64_t nnz, int64_t dim, int64_t* post_ptr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > dim) return;
    int64_t lo = 0, len = nnz;
    const int steps = post_steps(len);
    for (int s = 0; s < steps; ++s) {
        const int64_t half = len >> 1;
        const bool below = len > 0 && (int64_t)keys[lo + half] < t;
        lo = below ? lo + half + 1 : lo;
        len = below ? len - half - 1 : half;
    }
    post_ptr[t] = lo;
}

}  // namespace mvdb
