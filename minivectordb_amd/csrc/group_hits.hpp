// group_hits.hpp — group hits search (mvdb_index_search_groups): the k best groups of stored rows, each with its group_size
// best rows (include/mvdb.h "GROUP HITS SEARCH").  The k groups are distinct search's, computed by
// distinct_core unchanged; what is here fetches their members.
//
//   group_members_scan_kernel    one pass over the CODES of the selected rows, 4 bytes per row.  A block puts its query's k
//                                winning codes into a small LDS hash, then every wave walks the selected positions 256 at a
//                                time, four codes per lane in one 16-byte load, looks each code up and compacts the matching
//                                positions with a ballot prefix into a ring in LDS.  Whenever the ring holds a scan batch
//                                (64 / G x U rows), and once at the end, those rows — and only those — are read from the
//                                matrix and scored.  The per-row arithmetic is flat_scan_kernel's, restated as
//                                group_best_scan_kernel restates it: lane t of the row's G lanes takes chunks t, t + G, ...,
//                                C x 4 fmaf in chunk order, then the G/2 ... 1 xor butterfly, the same fused query
//                                normalisation — a score is bit for bit the single-query scan's.  make_key(score, position)
//                                goes to the wave's sorted list of the row's group, [k][group_size] in LDS, behind a look at
//                                that list's last entry.  The next 256 codes are requested before the current matches are
//                                scored, and the rows of a batch before the batch ahead of it is reduced: where every row
//                                matches, the pass is a stream of rows with the codes riding along, not a chain of round
//                                trips.  At the end the block merges its waves' lists and writes
//                                partials[slot][block][k][group_size], and behind them the number of matching rows it met.
//   group_members_select_kernel  one workgroup per query: merges the blocks' lists per group, writes D and I (a list position
//                                becomes its physical row), pads, and adds the query's matching rows to the index's counter.
//
// A key orders by (score, then LOWER position); NaN scores are never offered; every list is a maximum over integer keys, so
// the answer does not depend on the order of arrival.  No block waits for another; every loop is bounded by its trip count.
//
// Bytes per query: 4 n (the codes; + 8 n of a row list, + n / 8 of a bitmap) + the rows of the k groups x ld x 4 +
// 2 x grid.x x (k x group_size + 1) x 8 (the partials written, then read once).
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

constexpr int kGroupsMaxSize = 16;        // group_size
constexpr int kGroupsHash = 256;          // buckets of the membership table: at most kMaxFusedK = 64 codes, a quarter full
constexpr int kGroupsRing = 128;          // entries of a wave's ring: fewer than a scan batch (<= 16) left over + 64 new ones
constexpr int kGroupsStep = 4 * kWave;    // positions a wave takes per step: four consecutive codes per lane, one 16-byte load
constexpr int kGroupsSelectThreads = 1024;
static_assert(kGroupsHash >= 4 * kMaxFusedK && (kGroupsHash & (kGroupsHash - 1)) == 0, "linear probing ends at an empty bucket");

__device__ __forceinline__ int groups_hash(int32_t code) { return (int)(((uint32_t)code * 2654435761u) >> 24) & (kGroupsHash - 1); }

struct GroupMembersArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // positions to walk (m for a row list, the rows at creation for a bitmap)
    int64_t ld;            // row stride in floats (multiple of 4)
    int d4;                // valid 16-B chunks per row
    const float* q;        // [slots, ld] the sub-tile's queries (device), zero padded
    int normalize_q;       // L2-normalise the query in the prologue
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    const int32_t* codes;  // [n_phys] group code of every stored row
    const int32_t* G;      // [slots, k] the queries' winning codes, -1 = none
    int k, group_size;
    uint64_t* partials;    // [slots, gridDim.x, k * group_size + 1]: the block's lists, then its count of matching rows
};

template <int G, int C, int U, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void group_members_scan_kernel(GroupMembersArgs a) {
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per scan batch
    constexpr int CPL = kGroupsStep / kWave;  // codes per lane and step
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
    static_assert(RB + kWave <= kGroupsRing, "an append is at most 64 positions on top of fewer than RB");
    __shared__ int32_t hcode[kGroupsHash];
    __shared__ int32_t hslot[kGroupsHash];
    __shared__ uint32_t rpos[kScanWaves][kGroupsRing];   // the matching positions ...
    __shared__ uint32_t rphys[kScanWaves][kGroupsRing];  // ... their physical rows ...
    __shared__ uint32_t rgrp[kScanWaves][kGroupsRing];   // ... and which of the k groups each belongs to
    __shared__ uint64_t lists[kScanWaves][kMaxFusedK * kGroupsMaxSize];
    __shared__ unsigned long long wcount[kScanWaves];
    const int qi = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int k = a.k, gs = a.group_size;

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

    // ---- the membership table and the empty lists ---------------------------------------------
    for (int i = threadIdx.x; i < kGroupsHash; i += kScanThreads) hcode[i] = -1;
    uint64_t* const mylist = lists[wave];
    for (int i = lane; i < k * gs; i += kWave) mylist[i] = 0ull;
    __syncthreads();
    int32_t mine = -1;
    if ((int)threadIdx.x < k) mine = a.G[(int64_t)qi * k + threadIdx.x];
    if (mine >= 0) {  // (the codes of a query's groups are distinct: every one takes a bucket of its own)
        int h = groups_hash(mine);
        for (int p = 0; p < kGroupsHash; ++p) {
            if (atomicCAS(&hcode[h], -1, mine) == -1) {
                hslot[h] = (int)threadIdx.x;
                break;
            }
            h = (h + 1) & (kGroupsHash - 1);
        }
    }
    const int ngroups = __syncthreads_count(mine >= 0);

    // which of the k groups the code belongs to, -1: none (a bucket chain ends at an empty bucket within k + 1 probes)
    auto lookup = [&](int32_t code) -> int {
        int h = groups_hash(code);
        for (int p = 0; p <= kMaxFusedK; ++p) {
            const int32_t c = hcode[h];
            if (c == code) return hslot[h];
            if (c == -1) return -1;
            h = (h + 1) & (kGroupsHash - 1);
        }
        return -1;
    };

    int head = 0, cnt = 0;          // the wave's ring: wave-uniform
    unsigned long long found = 0;   // matching rows this wave has met: wave-uniform
    uint32_t* const mpos = rpos[wave];
    uint32_t* const mphys = rphys[wave];
    uint32_t* const mgrp = rgrp[wave];

    // A scan batch out of the ring: up to RB matching rows, U per lane group, on their way to registers.
    struct Batch {
        f32x4 x[U][C];
        uint32_t pos[U], grp[U];
        bool live[U];
    };
    // request entries [off, off + take) behind the ring's head (take <= RB); nothing waits here
    auto load_batch = [&](int off, int take, Batch& b) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = u * RPI + g;
            b.live[u] = e < take;
            const int at = (head + off + (b.live[u] ? e : 0)) & (kGroupsRing - 1);  // a spare lane re-reads the first row, result discarded
            b.pos[u] = mpos[at];
            b.grp[u] = mgrp[at];
            const float* p = a.X + (int64_t)mphys[at] * a.ld + t * 4;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const f32x4* src = reinterpret_cast<const f32x4*>(p + c * G * 4);
                if (MASKED)
                    b.x[u][c] = cvalid[c] ? __builtin_nontemporal_load(src) : f32x4{0, 0, 0, 0};
                else
                    b.x[u][c] = __builtin_nontemporal_load(src);
            }
        }
    };
    // reduce a batch with the scan's arithmetic and offer its rows to the lists
    auto consume_batch = [&](const Batch& b) {
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                acc = fmaf(b.x[u][c].x, qv[c].x, acc);
                acc = fmaf(b.x[u][c].y, qv[c].y, acc);
                acc = fmaf(b.x[u][c].z, qv[c].z, acc);
                acc = fmaf(b.x[u][c].w, qv[c].w, acc);
            }
            s[u] = acc;
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], m);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // a NaN fails s == s; the key carries the position (row number, or position in the row list)
            const bool pass = (t == 0) && b.live[u] && (s[u] == s[u]);
            const uint64_t key = pass ? make_key(s[u], b.pos[u]) : 0ull;
            uint64_t* const l = mylist + (pass ? b.grp[u] : 0u) * gs;
            // the list's last entry first: a group of millions of rows inserts a few dozen times
            uint64_t todo = __ballot(pass && key > l[gs - 1]);
            while (todo) {  // (at most 64 turns: a bit goes with each)
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint64_t kn = readlane_u64(key, src);
                const int gn = __builtin_amdgcn_readlane((int)b.grp[u], src);
                lds_list_insert(mylist + gn * gs, gs, kn, lane);
            }
        }
    };
    // Score the nb (>= 1) full batches at the head of the ring.  The rows of batch i + 1 are requested before batch i is
    // reduced and offered, so a wave waits for memory OR works on a batch, not one after the other: where every row matches,
    // a step leaves 64 / RB batches here.  (Up to eight 16-byte loads per lane and batch: a second batch of the widest rows
    // in registers would cost the kernel a resident block per CU.)
    constexpr bool AHEAD = U * C <= 8;
    auto score_full = [&](int nb) {
        Batch cur;
        if constexpr (AHEAD) {
            Batch nxt;
            load_batch(0, RB, cur);
            for (int i = 1; i < nb; ++i) {  // (nb <= 64 / RB + 1)
                load_batch(i * RB, RB, nxt);
                consume_batch(cur);
                cur = nxt;
            }
            consume_batch(cur);
        } else {
            for (int i = 0; i < nb; ++i) {
                load_batch(i * RB, RB, cur);
                consume_batch(cur);
            }
        }
        head = (head + nb * RB) & (kGroupsRing - 1);
        cnt -= nb * RB;
    };
    auto score_rest = [&]() {  // the fewer than RB entries left at the end
        Batch cur;
        load_batch(0, cnt, cur);
        consume_batch(cur);
        head = (head + cnt) & (kGroupsRing - 1);
        cnt = 0;
    };

    if (ngroups > 0) {
        const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
        const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
        const int64_t n4 = a.n & ~(int64_t)(CPL - 1);  // the positions the steps cover; the up to three behind them: the tail
        const int64_t nsteps = (n4 + kGroupsStep - 1) / kGroupsStep;

        // one position's verdict: look the code up, compact the matching lanes into the ring, score what fills a batch
        auto take = [&](int64_t r, int64_t ph, int32_t code, bool selected) {
            const int slot = (selected && code >= 0) ? lookup(code) : -1;
            const uint64_t hit = __ballot(slot >= 0);
            if (hit) {
                if (slot >= 0) {
                    const int at = (head + cnt + __popcll(hit & ((1ull << lane) - 1ull))) & (kGroupsRing - 1);
                    mpos[at] = (uint32_t)r;
                    mphys[at] = (uint32_t)ph;
                    mgrp[at] = (uint32_t)slot;
                }
                const int add = __popcll(hit);
                cnt += add;
                found += (unsigned long long)add;
                if (cnt >= RB) score_full(cnt / RB);
            }
        };

        // A step is 256 positions, four consecutive ones per lane: its codes are one 16-byte load per lane (a row list: two
        // 16-byte loads of row ids, one step further ahead, then four gathered codes), a bitmap adds one word.  Every request
        // is branch-free — a load under a branch is waited for where the branch ends, not where its value is used: a lane
        // whose positions lie behind n4, and every lane of a step behind the last, reads the words of position 0 instead
        // (n4 >= 4 here), and what it read is dropped at the use, by r < n4.
        auto step_base = [&](int64_t b) -> int64_t {
            const int64_t r0 = b * kGroupsStep + lane * CPL;
            return r0 < n4 ? r0 : 0;
        };
        auto step_rows = [&](int64_t b, int64_t (&pr)[CPL]) {  // SEL 1
            const i64x2* src = reinterpret_cast<const i64x2*>(a.rows + step_base(b));
            const i64x2 lo = src[0], hi = src[1];
            pr[0] = lo.x;
            pr[1] = lo.y;
            pr[2] = hi.x;
            pr[3] = hi.y;
        };
        auto step_codes = [&](int64_t b, const int64_t (&pr)[CPL], int32_t (&cd)[CPL]) {
            if (SEL == 1) {
#pragma unroll
                for (int j = 0; j < CPL; ++j) cd[j] = a.codes[pr[j]];
            } else {
                const i32x4 v = *reinterpret_cast<const i32x4*>(a.codes + step_base(b));
                cd[0] = v.x;
                cd[1] = v.y;
                cd[2] = v.z;
                cd[3] = v.w;
            }
        };
        // the bits of this lane's four positions (positions are 64 to a word of the bitmap, a lane's four lie in one)
        auto step_bits = [&](int64_t b) -> uint32_t {
            if (SEL != 2) return 0xFu;
            const int64_t r0 = step_base(b);
            return (uint32_t)(a.mask[r0 >> 6] >> (r0 & 63)) & 0xFu;
        };

        if (nsteps > 0) {
            int64_t phys[CPL], physn[CPL], physnn[CPL];
            int32_t code[CPL], coden[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j) phys[j] = physn[j] = physnn[j] = 0;
            if (SEL == 1) {
                step_rows(gw, phys);
                step_rows(gw + nwaves_total, physn);
            }
            step_codes(gw, phys, code);
            uint32_t bits = step_bits(gw);
            for (int64_t b = gw; b < nsteps; b += nwaves_total) {
                // the next step's codes (and the row ids of the step after it) are on their way while this step's matches are scored
                const int64_t bn = b + nwaves_total;
                step_codes(bn, physn, coden);
                const uint32_t bitsn = step_bits(bn);
                if (SEL == 1) step_rows(bn + nwaves_total, physnn);

                const int64_t r0 = b * kGroupsStep + lane * CPL;
#pragma unroll
                for (int j = 0; j < CPL; ++j) take(r0 + j, SEL == 1 ? phys[j] : r0 + j, code[j], r0 < n4 && ((bits >> j) & 1u));
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    phys[j] = physn[j];
                    physn[j] = physnn[j];
                    code[j] = coden[j];
                }
                bits = bitsn;
            }
        }
        if (gw == 0 && n4 < a.n) {  // the tail, one position per lane of the first wave
            const int64_t r = n4 + lane;
            const bool in = r < a.n;
            int64_t ph = r;
            int32_t code = -1;
            bool selected = in;
            if (in) {
                if (SEL == 1) ph = a.rows[r];
                code = a.codes[ph];
                if (SEL == 2) selected = (a.mask[r >> 6] >> (r & 63)) & 1ull;
            }
            take(r, ph, code, selected);
        }
        if (cnt > 0) score_rest();
    }

    // ---- merge the waves' lists per group; the block's count ----------------------------------
    if (lane == 0) wcount[wave] = found;
    __syncthreads();
    uint64_t* const out = a.partials + ((int64_t)qi * gridDim.x + blockIdx.x) * ((int64_t)k * gs + 1);
    for (int j = wave; j < k; j += kScanWaves) {
        WaveTopK tk;
        tk.init(gs);
        const int w = lane / gs, i = lane - w * gs;  // gs <= 16: the four lists of the group fit one offer
        tk.offer(w < kScanWaves ? lists[w][j * gs + i] : 0ull);
        if (lane < gs) out[j * gs + lane] = tk.key;
    }
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < kScanWaves; ++w) total += wcount[w];
        out[(int64_t)k * gs] = total;
    }
}

struct GroupMembersSelectArgs {
    const uint64_t* partials;  // [slots, nblocks, k * group_size + 1]
    int nblocks, k, group_size;
    const int64_t* rows;       // NULL, or the row list the keys' positions index
    int64_t label_offset;
    float* D;                  // [slots, k, group_size] the sub-tile's part of the call's output
    int64_t* I;
    unsigned int* ticket;      // one word of the call's workspace, zero between launches: the last block publishes the counter
    unsigned long long* ctr;   // NULL, or the index's device word: member rows met (a running total)
    volatile unsigned long long* host;  // its host-mapped mirror
};

// blockIdx.x: the slot.  Wave w takes groups w, w + 16, ...
__global__ __launch_bounds__(kGroupsSelectThreads) void group_members_select_kernel(GroupMembersSelectArgs a) {
    __shared__ unsigned long long part[kGroupsSelectThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    constexpr int nwaves = kGroupsSelectThreads / kWave;
    const int k = a.k, gs = a.group_size;
    const int64_t stride = (int64_t)k * gs + 1;
    const uint64_t* const src = a.partials + (int64_t)blockIdx.x * a.nblocks * stride;
    const int64_t total = (int64_t)a.nblocks * gs;
    for (int j = wave; j < k; j += nwaves) {
        WaveTopK tk;
        tk.init(gs);
        for (int64_t base = 0; base < total; base += kWave) {  // (the bound is uniform over the wave: offer is wave-cooperative)
            const int64_t e = base + lane;
            uint64_t key = 0ull;
            if (e < total) {
                const int64_t blk = e / gs;
                key = src[blk * stride + (int64_t)j * gs + (e - blk * gs)];
            }
            tk.offer(key);
        }
        if (lane < gs) {
            const int64_t o = ((int64_t)blockIdx.x * k + j) * gs + lane;
            if (tk.key) {
                const int64_t p = (int64_t)key_row(tk.key);
                a.D[o] = key_score(tk.key);
                a.I[o] = (a.rows ? a.rows[p] : p) + a.label_offset;
            } else {
                a.D[o] = -3.402823466e+38f;
                a.I[o] = -1;
            }
        }
    }
    if (a.ctr) {
        unsigned long long c = 0;
        for (int b = threadIdx.x; b < a.nblocks; b += kGroupsSelectThreads) c += src[(int64_t)b * stride + (int64_t)k * gs];
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) c += __shfl_xor(c, m);
        if (lane == 0) part[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long sum = 0;
            for (int w = 0; w < nwaves; ++w) sum += part[w];
            if (sum) atomicAdd(a.ctr, sum);
            __threadfence();
            if (atomicAdd(a.ticket, 1u) == gridDim.x - 1) {  // every block of the launch has counted
                *a.ticket = 0u;
                a.host[0] = atomicAdd(a.ctr, 0ull);
            }
        }
    }
}

}  // namespace mvdb
