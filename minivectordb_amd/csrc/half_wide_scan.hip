// half_wide_scan.hip — the certified pass's nomination kernel for the embedding widths above 1024 (d = 1536 / 2048 / 3072 / 4096).
// It shares the stream of flat_scan_h16_kernel (half_scan.hip): the fp16 shadow, DMA'd into the swizzled fragment image, NST
// stages in flight, counted vmcnt, one bare s_barrier per stage.  A translation unit of its own because it is compiled without
// the packed fp32 operations (Makefile), as maxsim_mfma.hip is.
//
// flat_scan_h16_kernel keeps a wave's 32 queries over the WHOLE of K in registers (4 per 16-k block): 256 registers at d = 1024 and
// no room beyond.  Here the query operand is spread over the workgroup instead:
//   * a workgroup serves QW = 32 QG queries as QG query groups, and a group's K is cut into NK parts held by NK waves: wave w is
//     part w % NK of group w / NK, eight waves in all (two per SIMD, 256 registers each);
//   * a stage is KS 16-k blocks of a 32-row tile (KS < KT: a whole tile is 96 - 256 KiB here); wave (g, p) multiplies the stage's
//     blocks [p KS / NK, (p + 1) KS / NK) against its fragments of those blocks — every wave issues MFMAs on every stage — and
//     keeps ONE accumulator per tile: a chain of d / NK products;
//   * at the end of a tile the parts p > 0 store their 32 x 32 fp32 partial tiles into the group's exchange window and go on to
//     the next tile; the part-0 wave (the group's owner) picks them up behind the next stage barrier — the window needs no barrier
//     of its own: a part is written behind the barrier of its tile's LAST stage and read behind the barrier of the next tile's
//     FIRST, and a tile has at least two stages —, adds them to its own in ascending part order (a fixed order: the same bits
//     run to run) and runs the gate of flat_scan_h16_kernel: threshold register, lds_list_insert, kHalfKeep keys per query.
// A launch covers ceil(nq / QW) query slabs (grid.y), each streaming the tiles itself: ALGORITHMIC bytes per launch = slabs x
// rows scanned x d x 2.  Candidates: cand[(query * gridDim.x + block) * kHalfKeep + lane], as flat_scan_h16_kernel.
// No bitmap, no L2 offsets, no tile flags: the route (mvdb.hip: wide_path_ok) is the unfiltered inner-product batch.
#include <cmath>

#include "common.hpp"
#include "half_scan.hpp"
#include "topk_device.hpp"

namespace mvdb {

typedef _Float16 hs_h8 __attribute__((ext_vector_type(8)));
typedef float hs_f4 __attribute__((ext_vector_type(4)));
typedef float hs_f16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* hs_lds_ptr;
typedef const __attribute__((address_space(1))) void* hs_gbl_ptr;

template <int KT, int QG, int NK, int KS, int NST>
__global__ __launch_bounds__(QG * NK * 64) void flat_scan_h16_wide_kernel(HalfScanArgs a) {
    constexpr int WV = QG * NK;
    constexpr int K = KT * 16;
    constexpr int NSTG = KT / KS;          // stages per tile
    constexpr int KSP = KS / NK;           // 16-k blocks of a stage per wave
    constexpr int HSL = KS * 2;            // 16-byte slots (8 fp16) per row and stage
    constexpr int kStage = 32 * HSL * 16;  // bytes
    constexpr int NP = kStage / 1024;      // DMA instructions per stage
    constexpr int DPW = NP / WV;           // ... per wave
    static_assert(KT % KS == 0 && KS % NK == 0 && HSL % 16 == 0 && NP % WV == 0 && DPW >= 1, "shape");
    static_assert(NSTG >= 2, "the exchange window relies on two stage barriers per tile");
    static_assert(NST >= 2 && (NST - 1) * DPW <= 63, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // NST stages | exchange window | lists
    unsigned char* const exch = smem + NST * kStage;                      // [group][part 1 .. NK - 1] 32 x 32 fp32
    uint64_t* const lists = reinterpret_cast<uint64_t*>(exch + QG * (NK - 1) * 4096);  // [group][32 queries][kHalfKeep] keys
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave / NK, part = wave % NK;
    const bool owner = part == 0;
    const int fr = lane & 31, fk = lane >> 5;
    uint64_t* const mylists = lists + (size_t)grp * 32 * kHalfKeep;
    if (owner)
        for (int e = lane; e < 32 * kHalfKeep; e += 64) mylists[e] = 0ull;

    // ---- this wave's share of its group's 32 queries: B[k = 16 kb + 8 fk + j][query fr] for kb = sg KS + part KSP + j
    const int myq = (blockIdx.y * QG + grp) * 32 + fr;
    hs_h8 Q[NSTG][KSP];
#pragma unroll
    for (int sg = 0; sg < NSTG; ++sg)
#pragma unroll
        for (int j = 0; j < KSP; ++j)
            Q[sg][j] = *reinterpret_cast<const hs_h8*>(a.qf + (int64_t)myq * K + (sg * KS + part * KSP + j) * 16 + fk * 8);
    float floor0 = myq < a.nq ? (a.thr0 ? a.thr0[myq] : -INFINITY) : INFINITY;
    if (!(floor0 == floor0)) floor0 = -INFINITY;
    float thr = floor0;
    uint32_t thr_row = 0u;
    float inv = a.qinv[myq];
    // consume every global load here: the hand-placed vmcnt waits below are invisible to hipcc (see flat_scan_seed_kernel)
#pragma unroll
    for (int sg = 0; sg < NSTG; ++sg)
#pragma unroll
        for (int j = 0; j < KSP; ++j) asm volatile("" : "+v"(Q[sg][j]));
    asm volatile("" : "+v"(floor0), "+v"(thr), "+v"(inv));

    const int64_t ntiles = a.tile1 - a.tile0;
    const int64_t last = a.n - 1;
    // DMA roles: piece p = wave DPW + i of a stage fills LDS bytes [1024 p, 1024 p + 1024) = rows (64 p + lane) / HSL; rows past
    // the end of the corpus (last tile) are READ like any other — the shadow keeps 32 rows of slack — and never nominated
    uint32_t voff[DPW];
#pragma unroll
    for (int i = 0; i < DPW; ++i) {
        const int j = (wave * DPW + i) * 64 + lane;
        const int row = j / HSL, ps = j % HSL;
        voff[i] = (uint32_t)(row * (K * 2) + ((ps ^ (row & 15)) << 4));
    }
    const int64_t step = gridDim.x;
    int64_t tile = blockIdx.x;
    // stage c of the block's flat sequence = (tile + (c / NSTG) step, K part c % NSTG); tiles past the end are clamped (re-reads
    // nobody consumes: the loop body is branch-free and every counted wait sees a full ring)
    auto issue_stage = [&](int64_t base, int c, int buf) {
        int64_t t = base + (int64_t)(c / NSTG) * step;
        t = t < ntiles ? t : (base < ntiles ? base : 0);
        const char* sbase = reinterpret_cast<const char*>(a.Xh) + ((a.tile0 + t) * 32 * (int64_t)K + (c % NSTG) * KS * 16) * 2;
        unsigned char* dst = smem + buf * kStage + wave * DPW * 1024;
#pragma unroll
        for (int i = 0; i < DPW; ++i)
            __builtin_amdgcn_global_load_lds((hs_gbl_ptr)(sbase + voff[i]), (hs_lds_ptr)(dst + i * 1024), 16, 0, 2 /* nt */);
    };
    const int frow = fr * HSL * 16;
    const int fsw = fr & 15;
    unsigned n_ins = 0, n_slow = 0;
    hs_f16 acc;
    // a part's tile: lane l stores acc[4 r4 .. 4 r4 + 3] at 1024 r4 + 16 l (conflict-free b128); the owner reads the same lanes
    auto exch_write = [&]() {
        unsigned char* dst = exch + ((grp * (NK - 1) + part - 1) * 4096) + lane * 16;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
            *reinterpret_cast<hs_f4*>(dst + r4 * 1024) = hs_f4{acc[4 * r4], acc[4 * r4 + 1], acc[4 * r4 + 2], acc[4 * r4 + 3]};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // in LDS before this wave reaches the next barrier
    };
    // owner: own part + parts 1 .. NK - 1 in that order, then the gate.  sc[e] is row (e & 3) + 8 (e >> 2) + 4 fk of the tile, query fr
    auto finish_tile = [&](int64_t m0) {
        float sc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = acc[e];
        const unsigned char* src = exch + (grp * (NK - 1) * 4096) + lane * 16;
#pragma unroll
        for (int p = 0; p < NK - 1; ++p)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const hs_f4 v = *reinterpret_cast<const hs_f4*>(src + p * 4096 + r4 * 1024);
#pragma unroll
                for (int i = 0; i < 4; ++i) sc[4 * r4 + i] += v[i];
            }
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            sc[e] *= inv;  // exact: 1 / (s_q s_x) is a power of two
            mx = fmaxf(mx, sc[e]);
        }
        if (__ballot(mx >= thr) == 0ull) return;
        ++n_slow;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rl = (e & 3) + 8 * (e >> 2);
            const float s = sc[e];
            uint64_t mask = __ballot(m0 + rl + 4 * fk <= last && beats_key(s, (uint32_t)(m0 + rl + 4 * fk), thr, thr_row));
            while (mask) {
                const int srcl = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                ++n_ins;
                const int sq = srcl & 31;
                const float sv = __uint_as_float(__builtin_amdgcn_readlane((int)__float_as_uint(s), srcl));
                const uint32_t rv = (uint32_t)(m0 + rl + 4 * (srcl >> 5));
                const uint64_t kth = lds_list_insert(mylists + (size_t)sq * kHalfKeep, kHalfKeep, make_key(sv, rv), lane);
                if (fr == sq) set_threshold(kth, floor0, thr, thr_row);  // both lane halves
            }
        }
    };

    const bool any = tile < ntiles;   // (block-uniform, as everything that decides whether a barrier is reached)
    if (any) {
#pragma unroll
        for (int c = 0; c < NST - 1; ++c) issue_stage(tile, c, c);
    }
    int buf = 0;
    int64_t m_prev = -1;              // first row of the tile whose parts wait in the window
    while (tile < ntiles) {
#pragma clang loop unroll(full)
        for (int sg = 0; sg < NSTG; ++sg) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * DPW) : "memory");  // this wave's pieces of the stage have landed
            __builtin_amdgcn_s_barrier();  // everybody's have; every wave is done reading the stage before; (sg = 0) the parts of the tile before are in the window
            __builtin_amdgcn_sched_barrier(0);
            const int abuf = buf == 0 ? NST - 1 : buf - 1;  // the look-ahead stage goes into the buffer of the stage before
            issue_stage(tile, sg + NST - 1, abuf);
            __builtin_amdgcn_sched_barrier(0);
            if (sg == 0) {
                if (owner && m_prev >= 0) finish_tile(m_prev);
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            }
            const unsigned char* src = smem + buf * kStage + frow;
            hs_h8 f[KSP];
#pragma unroll
            for (int j = 0; j < KSP; ++j) f[j] = *reinterpret_cast<const hs_h8*>(src + (((2 * (part * KSP + j) + fk) ^ fsw) << 4));
#pragma unroll
            for (int j = 0; j < KSP; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[j], Q[sg][j], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the fragments are in registers before the buffer may be refilled)
            buf = buf == NST - 1 ? 0 : buf + 1;
        }
        if (!owner) exch_write();
        m_prev = (a.tile0 + tile) * 32;
        tile += step;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped look-ahead DMAs must land before the LDS is released
    if (any) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();  // the last tile's parts are in the window
        __builtin_amdgcn_sched_barrier(0);
        if (owner) finish_tile(m_prev);
    }
    if (!owner) return;
    if (a.stats && lane == 0) {
        atomicAdd(a.stats, n_ins);
        atomicAdd(a.stats + 1, n_slow);
    }
#pragma unroll 1
    for (int q = 0; q < 32; ++q) {
        const int qq = (blockIdx.y * QG + grp) * 32 + q;
        if (qq >= a.nq) break;
        if (lane < kHalfKeep) a.cand[((int64_t)qq * gridDim.x + blockIdx.x) * kHalfKeep + lane] = mylists[(size_t)q * kHalfKeep + lane];
    }
}

// The shapes: eight waves (two per SIMD), stages of 32 16-k blocks (32 KiB, four DMA instructions per wave), a ring of three.
// Fragment registers per wave = 4 KT / NK: 96 / 128 / 96 / 128 at d = 1536 / 2048 / 3072 / 4096 (DESIGN.md section 4.3h has the
// compiler's report per instantiation).  Starting points derived from the register file and the LDS, not a measured sweep.
template <int KT_, int QG_, int NK_, int KS_, int NST_>
struct H16WideShape {
    static constexpr int KT = KT_, QG = QG_, NK = NK_, KS = KS_, NST = NST_, WV = QG_ * NK_, QW = 32 * QG_;
    static constexpr size_t kRing = (size_t)NST * 32 * KS * 2 * 16;
    static constexpr size_t kExch = (size_t)QG * (NK - 1) * 4096;
    static constexpr size_t kLists = (size_t)QG * 32 * kHalfKeep * 8;
    static constexpr size_t kLds = kRing + kExch + kLists;
};
template <typename Launch>
static int with_h16_wide_shape(int d, Launch launch) {
    switch (d) {
        case 1536: return launch(H16WideShape<96, 2, 4, 32, 3>{});
        case 2048: return launch(H16WideShape<128, 2, 4, 32, 3>{});
        case 3072: return launch(H16WideShape<192, 1, 8, 32, 3>{});
        case 4096: return launch(H16WideShape<256, 1, 8, 32, 3>{});
        default: return fail(MVDB_ERR_ARG, "no wide fp16-shadow kernel for d = %d", d);
    }
}
// K parts of a query group (the waves that share its K) and queries per workgroup at width d; 0: not a wide width
static int half_wide_parts(int d) { return d == 1536 || d == 2048 ? 4 : d == 3072 || d == 4096 ? 8 : 0; }
int half_wide_queries(int d) { return d == 1536 || d == 2048 ? 64 : d == 3072 || d == 4096 ? 32 : 0; }

// one launch of the wide kernel over tiles [tile0, tile1) for the pass's a.nq <= 128 queries: a seed launch where it has no floors
int launch_half_wide_scan(int d, const HalfScanArgs& a, int device, hipStream_t stream, int* nb) {
    if (a.mask || a.hn || a.tflags || a.gate || a.nq > 128)
        return fail(MVDB_ERR_ARG, "internal: the wide fp16-shadow kernel serves unfiltered inner-product passes of up to 128 queries");
    return with_h16_wide_shape(d, [&](auto shape) {
        using S = decltype(shape);
        static_assert(S::kLds <= 160 * 1024, "LDS budget of a CU");
        static_assert(S::KT * 16 / S::NK <= 512, "half_wide_eps: a wave's chain holds at most 512 products");
        const int64_t ntiles = a.tile1 - a.tile0;
        const int slabs = (a.nq + S::QW - 1) / S::QW;
        return launch_ring(flat_scan_h16_wide_kernel<S::KT, S::QG, S::NK, S::KS, S::NST>, a, S::kLds, S::WV * 64,
                           a.max_blocks > 0 ? std::min<int64_t>(ntiles, a.max_blocks) : ntiles, 1, slabs, device, stream, nb,
                           a.thr0 ? "ip_scan_half_wide" : "ip_scan_half_wide_seed", "flat_scan_h16_wide_kernel<%d, %d, %d, %d, %d>", S::KT, S::QG,
                           S::NK, S::KS, S::NST);
    });
}

// The bound of the wide route, per unit |q| max|x| (tests/test_wide_bound_cpu.py restates and checks it); 0 at every other width.
//   (1), (2) of half_eps (half_scan.hip): operand rounding and fp16 underflow, unchanged.
//   (3) accumulation: wave (g, p) adds its d / NK products of a tile — 384 or 512 at the four widths (launch_half_wide_scan asserts
//       <= 512): the chains are as long as the K split makes them, not cut further — into ONE fp32 accumulator, in ANY order, every
//       addition rounded or truncated (unit 2^-23); the owner then adds the NK partial sums in ascending part order, NK - 1
//       fp32 additions, the first part passing through all of them: gamma(d / NK + NK - 1) (1 + 2^-11)^2, each chain's error
//       relative to its own share of sum |q_i x_i|.
//   (4) the fp32 re-score of half_certify_kernel: lane l takes the 16-byte pieces l, l + 64, ... of the row — ceil(ceil(d / 4) / 64)
//       pieces of 4 fmaf — then 6 butterfly additions: depth 4 ceil(d / 256) + 6, round to nearest.  The kernel's loop has no
//       width in it: the depth formula of half_eps holds at any d (70 at d = 4096).
//   (5) |q| and the comparison, as in half_eps.
double half_wide_eps(int d) {
    const int nk = half_wide_parts(d);
    if (!nk) return 0.0;
    const double u11 = std::ldexp(1.0, -11), u23 = std::ldexp(1.0, -23), u24 = std::ldexp(1.0, -24);
    const double e_op = 2.0 * u11 + u11 * u11;
    const double e_uf = std::sqrt((double)d) * std::ldexp(1.0, -27) * (1.0 + u11) + d * std::ldexp(1.0, -56);
    const double n = d / nk + nk - 1.0;
    const double e_acc = n * u23 / (1.0 - n * u23) * (1.0 + u11) * (1.0 + u11);
    const double depth = ((d + 3) / 4 + 63) / 64 * 4 + 6;
    const double e_re = depth * u24 / (1.0 - depth * u24);
    return (e_op + e_uf + e_acc + e_re) * (1.0 + 4e-6) + 4.0 * u24;
}

}  // namespace mvdb
