// maxsim_mfma.hpp — the MaxSim scoring pass on the exact-fp32 matrix cores (index option "maxsim_mfma" = 1; DESIGN.md
// section 6k "On the matrix cores").  It replaces maxsim_scan_kernel's launch and nothing else: the table, the clear, the
// fold and the emit are maxsim_scan.hpp's.
//
//   maxsim_mfma_kernel   one pass over the selected rows for Tp <= 32 of the vectors.  A workgroup is 4 waves, grid-strided
//                        over TILES of 32 selected rows; a wave owns a tile: scores[32 rows, 32 vectors] = X_tile · Q^T on
//                        v_mfma_f32_32x32x2_f32, rows the A operand, vectors the B operand, d / 2 instructions per tile.
//
//   k order.  Lane l (row or vector l & 31, half h = l >> 5) feeds the instruction (kb, j) the k index 8 kb + 4 h + j: the four
//   instructions j = 0 .. 3 of a kb take the four components of ONE 16-byte chunk (chunk 2 kb + h) on both sides.  A and
//   B use the same permutation, the sum runs over all of d.
//
//   B.  The Tp vectors are normalised by the scan's prologue operations (sum of squares, 1 / sqrtf, multiply; a zero
//   vector stays zero), padded to 32 with zero vectors and kept in LDS in fragment order for the whole pass:
//   Qf[kb][l] is the 16-byte chunk 2 kb + h of vector l & 31, so a B fragment for four instructions is one lane-linear
//   ds_read_b128 (conflict-free).  32 d floats: 64 KiB at d = 512, 128 KiB at d = 1024 — they do not fit the registers.
//
//   A.  Rows go straight from HBM into A fragments, once per pass, 16-byte nontemporal loads: lane l loads chunk 2 kb + h
//   of row l & 31 of its tile, and that register IS the A operand of four instructions — no LDS ring.  A tile row is used
//   by exactly one wave and every element by exactly one lane, so a ring would add an LDS write and an LDS read per
//   element for no reuse, on the unit that already serves B; and the 32-byte pieces a load instruction takes from a row
//   are completed by the next three instructions of the same wave, which are in flight together.  The loads run as ONE
//   stream across the wave's tiles, PS steps (a step: 32 floats of every row, four loads, sixteen instructions) ahead of
//   the matrix instructions in a register ring with static slots, so the first rows of the next tile are on their way
//   while this tile's last steps and its epilogue run.  The rows' group codes (and row numbers of a list, bitmap words) are
//   fetched a tile ahead, behind the row loads.
//
//   Epilogue.  The accumulator of lane l holds vector l & 31 against 16 rows (8 (r >> 2) + 4 h + (r & 3)); the halves swap
//   theirs, so a lane has its vector's 32 scores in row order.  Rows past the end, rows a bitmap leaves out, pad vectors
//   and NaN scores make the key 0 (never offered); every other score makes maxsim_scan_kernel's key, make_key(score,
//   position).  A running 64-bit maximum walks the rows and is offered — the same plain load, then atomicMax — where the
//   next row's group code differs (the codes are wave-uniform, the branch is scalar): one atomic per (run of rows of one
//   group, vector) in place of one per (row, vector).  Half 0 offers the runs that end in rows 0 .. 15, half 1 the others.
//
// A score is an fp32 dot product in the instruction's accumulation order (chunk order as above): it does not depend on T,
// on the selection or on the rows around it, and it is NOT the single-query scan's bit pattern.
// Bytes of a pass: maxsim_scan_kernel's.
//
// The header takes nothing from maxsim_scan.hpp: the kernel is instantiated in a translation unit of its own
// (maxsim_mfma.hip, built without the packed fp32 operations), which hands mvdb.hip one launcher.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "topk_device.hpp"

namespace mvdb {

typedef float mx_f32x4 __attribute__((ext_vector_type(4)));
typedef float mx_f32x16 __attribute__((ext_vector_type(16)));

// MaxsimScanArgs' fields, with the same meaning (ld == d: d4 chunks are the whole row)
struct MaxsimMfmaArgs {
    const float* X;        // [n_phys, ld] corpus
    int64_t n;             // rows to score (m for a row list)
    int64_t ld;            // row stride in floats (= d)
    int d4;                // 16-B chunks per row (a multiple of 8)
    const float* q;        // [Tp, ld] the pass's query vectors (device)
    int Tp;                // vectors of this pass (<= 32)
    int normalize_q;       // L2-normalise every vector in the prologue
    const int64_t* rows;   // SEL 1: physical row of list position r
    const uint64_t* mask;  // SEL 2: bitmap over the physical rows
    const int32_t* codes;  // [n_phys] group code of every stored row
    uint64_t* table;       // the word of (group 0, first vector of the pass); group g, vector v of the pass: table[g * T + v]
    int T;                 // words per group
};

constexpr int kMaxsimMfmaTokens = 32;   // vectors of one pass: the B tile
constexpr int kMaxsimMfmaRows = 32;     // rows of a tile: the A tile
constexpr int kMaxsimMfmaThreads = 256;
constexpr int kMaxsimMfmaWaves = kMaxsimMfmaThreads / kWave;
constexpr int kMaxsimMfmaMaxD = 1024;

// the widths the pass takes: whole steps of 32 floats, packed rows, vectors that fit LDS
inline bool maxsim_mfma_width_ok(int64_t d, int64_t ld) { return ld == d && d % 32 == 0 && d >= 32 && d <= kMaxsimMfmaMaxD; }
inline size_t maxsim_mfma_lds_bytes(int64_t d) { return (size_t)kMaxsimMfmaTokens * (size_t)d * 4; }
// steps the row stream runs ahead (at most a tile: d / 32 steps)
constexpr int maxsim_mfma_ps(int64_t d) { return d >= 128 ? 4 : d >= 64 ? 2 : 1; }

template <int PS, int SEL>
__global__ __launch_bounds__(kMaxsimMfmaThreads) void maxsim_mfma_kernel(MaxsimMfmaArgs a) {
    extern __shared__ __align__(16) unsigned char maxsim_mfma_lds[];
    mx_f32x4* const Qf = reinterpret_cast<mx_f32x4*>(maxsim_mfma_lds);  // [d / 8][64] chunks, fragment order
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;   // k half of the instruction
    const int v = lane & 31;   // row of the tile (A), vector of the pass (B, accumulator)
    const int d4 = a.d4;       // chunks per row (ld == d)
    const int nsteps = d4 >> 3;
    const int Tp = a.Tp;

    // ---- the vectors -> LDS in fragment order: a wave per vector, lane c, c + 64, ... its chunks -------------------------------
    for (int t = wave; t < kMaxsimMfmaTokens; t += kMaxsimMfmaWaves) {  // (uniform over the wave)
        mx_f32x4 qv[kMaxsimMfmaMaxD / 4 / kWave];
        float nr = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxsimMfmaMaxD / 4 / kWave; ++c) {
            const int chunk = c * kWave + lane;
            qv[c] = (t < Tp && chunk < d4) ? *reinterpret_cast<const mx_f32x4*>(a.q + (int64_t)t * a.ld + chunk * 4) : mx_f32x4{0, 0, 0, 0};
            nr += qv[c].x * qv[c].x + qv[c].y * qv[c].y + qv[c].z * qv[c].z + qv[c].w * qv[c].w;
        }
        if (a.normalize_q) {
#pragma unroll
            for (int m = kWave / 2; m >= 1; m >>= 1) nr += __shfl_xor(nr, m);
            if (nr > 0.f) {
                const float inorm = 1.0f / sqrtf(nr);
#pragma unroll
                for (int c = 0; c < kMaxsimMfmaMaxD / 4 / kWave; ++c) qv[c] *= inorm;
            }
        }
#pragma unroll
        for (int c = 0; c < kMaxsimMfmaMaxD / 4 / kWave; ++c) {
            const int chunk = c * kWave + lane;
            if (chunk < d4) Qf[(chunk >> 1) * kWave + (chunk & 1) * 32 + t] = qv[c];
        }
    }
    __syncthreads();

    const int64_t stride = (int64_t)gridDim.x * kMaxsimMfmaWaves;
    const int64_t ntiles = (a.n + kMaxsimMfmaRows - 1) / kMaxsimMfmaRows;
    const int64_t last = a.n - 1;
    int64_t ct = (int64_t)blockIdx.x * kMaxsimMfmaWaves + wave;  // the tile the matrix instructions are in
    if (ct >= ntiles) return;

    // ---- the loader: the tile its next load belongs to, this lane's row of it and what the epilogue needs of that row -----------
    int64_t lt = ct;
    int lstep = 0;
    const mx_f32x4* lptr;
    int32_t lcd;
    uint64_t lword = 0;  // SEL 2: the bitmap word of the row
    int64_t nrow = 0;    // SEL 1: the row number of this lane's row of tile lt + stride
    auto list_row = [&](int64_t tile) {
        int64_t p = tile * kMaxsimMfmaRows + v;
        return a.rows[p < last ? p : last];
    };
    auto enter_tile = [&]() {  // lt is set: this lane's row (clamped: a tail lane re-reads the last row, never offered)
        int64_t r;
        if (SEL == 1) {
            r = nrow;
            nrow = list_row(lt + stride);
        } else {
            r = lt * kMaxsimMfmaRows + v;
            r = r < last ? r : last;
        }
        lcd = a.codes[r];
        if (SEL == 2) lword = a.mask[r >> 6];
        lptr = reinterpret_cast<const mx_f32x4*>(a.X + r * a.ld) + h;
        lstep = 0;
    };
    mx_f32x4 ring[PS][4];
    auto load_step = [&](mx_f32x4 (&x)[4]) {
        if (lt < ntiles) {  // (uniform)
#pragma unroll
            for (int m = 0; m < 4; ++m) x[m] = __builtin_nontemporal_load(lptr + (lstep * 4 + m) * 2);
            if (++lstep == nsteps) {
                lt += stride;
                enter_tile();
            }
        }
    };
    if (SEL == 1) nrow = list_row(lt);
    enter_tile();
    int32_t ccd = lcd;
    uint64_t cword = lword;
#pragma unroll
    for (int u = 0; u < PS; ++u) load_step(ring[u]);  // (PS <= nsteps: all of the first tile)

    mx_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    int cstep = 0;

    auto epilogue = [&]() {
        const int64_t pos0 = ct * kMaxsimMfmaRows;
        bool live = pos0 + v < a.n;
        if (SEL == 2) {
            const int64_t r = pos0 + v;
            live = live && ((cword >> (r & 63)) & 1ull);
        }
        const uint32_t rows_on = (uint32_t)__ballot(live);  // bit i: row i of the tile is offered (lanes 0 .. 31)
        float other[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) other[r] = __shfl_xor(acc[r], 32);
        uint64_t* const col = a.table + v;
        uint64_t run = 0ull;
#pragma unroll
        for (int i = 0; i < kMaxsimMfmaRows; ++i) {
            const int r = 4 * (i >> 3) + (i & 3);
            const float s = ((i >> 2) & 1) == h ? acc[r] : other[r];
            const uint64_t key = (v < Tp && ((rows_on >> i) & 1u) && s == s) ? make_key(s, (uint32_t)(pos0 + i)) : 0ull;
            run = key > run ? key : run;
            const int32_t ci = __builtin_amdgcn_readlane(ccd, i);
            const bool ends = i == kMaxsimMfmaRows - 1 || ci != __builtin_amdgcn_readlane(ccd, i + 1 < kMaxsimMfmaRows ? i + 1 : i);
            if (ends) {  // (uniform)
                if ((i >> 4) == h && run != 0ull) {
                    uint64_t* const w = col + (int64_t)ci * a.T;
                    if (run > *w) atomicMax((unsigned long long*)w, (unsigned long long)run);
                }
                run = 0ull;
            }
        }
    };

    while (ct < ntiles) {
#pragma unroll
        for (int u = 0; u < PS; ++u) {
            if (ct < ntiles) {  // (uniform)
                const mx_f32x4* const qf = Qf + (int64_t)cstep * 4 * kWave + lane;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const mx_f32x4 b = qf[m * kWave];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[u][m].x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[u][m].y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[u][m].z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[u][m].w, b.w, acc, 0, 0, 0);
                }
                if (++cstep == nsteps) {
                    epilogue();
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                    cstep = 0;
                    ct += stride;
                    // the loader entered tile ct at the latest when it issued this tile's last step (PS <= nsteps), and enters
                    // the one after only below
                    ccd = lcd;
                    cword = lword;
                }
                load_step(ring[u]);
            }
        }
    }
}

// the launch of one pass (maxsim_mfma.hip): SEL from a.rows / a.mask, the grid two workgroups per CU where the vectors leave
// LDS for them; lds_limit: what the device gives a workgroup
int launch_maxsim_mfma(const MaxsimMfmaArgs& a, int device, size_t lds_limit, hipStream_t stream);

}  // namespace mvdb
