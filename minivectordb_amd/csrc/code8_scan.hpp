// code8_scan.hpp — the int8 prefilter of the single-query search.
//
// Beside the fp32 matrix an index may keep, per stored row i, d int8 codes c_i, an fp32 scale a_i and an fp32 UPPER BOUND r_i
// of |x_i - a_i c_i|.  One pass over the codes (1 byte per element instead of 4) computes s~_i = q~ . (a_i c_i) exactly in
// integers (q~: the query rounded to 16 / 15 bits, held as two int8 planes) and keeps every row whose upper bound
// u_i = s~_i + m_i reaches a floor that is proven to lie at or below the final k-th best score.  The kept rows — a few
// thousand of 10M — are then scored by code8_rescore_kernel with flat_scan_kernel's arithmetic: the bits of (D, I) are the full scan's.
// The floor is the k-th best LOWER bound s~_i - m_i of a sample of rows: code8_seed_kernel, one launch in front of the pass,
// leaves one sorted k-list per block, and every block of the pass merges them at its head.
//
// The codes are stored as two planes in the same d bytes per row: the top 6 bits of every code (3 d / 4 bytes) and the low 2
// bits (d / 4 bytes).  The pass streams the first plane only, bounds what the missing bits can add, and fetches the second
// plane for the few rows that bound cannot reject: for those the integer sum is completed, so what is kept is what a pass
// over whole codes keeps.
//
// Roofline: HBM.  Algorithmic bytes per launch = n * (3 d / 4 + 8) + (rows refined) * d / 4: the high plane once, 8 bytes of
// (a, r) per row, the low plane of the rows the first stage cannot reject.
//
// Where the index also keeps the FRONT plane — the top 5 bits of every code, 5 d / 8 bytes per row — the kernel's front form
// streams that one instead and gathers the high plane for the rows 5 bits cannot reject: n * (5 d / 8 + 8) + (stage-0
// survivors) * (3 d / 4 + 8) + (rows refined) * d / 4.  The same rows are kept.
//
// Shape of the work (flat_scan_kernel's): G lanes share a row, one 16-code chunk (12 bytes) each (d = 512: G = 32, two rows
// per wave-instruction), U row groups in flight per wave, non-temporal loads, a persistent grid, no branch between the loads
// of a batch.  Per chunk: nine and / shift / or, eight v_dot4_i32_i8; per batch one halving reduction of the U sums and one
// epilogue (code8_reduce).
#pragma once
#include "scan_kernels.hpp"

namespace mvdb {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- the margin ---------------------------------------------------------------------------------------------------------------
// For a row with |x| <= B, residual bound r, and a query image q^ (as the prologue below computes it) with |q^| <= qn whose
// 16-bit rounding has step qstep:   | fl32(q . x) - s~ |  <=  alpha * r + beta      (derivation: DESIGN.md section 4.1b)
//   dq    = |q^ - qstep Q|           <= qstep sqrt(d) / 2 (+ the rounding of the division)
//   kap   = 8 u                      the fp32 steps that turn the integer sum into s~ (u = 2^-24)
//   gam   = (d + 8) u / (1 - (d + 8) u)   the fp32 rounding of the score flat_scan_kernel computes (any summation order)
//   eta   = 2 (d + 16) u             the exact kernel normalises the query itself: its image differs from q^ by this much
//   alpha = (qn + dq)(1 + kap)
//   beta  = B (dq + kap (qn + dq) + (gam (1 + eta) + eta) qn) + 1e-30   (the constant: products that underflow)
// both rounded up.
struct Code8Margin {
    float alpha, beta;
};
__host__ __device__ inline Code8Margin code8_margin(int d, float qnorm, float qstep, float row_norm_bound) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double qn = (double)qnorm, B = (double)row_norm_bound;
    const double dq = (double)qstep * sqrt((double)d) * 0.5 * 1.001 + qn * 4.0 * u;
    const double kap = 8.0 * u;
    const double gam = (d + 8) * u / (1.0 - (d + 8) * u);
    const double eta = 2.0 * (d + 16) * u;
    const double up = 1.0 + 9.5367431640625e-07;  // 2^-20: the conversions to fp32 below round either way
    Code8Margin m;
    m.alpha = (float)((qn + dq) * (1.0 + kap) * up);
    m.beta = (float)(B * (dq + kap * (qn + dq) + (gam * (1.0 + eta) + eta) * qn) * up + 1e-30);
    return m;
}
// most |Q| of the rounded query: 127 * 256 where d * 127 * |Q| fits an int32 (d <= 512), 127 * 128 up to d = 1024.
// The prefilter's first stage sums Q_j (H_j + 3 [Q_j > 0]) and Q_j H_j, H_j = c_j & ~3 (below): every factor lies in
// [-128, 127], and d * 128 * qmax = 2,130,706,432 < 2^31 at both values, so those sums fit an int32 as well.
__host__ __device__ inline int code8_qmax(int d) { return d <= 512 ? 32512 : 16256; }

constexpr float kCode8Tiny = 1e-15f;  // a row (a query) whose largest |element| is below this is coded as zero: r = |x| bound

// ---- the two planes of the code ---------------------------------------------------------------------------------------------------
// The d int8 codes of a row are stored as two planes in the same d bytes.  A 16-code chunk t — the dwords A, B, C, D of the
// codes 16 t .. 16 t + 15 — becomes
//   12 bytes of the HIGH plane (row stride 3 d / 4, chunk t at 12 t): A', B', C' = A, B, C with the low 2 bits of every byte
//      replaced by bits 7:6, 5:4, 3:2 of the matching byte of D — `x & 0xFCFCFCFC` is (c & ~3) of A, B, C as int8 dwords, and
//      three and / shift / or give D & 0xFCFCFCFC;
//   one dword of the LOW plane (row stride d / 4, chunk t at 4 t): the low 2 bits of A, B, C, D at bit pairs 0, 2, 4, 6 of
//      every byte — `(l >> 2 i) & 0x03030303` is (c & 3) of dword i.
// The low plane of an index lies behind its high plane at byte offset capacity * 3 d / 4 (capacity, not row count: add into
// reserved space moves nothing).  c = (c & ~3) + (c & 3) with 0 <= (c & 3) <= 3 in two's complement: -127 = -128 + 1.
constexpr uint32_t kCode8HiMask = 0xFCFCFCFCu, kCode8LoMask = 0x03030303u;
__host__ __device__ inline int code8_high_stride(int d) { return d / 4 * 3; }
__host__ __device__ inline int code8_low_stride(int d) { return d / 4; }
__host__ __device__ inline size_t code8_low_offset(int64_t cap, int d) { return (size_t)cap * (size_t)code8_high_stride(d); }

__host__ __device__ inline void code8_pack_chunk(const uint32_t (&c)[4], uint32_t (&h)[3], uint32_t& l) {
    h[0] = (c[0] & kCode8HiMask) | ((c[3] >> 6) & kCode8LoMask);
    h[1] = (c[1] & kCode8HiMask) | ((c[3] >> 4) & kCode8LoMask);
    h[2] = (c[2] & kCode8HiMask) | ((c[3] >> 2) & kCode8LoMask);
    l = (c[0] & kCode8LoMask) | ((c[1] & kCode8LoMask) << 2) | ((c[2] & kCode8LoMask) << 4) | ((c[3] & kCode8LoMask) << 6);
}
// (c & ~3) of the 16 codes, from the high plane alone
__host__ __device__ inline void code8_unpack_high(const uint32_t (&h)[3], uint32_t (&c)[4]) {
    c[0] = h[0] & kCode8HiMask;
    c[1] = h[1] & kCode8HiMask;
    c[2] = h[2] & kCode8HiMask;
    c[3] = ((h[0] & kCode8LoMask) << 6) | ((h[1] & kCode8LoMask) << 4) | ((h[2] & kCode8LoMask) << 2);
}
// (c & 3) of the 16 codes
__host__ __device__ inline void code8_unpack_low(uint32_t l, uint32_t (&c)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (l >> (2 * i)) & kCode8LoMask;
}
__host__ __device__ inline void code8_unpack_chunk(const uint32_t (&h)[3], uint32_t l, uint32_t (&c)[4]) {
    uint32_t lo[4];
    code8_unpack_high(h, c);
    code8_unpack_low(l, lo);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] |= lo[i];
}
// d codes of one row <-> its d * 3 / 4 high-plane bytes and d / 4 low-plane bytes (host: mvdb_code8_pack / mvdb_code8_unpack)
inline void code8_pack_row(int d, const int8_t* codes, uint8_t* high, uint8_t* low) {
    for (int t = 0; t < d / 16; ++t) {
        uint32_t c[4], h[3], l;
        memcpy(c, codes + 16 * t, 16);
        code8_pack_chunk(c, h, l);
        memcpy(high + 12 * t, h, 12);
        memcpy(low + 4 * t, &l, 4);
    }
}
inline void code8_unpack_row(int d, const uint8_t* high, const uint8_t* low, int8_t* codes) {
    for (int t = 0; t < d / 16; ++t) {
        uint32_t c[4], h[3], l;
        memcpy(h, high + 12 * t, 12);
        memcpy(&l, low + 4 * t, 4);
        code8_unpack_chunk(h, l, c);
        memcpy(codes + 16 * t, c, 16);
    }
}

// ---- the front plane: the top 5 bits of every code, a third store beside the two planes --------------------------------------------
// H5 = c & ~7 of every code at 5 d / 8 bytes per row: what the prefilter streams first (stage 0 of code8_scan_kernel's front
// form); the two planes above stay what they are and serve the rows this plane cannot reject.  Nothing else reads it.
// A 32-code chunk t — the dwords c[0 .. 8) of the codes 32 t .. 32 t + 31 — becomes five dwords f[0 .. 5): f[i] = c[i] with
// the low 3 bits of every byte replaced by top bits of the matching byte of c[5], c[6], c[7]:
//   f[0] bits 2:0 = c[5] bits 7:5,   f[1] bits 1:0 = c[5] bits 4:3,   f[1] bit 2 = c[7] bit 4,
//   f[2] bits 2:0 = c[6] bits 7:5,   f[3] bits 1:0 = c[6] bits 4:3,   f[3] bit 2 = c[7] bit 3,
//   f[4] bits 2:0 = c[7] bits 7:5.
// `f[i] & 0xF8F8F8F8` is (c & ~7) of c[0 .. 5) as int8 dwords; ten and / shift / or give the other three.
// Layout: f[0 .. 4) is the chunk's WIDE part (16 bytes), f[4] its NARROW part.  The plane is stored in tiles of R rows, R the
// rows one wave-instruction of the scan covers (code8_front_tile_rows): the wide parts of the tile's rows — row g at
// g * 16 * (d / 32), chunk t at 16 t — and behind them the narrow parts, row g at g * 4 * (d / 32), chunk t at 4 t.  A
// 16-byte load per lane then reads one contiguous span of the tile per wave-instruction, and so does the 4-byte load.  The
// plane is sized in whole tiles (code8_front_bytes): the rows of the last tile past the row count are never written.
//
// The QUAD layout (d = kCode8QuadDim): a lane QUAD per row, lane t of the quad owns the four chunks 4 t .. 4 t + 3 (128 codes),
// so a tile is the 16 rows of one wave-instruction and every load of the stream is 16 bytes per lane.  The tile's
// 16 x 5 d / 8 = 5 KiB are five contiguous 1-KiB slabs, lane (g, t) — row g of the tile — at (4 g + t) * 16 of each: slab
// s = 0 .. 3 holds the wide part of chunk 4 t + s, slab 4 the narrow parts of the chunks 4 t .. 4 t + 3 as one 16-byte unit.
// The row image (code8_front_pack_row) is the same in both layouts; only where its parts lie on the device differs, and every
// reader and writer of the plane goes through code8_front_wide_offset / code8_front_narrow_offset.
constexpr uint32_t kCode8FrontMask = 0xF8F8F8F8u;
#ifdef MVDB_CODE8_ABLATE
constexpr int kCode8QuadDim = 0;     // the timing-ablation library (Makefile: ABLATE) runs the one-chunk-per-lane form at every width
#else
constexpr int kCode8QuadDim = 512;   // the width that keeps the quad layout (0: none)
#endif
constexpr int kCode8QuadChunks = 4;  // chunks per lane of the quad layout
__host__ __device__ inline bool code8_front_dim(int d) { return d > 0 && d % 32 == 0 && d <= 2048; }
__host__ __device__ inline int code8_front_stride(int d) { return d / 8 * 5; }
// lanes per row of the scan's front form: the chunks of a row, rounded up to a power of two (the others are masked off) —
// a quarter of them in the quad layout
__host__ __device__ constexpr int code8_front_lanes(int d) {
    if (d == kCode8QuadDim) return d / (32 * kCode8QuadChunks);
    int g = 1;
    while (g * 32 < d) g *= 2;
    return g;
}
// whether the plane of this width is laid out in quads: a lane owns kCode8QuadChunks chunks
__host__ __device__ constexpr bool code8_front_quad(int d) { return code8_front_lanes(d) * 32 * kCode8QuadChunks == d; }
__host__ __device__ inline int code8_front_tile_rows(int d) { return 64 / code8_front_lanes(d); }
__host__ __device__ inline size_t code8_front_bytes(int64_t cap, int d) {
    const int64_t R = code8_front_tile_rows(d);
    return (size_t)((cap + R - 1) / R * R) * (size_t)code8_front_stride(d);
}
// byte offsets of the wide part (16 bytes) and the narrow part (4 bytes) of chunk `chunk` of a row in the plane
__host__ __device__ inline size_t code8_front_wide_offset(int64_t row, int chunk, int d) {
    const int64_t R = code8_front_tile_rows(d);
    const size_t tile = (size_t)(row / R * R) * (size_t)code8_front_stride(d);
    if (code8_front_quad(d)) {
        const int L = code8_front_lanes(d);
        return tile + (size_t)(chunk % kCode8QuadChunks) * (size_t)(R * L * 16) + (size_t)((row % R) * L + chunk / kCode8QuadChunks) * 16;
    }
    return tile + (size_t)(row % R) * (size_t)(d / 2) + (size_t)chunk * 16;
}
__host__ __device__ inline size_t code8_front_narrow_offset(int64_t row, int chunk, int d) {
    const int64_t R = code8_front_tile_rows(d);
    const size_t tile = (size_t)(row / R * R) * (size_t)code8_front_stride(d);
    if (code8_front_quad(d)) {
        const int L = code8_front_lanes(d);
        return tile + (size_t)kCode8QuadChunks * (size_t)(R * L * 16) + (size_t)((row % R) * L + chunk / kCode8QuadChunks) * 16 +
               (size_t)(chunk % kCode8QuadChunks) * 4;
    }
    return tile + (size_t)R * (size_t)(d / 2) + (size_t)(row % R) * (size_t)(d / 8) + (size_t)chunk * 4;
}

__host__ __device__ inline void code8_front_pack_chunk(const uint32_t (&c)[8], uint32_t (&f)[5]) {
    f[0] = (c[0] & kCode8FrontMask) | ((c[5] >> 5) & 0x07070707u);
    f[1] = (c[1] & kCode8FrontMask) | ((c[5] >> 3) & 0x03030303u) | ((c[7] >> 2) & 0x04040404u);
    f[2] = (c[2] & kCode8FrontMask) | ((c[6] >> 5) & 0x07070707u);
    f[3] = (c[3] & kCode8FrontMask) | ((c[6] >> 3) & 0x03030303u) | ((c[7] >> 1) & 0x04040404u);
    f[4] = (c[4] & kCode8FrontMask) | ((c[7] >> 5) & 0x07070707u);
}
// (c & ~7) of the 32 codes
__host__ __device__ inline void code8_front_unpack_chunk(const uint32_t (&f)[5], uint32_t (&c)[8]) {
#pragma unroll
    for (int i = 0; i < 5; ++i) c[i] = f[i] & kCode8FrontMask;
    c[5] = ((f[0] & 0x07070707u) << 5) | ((f[1] & 0x03030303u) << 3);
    c[6] = ((f[2] & 0x07070707u) << 5) | ((f[3] & 0x03030303u) << 3);
    c[7] = ((f[4] & 0x07070707u) << 5) | ((f[1] & 0x04040404u) << 2) | ((f[3] & 0x04040404u) << 1);
}
// d codes of one row <-> its image in the front plane, 5 d / 8 bytes: the wide parts of its chunks, then the narrow parts
// (host: mvdb_code8_front_pack / mvdb_code8_front_unpack; unpack yields c & ~7)
inline void code8_front_pack_row(int d, const int8_t* codes, uint8_t* image) {
    for (int t = 0; t < d / 32; ++t) {
        uint32_t c[8], f[5];
        memcpy(c, codes + 32 * t, 32);
        code8_front_pack_chunk(c, f);
        memcpy(image + 16 * t, f, 16);
        memcpy(image + d / 2 + 4 * t, &f[4], 4);
    }
}
inline void code8_front_unpack_row(int d, const uint8_t* image, int8_t* codes) {
    for (int t = 0; t < d / 32; ++t) {
        uint32_t c[8], f[5];
        memcpy(f, image + 16 * t, 16);
        memcpy(&f[4], image + d / 2 + 4 * t, 4);
        code8_front_unpack_chunk(f, c);
        memcpy(codes + 32 * t, c, 32);
    }
}

// ---- the bit plane: bit 2 of every code, a fourth store ----------------------------------------------------------------------------
// The front plane holds c & ~7 and stage 1 wants T6 = Q . (c & ~3): c & ~3 = (c & ~7) + 4 ((c >> 2) & 1) in two's complement,
// so T6 = T5 + 4 Q . b2 with b2 the plane of bit 2 — d / 8 bytes per row where the high plane is 3 d / 4.  The front form's
// lift (code8_scan_kernel, LIFT) reads it for the rows stage 0 cannot reject, in place of their chunks of the high plane.
// Layout: plain row-major over the capacity, d / 8 bytes per row; bit i of dword s of a row is bit 2 of code 32 s + i, so
// dword s belongs to the 32-code chunk s of the front plane and nibble j of it to dword j of that chunk.
__host__ __device__ inline int code8_bit2_stride(int d) { return d / 8; }
__host__ __device__ inline size_t code8_bit2_bytes(int64_t cap, int d) { return (size_t)cap * (size_t)code8_bit2_stride(d); }
__host__ __device__ inline uint32_t code8_bit2_pack_chunk(const uint32_t (&c)[8]) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        w |= (((c[j] >> 2) & 1u) | ((c[j] >> 9) & 2u) | ((c[j] >> 16) & 4u) | ((c[j] >> 23) & 8u)) << (4 * j);
    return w;
}
// nibble j of a dword of the plane -> four bytes of 0 / 1, bit 2 of the four codes of dword j of the chunk.  The product
// lays the nibble down at bits 0, 7, 14 and 21 — the four copies do not overlap, nothing carries — and the mask keeps bit b
// of the nibble at bit 8 b.
__host__ __device__ inline uint32_t code8_bit2_spread(uint32_t w, int j) { return (((w >> (4 * j)) & 0xFu) * 0x00204081u) & 0x01010101u; }
// d codes of one row <-> its d / 8 bytes of the plane (host: mvdb_code8_bit2_pack / mvdb_code8_bit2_unpack; unpack yields
// (c >> 2) & 1 of every code)
inline void code8_bit2_pack_row(int d, const int8_t* codes, uint8_t* bits) {
    for (int s = 0; s < d / 32; ++s) {
        uint32_t c[8];
        memcpy(c, codes + 32 * s, 32);
        const uint32_t w = code8_bit2_pack_chunk(c);
        memcpy(bits + 4 * s, &w, 4);
    }
}
inline void code8_bit2_unpack_row(int d, const uint8_t* bits, int8_t* codes) {
    for (int s = 0; s < d / 32; ++s) {
        uint32_t w, c[8];
        memcpy(&w, bits + 4 * s, 4);
        for (int j = 0; j < 8; ++j) c[j] = code8_bit2_spread(w, j);
        memcpy(codes + 32 * s, c, 32);
    }
}

// ---- build: rows [0, n) of X -> codes, (a, r) ------------------------------------------------------------------------------------
// One wave per row.  a = max|x| / 127, c = rint(x / a); r = sqrt(sum (x - a c)^2) rounded up.  A row with a non-finite element
// gets zero codes and r = +inf: it is always a candidate and the exact kernel treats it as it always has.
// list == NULL: rows [0, n) behind the four pointers.  list != NULL (set_rows): the n stored rows list[0 .. n), the pointers
// at row 0; a listed row at or above `limit` (not coded yet) is skipped.
// The codes go out as the two planes: a lane holds one dword of codes, the four lanes of a quad hold a 16-code chunk.
// front != NULL: the front plane of the whole index (tiled: addressed by the stored row's number, front_row0 + row); eight
// lanes hold a 32-code chunk (d is a multiple of 32 then: code8_front_dim).
// bit2 != NULL: the bit plane, at row 0 as the two planes are; the sixth lane of the eight stores the chunk's dword of it.
__global__ __launch_bounds__(256) void code8_build_kernel(const float* __restrict__ X, int64_t ld, int d, int64_t n,
                                                          uint8_t* __restrict__ high, uint8_t* __restrict__ low, float2* __restrict__ ar,
                                                          const int64_t* __restrict__ list, int64_t limit, uint8_t* __restrict__ front,
                                                          int64_t front_row0, uint8_t* __restrict__ bit2) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int d4 = d / 4;
    for (int64_t i = wave0; i < n; i += nw) {
        const int64_t row = list ? list[i] : i;
        if (list && row >= limit) continue;
        const f32x4* src = reinterpret_cast<const f32x4*>(X + row * ld);
        float mx = 0.f;
        bool bad = false;
        for (int c = lane; c < d4; c += 64) {
            const f32x4 v = src[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float av = fabsf(v[j]);
                bad = bad || !(av <= 3.402823466e+38f);
                mx = fmaxf(mx, av);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
        const bool anybad = __ballot(bad) != 0ull;
        const bool tiny = mx < kCode8Tiny;
        const float a = (anybad || tiny) ? 0.f : mx / 127.0f;
        float r2 = 0.f;
        uint32_t* hdst = reinterpret_cast<uint32_t*>(high + row * (int64_t)code8_high_stride(d));
        uint32_t* ldst = reinterpret_cast<uint32_t*>(low + row * (int64_t)code8_low_stride(d));
        // (d is a multiple of 16: the lanes of a quad run the same iterations)
        for (int c = lane; c < d4; c += 64) {
            uint32_t word = 0;
            if (a > 0.f) {
                const f32x4 v = src[c];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float cf = rintf(v[j] / a);
                    cf = fminf(fmaxf(cf, -127.f), 127.f);
                    const float e = fmaf(-a, cf, v[j]);
                    r2 = fmaf(e, e, r2);
                    word |= ((uint32_t)(uint8_t)(int8_t)(int)cf) << (8 * j);
                }
            }
            uint32_t chunk[4], h[3], l;
#pragma unroll
            for (int j = 0; j < 4; ++j) chunk[j] = (uint32_t)__shfl((int)word, (lane & ~3) + j);
            code8_pack_chunk(chunk, h, l);
            const int part = lane & 3;
            if (part < 3)
                hdst[3 * (c >> 2) + part] = part == 0 ? h[0] : part == 1 ? h[1] : h[2];
            else
                ldst[c >> 2] = l;
            if (front || bit2) {
                uint32_t oct[8], f[5];
#pragma unroll
                for (int j = 0; j < 8; ++j) oct[j] = (uint32_t)__shfl((int)word, (lane & ~7) + j);
                code8_front_pack_chunk(oct, f);
                const int fpart = lane & 7;
                if (bit2 && fpart == 5)
                    reinterpret_cast<uint32_t*>(bit2 + row * (int64_t)code8_bit2_stride(d))[c >> 3] = code8_bit2_pack_chunk(oct);
                if (!front) continue;
                if (fpart < 4)
                    reinterpret_cast<uint32_t*>(front + code8_front_wide_offset(front_row0 + row, c >> 3, d))[fpart] =
                        fpart == 0 ? f[0] : fpart == 1 ? f[1] : fpart == 2 ? f[2] : f[3];
                else if (fpart == 4)
                    *reinterpret_cast<uint32_t*>(front + code8_front_narrow_offset(front_row0 + row, c >> 3, d)) = f[4];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) r2 += __shfl_xor(r2, m);
        if (lane == 0) {
            float r;
            if (anybad)
                r = INFINITY;
            else if (tiny)
                r = fmaf(mx, sqrtf((float)d) * 1.01f, 1e-44f);
            else
                r = sqrtf(r2 + (float)d * 2e-38f) * 1.001f;  // (squares of residuals below 1e-19 underflow: d * 2e-38 covers them)
            if (!(r < INFINITY)) r = INFINITY;
            ar[row] = make_float2(a, r);
        }
    }
}

// ---- prologue: the query -> two int8 planes + the margin's terms -------------------------------------------------------------------
// par[0] = qstep, par[1] = alpha, par[2] = beta, par[3] = 1 when the query's norm is not finite (the call falls back)
// Run by every block of code8_seed_kernel, all threads of the block calling it.  The query is read ONCE: the first
// kCode8QueryThreads threads hold up to kCode8MaxDim / kCode8QueryThreads elements each and leave their partial sums in LDS;
// every wave then reduces the kCode8QueryThreads partials itself, in the order of a halving tree over them (t with t + 128,
// then t + 64, then the xor butterfly of a wave: float addition commutes, so every lane ends with the tree's bits) — an order
// that depends on neither the block's size nor the wave, so every block holds the same bits, and three barriers in all.
// qhi / qlo [d]: the block's LDS, complete for every thread when this returns; par: every thread's own copy.
constexpr int kCode8QueryThreads = 256;
constexpr int kCode8MaxDim = 1024;

struct Code8QueryShared {
    float nr[kCode8QueryThreads];
    float mx[kCode8QueryThreads];
    double n2[kCode8QueryThreads];
};

template <typename T, typename Op>
__device__ __forceinline__ T code8_query_reduce(const T* part, Op op) {
    const int lane = threadIdx.x & 63;
    T v = op(op(part[lane], part[lane + 128]), op(part[lane + 64], part[lane + 192]));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ void code8_query_image(const float* __restrict__ q, int d, int normalize_q, float row_norm_bound, int8_t* qhi,
                                                  int8_t* qlo, float (&par)[4], Code8QueryShared& sh) {
    constexpr int NT = kCode8QueryThreads;
    constexpr int E = kCode8MaxDim / NT;
    static_assert(NT == 256, "code8_query_reduce restates a halving tree over 256 partials");
    const int tid = threadIdx.x;
    const bool on = tid < NT;
    float qv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) qv[e] = (on && tid + e * NT < d) ? q[tid + e * NT] : 0.f;
    if (on) {
        float nr = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (tid + e * NT < d) nr = fmaf(qv[e], qv[e], nr);
        sh.nr[tid] = nr;
    }
    __syncthreads();
    const float nr = code8_query_reduce(sh.nr, [](float x, float y) { return x + y; });
    const float inorm = (normalize_q && nr > 0.f) ? 1.0f / sqrtf(nr) : 1.0f;
    if (on) {
        float mx = 0.f;
        double n2 = 0.0;
        bool bad = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (tid + e * NT < d) {
                const float v = qv[e] * inorm;
                bad = bad || !(fabsf(v) <= 3.402823466e+38f);
                mx = fmaxf(mx, fabsf(v));
                n2 += (double)v * (double)v;
            }
        }
        sh.n2[tid] = n2;
        sh.mx[tid] = bad ? INFINITY : mx;
    }
    __syncthreads();
    const float mx = code8_query_reduce(sh.mx, [](float x, float y) { return fmaxf(x, y); });
    const double n2 = code8_query_reduce(sh.n2, [](double x, double y) { return x + y; });
    const double qn_d = sqrt(n2) * (1.0 + 1e-6);
    const bool nonfinite = !(mx <= 3.402823466e+38f) || !(qn_d <= 3.0e38);
    const float qn = nonfinite ? 0.f : (float)qn_d;
    const int qmax = code8_qmax(d);
    const bool tiny = nonfinite || mx < kCode8Tiny;
    const float qstep = tiny ? 0.f : mx / (float)qmax;
    if (on) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = tid + e * NT;
            if (j < d) {
                int Q = 0;
                if (!tiny) {
                    float cf = rintf((qv[e] * inorm) / qstep);
                    cf = fminf(fmaxf(cf, -(float)qmax), (float)qmax);
                    Q = (int)cf;
                }
                const int lo = ((Q + 128) & 255) - 128;
                const int hi = (Q - lo) >> 8;
                qhi[j] = (int8_t)hi;
                qlo[j] = (int8_t)lo;
            }
        }
    }
    // a query coded as zero: all of it is "rounding error" (dq = qn)
    Code8Margin m = code8_margin(d, qn, qstep, row_norm_bound);
    if (tiny && !nonfinite) {
        m.alpha = qn * 1.00001f;
        m.beta = fmaf(qn * 1.00001f, row_norm_bound, 1e-30f) * 1.00001f;
    }
    par[0] = qstep;
    par[1] = m.alpha;
    par[2] = m.beta;
    par[3] = nonfinite ? 1.f : 0.f;
    __syncthreads();
}

// ---- block lists: merged at the head of the next launch ---------------------------------------------------------------------------
// code8_seed_kernel and code8_rescore_kernel end when every block has stored its sorted k-list; the launch behind them on the
// stream merges the lists before anything else (code8_scan_kernel: every block, for the floor; code8_finish_kernel: its one
// block, for (D, I)).  The kernel boundary orders the stores and makes them visible: plain stores, plain vector loads.
//
// The bar of a set of sorted k-lists: the best k-th key any of them holds.  That list alone has k keys at or above the bar, so
// no key below it is among the k best of the union: such keys are dropped before the inserts, which are serial (about
// 0.1 us each) and would otherwise take most keys of most lists — every list holds the best of its own rows.  0 (no list is
// full) drops nothing.  Keys are distinct (score, row): the k best of the union are the same keys with and without the bar,
// in whatever order the lists are walked.
__device__ __forceinline__ uint64_t code8_wave_max(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t code8_lists_bar(const uint64_t* lists, int nlists, int k) {
    const int lane = threadIdx.x & (kWave - 1);
    uint64_t bar = 0ull, top = 0ull;
    for (int l = lane; l < nlists; l += kWave) {
        const uint64_t v = lists[(int64_t)l * k + (k - 1)];
        const uint64_t f = lists[(int64_t)l * k];
        bar = v > bar ? v : bar;
        top = f > top ? f : top;
    }
    bar = code8_wave_max(bar);
    // The second bar, for many lists: every lane holds the best key of the lists it read — 64 keys of 64 disjoint sets of
    // lists — and the union holds k distinct keys at or above the k-th best of those.  Only a lower bound of that key is
    // needed: the largest T with k lanes whose key's upper word (the score's image) reaches T, found bit by bit; T << 32 is at
    // or below those k keys.  With the lists of 256 blocks it leaves a dozen keys to insert where the first bar leaves a third.
    const uint32_t hi = (uint32_t)(top >> 32);
    uint32_t T = 0u;
#pragma unroll
    for (int b = 31; b >= 0; --b) {
        const uint32_t c = T | (1u << b);
        if (__popcll(__ballot(hi >= c)) >= k) T = c;
    }
    const uint64_t bar2 = (uint64_t)T << 32;
    return bar2 > bar ? bar2 : bar;
}
// block_merge_topk with the bar of the waves' lists: the sorted lists of all waves of the block into wave 0's list.
// sh must hold (nwaves - 1) * 64 keys.  Must be called by every thread of the block.
__device__ __forceinline__ void code8_block_merge(WaveTopK& tk, uint64_t* sh, int nwaves) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    if (wave > 0) sh[(wave - 1) * kWave + lane] = tk.key;
    __syncthreads();
    if (wave == 0) {
        uint64_t bar = tk.thr;
        for (int w = 0; w < nwaves - 1; ++w) {
            const uint64_t v = sh[w * kWave + tk.k - 1];
            bar = v > bar ? v : bar;
        }
        for (int w = 0; w < nwaves - 1; ++w) {
            const uint64_t c = sh[w * kWave + lane];
            tk.offer(c >= bar ? c : 0ull);
        }
    }
}

// The waves of the block share the nlists k-lists out (merge_keys_kernel's walk: UNROLL x 64 keys per wave and step, loaded
// before any is offered), merge into wave 0's list.  Few lists: short steps, so that every wave has a share.
template <int UNROLL>
__device__ __forceinline__ void code8_offer_lists(WaveTopK& tk, const uint64_t* lists, int nlists, int k, int nwaves) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)nlists * k;
    uint64_t bar = 0ull;
    bool have_bar = false;
    for (int64_t base = (int64_t)wave * kWave * UNROLL; base < total; base += (int64_t)nwaves * kWave * UNROLL) {
        uint64_t c[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
            const int64_t i = base + j * kWave + lane;
            c[j] = i < total ? lists[i] : 0ull;
        }
        // (every wave for itself, behind its first keys' loads: one round trip for both, no barrier)
        if (!have_bar) bar = code8_lists_bar(lists, nlists, k);
        have_bar = true;
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) tk.offer(c[j] >= bar ? c[j] : 0ull);
    }
}
// Must be called by every thread of the block; sh as code8_block_merge's.  Wave 0's list holds the k best keys of the union.
__device__ __forceinline__ void code8_merge_lists(WaveTopK& tk, const uint64_t* lists, int nlists, int k, uint64_t* sh, int nwaves) {
    const int64_t total = (int64_t)nlists * k;
    tk.init(k);
    if (total <= (int64_t)nwaves * kWave * 4)
        code8_offer_lists<2>(tk, lists, nlists, k, nwaves);
    else
        code8_offer_lists<kMergeUnroll>(tk, lists, nlists, k, nwaves);
    code8_block_merge(tk, sh, nwaves);
}
// The floor of the prefilter, from the lists code8_seed_kernel's blocks left: the k-th best key of their union, -FLT_MAX
// with fewer than k keys (or a k-th of -inf).  Every thread of the block calls it and gets the same bits — in every block,
// whatever the number of lists: the k-th best of a set of distinct keys.  sh as code8_block_merge's; *word: one LDS float.
__device__ __forceinline__ float code8_lists_floor(const uint64_t* lists, int nlists, int k, uint64_t* sh, float* word, int nwaves) {
    WaveTopK tk;
    code8_merge_lists(tk, lists, nlists, k, sh, nwaves);
    if (threadIdx.x < kWave) {
        const uint64_t kth = readlane_u64(tk.key, k - 1);
        if (threadIdx.x == 0) *word = kth ? fmaxf(key_score(kth), -3.402823466e+38f) : -3.402823466e+38f;
    }
    __syncthreads();
    return *word;
}

// ---- the prefilter scan ---------------------------------------------------------------------------------------------------------
struct Code8ScanArgs {
    const uint8_t* high;   // [n, 3 d / 4] the high plane: streamed
    const uint8_t* low;    // [n, d / 4] the low plane: gathered for the rows the first stage cannot reject
    const float2* ar;      // [n] (a, r)
    int64_t n;
    int d;                 // codes per row (a multiple of 16)
    int hstride;           // bytes per row of the high plane (code8_high_stride)
    const int8_t* qhi;     // [d] the query's high / low planes (code8_query_image, left by code8_seed_kernel's block 0)
    const int8_t* qlo;
    const float* par;      // qstep, alpha, beta
    const uint64_t* lists; // [nlists, k] the sorted k-lists of code8_seed_kernel's blocks: lower bounds of the seed sample
    int nlists;
    int k;
    float* floor;          // out (block 0, for the probes): the floor every block derives from the lists (code8_lists_floor)
    uint32_t* cand;        // [cap] appended rows, in no order
    int64_t cap;
    unsigned long long* counter;  // zeroed by code8_seed_kernel's block 0; keeps counting past cap
    unsigned long long* survivors;  // diagnostic, never zeroed: the rows the first stage could not reject, over all calls
    // the front form only (GF > 0):
    const uint8_t* front;  // the front plane (tiled: code8_front_wide_offset): streamed; `high` is then gathered for its survivors
    unsigned long long* front_survivors;   // never zeroed: the rows stage 0 could not reject, over all calls of the front form
    unsigned int* front_calls;             // never zeroed: the calls of the front form
    volatile unsigned long long* front_msum;   // host-mapped: block 0 leaves both counts here at its head, as it finds them
    volatile unsigned int* front_mcalls;       //   (the calls before this one and their survivors: the host's window takes the mean)
    const uint8_t* bit2;   // the bit plane [n, d / 8] (LIFT only): read for the survivors of stage 0 in place of `high`
    int ring;              // entries of the survivor ring (HANDOFF only): a power of two, kCode8RingMin .. kCode8RingMax
};

// the survivor rings of the hand-off form (code8_scan_kernel, HANDOFF): 16-byte entries (row, T5, a, r) in LDS, `ring` entries
// in all, a quarter of them per producer wave — every ring has ONE writer and one reader.
constexpr int kCode8RingMin = 64, kCode8RingMax = 4096, kCode8RingDefault = 1024;
struct Code8Ring {
    i32x4 slot[kCode8RingMax];     // producer w: the slots [w * ring / 4, (w + 1) * ring / 4)
    uint32_t tail[kScanWaves];     // entries producer w has written so far (stored by it alone, with release behind the entries)
    uint32_t head[kScanWaves];     // entries of producer w's ring copied out so far (stored by the survivor wave, with release)
    uint32_t done;                 // producer waves that have ended
};

// lane l's value of v from lane l ^ M.  M = 1, 2, 8 stay inside a row of 16 lanes and are DPP operand modifiers (no
// LDS-crossbar trip, no address register); 4 and 16 are ds_swizzle's bit mode; 32 crosses the halves of the wave.
template <int M>
__device__ __forceinline__ int lane_xor(int v) {
    if constexpr (M == 1)
        return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);   // quad_perm [1, 0, 3, 2]
    else if constexpr (M == 2)
        return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    else if constexpr (M == 8)
        return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
    else if constexpr (M == 4 || M == 16)
        return __builtin_amdgcn_ds_swizzle(v, (M << 10) | 0x1F);           // bit mode: and 0x1F, or 0, xor M
    else
        return __shfl_xor(v, M);
}

// U per-lane partial sums T[0 .. U) -> ONE total per lane: the sum over the G lanes of a row group of T[ue], ue the
// bit reversal of (t & (U - 1)) in log2(U) bits.  A halving step sends the half of the values the partner keeps and keeps
// the other half: U - 1 exchanges, then log2(G / U) for the single value left — U - 1 + log2(G / U) cross-lane
// operations where a butterfly per value takes U log2(G).  Integer sums: any order gives the same bits.
template <int G, int U, int M = 1>
__device__ __forceinline__ int code8_reduce(int (&T)[U], int t) {
    if constexpr (M < U) {
        constexpr int H = U / (2 * M);   // values left after this step
        const bool hi = (t & M) != 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const int send = hi ? T[j] : T[j + H];
            const int keep = hi ? T[j + H] : T[j];
            T[j] = keep + lane_xor<M>(send);
        }
        return code8_reduce<G, U, M * 2>(T, t);
    } else if constexpr (M < G) {
        T[0] += lane_xor<M>(T[0]);
        return code8_reduce<G, U, M * 2>(T, t);
    } else {
        return T[0];
    }
}

// One wave takes batches of RB = (64 / G) U consecutive rows, 0.75 U KiB of the high plane (d = 16 G; 576 U bytes at d = 384).
// Per batch: U 12-byte loads per lane at one base per batch + a lane offset that never changes + u row-group strides, ONE
// 8-byte load of (a, r) (lane (g, t) reads the entry of the row whose total code8_reduce leaves in it), the unpacking of
// (c & ~3) (code8_unpack_high), 8 U v_dot4_i32_i8, the reduction above, and ONE epilogue + ballot for the RB rows of the
// batch (lanes t < U hold one row each).  Full batches run in a loop without a row clamp or a row test; the one partial batch
// at the end of the index is done by the wave whose turn it is, with both.
//
// Two stages.  With H = c & ~3 the loop has T6 = Q . H, and the row's integer sum is T = T6 + Q . (c & 3) with
// T6 - 3 N <= T <= T6 + 3 P, P (N) the sum of the positive (the magnitudes of the negative) Q_j.  Stage 1 evaluates the
// predicate at the upper end (stage1 below: it passes every row the predicate passes at T — DESIGN.md section 4.1b) and
// STAGES the (row, T6) pairs it cannot reject, one per lane.  When 64 are staged, and once at the wave's end, refine() gathers
// the low plane of the staged rows — batches of RB staged rows, lane t the dword of chunk t, U gathers in flight — completes
// T, and runs the predicate itself on T: what is appended is what the one-plane prefilter appended, row for row.
typedef int i32x3 __attribute__((ext_vector_type(3), aligned(4)));

// the narrow parts a lane of the front form holds per tile: the dword of its one chunk, or (the quad form) the 16-byte unit
// of its four chunks
template <bool QUAD>
struct Code8Narrow {
    typedef int type;
    static __device__ __forceinline__ int part(int v, int) { return v; }
};
template <>
struct Code8Narrow<true> {
    typedef i32x4 type;
    static __device__ __forceinline__ int part(const i32x4& v, int s) { return v[s]; }
};

//
// The front form (GF > 0: GF lanes per row, UF tiles per batch).  Stage 0 in front of the two: the loop streams the FRONT plane
// (H5 = c & ~7, 5 d / 8 bytes per row; a lane holds a 32-code chunk: one 16-byte and one 4-byte load), has T5 = Q . H5 and
// T5 - 7 N <= T <= T5 + 7 P, and evaluates the predicate at the upper end exactly as stage 1 does with 3 (the same proof, the
// same int32 argument: every factor H5_j + 7 [Q_j > 0] lies in [-128, 127]).  The rows it cannot reject are staged, 64 per
// wave; gather0() fetches their chunks of the high plane and their (a, r) in this kernel's (G, U) geometry, forms T6 with
// `scores` and hands it to stage 1: from there on the row goes the way it goes in the other form.  What is appended is the
// same set of rows; only the order of the appends differs.
// The quad form of stage 0 (GF = 4 at d = 512, the quad layout of the plane): a lane quad per row, a lane holds four chunks —
// five 16-byte loads per lane and tile, each one contiguous KiB per wave-instruction, 64 v_dot4 into one (hi, lo) pair, two
// quad-local DPP adds (code8_reduce<4, UF>) — and UF counts tiles of 16 rows.  T5 is the same integer: everything behind
// it is the other form's, statement for statement.
//
// LIFT (the index holds the bit plane): lift0 in place of gather0.  Stage 0 stages (row, T5, a, r) — all four were in the
// reporting lane's registers — and the survivors' T6 is LIFTED from T5: T6 = T5 + 4 Q . b2 (the bit plane above), in stage 0's
// own geometry and on its query registers.  Lane tf of a row's GF lanes loads the NC dwords of the row's bit plane that belong
// to its chunks (16 bytes in the quad form), spreads every nibble to four bytes of 0 / 1, runs 16 v_dot4 per 32 codes into one
// (hi, lo) pair, and the GF lanes add up (code8_reduce<GF, 1>: every lane ends with the total).  The int32 argument: every
// factor H5_j + 4 lies in [-128, 127].  stage1 gets the same rows with the same T6 and the same (a, r) as from gather0.
// A survivor fetches d / 8 bytes where gather0 fetches 3 d / 4 + 8.  The staged rows are drained inline when 64 are staged
// and at the wave's end (drain0), the loads of up to four wave-instructions — 4 x 64 / GF rows, all 64 in the quad form — in
// flight per lane: one round trip where gather0 takes four.  (Built and measured, not kept: the loads of 64 / GF staged rows
// issued behind each batch's stream loads and consumed behind its scoring — 1.7 us slower than the inline drains at 10M x 512,
// DESIGN.md section 4.1b, "The bit plane".)
//
// HANDOFF (the quad front form with the lift only): a FIFTH wave per block takes the survivors.  Waves 0 .. 3 are the
// producers: the parent's streaming waves, batch for batch (gw, nwaves_total and the owner of the partial batch are computed
// from four waves).  Every producer owns a ring in LDS (Code8Ring: a quarter of the entries each).  Where stage 0's ballot is
// not empty the wave reserves popcount(pass) slots of its ring — granted iff they fit between its tail and the head the
// survivor wave has released; the tail is the wave's own, so nothing is swapped —, every passing lane writes its 16-byte
// entry to the slot of its rank among the set bits, and the new tail is stored with release: the entries below it are
// complete.  A refused reservation (the ring is full) sends that batch's survivors down the parent's path: staged in the
// wave's own registers, drained inline at 64 and at the wave's end.  Wave 4 streams nothing: it polls the four tails
// (s_sleep between polls that find too little), copies up to 64 entries, ring after ring and each in its order, into the
// lift's staging registers, releases the heads, and runs drain0 -> stage1 -> refine -> append -> flush unchanged: a survivor
// meets the same arithmetic with the same (T5, a, r) on whichever wave takes it, and that wave counts it.
// (Built and measured first: ONE ring, slots reserved by a compare-and-swap on a shared tail, a ready word per slot — its
// two LDS round trips per batch with a survivor cost more than the parent's staging: DESIGN.md section 4.1b.)
// WAITING.  The only wait in this kernel is wave 4 waiting for the four producer waves OF ITS OWN BLOCK.  A producer never
// waits — not for its ring, not for wave 4, not for another producer — so it always ends and counts itself into `done`; wave 4
// leaves when done == 4 and the rings are empty.  Nothing waits on another block, on a count of resident blocks or on global
// memory: all five waves of a block are resident together by construction.  No block-wide barrier follows the head.
// ORDER.  `tail`, `head` and `done` are workgroup-scope atomics: release by the writer behind what it covers (the entries
// below the tail; the copies out of the slots below the head; the wave's last entries), acquire by the reader in front of
// what depends on it.  Nothing relies on the order of LDS instructions across waves.
template <int G, int U, bool MASKED, int GF = 0, int UF = 0, bool LIFT = false, bool HANDOFF = false>
__global__ __launch_bounds__(kScanThreads + (HANDOFF ? kWave : 0)) void code8_scan_kernel(Code8ScanArgs a) {
    constexpr int RPI = kWave / G;
    constexpr int RB = RPI * U;
    constexpr bool FRONT = GF > 0;
    static_assert(U >= 2 && U <= 8 && (U & (U - 1)) == 0 && U <= G, "code8_reduce halves U down to one value inside a row group");
    // (the quad form: a lane holds kCode8QuadChunks chunks of an unmasked row of 16 G codes; one tile per batch is allowed)
    constexpr bool QUAD = FRONT && !MASKED && GF * 32 * kCode8QuadChunks == G * 16;
    static_assert(!FRONT || (UF >= (QUAD ? 1 : 2) && UF <= 8 && (UF & (UF - 1)) == 0 && UF <= GF && kWave % GF == 0), "the same, for the front form");
    static_assert(!HANDOFF || (QUAD && LIFT), "the survivor wave serves the quad front form with the lift");
    constexpr int NW = kScanWaves + (HANDOFF ? 1 : 0);   // waves of the block: the head's merge is shared out among all of them
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = lane % G;
    const int g = lane / G;
    const bool valid = !MASKED || t * 16 < a.d;

    i32x4 qh = {0, 0, 0, 0}, ql = {0, 0, 0, 0};
    if (valid) {
        qh = *reinterpret_cast<const i32x4*>(a.qhi + t * 16);
        ql = *reinterpret_cast<const i32x4*>(a.qlo + t * 16);
    }
    const float qstep = a.par[0], alpha = a.par[1], beta = a.par[2];
    float floor = 0.f;   // (set below, behind the first batch's loads, before anything reads it)

    // 3 P and 3 N of the query, from the lane's planes (a masked lane holds zeros); at most 3 d qmax < 2^26
    int p3 = 0, n3 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int Q = ((qh[j] << (24 - 8 * b)) >> 24) * 256 + ((ql[j] << (24 - 8 * b)) >> 24);
            p3 += Q > 0 ? Q : 0;
            n3 += Q < 0 ? -Q : 0;
        }
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        p3 += __shfl_xor(p3, m);
        n3 += __shfl_xor(n3, m);
    }
    const int p7 = __builtin_amdgcn_readfirstlane(p3) * 7, n7 = __builtin_amdgcn_readfirstlane(n3) * 7;   // (stage 0; at most 7 d qmax < 2^27)
    p3 = __builtin_amdgcn_readfirstlane(p3) * 3;
    n3 = __builtin_amdgcn_readfirstlane(n3) * 3;

    // the wave's staged rows (range_scan_kernel's append path)
    uint32_t stage = 0;
    int nst = 0;
    const unsigned long long cap = (unsigned long long)a.cap;
    auto flush = [&]() __attribute__((always_inline)) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.counter, (unsigned long long)nst);
        base = readlane_u64(base, 0);
        if (lane < nst && base + (unsigned long long)lane < cap) a.cand[base + lane] = stage;
        nst = 0;
    };
    auto append = [&](uint64_t m, uint32_t row) __attribute__((always_inline)) {
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)row, src);
            if (lane == nst) stage = v;
            if (++nst == kWave) flush();
        }
    };

    // the row of the batch whose total this lane ends up with (code8_reduce), and whether it is the lane that reports it
    int ue = 0;
#pragma unroll
    for (int m = 1, h = U / 2; m < U; m <<= 1, h >>= 1) ue += (t & m) ? h : 0;
    const int erow = ue * RPI + g;
    const uint64_t elanes = __ballot(t < U);

    // (c & ~3) of the lane's chunks against the query's planes: T6
    auto scores = [&](const i32x3 (&x)[U], int (&T)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t h[3] = {(uint32_t)x[u].x, (uint32_t)x[u].y, (uint32_t)x[u].z};
            uint32_t c[4];
            code8_unpack_high(h, c);
            int hi = 0, lo = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                hi = __builtin_amdgcn_sdot4((int)c[j], qh[j], hi, false);
                lo = __builtin_amdgcn_sdot4((int)c[j], ql[j], lo, false);
            }
            T[u] = hi * 256 + lo;
        }
    };
    // THE predicate, on the row's integer sum.  Every lane evaluates it (its (a, r) load is issued with the batch's loads, not
    // behind a lane test); `mine` keeps the bits of the lanes that report a row
    auto epilogue = [&](int tot, float2 sr, uint64_t mine, int64_t r) __attribute__((always_inline)) {
        const float s = ((float)tot * qstep) * sr.x;
        float m = fmaf(alpha, sr.y, beta);
        m = fmaf(fabsf(s) + m, 2.4e-7f, m);   // the rounding of s + m itself
        const float ub = s + m;
        // NaN (0 * inf: a zero query against a row of unbounded residual) passes
        const uint64_t pass = __ballot(!(ub < floor)) & mine;
        if (pass) append(pass, (uint32_t)r);
    };

    // ---- stage 2: the staged (row, T6) pairs -> T -> the predicate ----
    uint32_t srow = 0;
    int st6 = 0, ns1 = 0;
    unsigned long long nrefined = 0;   // (the diagnostic count: one atomic per wave, at its end)
    const int lstride4 = a.d / 16;   // dwords per row of the low plane
    auto refine = [&]() __attribute__((always_inline)) {
        nrefined += (unsigned long long)ns1;
        for (int base = 0; base < ns1; base += RB) {
            // staged entries past the last re-read the last one, their result is discarded
            uint32_t lw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int e = base + u * RPI + g;
                e = e < ns1 - 1 ? e : ns1 - 1;
                const uint32_t row = (uint32_t)__shfl((int)srow, e);
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.low) + (int64_t)row * lstride4 + t;
                if (MASKED)
                    lw[u] = valid ? *src : 0u;
                else
                    lw[u] = *src;
            }
            const int e = base + erow;
            const int ec = e < ns1 - 1 ? e : ns1 - 1;
            const uint32_t row = (uint32_t)__shfl((int)srow, ec);
            const int t6 = __shfl(st6, ec);
            const float2 sr = a.ar[row];
            int T[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t c[4];
                code8_unpack_low(lw[u], c);
                int hi = 0, lo = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    hi = __builtin_amdgcn_sdot4((int)c[j], qh[j], hi, false);
                    lo = __builtin_amdgcn_sdot4((int)c[j], ql[j], lo, false);
                }
                T[u] = hi * 256 + lo;
            }
            epilogue(t6 + code8_reduce<G, U>(T, t), sr, __ballot(t < U && e < ns1), row);
        }
        ns1 = 0;
    };
    // ---- stage 1: the predicate at the upper end of what the low plane can make of T6 ----
    // s(T) is monotone in T (the conversion and the two products by qstep, a >= 0 round monotonically): sl <= s(T) <= su, so
    // |s(T)| <= max(|sl|, |su|), the margin formed from that is >= the predicate's, and su + it is >= the predicate's bound, bit
    // for bit (fp32 + and fma are monotone in every operand) — or NaN, which passes.  The lower end saturates at INT_MIN: still
    // <= T, which fits (code8_qmax).
    auto stage1 = [&](int t6, float2 sr, uint64_t mine, int64_t r) __attribute__((always_inline)) {
        const int tl = (t6 > INT_MIN + n3 ? t6 : INT_MIN + n3) - n3;
        const float su = ((float)(t6 + p3) * qstep) * sr.x;
        const float sl = ((float)tl * qstep) * sr.x;
        float m = fmaf(alpha, sr.y, beta);
        m = fmaf(fmaxf(fabsf(su), fabsf(sl)) + m, 2.4e-7f, m);
        const float ub = su + m;
        uint64_t pass = __ballot(!(ub < floor)) & mine;
        while (pass) {
            const int src = __ffsll((long long)pass) - 1;
            pass &= pass - 1;
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r, src);
            const int w = __builtin_amdgcn_readlane(t6, src);
            if (lane == ns1) {
                srow = v;
                st6 = w;
            }
            if (++ns1 == kWave) refine();
        }
    };

    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    __shared__ float sfloor;

    if constexpr (FRONT) {
        constexpr int RPF = kWave / GF;
        constexpr int RBF = RPF * UF;
        const int tf = lane % GF;
        const int gf = lane / GF;
        const bool validf = !MASKED || tf * 32 < a.d;
        // the chunks a lane holds: one, or (the quad form) the chunks NC tf .. NC tf + NC - 1 — 32 NC dimensions of the query's
        // planes, 4 NC i32x4; their narrow parts arrive as ONE word of the lane's (one dword, or the quad layout's 16-byte unit)
        constexpr int NC = QUAD ? kCode8QuadChunks : 1;
        typedef typename Code8Narrow<QUAD>::type narrow_t;
        i32x4 fh[NC][2], fl[NC][2];
#pragma unroll
        for (int s = 0; s < NC; ++s) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fh[s][i] = i32x4{0, 0, 0, 0};
                fl[s][i] = i32x4{0, 0, 0, 0};
                if (validf) {
                    fh[s][i] = *reinterpret_cast<const i32x4*>(a.qhi + (tf * NC + s) * 32 + 16 * i);
                    fl[s][i] = *reinterpret_cast<const i32x4*>(a.qlo + (tf * NC + s) * 32 + 16 * i);
                }
            }
        }
        int uef = 0;
#pragma unroll
        for (int m = 1, h = UF / 2; m < UF; m <<= 1, h >>= 1) uef += (tf & m) ? h : 0;
        const int erowf = uef * RPF + gf;
        const uint64_t elanesf = __ballot(tf < UF);

        // the counts as block 0 finds them, for the host's window (index_state.hpp): no synchronisation, they lag
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const unsigned int calls = atomicAdd(a.front_calls, 1u);
            const unsigned long long sum = atomicAdd(a.front_survivors, 0ull);
            if (a.front_msum) {
                *a.front_msum = sum;
                *a.front_mcalls = calls;
            }
        }

        // (c & ~7) of the lane's chunks against the query's planes: T5
        // (ONE running (hi, lo) pair over the lane's chunks, T5 = hi * 256 + lo formed once: the partial sums are smaller in
        // magnitude than the bound of the row's total, so the int32 argument holds for them)
        auto scores0 = [&](const i32x4 (&xw)[UF][NC], const narrow_t (&xn)[UF], int (&T)[UF]) {
#pragma unroll
            for (int u = 0; u < UF; ++u) {
                int hi = 0, lo = 0;
#pragma unroll
                for (int s = 0; s < NC; ++s) {
                    const uint32_t f[5] = {(uint32_t)xw[u][s].x, (uint32_t)xw[u][s].y, (uint32_t)xw[u][s].z, (uint32_t)xw[u][s].w,
                                           (uint32_t)Code8Narrow<QUAD>::part(xn[u], s)};
                    uint32_t c[8];
                    code8_front_unpack_chunk(f, c);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        hi = __builtin_amdgcn_sdot4((int)c[j], fh[s][j >> 2][j & 3], hi, false);
                        lo = __builtin_amdgcn_sdot4((int)c[j], fl[s][j >> 2][j & 3], lo, false);
                    }
                }
                T[u] = hi * 256 + lo;
            }
        };
        // ---- the rows stage 0 staged -> their chunks of the high plane -> T6 -> stage 1 ----
        uint32_t s0row = 0;
        int ns0 = 0;
        unsigned long long nfront = 0;   // (one atomic per wave, at its end)
        auto gather0 = [&]() __attribute__((always_inline)) {
            nfront += (unsigned long long)ns0;
#if defined(MVDB_CODE8_ABLATE_GATHER) && MVDB_CODE8_ABLATE_GATHER == 2
            ns0 = 0;   // (the timing ablation: the survivors are counted and discarded)
#endif
            for (int base = 0; base < ns0; base += RB) {
                // staged entries past the last re-read the last one, their result is discarded
                i32x3 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    int e = base + u * RPI + g;
                    e = e < ns0 - 1 ? e : ns0 - 1;
                    const uint32_t row = (uint32_t)__shfl((int)s0row, e);
                    const i32x3* src = reinterpret_cast<const i32x3*>(a.high + (int64_t)row * a.hstride + t * 12);
                    if (MASKED)
                        x[u] = valid ? *src : i32x3{0, 0, 0};
                    else
                        x[u] = *src;
                }
                const int e = base + erow;
                const int ec = e < ns0 - 1 ? e : ns0 - 1;
                const uint32_t row = (uint32_t)__shfl((int)s0row, ec);
                const float2 sr = a.ar[row];
#if defined(MVDB_CODE8_ABLATE_GATHER) && MVDB_CODE8_ABLATE_GATHER == 3
                // (the timing ablation: the gathers are waited for — an empty statement takes their registers — and dropped)
#pragma unroll
                for (int u = 0; u < U; ++u) asm volatile("" ::"v"(x[u].x), "v"(x[u].y), "v"(x[u].z));
                asm volatile("" ::"v"(sr.x), "v"(sr.y));
                continue;
#endif
                int T[U];
                scores(x, T);
                stage1(code8_reduce<G, U>(T, t), sr, __ballot(t < U && e < ns0), row);
            }
            ns0 = 0;
        };
        // ---- LIFT: the rows stage 0 staged -> their dwords of the bit plane -> T6 = T5 + 4 Q . b2 -> stage 1 ----
        // (staged per lane beside the row: T5 and (a, r) as the reporting lane held them)
        int st5 = 0;
        float sta = 0.f, str = 0.f;
        // the loads of the staged rows base + gf (lane (gf, tf): the dwords of its own chunks); entries past the last
        // re-read the last one
        auto lift_load = [&](int base) __attribute__((always_inline)) {
            int e = base + gf;
            e = e < ns0 - 1 ? e : ns0 - 1;
            const uint32_t row = (uint32_t)__shfl((int)s0row, e);
            const narrow_t* src = reinterpret_cast<const narrow_t*>(a.bit2 + (int64_t)row * code8_bit2_stride(a.d) + tf * (NC * 4));
            if (MASKED) return validf ? *src : narrow_t{};
            return *src;
        };
        auto lift_use = [&](const narrow_t& w, int base) __attribute__((always_inline)) {
            int hi = 0, lo = 0;
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                const uint32_t word = (uint32_t)Code8Narrow<QUAD>::part(w, s);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int b2 = (int)code8_bit2_spread(word, j);
                    hi = __builtin_amdgcn_sdot4(b2, fh[s][j >> 2][j & 3], hi, false);
                    lo = __builtin_amdgcn_sdot4(b2, fl[s][j >> 2][j & 3], lo, false);
                }
            }
            int T[1] = {hi * 256 + lo};
            const int tot = code8_reduce<GF, 1>(T, tf);
            const int e = base + gf;
            const int ec = e < ns0 - 1 ? e : ns0 - 1;
            const uint32_t row = (uint32_t)__shfl((int)s0row, ec);
            const int t5 = __shfl(st5, ec);
            const float2 sr = make_float2(__shfl(sta, ec), __shfl(str, ec));
            stage1(t5 + 4 * tot, sr, __ballot(tf == 0 && e < ns0), row);
        };
        // all staged rows, inline: the loads of up to four wave-instructions in flight
        auto drain0 = [&]() __attribute__((always_inline)) {
            constexpr int UL = 4;
            nfront += (unsigned long long)ns0;
#if defined(MVDB_CODE8_ABLATE_GATHER) && MVDB_CODE8_ABLATE_GATHER == 2
            ns0 = 0;   // (the timing ablation: the survivors are counted and discarded)
#endif
            for (int base = 0; base < ns0; base += UL * RPF) {
                narrow_t w[UL];
#pragma unroll
                for (int u = 0; u < UL; ++u) w[u] = lift_load(base + u * RPF);
#if defined(MVDB_CODE8_ABLATE_GATHER) && MVDB_CODE8_ABLATE_GATHER == 3
                // (the timing ablation: the loads are waited for — an empty statement takes their registers — and dropped)
#pragma unroll
                for (int u = 0; u < UL; ++u) asm volatile("" ::"v"(w[u]));
                continue;
#endif
                // (ONE copy of lift_use and of what stage1 inlines: the words move down instead)
#pragma unroll 1
                for (int at = base; at < ns0 && at < base + UL * RPF; at += RPF) {
                    lift_use(w[0], at);
#pragma unroll
                    for (int u = 0; u + 1 < UL; ++u) w[u] = w[u + 1];
                }
            }
            ns0 = 0;
        };
        // ---- HANDOFF: the ring, and a batch's survivors into it (false: refused, the caller stages them itself) ----
        [[maybe_unused]] Code8Ring* rg = nullptr;
        if constexpr (HANDOFF) {
            __shared__ Code8Ring ring_store;
            rg = &ring_store;
        }
        [[maybe_unused]] const uint32_t rsub = (uint32_t)a.ring / kScanWaves, rmask = rsub - 1u;   // entries of one producer's ring
        [[maybe_unused]] uint32_t mytail = 0u;    // this producer's tail (wave-uniform)
        [[maybe_unused]] uint32_t hd_seen = 0u;   // its ring's head as the wave last read it: read again only when that one refuses
        [[maybe_unused]] auto ring_put = [&](uint64_t pass, int t5, float2 sr, uint32_t r) __attribute__((always_inline)) {
            const uint32_t cnt = (uint32_t)__popcll(pass);
            // (the head only grows: a stale value refuses too early, never too late — and was read with acquire, so the slots
            // below it + rsub have been copied out)
            if (mytail - hd_seen + cnt > rsub) {
                hd_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&rg->head[wave], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (mytail - hd_seen + cnt > rsub) return false;
            }
            if ((pass >> lane) & 1ull) {
                const uint32_t slot = (uint32_t)wave * rsub + ((mytail + (uint32_t)__popcll(pass & ((1ull << lane) - 1ull))) & rmask);
                rg->slot[slot] = i32x4{(int)r, t5, (int)__float_as_uint(sr.x), (int)__float_as_uint(sr.y)};
            }
            mytail += cnt;
            // (the entries, by every lane that wrote one, in front of the tail that covers them)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&rg->tail[wave], mytail, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            return true;
        };
        // ---- stage 0: the predicate at the upper end of what the missing 3 bits can make of T5 (stage1's form, 7 for 3) ----
        auto stage0 = [&](int t5, float2 sr, uint64_t mine, int64_t r) __attribute__((always_inline)) {
            const int tl = (t5 > INT_MIN + n7 ? t5 : INT_MIN + n7) - n7;
            const float su = ((float)(t5 + p7) * qstep) * sr.x;
            const float sl = ((float)tl * qstep) * sr.x;
            float m = fmaf(alpha, sr.y, beta);
            m = fmaf(fmaxf(fabsf(su), fabsf(sl)) + m, 2.4e-7f, m);
            const float ub = su + m;
            uint64_t pass = __ballot(!(ub < floor)) & mine;
            if constexpr (HANDOFF) {
                if (pass && ring_put(pass, t5, sr, (uint32_t)r)) pass = 0ull;
            }
            while (pass) {
                const int src = __ffsll((long long)pass) - 1;
                pass &= pass - 1;
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r, src);
                if constexpr (LIFT) {
                    const int w = __builtin_amdgcn_readlane(t5, src);
                    const float fa = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(sr.x), src));
                    const float fr = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(sr.y), src));
                    if (lane == ns0) {
                        s0row = v;
                        st5 = w;
                        sta = fa;
                        str = fr;
                    }
                    if (++ns0 == kWave) drain0();
                } else {
                    if (lane == ns0) s0row = v;
                    if (++ns0 == kWave) gather0();
                }
            }
        };

        // one tile's loads of a lane: NC 16-byte loads and the narrow word, each a contiguous span of the tile per
        // wave-instruction.  The quad layout: five 1-KiB slabs, the lane's unit at lane * 16 of each.
        const int nch = a.d / 32;
        const int64_t tile_bytes = (int64_t)RPF * code8_front_stride(a.d);
        const int64_t batch_bytes = (int64_t)UF * tile_bytes;
        constexpr int slab = QUAD ? kWave * 16 : 0;
        const int wide_off = QUAD ? lane * 16 : gf * 16 * nch + tf * 16;
        const int narrow_off = QUAD ? NC * slab + lane * 16 : RPF * 16 * nch + gf * 4 * nch + tf * 4;
        const int64_t nfull = a.n / RBF;
        auto load_tile = [&](const uint8_t* tile, i32x4 (&w)[NC], narrow_t& nr) __attribute__((always_inline)) {
            const narrow_t* ns = reinterpret_cast<const narrow_t*>(tile + narrow_off);
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                const i32x4* ws = reinterpret_cast<const i32x4*>(tile + s * slab + wide_off);
                if (MASKED)
                    w[s] = validf ? __builtin_nontemporal_load(ws) : i32x4{0, 0, 0, 0};
                else
                    w[s] = __builtin_nontemporal_load(ws);
            }
#ifdef MVDB_CODE8_ABLATE
            nr = narrow_t{};   // (the timing ablation: the narrow loads left out — the results are wrong, only the time counts)
            (void)ns;
#else
            if (MASKED)
                nr = validf ? __builtin_nontemporal_load(ns) : narrow_t{};
            else
                nr = __builtin_nontemporal_load(ns);
#endif
        };
        auto load0 = [&](i32x4 (&xw)[UF][NC], narrow_t (&xn)[UF], float2& sr, int64_t b) {
            const uint8_t* base = a.front + b * batch_bytes;
#pragma unroll
            for (int u = 0; u < UF; ++u) load_tile(base + u * tile_bytes, xw[u], xn[u]);
            sr = a.ar[b * RBF + erowf];
        };
        // the head, as in the other form: the first batch's loads, then the floor
        int64_t b = gw;
        const bool head = (!HANDOFF || wave < kScanWaves) && b < nfull;
        i32x4 xw0[UF][NC];
        narrow_t xn0[UF];
        float2 sr0 = make_float2(0.f, 0.f);
        if (head) load0(xw0, xn0, sr0, b);
        if constexpr (HANDOFF) {
            // the empty rings: the barriers of the head stand between these stores and the first entry
            if (threadIdx.x < kScanWaves) {
                rg->tail[threadIdx.x] = 0u;
                rg->head[threadIdx.x] = 0u;
            }
            if (threadIdx.x == 0) rg->done = 0u;
        }
        floor = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__float_as_uint(code8_lists_floor(a.lists, a.nlists, a.k, sh, &sfloor, NW))));
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.floor = floor;
        if constexpr (HANDOFF) {
            if (wave == kScanWaves) {
                // ---- the survivor wave ----
                const uint32_t want = rsub < (uint32_t)kWave ? rsub : (uint32_t)kWave;   // (a full ring always holds as many)
                uint32_t hd[kScanWaves] = {0u, 0u, 0u, 0u};
                for (;;) {
                    // `done` in front of the tails: with all producers ended, the tails are final
                    const uint32_t dn = __hip_atomic_load(&rg->done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    // up to 64 entries: ring after ring, each from its head
                    uint32_t take[kScanWaves], total = 0u;
#pragma unroll
                    for (int w = 0; w < kScanWaves; ++w) {
                        const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&rg->tail[w], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                        const uint32_t av = tl - hd[w], room = (uint32_t)kWave - total;
                        take[w] = av < room ? av : room;
                        total += take[w];
                    }
                    const bool ended = dn == (uint32_t)kScanWaves;
                    if (total >= want || (ended && total > 0u)) {
                        uint32_t o = (uint32_t)lane, at = 0u;   // the lane's entry: the o-th taken of ring w, slot `at`
                        bool found = false;
#pragma unroll
                        for (int w = 0; w < kScanWaves; ++w) {
                            if (!found && o < take[w]) {
                                at = (uint32_t)w * rsub + ((hd[w] + o) & rmask);
                                found = true;
                            }
                            if (!found) o -= take[w];
                            hd[w] += take[w];
                        }
                        if (found) {
                            const i32x4 e = rg->slot[at];
                            s0row = (uint32_t)e.x;
                            st5 = e.y;
                            sta = __uint_as_float((uint32_t)e.z);
                            str = __uint_as_float((uint32_t)e.w);
                        }
                        ns0 = (int)total;
                        // (copied out, by every lane, before the slots can be written again)
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        const uint32_t hmine = lane == 0 ? hd[0] : lane == 1 ? hd[1] : lane == 2 ? hd[2] : hd[3];
                        if (lane < kScanWaves) __hip_atomic_store(&rg->head[lane], hmine, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        drain0();
                    } else if (ended) {
                        break;   // all producers have ended and their rings are empty
                    } else {
                        __builtin_amdgcn_s_sleep(8);
                    }
                }
                if (ns1) refine();
                if (nfront && lane == 0) atomicAdd(a.front_survivors, nfront);
                if (nrefined && lane == 0) atomicAdd(a.survivors, nrefined);
                if (nst) flush();
                return;
            }
        }
        if (head) {
            int T[UF];
            scores0(xw0, xn0, T);
            stage0(code8_reduce<GF, UF>(T, tf), sr0, elanesf, b * RBF + erowf);
            b += nwaves_total;
        }
        for (; b < nfull; b += nwaves_total) {
            i32x4 xw[UF][NC];
            narrow_t xn[UF];
            float2 sr;
            load0(xw, xn, sr, b);
            int T[UF];
            scores0(xw, xn, T);
            stage0(code8_reduce<GF, UF>(T, tf), sr, elanesf, b * RBF + erowf);
        }
        // the partial batch behind the full ones: tiles past the last re-read the last tile (the plane is whole tiles), rows
        // past the end are discarded
        if (nfull * RBF < a.n && nfull % nwaves_total == gw) {
            const int64_t last = a.n - 1;
            const int64_t last_tile = last / RPF;
            i32x4 xw[UF][NC];
            narrow_t xn[UF];
#pragma unroll
            for (int u = 0; u < UF; ++u) {
                int64_t tile = nfull * UF + u;
                tile = tile < last_tile ? tile : last_tile;
                load_tile(a.front + tile * tile_bytes, xw[u], xn[u]);
            }
            const int64_t r = nfull * RBF + erowf;
            const float2 sr = a.ar[r < last ? r : last];
            int T[UF];
            scores0(xw, xn, T);
            stage0(code8_reduce<GF, UF>(T, tf), sr, __ballot(tf < UF && r < a.n), r);
        }
        if constexpr (LIFT) {
            if (ns0) drain0();
        } else {
            if (ns0) gather0();
        }
        if (ns1) refine();
        if (nfront && lane == 0) atomicAdd(a.front_survivors, nfront);
        if (nrefined && lane == 0) atomicAdd(a.survivors, nrefined);
        if (nst) flush();
        if constexpr (HANDOFF) {
            // the wave's entries are ready (release, by every lane that wrote one): it ends
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_fetch_add(&rg->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return;
    }

    const int64_t nfull = a.n / RB;
    const int64_t batch_bytes = (int64_t)RB * a.hstride;
    const int64_t group_bytes = (int64_t)RPI * a.hstride;
    const int lane_off = g * a.hstride + t * 12;

    auto load = [&](i32x3 (&x)[U], float2& sr, int64_t b) {
        const uint8_t* base = a.high + b * batch_bytes + lane_off;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i32x3* src = reinterpret_cast<const i32x3*>(base + u * group_bytes);
            if (MASKED)
                x[u] = valid ? __builtin_nontemporal_load(src) : i32x3{0, 0, 0};
            else
                x[u] = __builtin_nontemporal_load(src);
        }
        sr = a.ar[b * RB + erow];
    };
    // The head: the floor, merged by every block from the lists the seed launch's blocks left (the same bits in every block:
    // code8_lists_floor).  The wave's first batch depends on neither the floor nor the merge: its loads are issued first.
    int64_t b = gw;
    const bool head = b < nfull;
    i32x3 x0[U];
    float2 sr0 = make_float2(0.f, 0.f);
    if (head) load(x0, sr0, b);
    // (wave-uniform: held in a scalar register, so that the loop's compare takes it as an SGPR operand)
    floor = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane(
        (int)__float_as_uint(code8_lists_floor(a.lists, a.nlists, a.k, sh, &sfloor, kScanWaves))));
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.floor = floor;
    if (head) {
        int T[U];
        scores(x0, T);
        stage1(code8_reduce<G, U>(T, t), sr0, elanes, b * RB + erow);
        b += nwaves_total;
    }
    for (; b < nfull; b += nwaves_total) {
        i32x3 x[U];
        float2 sr;
        load(x, sr, b);
        int T[U];
        scores(x, T);
        stage1(code8_reduce<G, U>(T, t), sr, elanes, b * RB + erow);
    }
    // the partial batch behind the full ones: rows past the end re-read the last row, their result is discarded
    if (nfull * RB < a.n && nfull % nwaves_total == gw) {
        const int64_t last = a.n - 1;
        i32x3 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = nfull * RB + (int64_t)u * RPI + g;
            r = r < last ? r : last;
            const i32x3* src = reinterpret_cast<const i32x3*>(a.high + r * (int64_t)a.hstride + t * 12);
            if (MASKED)
                x[u] = valid ? __builtin_nontemporal_load(src) : i32x3{0, 0, 0};
            else
                x[u] = __builtin_nontemporal_load(src);
        }
        const int64_t r = nfull * RB + erow;
        const float2 sr = a.ar[r < last ? r : last];
        int T[U];
        scores(x, T);
        stage1(code8_reduce<G, U>(T, t), sr, __ballot(t < U && r < a.n), r);
    }
    if (ns1) refine();
    if (nrefined && lane == 0) atomicAdd(a.survivors, nrefined);
    if (nst) flush();
}

// ---- the floor: lower bounds of a sample of rows, from the codes -----------------------------------------------------------------
// The sample: rows (i * n) / kCode8Seed, i in [0, kCode8Seed) (n >= kCode8Seed: distinct, ascending).  For each, the coded score
// s~ and the margin m exactly as code8_scan_kernel's epilogue forms them, then lb = s~ - m in fp32: the exact kernel's score
// of the row is >= lb (the lower half of the route's bound).  floor = the k-th best lb: k distinct rows score at least that, so
// the final k-th best score does — the unchanged prefilter predicate !(ub < floor) keeps every row of the final top-k
// (DESIGN.md section 4.1b).  Fewer than k lower bounds (or a k-th of -inf): floor = -FLT_MAX, everything passes, the call
// falls back.  A NaN lb (0 * inf) fails the gate and never enters a list.
// This launch ends when every block has stored the k best lower bounds of its share of the sample; the k-th best of their
// union is taken by the prefilter's blocks (code8_lists_floor).
//
// The index keeps the sample's codes and (a, r) a second time, slot i at i, in one allocation (kCode8Seed * (d + 8) bytes:
// the codes, then the (a, r) entries); code8_sample_kernel gathers it whenever the code it copies was written (the rule:
// Code8Store::gather_sample in mvdb.hip).  The copy is plain int8, d bytes per slot (put together from the two planes): the floor's
// launch streams it in 16-byte chunks, batch by batch as code8_scan_kernel streams the high plane.
// Roofline: HBM; bytes = kCode8Seed * (d + 8).
constexpr int64_t kCode8Seed = 131072;
constexpr int kCode8SeedMaxThreads = 1024;
constexpr int kCode8SeedThreads = 512;   // one block of this many per CU: measured

__host__ __device__ inline int64_t code8_sample_row(int64_t slot, int64_t n) { return (slot * n) / kCode8Seed; }
inline size_t code8_sample_bytes(int d) { return (size_t)kCode8Seed * ((size_t)d + sizeof(float2)); }

// One thread per 16-code chunk of a slot: the chunk's 12 + 4 bytes of the two planes are put together again — the stored
// sample is plain int8, d bytes per slot.  The thread of a slot's first chunk also copies its (a, r).
__global__ __launch_bounds__(256) void code8_sample_kernel(const uint8_t* __restrict__ high, const uint8_t* __restrict__ low,
                                                           const float2* __restrict__ ar, int64_t n, int d, int8_t* __restrict__ scodes,
                                                           float2* __restrict__ sar) {
    const int d16 = d / 16;
    const int64_t total = kCode8Seed * d16;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = j / d16;
        const int c = (int)(j - slot * d16);
        const int64_t row = code8_sample_row(slot, n);
        const uint32_t* hsrc = reinterpret_cast<const uint32_t*>(high + row * code8_high_stride(d)) + 3 * c;
        const uint32_t h[3] = {hsrc[0], hsrc[1], hsrc[2]};
        uint32_t w[4];
        code8_unpack_chunk(h, reinterpret_cast<const uint32_t*>(low + row * code8_low_stride(d))[c], w);
        reinterpret_cast<i32x4*>(scodes + slot * d)[c] = i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        if (c == 0) sar[slot] = ar[row];
    }
}

struct Code8SeedArgs {
    const int8_t* scodes;   // [kCode8Seed, d] the stored sample (code8_sample_kernel)
    const float2* sar;      // [kCode8Seed]
    int d;
    const float* q;         // the query as the caller gave it
    int normalize_q;
    float row_norm_bound;
    int8_t* qhi;            // out (block 0): the planes and the terms, for the prefilter and the re-score
    int8_t* qlo;
    float* par;
    unsigned long long* counter;   // out (block 0): the candidate counter, zeroed
    int k;
    uint64_t* lists;        // out: [gridDim.x, k] every block's sorted k-list (slots it does not fill: 0)
};

// Every block computes the query's image itself (code8_query_image: the same bits in every block) and takes the planes from
// LDS; block 0 also leaves the image and the zeroed candidate counter in the workspace for the launches behind this one.
// Every block of the grid stores a list — there is no path from the kernel's entry to the store that returns.
template <int G, int U, bool MASKED>
__global__ __launch_bounds__(kCode8SeedMaxThreads) void code8_seed_kernel(Code8SeedArgs a) {
    constexpr int RPI = kWave / G;
    constexpr int RB = RPI * U;
    static_assert(U >= 2 && U <= 8 && (U & (U - 1)) == 0 && U <= G, "code8_reduce halves U down to one value inside a row group");
    static_assert(kCode8Seed % RB == 0, "the sample is whole batches");
    __shared__ uint64_t sh[(kCode8SeedMaxThreads / kWave - 1) * kWave];
    __shared__ Code8QueryShared shq;
    __shared__ __attribute__((aligned(16))) int8_t splanes[2 * kCode8MaxDim];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int t = lane % G;
    const int g = lane / G;
    const bool valid = !MASKED || t * 16 < a.d;

    int ue = 0;
#pragma unroll
    for (int m = 1, h = U / 2; m < U; m <<= 1, h >>= 1) ue += (t & m) ? h : 0;
    const int erow = ue * RPI + g;
    const bool reports = t < U;

    // code8_scan_kernel's load over the stored sample: one base per batch + the constant lane offset + u row-group strides
    const int64_t batch_bytes = (int64_t)RB * a.d;
    const int64_t group_bytes = (int64_t)RPI * a.d;
    const int lane_off = g * a.d + t * 16;
    auto load = [&](i32x4 (&x)[U], float2& sr, int64_t b) {
        const int8_t* base = a.scodes + b * batch_bytes + lane_off;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i32x4* src = reinterpret_cast<const i32x4*>(base + u * group_bytes);
            if (MASKED)
                x[u] = valid ? __builtin_nontemporal_load(src) : i32x4{0, 0, 0, 0};
            else
                x[u] = __builtin_nontemporal_load(src);
        }
        sr = a.sar[b * RB + erow];
    };

    // the wave's first batch does not depend on the query: its loads are in flight while the image is computed
    const int64_t nb = kCode8Seed / RB;
    const int64_t stride = (int64_t)gridDim.x * nwaves;
    int64_t b = (int64_t)blockIdx.x * nwaves + wave;
    i32x4 x[U];
    float2 sr = make_float2(0.f, 0.f);
    if (b < nb) load(x, sr, b);

    float par[4];
    code8_query_image(a.q, a.d, a.normalize_q, a.row_norm_bound, splanes, splanes + kCode8MaxDim, par, shq);
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < a.d; j += blockDim.x) {
            a.qhi[j] = splanes[j];
            a.qlo[j] = splanes[kCode8MaxDim + j];
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a.par[j] = par[j];
            *a.counter = 0ull;
        }
    }
    i32x4 qh = {0, 0, 0, 0}, ql = {0, 0, 0, 0};
    if (valid) {
        qh = *reinterpret_cast<const i32x4*>(splanes + t * 16);
        ql = *reinterpret_cast<const i32x4*>(splanes + kCode8MaxDim + t * 16);
    }
    const float qstep = par[0], alpha = par[1], beta = par[2];

    WaveTopK tk;
    tk.init(a.k);

    // (the key's row is the SLOT: only the scores decide the floor)
    auto consume = [&](const i32x4 (&x)[U], float2 sr, int64_t b) {
        int T[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int hi = 0, lo = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                hi = __builtin_amdgcn_sdot4(x[u][j], qh[j], hi, false);
                lo = __builtin_amdgcn_sdot4(x[u][j], ql[j], lo, false);
            }
            T[u] = hi * 256 + lo;
        }
        const int tot = code8_reduce<G, U>(T, t);
        const float s = ((float)tot * qstep) * sr.x;
        float m = fmaf(alpha, sr.y, beta);
        m = fmaf(fabsf(s) + m, 2.4e-7f, m);
        const float lb = s - m;
        const bool pass = reports && lb >= tk.thr_score;   // NaN fails
        if (__ballot(pass)) tk.offer(pass ? make_key(lb, (uint32_t)(b * RB + erow)) : 0ull);
    };

    // the next batch's loads are issued before this batch is consumed
    for (; b < nb; b += stride) {
        i32x4 xn[U];
        float2 srn = sr;
        const int64_t bn = b + stride;
        if (bn < nb) load(xn, srn, bn);
        consume(x, sr, b);
        if (bn < nb) {
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = xn[u];
        }
        sr = srn;
    }

    code8_block_merge(tk, sh, nwaves);
    if (wave == 0 && lane < a.k) a.lists[(int64_t)blockIdx.x * a.k + lane] = tk.key;
}

// ---- the exact re-score of the candidates, in one launch -------------------------------------------------------------------------
// Decides the fallback as the route always has (the candidates overflowed the capacity, are fewer than k, or the query's norm
// is not finite: *gate = 1 and nothing is written to D or I — the gated exact scan behind this launch answers the call), else
// scores the candidates straight from cand[], in the order the prefilter appended them, and keeps make_key(score, ROW): the
// key order (score descending, row ascending) is the exact scan's tie rule, so no sorted list, no padding and no relabelling
// are needed.  stats (host-mapped): [0] fallbacks so far, [1] candidates of the latest call, [2] calls so far.
// The arithmetic restates flat_scan_kernel<G, C, ...>'s for the shape choose_shape picks (the same prologue, the same fmaf
// chain over chunks c then .x .y .z .w, the same xor butterfly): the scores are the exact scan's bit for bit.
// The grid is fixed at launch; the blocks that work are the first `active`, derived from the count (kCode8RescoreRows per
// block, clamped to the grid); the others return at once.  Every active block ends with the store of its sorted k-list, and
// block 0 leaves `active` (0: the call falls back) in the workspace: code8_finish_kernel, the route's last launch, merges
// exactly those lists and writes (D, I).
constexpr int kCode8RescoreRows = 32;   // measured

struct Code8RescoreArgs {
    const float* X;
    int64_t ld;
    int d4;
    const float* q;
    int normalize_q;
    int k;
    const uint32_t* cand;
    const unsigned long long* counter;
    int64_t cap;
    const float* par;
    int rows_per_block;
    uint64_t* lists;        // out: [active, k]
    int* active;            // out (block 0): the lists this call stored
    int* gate;
    unsigned int* ctr_dev;  // [0] fallbacks, [1] calls
    volatile unsigned int* stats;
};

template <int G, int C, int U, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void code8_rescore_kernel(Code8RescoreArgs a) {
    constexpr int RPI = kWave / G;
    constexpr int RB = RPI * U;
    __shared__ uint64_t sh[(kScanWaves - 1) * kWave];
    const unsigned long long count = *a.counter;
    const bool fallback = count > (unsigned long long)a.cap || count < (unsigned long long)a.k || a.par[3] != 0.f;
    const int64_t cnt = (int64_t)count;   // no fallback: k <= cnt <= cap
    const int64_t want = (cnt + a.rows_per_block - 1) / a.rows_per_block;
    const int active = fallback ? 0 : (int)(want < (int64_t)gridDim.x ? want : (int64_t)gridDim.x);   // no fallback: >= 1
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.gate = fallback ? 1 : 0;
        *a.active = active;
        // (searches of one index on several streams run this concurrently: atomic)
        const unsigned int fb = atomicAdd(&a.ctr_dev[0], fallback ? 1u : 0u) + (fallback ? 1u : 0u);
        const unsigned int calls = atomicAdd(&a.ctr_dev[1], 1u) + 1u;
        if (a.stats) {
            a.stats[0] = fb;
            a.stats[1] = (unsigned int)(count > 0xFFFFFFFFull ? 0xFFFFFFFFull : count);
            a.stats[2] = calls;
        }
    }
    if ((int)blockIdx.x >= active) return;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;
    const int g = lane / G;

    // ---- query -> registers (flat_scan_kernel's prologue) -------------------------------------------
    f32x4 qv[C];
    bool cvalid[C];
    const float* qptr = a.q;
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

    const int64_t nwaves_total = (int64_t)active * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t nbatches = (cnt + RB - 1) / RB;
    const int64_t last = cnt - 1;

    auto batch_rows = [&](int64_t b, uint32_t (&pr)[U]) {
        const int64_t i0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t i = i0 + (int64_t)u * RPI;
            i = i < last ? i : last;  // clamp: tail lanes re-read the last candidate, result discarded
            pr[u] = a.cand[i];
        }
    };
    auto load_batch = [&](const uint32_t (&pr)[U], f32x4 (&x)[U][C]) {
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
    };
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C], const uint32_t (&pr)[U]) {
        const int64_t i0 = b * RB + g;
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
        for (int m = G / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], m);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + (int64_t)u * RPI;
            // gate on the score alone (NaN fails); exact 64-bit order decided inside offer()
            const bool pass = (t == 0) && (i < cnt) && (s[u] >= tk.thr_score);
            if (__ballot(pass)) tk.offer(pass ? make_key(s[u], pr[u]) : 0ull);
        }
    };

    // the candidate ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
    uint32_t pr[U], pn[U];
    if (gw < nbatches) batch_rows(gw, pr);
    for (int64_t b = gw; b < nbatches; b += nwaves_total) {
        f32x4 x[U][C];
        load_batch(pr, x);
        const int64_t bn = b + nwaves_total;
        batch_rows(bn < nbatches ? bn : b, pn);
        consume_batch(b, x, pr);
#pragma unroll
        for (int u = 0; u < U; ++u) pr[u] = pn[u];
    }

    code8_block_merge(tk, sh, kScanWaves);
    if (wave == 0 && lane < a.k) a.lists[(int64_t)blockIdx.x * a.k + lane] = tk.key;
}

// ---- the route's last launch: the block lists of this call -> (D, I) ---------------------------------------------------------------
// One block.  *gate set (the call fell back): the `fallback_lists` lists the gated exact scan left — its grid, known to the
// host; else the `*active` lists code8_rescore_kernel's blocks left.  Both went through the same buffer, the scan's behind
// the re-score's: the count that is read is the one THIS call wrote, so lists of an earlier call with more blocks, or of the
// seed launch, are never merged.  Merged with the bar and the walk of code8_merge_lists; labels and missing slots as
// merge_keys_kernel writes them.
constexpr int kCode8FinishThreads = 1024;

struct Code8FinishArgs {
    const uint64_t* lists;
    const int* gate;
    const int* active;
    int fallback_lists;
    int k;
    int64_t label_offset;
    float* D;
    int64_t* I;
};

__global__ __launch_bounds__(kCode8FinishThreads) void code8_finish_kernel(Code8FinishArgs a) {
    constexpr int NW = kCode8FinishThreads / kWave;
    __shared__ uint64_t sh[(NW - 1) * kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int nlists = *a.gate != 0 ? a.fallback_lists : *a.active;
    WaveTopK tk;
    code8_merge_lists(tk, a.lists, nlists, a.k, sh, NW);
    if (wave == 0 && lane < a.k) {
        const uint64_t key = tk.key;
        float d;
        int64_t id;
        if (key) {
            d = key_score(key);
            id = a.label_offset + (int64_t)key_row(key);
        } else {  // faiss convention for missing results (merge_keys_kernel's)
            d = -3.402823466e+38f;
            id = -1;
        }
        a.D[lane] = d;
        a.I[lane] = id;
    }
}

}  // namespace mvdb
