// code8_scan.hpp — the int8 prefilter of the single-query search.
//
// Beside the fp32 matrix an index may keep, per stored row i, d int8 codes c_i, an fp32 scale a_i and an fp32 UPPER BOUND r_i
// of |x_i - a_i c_i|.  One pass over the codes (1 byte per element instead of 4) computes s~_i = q~ . (a_i c_i) exactly in
// integers (q~: the query rounded to 16 / 15 bits, held as two int8 planes) and keeps every row whose upper bound
// u_i = s~_i + m_i reaches a floor that is proven to lie at or below the final k-th best score.  The kept rows — a few
// thousand of 10M — are then scored by flat_scan_kernel's row-list form: the bits of (D, I) are the full scan's.
//
// Roofline: HBM.  Algorithmic bytes per launch = n * (d + 8): every code once, 8 bytes of (a, r) per row.
//
// Shape of the work (flat_scan_kernel's): G lanes share a row, one 16-byte chunk each (d = 512: G = 32, two rows per
// wave-instruction), U row groups in flight per wave, non-temporal loads, a persistent grid, no branch between the loads of a
// batch.  Per 16 bytes: eight v_dot4_i32_i8; per batch one halving reduction of the U sums and one epilogue (code8_reduce).
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
// most |Q| of the rounded query: 127 * 256 where d * 127 * |Q| fits an int32 (d <= 512), 127 * 128 up to d = 1024
__host__ __device__ inline int code8_qmax(int d) { return d <= 512 ? 32512 : 16256; }

constexpr float kCode8Tiny = 1e-15f;  // a row (a query) whose largest |element| is below this is coded as zero: r = |x| bound

// ---- build: rows [0, n) of X -> codes, (a, r) ------------------------------------------------------------------------------------
// One wave per row.  a = max|x| / 127, c = rint(x / a); r = sqrt(sum (x - a c)^2) rounded up.  A row with a non-finite element
// gets zero codes and r = +inf: it is always a candidate and the exact kernel treats it as it always has.
// list == NULL: rows [0, n) behind the three pointers.  list != NULL (set_rows): the n stored rows list[0 .. n), the pointers
// at row 0; a listed row at or above `limit` (not coded yet) is skipped.
__global__ __launch_bounds__(256) void code8_build_kernel(const float* __restrict__ X, int64_t ld, int d, int64_t n,
                                                          int8_t* __restrict__ codes, float2* __restrict__ ar,
                                                          const int64_t* __restrict__ list, int64_t limit) {
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
        uint32_t* dst = reinterpret_cast<uint32_t*>(codes + row * (int64_t)d);
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
            dst[c] = word;
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

// rows of the seed sample: S rows spread evenly over [0, n) (n >= S: distinct, ascending)
__global__ void code8_seed_rows_kernel(int64_t* __restrict__ rows, int64_t S, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) rows[i] = (i * n) / S;
}
// (the padding row of the candidate list)
__global__ void code8_fill_nan_kernel(float* __restrict__ p, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = __uint_as_float(0x7FC00000u);
}

// ---- prologue: the query -> two int8 planes + the margin's terms; zeroes the candidate counter ---------------------------------
// par[0] = qstep, par[1] = alpha, par[2] = beta, par[3] = 1 when the query's norm is not finite (the call falls back)
__global__ __launch_bounds__(256) void code8_query_kernel(const float* __restrict__ q, int d, int normalize_q, float row_norm_bound,
                                                          int8_t* __restrict__ qhi, int8_t* __restrict__ qlo, float* __restrict__ par,
                                                          unsigned long long* __restrict__ counter) {
    __shared__ float shf[256];
    __shared__ double shd[256];
    const int tid = threadIdx.x;
    auto block_sum_f = [&](float v) {
        shf[tid] = v;
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if (tid < s) shf[tid] += shf[tid + s];
            __syncthreads();
        }
        const float out = shf[0];
        __syncthreads();
        return out;
    };
    float nr = 0.f;
    for (int j = tid; j < d; j += 256) nr = fmaf(q[j], q[j], nr);
    nr = block_sum_f(nr);
    const float inorm = (normalize_q && nr > 0.f) ? 1.0f / sqrtf(nr) : 1.0f;
    float mx = 0.f;
    double n2 = 0.0;
    bool bad = false;
    for (int j = tid; j < d; j += 256) {
        const float v = q[j] * inorm;
        bad = bad || !(fabsf(v) <= 3.402823466e+38f);
        mx = fmaxf(mx, fabsf(v));
        n2 += (double)v * (double)v;
    }
    shd[tid] = n2;
    shf[tid] = bad ? INFINITY : mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            shd[tid] += shd[tid + s];
            shf[tid] = fmaxf(shf[tid], shf[tid + s]);
        }
        __syncthreads();
    }
    mx = shf[0];
    const double qn_d = sqrt(shd[0]) * (1.0 + 1e-6);
    const bool nonfinite = !(mx <= 3.402823466e+38f) || !(qn_d <= 3.0e38);
    const float qn = nonfinite ? 0.f : (float)qn_d;
    const int qmax = code8_qmax(d);
    const bool tiny = nonfinite || mx < kCode8Tiny;
    const float qstep = tiny ? 0.f : mx / (float)qmax;
    for (int j = tid; j < d; j += 256) {
        int Q = 0;
        if (!tiny) {
            float cf = rintf((q[j] * inorm) / qstep);
            cf = fminf(fmaxf(cf, -(float)qmax), (float)qmax);
            Q = (int)cf;
        }
        const int lo = ((Q + 128) & 255) - 128;
        const int hi = (Q - lo) >> 8;
        qhi[j] = (int8_t)hi;
        qlo[j] = (int8_t)lo;
    }
    if (tid == 0) {
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
        *counter = 0ull;
    }
}

// ---- the prefilter scan ---------------------------------------------------------------------------------------------------------
struct Code8ScanArgs {
    const int8_t* codes;   // [n, d]
    const float2* ar;      // [n] (a, r)
    int64_t n;
    int d;                 // bytes per row (a multiple of 16)
    const int8_t* qhi;     // [d] the query's high / low planes (code8_query_kernel)
    const int8_t* qlo;
    const float* par;      // qstep, alpha, beta
    const float* floor;    // a proven lower bound of the final k-th best score (the seed sample's exact k-th best)
    uint32_t* cand;        // [cap] appended rows, in no order
    int64_t cap;
    unsigned long long* counter;  // zeroed by the prologue; keeps counting past cap
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

// One wave takes batches of RB = (64 / G) U consecutive rows, U KiB of codes (d = 16 G; 768 U bytes at d = 384).  Per batch:
// U 16-byte loads per lane at one base per batch + a lane offset that never changes + u row-group strides, ONE 8-byte load of
// (a, r) (lane (g, t) reads the entry of the row whose total code8_reduce leaves in it), 8 U v_dot4_i32_i8, the reduction
// above, and ONE epilogue + ballot for the RB rows of the batch (lanes t < U hold one row each).  Full batches run in a loop
// without a row clamp or a row test; the one partial batch at the end of the index is done by the wave whose turn it is,
// with both.
template <int G, int U, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void code8_scan_kernel(Code8ScanArgs a) {
    constexpr int RPI = kWave / G;
    constexpr int RB = RPI * U;
    static_assert(U >= 2 && U <= 8 && (U & (U - 1)) == 0 && U <= G, "code8_reduce halves U down to one value inside a row group");
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
    const float floor = *a.floor;

    // the wave's staged rows (range_scan_kernel's append path)
    uint32_t stage = 0;
    int nst = 0;
    const unsigned long long cap = (unsigned long long)a.cap;
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.counter, (unsigned long long)nst);
        base = readlane_u64(base, 0);
        if (lane < nst && base + (unsigned long long)lane < cap) a.cand[base + lane] = stage;
        nst = 0;
    };
    auto append = [&](uint64_t m, uint32_t row) {
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

    auto scores = [&](const i32x4 (&x)[U], int (&T)[U]) {
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
    };
    // every lane evaluates the predicate (its (a, r) load is issued with the batch's code loads, not behind a lane test);
    // `mine` keeps the bits of the lanes that report a row
    auto epilogue = [&](int tot, float2 sr, uint64_t mine, int64_t r) {
        const float s = ((float)tot * qstep) * sr.x;
        float m = fmaf(alpha, sr.y, beta);
        m = fmaf(fabsf(s) + m, 2.4e-7f, m);   // the rounding of s + m itself
        const float ub = s + m;
        // NaN (0 * inf: a zero query against a row of unbounded residual) passes
        const uint64_t pass = __ballot(!(ub < floor)) & mine;
        if (pass) append(pass, (uint32_t)r);
    };

    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t nfull = a.n / RB;
    const int64_t batch_bytes = (int64_t)RB * a.d;
    const int64_t group_bytes = (int64_t)RPI * a.d;
    const int lane_off = g * a.d + t * 16;

    auto load = [&](i32x4 (&x)[U], float2& sr, int64_t b) {
        const int8_t* base = a.codes + b * batch_bytes + lane_off;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i32x4* src = reinterpret_cast<const i32x4*>(base + u * group_bytes);
            if (MASKED)
                x[u] = valid ? __builtin_nontemporal_load(src) : i32x4{0, 0, 0, 0};
            else
                x[u] = __builtin_nontemporal_load(src);
        }
        sr = a.ar[b * RB + erow];
    };
    for (int64_t b = gw; b < nfull; b += nwaves_total) {
        i32x4 x[U];
        float2 sr;
        load(x, sr, b);
        int T[U];
        scores(x, T);
        epilogue(code8_reduce<G, U>(T, t), sr, elanes, b * RB + erow);
    }
    // the partial batch behind the full ones: rows past the end re-read the last row, their result is discarded
    if (nfull * RB < a.n && nfull % nwaves_total == gw) {
        const int64_t last = a.n - 1;
        i32x4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = nfull * RB + (int64_t)u * RPI + g;
            r = r < last ? r : last;
            const i32x4* src = reinterpret_cast<const i32x4*>(a.codes + r * (int64_t)a.d + t * 16);
            if (MASKED)
                x[u] = valid ? __builtin_nontemporal_load(src) : i32x4{0, 0, 0, 0};
            else
                x[u] = __builtin_nontemporal_load(src);
        }
        const int64_t r = nfull * RB + erow;
        const float2 sr = a.ar[r < last ? r : last];
        int T[U];
        scores(x, T);
        epilogue(code8_reduce<G, U>(T, t), sr, __ballot(t < U && r < a.n), r);
    }
    if (nst) flush();
}

// ---- candidates -> the ascending row list of the exact re-score -------------------------------------------------------------------
// Thread i ranks candidate i among the count candidates (rows are distinct: the rank is its place in ascending order) and
// writes it there; places from the count on get `pad`, the row of NaN in the matrix' slack that no scan ever offers.  The call falls back to the full
// exact scan (*gate = 1; the list is all padding) when the candidates overflowed the capacity, are fewer than k, or the query's
// norm is not finite.  stats (host-mapped): [0] fallbacks so far, [1] candidates of the latest call, [2] calls so far.
__global__ __launch_bounds__(256) void code8_list_kernel(const uint32_t* __restrict__ cand, const unsigned long long* __restrict__ counter,
                                                         int64_t cap, int k, const float* __restrict__ par, int64_t pad,
                                                         int64_t* __restrict__ rows, int* __restrict__ gate, unsigned int* __restrict__ ctr_dev,
                                                         volatile unsigned int* stats) {
    __shared__ uint32_t sh[256];
    const unsigned long long count = *counter;
    const bool fallback = count > (unsigned long long)cap || count < (unsigned long long)k || par[3] != 0.f;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *gate = fallback ? 1 : 0;
        // (searches of one index on several streams run this concurrently: atomic)
        const unsigned int fb = atomicAdd(&ctr_dev[0], fallback ? 1u : 0u) + (fallback ? 1u : 0u);
        const unsigned int calls = atomicAdd(&ctr_dev[1], 1u) + 1u;
        if (stats) {
            stats[0] = fb;
            stats[1] = (unsigned int)(count > 0xFFFFFFFFull ? 0xFFFFFFFFull : count);
            stats[2] = calls;
        }
    }
    const int64_t cnt = fallback ? 0 : (int64_t)count;
    if ((int64_t)blockIdx.x * 256 >= cnt) {
        if (i < cap) rows[i] = pad;
        return;
    }
    const uint32_t mine = i < cnt ? cand[i] : 0xFFFFFFFFu;
    int rank = 0;
    for (int64_t base = 0; base < cnt; base += 256) {
        const int64_t j = base + threadIdx.x;
        sh[threadIdx.x] = j < cnt ? cand[j] : 0xFFFFFFFFu;
        __syncthreads();
#pragma unroll 8
        for (int e = 0; e < 256; ++e) rank += sh[e] < mine ? 1 : 0;
        __syncthreads();
    }
    if (i < cnt)
        rows[rank] = (int64_t)mine;
    else if (i < cap)
        rows[i] = pad;
}

// positions of the row list -> row numbers (the re-score's keys carry positions)
__global__ void code8_relabel_kernel(int64_t* __restrict__ I, int k, const int64_t* __restrict__ rows, int64_t label_offset) {
    const int i = threadIdx.x;
    if (i < k) {
        const int64_t p = I[i];
        I[i] = p >= 0 ? rows[p] + label_offset : -1;
    }
}

}  // namespace mvdb
