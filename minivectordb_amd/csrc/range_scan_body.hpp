// range_scan_body.hpp — the statements of range_scan_kernel (range_scan.hpp) and join_scan_kernel (join_scan.hpp).  NOT a header
// of its own: it is included inside the two kernels' braces, which define
//   G, C, U, METRIC, SEL, MASKED   the kernel's template parameters
//   a                              RangeScanArgs (or a struct derived from it)
//   BOUND, bounds                  constexpr bool, const int64_t*: with BOUND, query i is matched against rows below bounds[i]
//                                  only.  The streamed forms end their batch loop there; the gathered form, whose list may be in
//                                  any order, gates a passing row on its physical row number.
    constexpr bool SUBSET = SEL == 1;
    constexpr int RPI = kWave / G;  // rows per wave-instruction
    constexpr int RB = RPI * U;     // rows per wave batch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int t = lane % G;  // chunk lane within the row
    const int g = lane / G;  // row slot within the instruction
    const int qi = blockIdx.y;
    if (a.gate_count && a.gate_count[qi] <= a.gate_cap) return;
    const float thr = a.thrs ? a.thrs[qi] : a.thr;
    int64_t before = 0;
    if constexpr (BOUND) before = bounds[qi];
    const int64_t n = BOUND && !SUBSET && before < a.n ? before : a.n;  // positions [0, n) are scored
    if (BOUND && n <= 0) return;

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

    // ---- the wave's staged keys ------------------------------------------------------------------
    uint64_t stage = 0;  // lane i: the i-th key staged since the last flush
    int nst = 0;         // wave-uniform: keys staged
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
    // every lane offers one key (0: none); wave-uniform control flow
    auto append = [&](uint64_t cand) {
        uint64_t m = __ballot(cand != 0ull);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint64_t key = readlane_u64(cand, src);
            if (lane == nst) stage = key;
            if (++nst == kWave) flush();
        }
    };

    const int64_t nwaves_total = (int64_t)gridDim.x * kScanWaves;
    const int64_t gw = (int64_t)blockIdx.x * kScanWaves + wave;
    const int64_t nbatches = (n + RB - 1) / RB;
    const int64_t last = n - 1;

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
    auto batch_bits = [&](int64_t b, bool (&sel)[U]) {
        const int64_t row0 = b * RB + g;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t r = row0 + (int64_t)u * RPI;
            r = r < last ? r : last;
            sel[u] = (a.mask[r >> 6] >> (r & 63)) & 1ull;
        }
    };
    auto consume_batch = [&](int64_t b, f32x4 (&x)[U][C], const bool (&sel)[U], const int64_t (&pr)[U]) {
        const int64_t row0 = b * RB + g;
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (METRIC == 0) {
                    acc = fmaf(x[u][c].x, qv[c].x, acc);
                    acc = fmaf(x[u][c].y, qv[c].y, acc);
                    acc = fmaf(x[u][c].z, qv[c].z, acc);
                    acc = fmaf(x[u][c].w, qv[c].w, acc);
                } else {
                    const f32x4 df = qv[c] - x[u][c];
                    acc = fmaf(df.x, df.x, acc);
                    acc = fmaf(df.y, df.y, acc);
                    acc = fmaf(df.z, df.z, acc);
                    acc = fmaf(df.w, df.w, acc);
                }
            }
            s[u] = acc;
        }
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], m);
        }
        if (METRIC != 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = -s[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = row0 + (int64_t)u * RPI;
            // NaN fails the comparison; the key carries the position (row number, or position in the row list)
            const bool pass = (t == 0) && (r < n) && (SEL != 2 || sel[u]) && (!(BOUND && SUBSET) || pr[u] < before) && (s[u] >= thr);
            if (__ballot(pass)) append(pass ? make_key(s[u], (uint32_t)r) : 0ull);
        }
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
            batch_rows(b, pr);
            load_batch(pr, x);
            const int64_t bn = b + nwaves_total;
            batch_bits(bn < nbatches ? bn : b, seln);  // behind the row loads: never waited for by its own batch
            consume_batch(b, x, sel, pr);
#pragma unroll
            for (int u = 0; u < U; ++u) sel[u] = seln[u];
        }
    } else if (SUBSET) {
        // the row ids of the NEXT batch are fetched behind this batch's row loads (flat_scan_kernel's SUBSET loop)
        int64_t pr[U], pn[U];
        if (gw < nbatches) batch_rows(gw, pr);
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            load_batch(pr, x);
            const int64_t bn = b + nwaves_total;
            batch_rows(bn < nbatches ? bn : b, pn);
            consume_batch(b, x, all_rows, pr);
#pragma unroll
            for (int u = 0; u < U; ++u) pr[u] = pn[u];
        }
    } else {
        for (int64_t b = gw; b < nbatches; b += nwaves_total) {
            f32x4 x[U][C];
            int64_t pr[U];
            batch_rows(b, pr);
            load_batch(pr, x);
            consume_batch(b, x, all_rows, pr);
        }
    }
    if (nst) flush();
