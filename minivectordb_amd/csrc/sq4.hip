// sq4.hip — C-ABI (include/mvdb.h "4-bit scalar-quantised index") of the 4-bit index behind SQ4VectorDatabase: nibble rows on the
// device, exact integer top-k against an int8 query.  faiss.IndexScalarQuantizer(QT_4bit)'s place in the flat family.
//
// HBM layout: rows[cap, d / 2], rows [0, n) live; d is a multiple of 32, so a row is 1 to 128 whole 16-byte chunks and nothing is
// padded.  ranges[3, d] fp32: lo, inv = 15 / (hi - lo), s = (hi - lo) / 15, derived on the host.  No fp32 rows are kept.  The host
// shape is bits.hip's: workspaces per stream, exclusive mutators on a private stream, compacting removal through a staging copy.
#include <algorithm>
#include <cmath>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "sq4_kernels.hpp"

using namespace mvdb;

namespace {

struct Sq4Workspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> qf;        // host API: the queries staged on the device
    DevBuf<int8_t> q8;       // the int8 queries, de-interleaved
    DevBuf<double> scale;    // step [nq] | bias [nq]
    DevBuf<int> valid;
    DevBuf<uint64_t> mask;   // host API: the bitmap of this call
    DevBuf<uint64_t> cand;   // partial top-k lists
    DevBuf<int64_t> out;     // host API results, packed [I | D | S]
    PinnedBuf pin, pin_out;
    std::mutex use_mu;       // one search at a time per workspace
    bool captured = false;
    std::vector<void*> retired;

    int init(hipStream_t s, bool own) {
        if (own) {
            MVDB_HIP(hipStreamCreateWithFlags(&owned.h, hipStreamNonBlocking));
            stream = owned.h;
        } else {
            stream = s;
        }
        return 0;
    }
    ~Sq4Workspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_sq4 {
    int d = 0, rb = 0, nchunk = 0, device = 0;
    bool ranged = false;       // ranges set (set_ranges or train)
    int64_t n = 0, cap = 0;
    uint8_t* rows = nullptr;
    float* ranges = nullptr;   // [3, d] on the device: lo | inv | s
    std::vector<float> lo_h, hi_h;
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add / set_rows on their way to the encoder
    DevBuf<uint8_t> stage_codes;  // set_rows_codes: nibble rows on their way to their places
    DevBuf<int64_t> stage_rows;
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, Sq4Workspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<Sq4Workspace*> pool, idle;           // host-API calls: private streams
    const float* lo() const { return ranges; }
    const float* inv() const { return ranges + d; }
    const float* s() const { return ranges + 2 * d; }
};

namespace {

// ---- the shape table -------------------------------------------------------------------------------------------------------
// Per row width (16-byte chunks): G lanes per row — the power of two >= the chunk count, at most 64 —, NCH chunks per lane (2
// above 64 chunks), U batches in flight per wave.  kSq4Blocks is the most resident blocks per CU of the VALU form (the occupancy
// query may say fewer), kSq4MfmaMinNq the batch size from which the matrix-core form serves where the width allows it.  U, the
// blocks per CU and the waves per block are first guesses; the hand-over is measured at d = 512 and 1024.
constexpr int kSq4Blocks = 8;
constexpr int kSq4MfmaMinNq = 5;
constexpr size_t kSq4LdsPerCu = 160 * 1024;

template <int G_, int NCH_, int U_>
struct Sq4Shape {
    static constexpr int G = G_, NCH = NCH_, U = U_;
};
template <typename Launch>
int with_sq4_shape(int nchunk, Launch launch) {
    if (nchunk <= 1) return launch(Sq4Shape<1, 1, 4>{});
    if (nchunk <= 2) return launch(Sq4Shape<2, 1, 4>{});
    if (nchunk <= 4) return launch(Sq4Shape<4, 1, 4>{});
    if (nchunk <= 8) return launch(Sq4Shape<8, 1, 4>{});
    if (nchunk <= 16) return launch(Sq4Shape<16, 1, 4>{});
    if (nchunk <= 32) return launch(Sq4Shape<32, 1, 4>{});
    if (nchunk <= 64) return launch(Sq4Shape<64, 1, 4>{});
    return launch(Sq4Shape<64, 2, 2>{});
}

// the grid rule of the row scans: tiles -> waves -> blocks, at most per_cu resident blocks per CU
int sq4_grid(int64_t n, int rows_per_wave, int waves, int per_cu, int device) {
    const int64_t ntiles = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t want = (ntiles + waves - 1) / waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}

int queries_per_pass(int nq) { return nq >= 3 ? 4 : nq; }  // NQ in {1, 2, 4}

template <int G, int NCH, int U>
const void* scan_kernel_for(int NQ) {
    void (*k1)(Sq4ScanArgs) = sq4_scan_kernel<G, NCH, U, 1>;
    void (*k2)(Sq4ScanArgs) = sq4_scan_kernel<G, NCH, U, 2>;
    void (*k4)(Sq4ScanArgs) = sq4_scan_kernel<G, NCH, U, 4>;
    return NQ == 1 ? (const void*)k1 : NQ == 2 ? (const void*)k2 : (const void*)k4;
}

template <int G, int NCH, int U>
int scan_blocks(int64_t n, int NQ, int device) {
    const int per_cu = std::max(1, std::min(cached_occupancy(scan_kernel_for<G, NCH, U>(NQ), kSq4Threads, 0, 4), kSq4Blocks));
    return sq4_grid(n, (kWave / G) * U, kSq4Threads / kWave, per_cu, device);
}

template <int G, int NCH, int U>
int launch_scan(const Sq4ScanArgs& a, int NQ, dim3 grid, hipStream_t s) {
    if (NQ == 1) hipLaunchKernelGGL((sq4_scan_kernel<G, NCH, U, 1>), grid, dim3(kSq4Threads), 0, s, a);
    else if (NQ == 2) hipLaunchKernelGGL((sq4_scan_kernel<G, NCH, U, 2>), grid, dim3(kSq4Threads), 0, s, a);
    else hipLaunchKernelGGL((sq4_scan_kernel<G, NCH, U, 4>), grid, dim3(kSq4Threads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// The block of the matrix-core form (bits_mfma_block's rule): QB = 2 blocks of 32 queries per row read when the call has more
// than 32 queries and 64 queries fit the LDS beside one wave's lists; then as many waves, up to 8, as the lists leave room for,
// two blocks of 4 waves where two fit the CU's 160 KiB.
struct Sq4MfmaPlan {
    int QB = 1, waves = 1, per_cu = 1;
    size_t lds = 0;
};
Sq4MfmaPlan sq4_mfma_block(int d, int k, int nq) {
    Sq4MfmaPlan p;
    p.QB = (nq > 32 && sq4_mfma_lds_bytes(d, k, 2, 1) <= kSq4LdsPerCu) ? 2 : 1;
    int nw = 8;
    while (nw > 1 && sq4_mfma_lds_bytes(d, k, p.QB, nw) > kSq4LdsPerCu) nw >>= 1;
    if (nw == 8 && sq4_mfma_lds_bytes(d, k, p.QB, 4) * 2 <= kSq4LdsPerCu) nw = 4;
    p.waves = nw;
    p.lds = sq4_mfma_lds_bytes(d, k, p.QB, nw);
    p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(8 / nw, kSq4LdsPerCu / p.lds));
    return p;
}

// form: 0 by the shape table, 1 the VALU form, 2 the matrix-core form (the benchmark times both where both can serve)
bool mfma_serves(const mvdb_sq4* ix, int nq, int form) {
    if (form) return form == 2;
    return ix->d <= kSq4MfmaMaxDim && nq >= kSq4MfmaMinNq;
}

// ---- workspaces (as bits.hip) ----------------------------------------------------------------------------------------------
Sq4Workspace* ws_for_stream(const mvdb_sq4* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    Sq4Workspace* ws = new Sq4Workspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

Sq4Workspace* ws_acquire(const mvdb_sq4* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        Sq4Workspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    Sq4Workspace* ws = new Sq4Workspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

void ws_release(const mvdb_sq4* ix, Sq4Workspace* ws) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    ix->idle.push_back(ws);
}

struct WsBack {
    const mvdb_sq4* ix;
    Sq4Workspace* ws;
    ~WsBack() { ws_release(ix, ws); }
};

// Mutators hold the index exclusively; they wait for every stream a search of this index was enqueued on and for the private
// ones, and for nothing else (bits.hip: quiesce).
int quiesce(mvdb_sq4* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    bool device_wide = false;
    for (auto it = ix->by_stream.begin(); it != ix->by_stream.end();) {
        const hipError_t e = hipStreamSynchronize(it->first);
        if (e == hipSuccess) {
            ++it;
            continue;
        }
        (void)hipGetLastError();
        if (e == hipErrorInvalidHandle || e == hipErrorInvalidResourceHandle || e == hipErrorContextIsDestroyed) {
            delete it->second;
            it = ix->by_stream.erase(it);
        } else {
            device_wide = true;
            ++it;
        }
    }
    for (Sq4Workspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "sq4 search: the workspace of this stream is too small to capture this shape; run it once "
                                  "eagerly on the stream first");
    return b.reserve(n);
}

int grow(mvdb_sq4* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "sq4: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    uint8_t* r = nullptr;
    if (hipMalloc((void**)&r, (size_t)cap * ix->rb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVDB_ERR_OOM, "sq4: cannot allocate %lld rows", (long long)cap);
    }
    if (ix->n) {
        MVDB_HIP(hipMemcpyAsync(r, ix->rows, (size_t)ix->n * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    if (ix->rows) (void)hipFree(ix->rows);
    ix->rows = r;
    ix->cap = cap;
    return 0;
}

int need_ranges(const mvdb_sq4* ix, const char* what) {
    if (!ix->ranged) return fail(MVDB_ERR_ARG, "sq4 %s: the index has no ranges (set_ranges or train first)", what);
    return 0;
}

// lo, hi -> the device's lo | inv | s, derived here in IEEE fp32; a dimension whose hi - lo is not a positive finite number
// gets inv = s = 0 (every code 0)
int install_ranges(mvdb_sq4* ix, const float* lo, const float* hi) {
    const int d = ix->d;
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]))
            return fail(MVDB_ERR_ARG, "sq4 ranges: lo[%d] or hi[%d] is not finite", i, i);
    MVDB_TRY(ix->pin.reserve((size_t)3 * d * sizeof(float)));
    float* r = (float*)ix->pin.p;
    for (int i = 0; i < d; ++i) {
        // volatile: each of the three is rounded to fp32 where it stands — the host compiler may neither carry a wider
        // intermediate into the divisions nor fold them into one another
        const volatile float span = hi[i] - lo[i];
        const bool ok = span > 0.0f && std::isfinite(span);
        const volatile float inv = 15.0f / span, s = span / 15.0f;
        r[i] = lo[i];
        r[d + i] = ok ? inv : 0.0f;
        r[2 * d + i] = ok ? s : 0.0f;
    }
    MVDB_HIP(hipMemcpyAsync(ix->ranges, r, (size_t)3 * d * sizeof(float), hipMemcpyHostToDevice, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->lo_h.assign(lo, lo + d);
    ix->hi_h.assign(hi, hi + d);
    ix->ranged = true;
    return 0;
}

// fp32 [n, d] on the device -> nibble rows at out (rows_dev == nullptr: consecutive from out; else row rows_dev[i] of out)
int encode_into(const mvdb_sq4* ix, const float* x_dev, int64_t n, const int64_t* rows_dev, uint8_t* out, hipStream_t s) {
    if (n <= 0) return 0;
    constexpr int per_block = kSq4Threads / kWave;
    hipLaunchKernelGGL(sq4_encode_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kSq4Threads), 0, s, x_dev, n,
                       ix->d, ix->lo(), ix->inv(), rows_dev, out);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// the call's int8 queries, one launch: q_dev [nq, d] -> ws->q8, ws->scale (step | bias), ws->valid
int build_queries(const mvdb_sq4* ix, Sq4Workspace* ws, const float* q_dev, int nq, bool capturing, hipStream_t s) {
    MVDB_TRY(ws_reserve(ws->q8, (size_t)nq * ix->d, capturing));
    MVDB_TRY(ws_reserve(ws->scale, (size_t)2 * nq, capturing));
    MVDB_TRY(ws_reserve(ws->valid, (size_t)nq, capturing));
    Sq4QueryArgs a{q_dev, ix->lo(), ix->s(), ix->d, ws->q8.p, ws->scale.p, ws->scale.p + nq, ws->valid.p};
    hipLaunchKernelGGL(sq4_query_kernel, dim3((unsigned)nq), dim3(kSq4Threads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

template <int QB>
int launch_mfma(const mvdb_sq4* ix, const Sq4MfmaArgs& a, const Sq4MfmaPlan& p, int nblocks, hipStream_t s) {
    MVDB_TRY(ensure_dynamic_lds((const void*)sq4_mfma_kernel<QB>, p.lds, ix->device));
    hipLaunchKernelGGL(sq4_mfma_kernel<QB>, dim3((unsigned)nblocks, (unsigned)((a.nq + 32 * QB - 1) / (32 * QB))),
                       dim3(p.waves * kWave), p.lds, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// Everything on stream s, no synchronisation.  q_dev: fp32 [nq, d]; mask_dev: nullptr or the bitmap, on the device.
int search_core(const mvdb_sq4* ix, Sq4Workspace* ws, const float* q_dev, int nq, int k, const uint64_t* mask_dev, int form,
                float* D, int64_t* I, int32_t* S, bool capturing, hipStream_t s) {
    if (ix->n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(sq4_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, S, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    MVDB_TRY(build_queries(ix, ws, q_dev, nq, capturing, s));
    int nblocks = 0;
    if (mfma_serves(ix, nq, form)) {
        const Sq4MfmaPlan p = sq4_mfma_block(ix->d, k, nq);
        nblocks = sq4_grid(ix->n, 32, p.waves, p.per_cu, ix->device);
        MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
        Sq4MfmaArgs a{ix->rows, ix->nchunk, ix->d, ix->n, mask_dev, ws->q8.p, nq, k, ws->cand.p};
        MVDB_TRY(p.QB == 2 ? launch_mfma<2>(ix, a, p, nblocks, s) : launch_mfma<1>(ix, a, p, nblocks, s));
    } else {
        const int NQ = queries_per_pass(nq);
        MVDB_TRY(with_sq4_shape(ix->nchunk, [&](auto sh) {
            using Sh = decltype(sh);
            nblocks = scan_blocks<Sh::G, Sh::NCH, Sh::U>(ix->n, NQ, ix->device);
            MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
            Sq4ScanArgs a{ix->rows, ix->nchunk, ix->n, mask_dev, ws->q8.p, nq, k, ws->cand.p};
            return launch_scan<Sh::G, Sh::NCH, Sh::U>(a, NQ, dim3((unsigned)nblocks, (unsigned)((nq + NQ - 1) / NQ)), s);
        }));
    }
    hipLaunchKernelGGL(sq4_merge_kernel, dim3(nq), dim3(kSq4Threads), 0, s, ws->cand.p, nblocks, k, ws->scale.p,
                       ws->scale.p + nq, ws->valid.p, D, I, S);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_search(const mvdb_sq4* ix, const void* q, int nq, int k, int form, const void* D, const void* I) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "sq4: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    if (form < 0 || form > 2) return fail(MVDB_ERR_ARG, "sq4: form must be 0 (by the shape table), 1 (VALU) or 2 (matrix cores)");
    if (form == 2 && ix->d > kSq4MfmaMaxDim)
        return fail(MVDB_ERR_ARG, "sq4: the matrix-core form serves d <= %d (this index: %d)", kSq4MfmaMaxDim, ix->d);
    return need_ranges(ix, "search");
}

// host queries -> ws->qf on the workspace's stream (and the bitmap -> ws->mask behind them in the same pinned buffer)
int stage_queries(const mvdb_sq4* ix, Sq4Workspace* ws, const float* q_host, int nq, const uint64_t* mask_host,
                  const uint64_t** mask_dev) {
    const size_t qbytes = (size_t)nq * ix->d * sizeof(float);
    const size_t words = mask_host ? (size_t)((ix->n + 63) / 64) : 0;
    MVDB_TRY(ws->pin.reserve(qbytes + words * sizeof(uint64_t)));
    memcpy(ws->pin.p, q_host, qbytes);
    MVDB_TRY(ws->qf.reserve((size_t)nq * ix->d));
    MVDB_HIP(hipMemcpyAsync(ws->qf.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
    if (mask_dev) *mask_dev = nullptr;
    if (words) {
        MVDB_TRY(ws->mask.reserve(words));
        memcpy((char*)ws->pin.p + qbytes, mask_host, words * sizeof(uint64_t));
        MVDB_HIP(hipMemcpyAsync(ws->mask.p, (char*)ws->pin.p + qbytes, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
        *mask_dev = ws->mask.p;
    }
    return 0;
}

// host API: stage the queries (and the bitmap), search on a private stream, one packed D2H, wait
int search_host(const mvdb_sq4* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, int form, float* D_host,
                int64_t* I_host, int32_t* S_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, form, D_host, I_host));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    Sq4Workspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "sq4: cannot create a search workspace");
    WsBack back{ix, ws};
    const uint64_t* mask_dev = nullptr;
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, mask_host, &mask_dev));
    const size_t total = (size_t)nq * k;
    MVDB_TRY(ws->out.reserve(2 * total + 1));  // I: total int64; D, S: total 4-byte values each
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    int32_t* So = (int32_t*)(Do + total);
    MVDB_TRY(search_core(ix, ws, ws->qf.p, nq, k, mask_dev, form, Do, Io, So, false, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(float) + sizeof(int32_t));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    const char* got = (const char*)ws->pin_out.p;
    memcpy(I_host, got, total * sizeof(int64_t));
    memcpy(D_host, got + total * sizeof(int64_t), total * sizeof(float));
    if (S_host) memcpy(S_host, got + total * (sizeof(int64_t) + sizeof(float)), total * sizeof(int32_t));
    return 0;
}

// ---- ingest ----------------------------------------------------------------------------------------------------------------
int check_mutation(const mvdb_sq4* ix, const void* x, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x)) return fail(MVDB_ERR_ARG, "bad rows");
    return 0;
}

// rows appended from the host in chunks of at most 64 MiB: nibble rows straight to their place, fp32 through the encoder
int add_host(mvdb_sq4* ix, const void* x_host, bool is_float, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_ranges(ix, "add"));
    if (n == 0) return 0;
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t row_bytes = is_float ? (int64_t)ix->d * 4 : ix->rb;
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    if (is_float) MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        const size_t bytes = (size_t)(m * row_bytes);
        uint8_t* dst = ix->rows + (ix->n + r0) * ix->rb;
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        memcpy(ix->pin.p, (const char*)x_host + r0 * row_bytes, bytes);
        MVDB_HIP(hipMemcpyAsync(is_float ? (void*)ix->stage.p : (void*)dst, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
        if (is_float) MVDB_TRY(encode_into(ix, ix->stage.p, m, nullptr, dst, ix->ms));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int check_rows(const mvdb_sq4* ix, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= ix->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)ix->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

// set_rows: the rows are staged on the device chunk by chunk, their row numbers with them; fp32 rows then go through the
// encoder to their places, nibble rows through the scatter
int set_rows_host(mvdb_sq4* ix, const int64_t* rows_host, const void* x_host, bool is_float, int64_t m) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    if (!x_host) return fail(MVDB_ERR_ARG, "x is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    {   // validate first, write after
        std::vector<int64_t> v;
        MVDB_TRY(check_rows(ix, rows_host, m, &v));
    }
    MVDB_TRY(quiesce(ix));
    const int64_t row_bytes = is_float ? (int64_t)ix->d * 4 : ix->rb;
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->stage_rows.reserve((size_t)chunk));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    if (is_float) MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
    else MVDB_TRY(ix->stage_codes.reserve((size_t)chunk * ix->rb));
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        const size_t bytes = (size_t)(rows * row_bytes);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        MVDB_HIP(hipMemcpyAsync(ix->stage_rows.p, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        void* staged = is_float ? (void*)ix->stage.p : (void*)ix->stage_codes.p;
        memcpy(ix->pin.p, (const char*)x_host + i0 * row_bytes, bytes);
        MVDB_HIP(hipMemcpyAsync(staged, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
        if (is_float) {
            MVDB_TRY(encode_into(ix, ix->stage.p, rows, ix->stage_rows.p, ix->rows, ix->ms));
        } else {
            const int64_t work = rows * ix->nchunk;
            hipLaunchKernelGGL(sq4_scatter_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms,
                               (const uint8_t*)staged, (const int64_t*)ix->stage_rows.p, rows, ix->nchunk, ix->rows);
            MVDB_HIP(hipGetLastError());
        }
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

}  // namespace

extern "C" {

int mvdb_sq4_create(int d, int device, mvdb_sq4** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d < 32 || d > kSq4MaxDim || d % 32)
        return fail(MVDB_ERR_ARG, "sq4: dimension %d is not a multiple of 32 in [32, %d]", d, kSq4MaxDim);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_sq4* ix = new mvdb_sq4();
    ix->d = d;
    ix->rb = d / 2;
    ix->nchunk = d / 32;
    ix->device = device;
    if (hipMalloc((void**)&ix->ranges, (size_t)3 * d * sizeof(float)) != hipSuccess ||
        hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        if (ix->ranges) (void)hipFree(ix->ranges);
        delete ix;
        return fail(MVDB_ERR_HIP, "sq4: cannot create the ranges or a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_sq4_free(mvdb_sq4* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (Sq4Workspace* ws : ix->pool) delete ws;
        if (ix->rows) (void)hipFree(ix->rows);
        if (ix->ranges) (void)hipFree(ix->ranges);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_sq4_reset(mvdb_sq4* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    return 0;
}

int mvdb_sq4_reserve(mvdb_sq4* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_sq4_ntotal(const mvdb_sq4* ix) { return ix ? ix->n : -1; }
int mvdb_sq4_dim(const mvdb_sq4* ix) { return ix ? ix->d : -1; }

int mvdb_sq4_set_ranges(mvdb_sq4* ix, const float* lo_host, const float* hi_host) {
    if (!ix || !lo_host || !hi_host) return fail(MVDB_ERR_ARG, "NULL argument");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (ix->n) return fail(MVDB_ERR_ARG, "sq4 set_ranges: the index holds %lld rows coded by the present ranges", (long long)ix->n);
    MVDB_TRY(quiesce(ix));
    return install_ranges(ix, lo_host, hi_host);
}

int mvdb_sq4_get_ranges(const mvdb_sq4* ix, float* lo_host, float* hi_host) {
    if (!ix || !lo_host || !hi_host) return fail(MVDB_ERR_ARG, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_ranges(ix, "get_ranges"));
    memcpy(lo_host, ix->lo_h.data(), (size_t)ix->d * sizeof(float));
    memcpy(hi_host, ix->hi_h.data(), (size_t)ix->d * sizeof(float));
    return 0;
}

// per-dimension min and max over the finite values of the sample, on the device: the sample is uploaded once, stage 1 leaves
// 4 partials per slab of rows, stage 2 folds them; the ranges are then derived on the host like any others
int mvdb_sq4_train(mvdb_sq4* ix, const float* x_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    if (n <= 0 || n > (1ll << 20)) return fail(MVDB_ERR_ARG, "sq4 train: n = %lld is not in [1, 1048576]", (long long)n);
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (ix->n) return fail(MVDB_ERR_ARG, "sq4 train: the index holds %lld rows coded by the present ranges", (long long)ix->n);
    MVDB_TRY(quiesce(ix));
    const int d = ix->d;
    constexpr int lanes = kSq4Threads / kSq4MinmaxCols;
    const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(64, n / 64));
    const int64_t slab_rows = (n + slabs - 1) / slabs;
    const int64_t partials = slabs * lanes;
    DevBuf<float> x, ext;
    DevBuf<uint32_t> part;
    MVDB_TRY(x.reserve((size_t)n * d));
    MVDB_TRY(part.reserve((size_t)2 * partials * d));
    MVDB_TRY(ext.reserve((size_t)2 * d));
    const int64_t row_bytes = (int64_t)d * sizeof(float);
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)std::max<int64_t>(chunk * row_bytes, 2 * row_bytes)));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t bytes = (size_t)(std::min(chunk, n - r0) * row_bytes);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the pinned buffer is reused
        memcpy(ix->pin.p, (const char*)x_host + r0 * row_bytes, bytes);
        MVDB_HIP(hipMemcpyAsync((char*)x.p + r0 * row_bytes, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
    }
    const unsigned colblocks = (unsigned)((d + kSq4MinmaxCols - 1) / kSq4MinmaxCols);
    uint32_t* plo = part.p;
    uint32_t* phi = part.p + partials * d;
    hipLaunchKernelGGL(sq4_minmax_kernel, dim3(colblocks, (unsigned)slabs), dim3(kSq4Threads), 0, ix->ms, (const void*)x.p, n, d,
                       slab_rows, 0, plo, phi, (float*)nullptr, (float*)nullptr);
    MVDB_HIP(hipGetLastError());
    hipLaunchKernelGGL(sq4_minmax_kernel, dim3(colblocks, 1), dim3(kSq4Threads), 0, ix->ms, (const void*)nullptr, partials, d,
                       (int64_t)0, 1, plo, phi, ext.p, ext.p + d);
    MVDB_HIP(hipGetLastError());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    std::vector<float> got((size_t)2 * d);
    MVDB_HIP(hipMemcpy(got.data(), ext.p, got.size() * sizeof(float), hipMemcpyDeviceToHost));
    return install_ranges(ix, got.data(), got.data() + d);
}

int mvdb_sq4_geometry(const mvdb_sq4* ix, int nq, int k, int* form, int64_t* stride_rows) {
    if (!ix || !form || !stride_rows) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0 || k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "sq4 geometry: bad nq or k");
    DeviceGuard g(ix->device);
    if (mfma_serves(ix, nq, 0)) {
        const Sq4MfmaPlan p = sq4_mfma_block(ix->d, k, nq);
        *form = 2;
        *stride_rows = (int64_t)device_cus(ix->device) * p.per_cu * p.waves * 32;
        return 0;
    }
    *form = 1;
    return with_sq4_shape(ix->nchunk, [&](auto sh) {
        using Sh = decltype(sh);
        constexpr int tile = (kWave / Sh::G) * Sh::U;
        *stride_rows = (int64_t)scan_blocks<Sh::G, Sh::NCH, Sh::U>(INT64_MAX / 2, queries_per_pass(nq), ix->device) *
                       (kSq4Threads / kWave) * tile;
        return 0;
    });
}

int mvdb_sq4_add(mvdb_sq4* ix, const float* x_host, int64_t n) { return add_host(ix, x_host, true, n); }
int mvdb_sq4_add_codes(mvdb_sq4* ix, const uint8_t* codes_host, int64_t n) { return add_host(ix, codes_host, false, n); }

int mvdb_sq4_add_device(mvdb_sq4* ix, const float* x_dev, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_dev, n));
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_ranges(ix, "add"));
    if (n == 0) return 0;
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(encode_into(ix, x_dev, n, nullptr, ix->rows + ix->n * ix->rb, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_sq4_get_codes(const mvdb_sq4* ix, int64_t row0, int64_t n, uint8_t* codes_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (!codes_host) return fail(MVDB_ERR_ARG, "codes_host is NULL");
    MVDB_HIP(hipMemcpy(codes_host, ix->rows + row0 * ix->rb, (size_t)n * ix->rb, hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_sq4_remove_rows(mvdb_sq4* ix, const int64_t* rows_host, int64_t m) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0 || (m > 0 && !rows_host)) return fail(MVDB_ERR_ARG, "bad row list");
    if (m == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::vector<int64_t> doomed;
    MVDB_TRY(check_rows(ix, rows_host, m, &doomed));
    MVDB_TRY(quiesce(ix));
    // the tail behind the first removed row, compacted through a staging copy of its survivors, then written back in place
    const int64_t r0 = doomed[0];
    std::vector<int64_t> keep;
    keep.reserve((size_t)(ix->n - r0 - m));
    for (int64_t r = r0, j = 0; r < ix->n; ++r) {
        if (j < m && doomed[j] == r) {
            ++j;
            continue;
        }
        keep.push_back(r);
    }
    const int64_t kept = (int64_t)keep.size();
    if (kept) {
        DevBuf<int64_t> keep_dev;
        DevBuf<uint8_t> tmp;
        MVDB_TRY(keep_dev.reserve((size_t)kept));
        MVDB_TRY(tmp.reserve((size_t)kept * ix->rb));
        MVDB_HIP(hipMemcpyAsync(keep_dev.p, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        const int64_t work = kept * ix->nchunk;
        hipLaunchKernelGGL(sq4_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, ix->rows, keep_dev.p,
                           kept, ix->nchunk, tmp.p);
        MVDB_HIP(hipGetLastError());
        MVDB_HIP(hipMemcpyAsync(ix->rows + r0 * ix->rb, tmp.p, (size_t)kept * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    ix->n -= m;
    return 0;
}

int mvdb_sq4_set_rows(mvdb_sq4* ix, const int64_t* rows_host, const float* x_host, int64_t m) {
    return set_rows_host(ix, rows_host, x_host, true, m);
}
int mvdb_sq4_set_rows_codes(mvdb_sq4* ix, const int64_t* rows_host, const uint8_t* codes_host, int64_t m) {
    return set_rows_host(ix, rows_host, codes_host, false, m);
}

int mvdb_sq4_query(const mvdb_sq4* ix, const float* q_host, int nq, int8_t* q8_host, double* step_host, double* bias_host) {
    if (!ix || !q_host || !q8_host || !step_host || !bias_host) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_ranges(ix, "query"));
    Sq4Workspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "sq4: cannot create a search workspace");
    WsBack back{ix, ws};
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, nullptr, nullptr));
    MVDB_TRY(build_queries(ix, ws, ws->qf.p, nq, false, ws->stream));
    std::vector<int8_t> slots((size_t)nq * ix->d);
    MVDB_HIP(hipMemcpyAsync(slots.data(), ws->q8.p, slots.size(), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(step_host, ws->scale.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(bias_host, ws->scale.p + nq, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    for (int qi = 0; qi < nq; ++qi)  // the scan's order -> natural dimension order
        for (int i = 0; i < ix->d; ++i) q8_host[(size_t)qi * ix->d + i] = slots[(size_t)qi * ix->d + sq4_query_slot(i)];
    return 0;
}

int mvdb_sq4_search(const mvdb_sq4* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, float* D_host,
                    int64_t* I_host, int32_t* S_host) {
    return search_host(ix, q_host, nq, k, mask_host, 0, D_host, I_host, S_host);
}
int mvdb_sq4_search_form(const mvdb_sq4* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, int form,
                         float* D_host, int64_t* I_host, int32_t* S_host) {
    return search_host(ix, q_host, nq, k, mask_host, form, D_host, I_host, S_host);
}

int mvdb_sq4_search_device(const mvdb_sq4* ix, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D_dev,
                           int64_t* I_dev, int32_t* S_dev, void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, 0, D_dev, I_dev));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    hipStream_t s = (hipStream_t)stream;
    Sq4Workspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "sq4: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    return search_core(ix, ws, q_dev, nq, k, mask_dev, 0, D_dev, I_dev, S_dev, capturing, s);
}

}  // extern "C"
