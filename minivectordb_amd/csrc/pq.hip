// pq.hip — C-ABI (include/mvdb.h "product-quantised index") of the product-quantised index behind PQVectorDatabase: M code
// bytes per row on the device, asymmetric distance computation (ADC) top-k.  faiss.IndexPQ's place in the flat family.
//
// HBM layout: codes[cap, M], rows [0, n) live; M is a multiple of 16, so a row is 1 to 16 whole 16-byte chunks and nothing is
// padded.  codebooks[M, 256, dsub] fp32.  No fp32 rows are kept.  The host shape is bits.hip's: workspaces per stream,
// exclusive mutators on a private stream, compacting removal through a staging copy.
#include <algorithm>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "pq_kernels.hpp"

using namespace mvdb;

namespace {

struct PqWorkspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> q;         // host API: the queries staged on the device
    DevBuf<uint64_t> mask;   // host API: the bitmap of this call
    DevBuf<float> t, lo, hi; // the table launch's fp32 entries and per-m extremes
    DevBuf<int> bad, ticket, valid;
    DevBuf<float> step, bias;
    DevBuf<uint16_t> lut;    // the interleaved tables of the call's passes
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
    ~PqWorkspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_pq {
    int d = 0, M = 0, dsub = 0, lg_dsub = 0, nchunk = 0, metric = 0, device = 0;
    bool trained = false;      // codebooks set (set_codebooks or train)
    int64_t n = 0, cap = 0;
    uint8_t* codes = nullptr;
    float* cb = nullptr;       // [M, 256, dsub]
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add on their way to the encoder
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, PqWorkspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<PqWorkspace*> pool, idle;           // host-API calls: private streams
    size_t cb_floats() const { return (size_t)M * kPqCentroids * dsub; }
};

namespace {

// ---- the scan's shape ------------------------------------------------------------------------------------------------------
// G lanes per row: the power of two >= M / 16.  NQ queries per pass: the largest of {4, 2, 1} whose table fits 128 KiB of LDS
// (4 up to M = 64, 2 up to 128, 1 up to 256), capped by the queries of the call (3 queries ride a pass of 4).  The block and
// the blocks per CU follow from the LDS the table and the merge lists take (bits_mfma_block is the precedent): a table that
// owns the CU gets 16 waves, one that leaves room for two or three blocks 8 waves each, a smaller one 4.  U and these wave
// counts are first guesses.
constexpr size_t kPqLdsPerCu = 160 * 1024;
constexpr size_t kPqTableBudget = 128 * 1024;

int pq_queries_per_pass(int M, int nq) {
    const int cap = pq_table_bytes(M, 4) <= kPqTableBudget ? 4 : pq_table_bytes(M, 2) <= kPqTableBudget ? 2 : 1;
    return std::min(cap, nq >= 3 ? 4 : nq);
}

struct PqPlan {
    int NQ = 1, waves = 4, per_cu = 1;
    size_t lds = 0;
};

template <typename Launch>
int with_pq_group(int nchunk, Launch launch) {
    if (nchunk <= 1) return launch(std::integral_constant<int, 1>{});
    if (nchunk <= 2) return launch(std::integral_constant<int, 2>{});
    if (nchunk <= 4) return launch(std::integral_constant<int, 4>{});
    if (nchunk <= 8) return launch(std::integral_constant<int, 8>{});
    return launch(std::integral_constant<int, 16>{});
}

template <int G>
const void* scan_kernel_for(int NQ) {
    void (*k1)(PqScanArgs) = pq_scan_kernel<G, kPqScanU, 1>;
    void (*k2)(PqScanArgs) = pq_scan_kernel<G, kPqScanU, 2>;
    void (*k4)(PqScanArgs) = pq_scan_kernel<G, kPqScanU, 4>;
    return NQ == 1 ? (const void*)k1 : NQ == 2 ? (const void*)k2 : (const void*)k4;
}

int pq_group(int nchunk) {
    int g = 1;
    (void)with_pq_group(nchunk, [&](auto G) {
        g = decltype(G)::value;
        return 0;
    });
    return g;
}

int make_plan(const mvdb_pq* ix, int nq, PqPlan* p) {
    p->NQ = pq_queries_per_pass(ix->M, nq);
    const size_t fit = kPqLdsPerCu / pq_scan_lds_bytes(ix->M, p->NQ, 16);
    p->waves = fit <= 1 ? 16 : fit <= 3 ? 8 : 4;
    p->lds = pq_scan_lds_bytes(ix->M, p->NQ, p->waves);
    int per_cu = (int)std::min<size_t>(std::min<size_t>(kPqLdsPerCu / p->lds, (size_t)(32 / p->waves)), 8);
    const void* kern = nullptr;
    (void)with_pq_group(ix->nchunk, [&](auto G) {
        kern = scan_kernel_for<decltype(G)::value>(p->NQ);
        return 0;
    });
    MVDB_TRY(ensure_dynamic_lds(kern, p->lds, ix->device));
    per_cu = std::min(per_cu, cached_occupancy(kern, p->waves * kWave, p->lds, per_cu));
    p->per_cu = std::max(1, per_cu);
    return 0;
}

// the grid rule of the row scans: tiles -> waves -> blocks, at most per_cu resident blocks per CU
int pq_grid(const mvdb_pq* ix, const PqPlan& p, int64_t n) {
    const int tile = (kWave / pq_group(ix->nchunk)) * kPqScanU;
    const int64_t ntiles = (n + tile - 1) / tile;
    const int64_t want = (ntiles + p.waves - 1) / p.waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(ix->device) * p.per_cu));
}

// ---- workspaces (as bits.hip) ----------------------------------------------------------------------------------------------
PqWorkspace* ws_for_stream(const mvdb_pq* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    PqWorkspace* ws = new PqWorkspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

PqWorkspace* ws_acquire(const mvdb_pq* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        PqWorkspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    PqWorkspace* ws = new PqWorkspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

void ws_release(const mvdb_pq* ix, PqWorkspace* ws) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    ix->idle.push_back(ws);
}

struct WsBack {
    const mvdb_pq* ix;
    PqWorkspace* ws;
    ~WsBack() { ws_release(ix, ws); }
};

// Mutators hold the index exclusively; they wait for every stream a search of this index was enqueued on and for the private
// ones, and for nothing else (bits.hip: quiesce).
int quiesce(mvdb_pq* ix) {
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
    for (PqWorkspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "pq search: the workspace of this stream is too small to capture this shape; run it once "
                                  "eagerly on the stream first");
    return b.reserve(n);
}

int grow(mvdb_pq* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "pq: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    uint8_t* r = nullptr;
    if (hipMalloc((void**)&r, (size_t)cap * ix->M) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVDB_ERR_OOM, "pq: cannot allocate %lld rows", (long long)cap);
    }
    if (ix->n) {
        MVDB_HIP(hipMemcpyAsync(r, ix->codes, (size_t)ix->n * ix->M, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    if (ix->codes) (void)hipFree(ix->codes);
    ix->codes = r;
    ix->cap = cap;
    return 0;
}

int need_codebooks(const mvdb_pq* ix, const char* what) {
    if (!ix->trained) return fail(MVDB_ERR_ARG, "pq %s: the index has no codebooks (set_codebooks or train first)", what);
    return 0;
}

// fp32 rows [n, d] on the device -> codes [n, M] at out
int encode_into(const mvdb_pq* ix, const float* x_dev, int64_t n, uint8_t* out, hipStream_t s) {
    if (n <= 0) return 0;
    const dim3 grid((unsigned)((n + kPqThreads - 1) / kPqThreads)), block(kPqThreads);
    switch (ix->dsub) {
        case 1: hipLaunchKernelGGL(pq_encode_kernel<1>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
        case 2: hipLaunchKernelGGL(pq_encode_kernel<2>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
        case 4: hipLaunchKernelGGL(pq_encode_kernel<4>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
        case 8: hipLaunchKernelGGL(pq_encode_kernel<8>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
        case 16: hipLaunchKernelGGL(pq_encode_kernel<16>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
        default: hipLaunchKernelGGL(pq_encode_kernel<32>, grid, block, 0, s, x_dev, n, ix->M, ix->cb, out); break;
    }
    MVDB_HIP(hipGetLastError());
    return 0;
}

template <int DSUB>
int launch_update(const mvdb_pq* ix, const float* x_dev, const uint8_t* codes, int64_t n, hipStream_t s) {
    const size_t lds = (size_t)kPqThreads * DSUB * sizeof(double) + kPqThreads * sizeof(int);
    MVDB_TRY(ensure_dynamic_lds((const void*)pq_update_kernel<DSUB>, lds, ix->device));
    hipLaunchKernelGGL(pq_update_kernel<DSUB>, dim3((unsigned)(ix->M * kPqCentroids)), dim3(kPqThreads), lds, s, x_dev, codes, n,
                       ix->M, ix->cb);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int update_from(const mvdb_pq* ix, const float* x_dev, const uint8_t* codes, int64_t n, hipStream_t s) {
    switch (ix->dsub) {
        case 1: return launch_update<1>(ix, x_dev, codes, n, s);
        case 2: return launch_update<2>(ix, x_dev, codes, n, s);
        case 4: return launch_update<4>(ix, x_dev, codes, n, s);
        case 8: return launch_update<8>(ix, x_dev, codes, n, s);
        case 16: return launch_update<16>(ix, x_dev, codes, n, s);
        default: return launch_update<32>(ix, x_dev, codes, n, s);
    }
}

// host rows -> dst on the device through the index's pinned buffer, in chunks of at most 64 MiB, on the mutators' stream
int upload_rows(mvdb_pq* ix, const void* host, int64_t n, int64_t row_bytes, void* dst) {
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const size_t bytes = (size_t)(std::min(chunk, n - r0) * row_bytes);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the pinned buffer is reused
        memcpy(ix->pin.p, (const char*)host + r0 * row_bytes, bytes);
        MVDB_HIP(hipMemcpyAsync((char*)dst + r0 * row_bytes, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// The call's tables, one launch: q_dev [nq, d] -> ws->lut interleaved by the NQ queries of a pass, ws->step / bias / valid.
int build_tables(const mvdb_pq* ix, PqWorkspace* ws, const float* q_dev, int nq, int NQ, bool capturing, hipStream_t s) {
    const int npass = (nq + NQ - 1) / NQ;
    const int nslab = ix->M / pq_lut_slab(ix->dsub);
    const size_t entries = (size_t)ix->M * kPqCentroids;
    MVDB_TRY(ws_reserve(ws->t, (size_t)nq * entries, capturing));
    MVDB_TRY(ws_reserve(ws->lo, (size_t)nq * ix->M, capturing));
    MVDB_TRY(ws_reserve(ws->hi, (size_t)nq * ix->M, capturing));
    MVDB_TRY(ws_reserve(ws->bad, (size_t)nq * nslab, capturing));
    MVDB_TRY(ws_reserve(ws->valid, (size_t)nq, capturing));
    MVDB_TRY(ws_reserve(ws->step, (size_t)nq, capturing));
    MVDB_TRY(ws_reserve(ws->bias, (size_t)nq, capturing));
    MVDB_TRY(ws_reserve(ws->lut, (size_t)npass * NQ * entries, capturing));
    if ((size_t)nq > ws->ticket.cap) {
        // a fresh ticket array starts at zero (cleared by a kernel, never a memset node); every launch leaves it at zero
        MVDB_TRY(ws_reserve(ws->ticket, (size_t)nq, capturing));
        const int cap = (int)ws->ticket.cap;
        hipLaunchKernelGGL(pq_zero_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, ws->ticket.p, cap);
        MVDB_HIP(hipGetLastError());
    }
    PqLutArgs a{q_dev, ix->cb, ix->d, ix->M, ix->dsub, ix->lg_dsub, ix->metric, nq, NQ, nslab, ws->t.p, ws->lo.p, ws->hi.p,
                ws->bad.p, ws->ticket.p, ws->lut.p, ws->step.p, ws->bias.p, ws->valid.p};
    hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)nslab, (unsigned)nq), dim3(kPqThreads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

template <int G>
int launch_scan(const PqScanArgs& a, const PqPlan& p, dim3 grid, hipStream_t s) {
    const dim3 block(p.waves * kWave);
    if (p.NQ == 1) hipLaunchKernelGGL((pq_scan_kernel<G, kPqScanU, 1>), grid, block, p.lds, s, a);
    else if (p.NQ == 2) hipLaunchKernelGGL((pq_scan_kernel<G, kPqScanU, 2>), grid, block, p.lds, s, a);
    else hipLaunchKernelGGL((pq_scan_kernel<G, kPqScanU, 4>), grid, block, p.lds, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// Everything on stream s, no synchronisation.  q_dev: fp32 [nq, d]; mask_dev: nullptr or the bitmap, on the device.
int search_core(const mvdb_pq* ix, PqWorkspace* ws, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D,
                int64_t* I, int32_t* S, bool capturing, hipStream_t s) {
    if (ix->n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(pq_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, S, total,
                           ix->metric);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    PqPlan p;
    MVDB_TRY(make_plan(ix, nq, &p));
    MVDB_TRY(build_tables(ix, ws, q_dev, nq, p.NQ, capturing, s));
    const int nblocks = pq_grid(ix, p, ix->n);
    MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
    PqScanArgs a{ix->codes, ix->nchunk, ix->M, ix->n, mask_dev, ws->lut.p, nq, k, ws->cand.p};
    const dim3 grid((unsigned)nblocks, (unsigned)((nq + p.NQ - 1) / p.NQ));
    MVDB_TRY(with_pq_group(ix->nchunk, [&](auto G) { return launch_scan<decltype(G)::value>(a, p, grid, s); }));
    hipLaunchKernelGGL(pq_merge_kernel, dim3(nq), dim3(kPqThreads), 0, s, ws->cand.p, nblocks, k, ix->metric, ws->step.p,
                       ws->bias.p, ws->valid.p, D, I, S);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_search(const mvdb_pq* ix, const void* q, int nq, int k, const void* D, const void* I) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "pq: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    return need_codebooks(ix, "search");
}

int check_rows(const mvdb_pq* ix, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= ix->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)ix->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

int check_mutation(mvdb_pq* ix, const void* x, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x)) return fail(MVDB_ERR_ARG, "bad rows");
    return 0;
}

}  // namespace

extern "C" {

int mvdb_pq_create(int d, int M, int metric, int device, mvdb_pq** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (metric != MVDB_METRIC_IP && metric != MVDB_METRIC_L2) return fail(MVDB_ERR_ARG, "pq: unknown metric %d", metric);
    if (M < 16 || M > kPqMaxM || M % 16) return fail(MVDB_ERR_ARG, "pq: M = %d is not a multiple of 16 in [16, %d]", M, kPqMaxM);
    if (d <= 0 || d > 4096 || d % M) return fail(MVDB_ERR_ARG, "pq: d = %d is not a multiple of M = %d in [M, 4096]", d, M);
    const int dsub = d / M;
    if (dsub > 32 || (dsub & (dsub - 1)))
        return fail(MVDB_ERR_ARG, "pq: d / M = %d is not one of 1, 2, 4, 8, 16, 32", dsub);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_pq* ix = new mvdb_pq();
    ix->d = d;
    ix->M = M;
    ix->dsub = dsub;
    while ((1 << ix->lg_dsub) < dsub) ++ix->lg_dsub;
    ix->nchunk = M / 16;
    ix->metric = metric;
    ix->device = device;
    if (hipMalloc((void**)&ix->cb, ix->cb_floats() * sizeof(float)) != hipSuccess ||
        hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        if (ix->cb) (void)hipFree(ix->cb);
        delete ix;
        return fail(MVDB_ERR_HIP, "pq: cannot create the codebooks or a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_pq_free(mvdb_pq* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (PqWorkspace* ws : ix->pool) delete ws;
        if (ix->codes) (void)hipFree(ix->codes);
        if (ix->cb) (void)hipFree(ix->cb);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_pq_reset(mvdb_pq* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    return 0;
}

int mvdb_pq_reserve(mvdb_pq* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_pq_ntotal(const mvdb_pq* ix) { return ix ? ix->n : -1; }
int mvdb_pq_dim(const mvdb_pq* ix) { return ix ? ix->d : -1; }
int mvdb_pq_m(const mvdb_pq* ix) { return ix ? ix->M : -1; }

int mvdb_pq_set_codebooks(mvdb_pq* ix, const float* cb_host) {
    if (!ix || !cb_host) return fail(MVDB_ERR_ARG, "NULL argument");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (ix->n) return fail(MVDB_ERR_ARG, "pq set_codebooks: the index holds %lld rows coded by the present codebooks", (long long)ix->n);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(upload_rows(ix, cb_host, ix->M, (int64_t)kPqCentroids * ix->dsub * sizeof(float), ix->cb));
    ix->trained = true;
    return 0;
}

int mvdb_pq_get_codebooks(const mvdb_pq* ix, float* cb_host) {
    if (!ix || !cb_host) return fail(MVDB_ERR_ARG, "NULL argument");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "get_codebooks"));
    MVDB_HIP(hipMemcpy(cb_host, ix->cb, ix->cb_floats() * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// Lloyd's algorithm per sub-space under L2 from the codebooks now set: the sample is uploaded once, its codes live beside it,
// and an iteration is the encoder followed by the update.
int mvdb_pq_train(mvdb_pq* ix, const float* x_host, int64_t n, int iters) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    if (n <= 0 || n > (1ll << 20)) return fail(MVDB_ERR_ARG, "pq train: n = %lld is not in [1, 1048576]", (long long)n);
    if (iters < 0) return fail(MVDB_ERR_ARG, "pq train: negative iteration count");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "train"));
    if (ix->n) return fail(MVDB_ERR_ARG, "pq train: the index holds %lld rows coded by the present codebooks", (long long)ix->n);
    MVDB_TRY(quiesce(ix));
    DevBuf<float> x;
    DevBuf<uint8_t> codes;
    MVDB_TRY(x.reserve((size_t)n * ix->d));
    MVDB_TRY(codes.reserve((size_t)n * ix->M));
    MVDB_TRY(upload_rows(ix, x_host, n, (int64_t)ix->d * sizeof(float), x.p));
    for (int it = 0; it < iters; ++it) {
        MVDB_TRY(encode_into(ix, x.p, n, codes.p, ix->ms));
        MVDB_TRY(update_from(ix, x.p, codes.p, n, ix->ms));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

int mvdb_pq_add(mvdb_pq* ix, const float* x_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "add"));
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t row_bytes = (int64_t)ix->d * sizeof(float);
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        MVDB_TRY(upload_rows(ix, (const char*)x_host + r0 * row_bytes, m, row_bytes, ix->stage.p));
        MVDB_TRY(encode_into(ix, ix->stage.p, m, ix->codes + (ix->n + r0) * ix->M, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffer is reused
    }
    ix->n += n;
    return 0;
}

int mvdb_pq_add_device(mvdb_pq* ix, const float* x_dev, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_dev, n));
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "add"));
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(encode_into(ix, x_dev, n, ix->codes + ix->n * ix->M, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_pq_add_codes(mvdb_pq* ix, const uint8_t* codes_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, codes_host, n));
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "add_codes"));
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(upload_rows(ix, codes_host, n, ix->M, ix->codes + ix->n * ix->M));
    ix->n += n;
    return 0;
}

int mvdb_pq_get_codes(const mvdb_pq* ix, int64_t row0, int64_t n, uint8_t* codes_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (!codes_host) return fail(MVDB_ERR_ARG, "codes_host is NULL");
    MVDB_HIP(hipMemcpy(codes_host, ix->codes + row0 * ix->M, (size_t)n * ix->M, hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_pq_remove_rows(mvdb_pq* ix, const int64_t* rows_host, int64_t m) {
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
        MVDB_TRY(tmp.reserve((size_t)kept * ix->M));
        MVDB_HIP(hipMemcpyAsync(keep_dev.p, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        const int64_t work = kept * ix->nchunk;
        hipLaunchKernelGGL(pq_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, ix->codes, keep_dev.p,
                           kept, ix->nchunk, tmp.p);
        MVDB_HIP(hipGetLastError());
        MVDB_HIP(hipMemcpyAsync(ix->codes + r0 * ix->M, tmp.p, (size_t)kept * ix->M, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    ix->n -= m;
    return 0;
}

int mvdb_pq_geometry(const mvdb_pq* ix, int nq, int k, int* queries_per_pass, int64_t* stride_rows) {
    if (!ix || !queries_per_pass || !stride_rows) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0 || k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "pq geometry: bad nq or k");
    DeviceGuard g(ix->device);
    PqPlan p;
    MVDB_TRY(make_plan(ix, nq, &p));
    *queries_per_pass = p.NQ;
    const int tile = (kWave / pq_group(ix->nchunk)) * kPqScanU;
    *stride_rows = (int64_t)pq_grid(ix, p, INT64_MAX / 2) * p.waves * tile;
    return 0;
}

int mvdb_pq_lut(const mvdb_pq* ix, const float* q_host, int nq, uint16_t* lut_host, float* step_host, float* bias_host) {
    if (!ix || !q_host || !lut_host || !step_host || !bias_host) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(need_codebooks(ix, "lut"));
    PqWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "pq: cannot create a search workspace");
    WsBack back{ix, ws};
    const int NQ = pq_queries_per_pass(ix->M, nq), npass = (nq + NQ - 1) / NQ;
    const size_t qbytes = (size_t)nq * ix->d * sizeof(float), entries = (size_t)ix->M * kPqCentroids;
    MVDB_TRY(ws->pin.reserve(qbytes));
    memcpy(ws->pin.p, q_host, qbytes);
    MVDB_TRY(ws->q.reserve((size_t)nq * ix->d));
    MVDB_HIP(hipMemcpyAsync(ws->q.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
    MVDB_TRY(build_tables(ix, ws, ws->q.p, nq, NQ, false, ws->stream));
    std::vector<uint16_t> inter((size_t)npass * NQ * entries);
    MVDB_HIP(hipMemcpyAsync(inter.data(), ws->lut.p, inter.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(step_host, ws->step.p, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(bias_host, ws->bias.p, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    for (int qi = 0; qi < nq; ++qi) {  // lut[pass][m][c][NQ] -> [nq][m][c]
        const uint16_t* src = inter.data() + (size_t)(qi / NQ) * NQ * entries + qi % NQ;
        for (size_t e = 0; e < entries; ++e) lut_host[(size_t)qi * entries + e] = src[e * NQ];
    }
    return 0;
}

// host API: stage the queries (and the bitmap), search on a private stream, one packed D2H, wait
int mvdb_pq_search(const mvdb_pq* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, float* D_host,
                   int64_t* I_host, int32_t* S_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, D_host, I_host));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    PqWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "pq: cannot create a search workspace");
    WsBack back{ix, ws};
    const size_t qbytes = (size_t)nq * ix->d * sizeof(float);
    const size_t words = mask_host ? (size_t)((ix->n + 63) / 64) : 0, total = (size_t)nq * k;
    MVDB_TRY(ws->pin.reserve(qbytes + words * sizeof(uint64_t)));
    memcpy(ws->pin.p, q_host, qbytes);
    MVDB_TRY(ws->q.reserve((size_t)nq * ix->d));
    MVDB_HIP(hipMemcpyAsync(ws->q.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
    const uint64_t* mask_dev = nullptr;
    if (words) {
        MVDB_TRY(ws->mask.reserve(words));
        memcpy((char*)ws->pin.p + qbytes, mask_host, words * sizeof(uint64_t));
        MVDB_HIP(hipMemcpyAsync(ws->mask.p, (char*)ws->pin.p + qbytes, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
        mask_dev = ws->mask.p;
    }
    MVDB_TRY(ws->out.reserve(2 * total + 1));  // I: total int64; D, S: total 4-byte values each
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    int32_t* So = (int32_t*)(Do + total);
    MVDB_TRY(search_core(ix, ws, ws->q.p, nq, k, mask_dev, Do, Io, So, false, ws->stream));
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

int mvdb_pq_search_device(const mvdb_pq* ix, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D_dev,
                          int64_t* I_dev, int32_t* S_dev, void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, D_dev, I_dev));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    hipStream_t s = (hipStream_t)stream;
    PqWorkspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "pq: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    return search_core(ix, ws, q_dev, nq, k, mask_dev, D_dev, I_dev, S_dev, capturing, s);
}

}  // extern "C"
