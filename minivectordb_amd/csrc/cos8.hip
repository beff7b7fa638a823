// cos8.hip — C-ABI (include/mvdb.h "int8 cosine index") of the exact int8 cosine index behind
// ShardedVectorDatabaseUsearch: device store of int8 codes + a2, quantising ingest, exact scans, resident row sets.
//
// HBM layout: codes[cap, stride] (stride = d rounded up to 16 bytes, zero padded) and a2[cap]; rows [0, n) live.
// The fp32 rows stay on the host (the Python layer keeps them for get_vector and the shard files).
//
// Build note: no fast-math.  The distance's fp64 division and square root must be the IEEE operations.
#include <algorithm>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "cos8_kernels.hpp"

using namespace mvdb;

namespace mvdb {
size_t select_state_bytes();                                              // mvdb.hip
int select_scores_topk(const float* scores, int64_t n, int k, int64_t label_offset, float* D, int64_t* I, void* state,
                       uint64_t* keys, int device, hipStream_t s);        // mvdb.hip
}  // namespace mvdb

namespace {

constexpr int kCos8MaxK = 1 << 20;

int64_t pow2_at_least(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

struct Cos8Workspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> q;         // host queries staged on the device
    DevBuf<int8_t> qcodes;   // [nq, stride]
    DevBuf<int32_t> qb2;     // [nq]
    DevBuf<uint64_t> cand;   // partial top-k lists
    DevBuf<float> scores;    // large k: every -distance
    DevBuf<uint64_t> selkeys;
    DevBuf<int64_t> out;     // host API results, packed [I | D]
    void* st = nullptr;      // SelectState
    PinnedBuf pin, pin_out;
    std::mutex use_mu;       // one search at a time per workspace
    bool captured = false;
    std::vector<void*> retired;

    int init(int device, hipStream_t s, bool own) {
        (void)device;
        if (own) {
            MVDB_HIP(hipStreamCreateWithFlags(&owned.h, hipStreamNonBlocking));
            stream = owned.h;
        } else {
            stream = s;
        }
        MVDB_HIP(hipMalloc(&st, select_state_bytes()));
        return 0;
    }
    ~Cos8Workspace() {   // (also of a workspace whose init() failed half-way)
        if (st) (void)hipFree(st);
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_cos8 {
    int d = 0, stride = 0, nchunk = 0, device = 0;
    int64_t n = 0, cap = 0;
    int8_t* codes = nullptr;
    int32_t* a2 = nullptr;
    uint64_t gen = 0;  // bumped when rows are renumbered (remove_rows / reset)
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;
    DevBuf<int64_t> stage_rows;  // set_rows: the row numbers of the staged chunk
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, Cos8Workspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<Cos8Workspace*> pool, idle;           // host-API calls: private streams
};

struct mvdb_cos8_rowset {
    const mvdb_cos8* ix = nullptr;
    int device = 0;
    uint64_t gen = 0;
    int64_t n_base = 0;    // rows of the index when the set was built (a bitmap covers these)
    int64_t size = 0;      // rows selected
    bool bitmap = false;
    int64_t* rows = nullptr;   // sorted row list
    int64_t m = 0;
    uint64_t* mask = nullptr;  // bit set = row excluded
};

namespace {

// ---- workspaces ---------------------------------------------------------------------------------------
Cos8Workspace* ws_for_stream(const mvdb_cos8* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    Cos8Workspace* ws = new Cos8Workspace();
    if (ws->init(ix->device, s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

Cos8Workspace* ws_acquire(const mvdb_cos8* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        Cos8Workspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    Cos8Workspace* ws = new Cos8Workspace();
    if (ws->init(ix->device, nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

void ws_release(const mvdb_cos8* ix, Cos8Workspace* ws) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    ix->idle.push_back(ws);
}

// Mutators run with the index held exclusively: no host call is inside a search, but device-API searches may still be
// queued on their streams.  Wait for every stream a search of this index was enqueued on, and for the private ones — and
// for nothing else (no device-wide wait: other work on the device keeps running).  As mvdb.hip's quiesce: a stream the
// caller has destroyed since (hipStreamDestroy completes its work first) is forgotten with its workspace; any other failure
// (e.g. the stream is being captured) falls back to a device-wide wait, so that no stream can wedge the mutators.
int quiesce(mvdb_cos8* ix) {
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
    for (Cos8Workspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

// A buffer that must grow while its stream is being captured cannot be allocated (allocation is not capturable).
template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "cos8 search: the workspace of this stream is too small to capture this shape; run it "
                                  "once eagerly on the stream first");
    return b.reserve(n);
}

int grow(mvdb_cos8* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "cos8: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    int8_t* c = nullptr;
    int32_t* a = nullptr;
    MVDB_HIP(hipMalloc((void**)&c, (size_t)cap * ix->stride));
    if (hipMalloc((void**)&a, (size_t)cap * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(c);
        return fail(MVDB_ERR_OOM, "cos8: cannot allocate %lld rows", (long long)cap);
    }
    if (ix->n) {
        MVDB_HIP(hipMemcpyAsync(c, ix->codes, (size_t)ix->n * ix->stride, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipMemcpyAsync(a, ix->a2, (size_t)ix->n * sizeof(int32_t), hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    if (ix->codes) (void)hipFree(ix->codes);
    if (ix->a2) (void)hipFree(ix->a2);
    ix->codes = c;
    ix->a2 = a;
    ix->cap = cap;
    return 0;
}

int quantize_into(const mvdb_cos8* ix, const float* x_dev, int64_t n, int8_t* codes, int32_t* a2, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(cos8_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x_dev, n, ix->d,
                       ix->stride, codes, a2);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// ---- scan dispatch ------------------------------------------------------------------------------------------
template <int G, int NCH, int Q>
int launch_q(const Cos8ScanArgs& a, int F, bool scores, dim3 grid, hipStream_t s) {
#define MVDB_COS8_CASE(FF, SC)                                                                     \
    if (F == FF && scores == SC) {                                                                 \
        hipLaunchKernelGGL((cos8_scan_kernel<G, NCH, Q, FF, SC>), grid, dim3(kCos8Threads), 0, s, a); \
        MVDB_HIP(hipGetLastError());                                                               \
        return 0;                                                                                  \
    }
    MVDB_COS8_CASE(0, false)
    MVDB_COS8_CASE(1, false)
    MVDB_COS8_CASE(2, false)
    MVDB_COS8_CASE(0, true)
    MVDB_COS8_CASE(1, true)
    MVDB_COS8_CASE(2, true)
#undef MVDB_COS8_CASE
    return fail(MVDB_ERR_ARG, "cos8: bad filter form %d", F);
}

template <int G, int NCH>
int launch_g(const Cos8ScanArgs& a, int Q, int F, bool scores, dim3 grid, hipStream_t s) {
    if (Q == 1) return launch_q<G, NCH, 1>(a, F, scores, grid, s);
    if (NCH == 1) return launch_q<G, NCH, 8>(a, F, scores, grid, s);
    return launch_q<G, NCH, 4>(a, F, scores, grid, s);
}

int launch_scan(const Cos8ScanArgs& a, int Q, int F, bool scores, dim3 grid, hipStream_t s) {
    if (a.nchunk > 64) return launch_g<64, 4>(a, Q, F, scores, grid, s);
    if (a.nchunk > 32) return launch_g<64, 1>(a, Q, F, scores, grid, s);
    if (a.nchunk > 16) return launch_g<32, 1>(a, Q, F, scores, grid, s);
    if (a.nchunk > 8) return launch_g<16, 1>(a, Q, F, scores, grid, s);
    if (a.nchunk > 4) return launch_g<8, 1>(a, Q, F, scores, grid, s);
    if (a.nchunk > 2) return launch_g<4, 1>(a, Q, F, scores, grid, s);
    if (a.nchunk > 1) return launch_g<2, 1>(a, Q, F, scores, grid, s);
    return launch_g<1, 1>(a, Q, F, scores, grid, s);
}

// The matrix-core batch pass: 8+ queries per call, every row or an exclusion bitmap (a row list keeps few rows: the
// gathered sdot4 scan serves it), d <= 1024 (its queries sit in LDS).
constexpr int kCos8MfmaMinNq = 8;
bool mfma_pass_ok(const mvdb_cos8* ix, int nq, int F) { return nq >= kCos8MfmaMinNq && ix->nchunk <= 64 && F != 1; }

int queries_per_pass(const mvdb_cos8* ix, int nq) { return nq == 1 ? 1 : (ix->nchunk > 64 ? 4 : 8); }

// Everything on stream s, no synchronisation.  q_dev: dense fp32 [nq, d].
int search_core(const mvdb_cos8* ix, Cos8Workspace* ws, const float* q_dev, int nq, int k, const mvdb_cos8_rowset* rs,
                int64_t label_offset, float* D, int64_t* I, hipStream_t s) {
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);

    MVDB_TRY(ws_reserve(ws->qcodes, (size_t)nq * ix->stride, capturing));
    MVDB_TRY(ws_reserve(ws->qb2, (size_t)nq, capturing));
    MVDB_TRY(quantize_into(ix, q_dev, nq, ws->qcodes.p, ws->qb2.p, s));

    Cos8ScanArgs a{};
    a.codes = ix->codes;
    a.a2 = ix->a2;
    a.stride = ix->stride;
    a.nchunk = ix->nchunk;
    a.qcodes = ws->qcodes.p;
    a.qb2 = ws->qb2.p;
    a.nq = nq;
    a.k = k;
    int F = 0;
    a.n = ix->n;
    if (rs) {
        if (rs->bitmap) {
            F = 2;
            a.n = rs->n_base;
            a.mask = rs->mask;
        } else {
            F = 1;
            a.n = rs->m;
            a.rows = rs->rows;
        }
    }
    if (a.n == 0 || (rs && rs->size == 0)) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(cos8_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    const int Q = queries_per_pass(ix, nq);
    const int cus = device_cus(ix->device);
    const int64_t nblocks = std::max<int64_t>(1, std::min<int64_t>((a.n + 2047) / 2048, (int64_t)cus * 4));
    a.per_block = (a.n + nblocks - 1) / nblocks;
    const dim3 grid((unsigned)nblocks, (unsigned)((nq + Q - 1) / Q));

    if (k <= kMaxFusedK && mfma_pass_ok(ix, nq, F)) {
        // 32 queries per corpus pass on the matrix cores
        const int64_t tiles = (a.n + 31) / 32;
        const int64_t mb = std::max<int64_t>(1, std::min<int64_t>((tiles + 31) / 32, (int64_t)cus * 2));
        a.per_block = ((tiles + mb - 1) / mb) * 32;
        const dim3 mgrid((unsigned)mb, (unsigned)((nq + kCos8MfmaQ - 1) / kCos8MfmaQ));
        MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * mb * k, capturing));
        a.cand = ws->cand.p;
        const size_t lds = (size_t)kCos8MfmaQ * cos8_mfma_lds_stride(ix->stride) +
                           (size_t)(kCos8Threads / kWave) * kCos8MfmaQ * k * sizeof(uint64_t);
        if (F == 2) {
            MVDB_TRY(ensure_dynamic_lds((const void*)cos8_mfma_kernel<2>, lds, ix->device));
            hipLaunchKernelGGL(cos8_mfma_kernel<2>, mgrid, dim3(kCos8Threads), lds, s, a);
        } else {
            MVDB_TRY(ensure_dynamic_lds((const void*)cos8_mfma_kernel<0>, lds, ix->device));
            hipLaunchKernelGGL(cos8_mfma_kernel<0>, mgrid, dim3(kCos8Threads), lds, s, a);
        }
        MVDB_HIP(hipGetLastError());
        hipLaunchKernelGGL(cos8_merge_kernel, dim3(nq), dim3(kCos8Threads), 0, s, ws->cand.p, (int)mb, k, label_offset,
                           D, I);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    if (k <= kMaxFusedK) {
        MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
        a.cand = ws->cand.p;
        MVDB_TRY(launch_scan(a, Q, F, false, grid, s));
        hipLaunchKernelGGL(cos8_merge_kernel, dim3(nq), dim3(kCos8Threads), 0, s, ws->cand.p, (int)nblocks, k,
                           label_offset, D, I);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    // large k: every distance, then the radix select per query
    MVDB_TRY(ws_reserve(ws->scores, (size_t)nq * a.n, capturing));
    MVDB_TRY(ws_reserve(ws->selkeys, (size_t)pow2_at_least(std::max(k, 2)), capturing));
    a.scores = ws->scores.p;
    MVDB_TRY(launch_scan(a, Q, F, true, grid, s));
    for (int qi = 0; qi < nq; ++qi)
        MVDB_TRY(select_scores_topk(ws->scores.p + (int64_t)qi * a.n, a.n, k, label_offset, D + (int64_t)qi * k,
                                    I + (int64_t)qi * k, ws->st, ws->selkeys.p, ix->device, s));
    if (F == 1) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(cos8_map_positions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, I, total,
                           rs->rows, label_offset);
        MVDB_HIP(hipGetLastError());
    }
    return 0;
}

int check_search(const mvdb_cos8* ix, const void* q, int nq, int k, const void* D, const void* I,
                 const mvdb_cos8_rowset* rs) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kCos8MaxK) return fail(MVDB_ERR_ARG, "k must be in [1, %d] (got %d)", kCos8MaxK, k);
    if (rs) {
        if (rs->ix != ix) return fail(MVDB_ERR_ARG, "row set belongs to another index");
        if (rs->gen != ix->gen) return fail(MVDB_ERR_ARG, "row set is stale: rows were removed since it was built");
    }
    return 0;
}

// host API: stage queries, search on a private stream, one packed D2H, wait
int search_host(const mvdb_cos8* ix, const float* q_host, int nq, int k, const mvdb_cos8_rowset* rs, float* D_host,
                int64_t* I_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, D_host, I_host, rs));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (rs && rs->gen != ix->gen) return fail(MVDB_ERR_ARG, "row set is stale: rows were removed since it was built");
    Cos8Workspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "cos8: cannot create a search workspace");
    struct Back {
        const mvdb_cos8* ix;
        Cos8Workspace* ws;
        ~Back() { ws_release(ix, ws); }
    } back{ix, ws};
    const size_t qe = (size_t)nq * ix->d, total = (size_t)nq * k;
    MVDB_TRY(ws->q.reserve(qe));
    MVDB_TRY(ws->pin.reserve(qe * sizeof(float)));
    memcpy(ws->pin.p, q_host, qe * sizeof(float));
    MVDB_HIP(hipMemcpyAsync(ws->q.p, ws->pin.p, qe * sizeof(float), hipMemcpyHostToDevice, ws->stream));
    MVDB_TRY(ws->out.reserve(total + (total + 1) / 2));
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    MVDB_TRY(search_core(ix, ws, ws->q.p, nq, k, rs, 0, Do, Io, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(float));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    memcpy(I_host, ws->pin_out.p, total * sizeof(int64_t));
    memcpy(D_host, (const char*)ws->pin_out.p + total * sizeof(int64_t), total * sizeof(float));
    return 0;
}

int search_dev(const mvdb_cos8* ix, const float* q_dev, int nq, int k, const mvdb_cos8_rowset* rs, int64_t label_offset,
               float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, D_dev, I_dev, rs));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (rs && rs->gen != ix->gen) return fail(MVDB_ERR_ARG, "row set is stale: rows were removed since it was built");
    hipStream_t s = (hipStream_t)stream;
    Cos8Workspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "cos8: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    return search_core(ix, ws, q_dev, nq, k, rs, label_offset, D_dev, I_dev, s);
}

}  // namespace

extern "C" {

int mvdb_cos8_create(int d, int device, mvdb_cos8** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d <= 0 || d > 16 * kCos8MaxChunks)
        return fail(MVDB_ERR_ARG, "cos8: dimension %d out of range [1, %d]", d, 16 * kCos8MaxChunks);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_cos8* ix = new mvdb_cos8();
    ix->d = d;
    ix->stride = (d + 15) / 16 * 16;
    ix->nchunk = ix->stride / 16;
    ix->device = device;
    if (hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess) {
        delete ix;
        return fail(MVDB_ERR_HIP, "cos8: cannot create a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_cos8_free(mvdb_cos8* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (Cos8Workspace* ws : ix->pool) delete ws;
        if (ix->codes) (void)hipFree(ix->codes);
        if (ix->a2) (void)hipFree(ix->a2);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_cos8_reset(mvdb_cos8* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    ix->gen++;
    return 0;
}

int mvdb_cos8_reserve(mvdb_cos8* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_cos8_ntotal(const mvdb_cos8* ix) { return ix ? ix->n : -1; }
int mvdb_cos8_dim(const mvdb_cos8* ix) { return ix ? ix->d : -1; }

int mvdb_cos8_add(mvdb_cos8* ix, const float* x_host, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x_host)) return fail(MVDB_ERR_ARG, "bad rows");
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)ix->d * 4));
    const int64_t first = std::min(n, chunk);
    MVDB_TRY(ix->stage.reserve((size_t)first * ix->d));
    MVDB_TRY(ix->pin.reserve((size_t)first * ix->d * sizeof(float)));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        const size_t bytes = (size_t)m * ix->d * sizeof(float);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        memcpy(ix->pin.p, x_host + r0 * ix->d, bytes);
        MVDB_HIP(hipMemcpyAsync(ix->stage.p, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
        MVDB_TRY(quantize_into(ix, ix->stage.p, m, ix->codes + (ix->n + r0) * ix->stride, ix->a2 + ix->n + r0, ix->ms));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_cos8_add_device(mvdb_cos8* ix, const float* x_dev, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x_dev)) return fail(MVDB_ERR_ARG, "bad rows");
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(quantize_into(ix, x_dev, n, ix->codes + ix->n * ix->stride, ix->a2 + ix->n, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

// ---- set_rows: stored rows overwritten in place ---------------------------------------------------------------------------------
namespace {
int set_rows_entry(mvdb_cos8* ix, const int64_t* rows_host, const float* x, bool x_on_device, int64_t m) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    if (!x) return fail(MVDB_ERR_ARG, "x is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    {   // validate first, write after
        std::vector<int64_t> v(rows_host, rows_host + m);
        std::sort(v.begin(), v.end());
        for (int64_t i = 0; i < m; ++i) {
            if (v[i] < 0 || v[i] >= ix->n)
                return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)v[i], (long long)ix->n);
            if (i && v[i] == v[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)v[i]);
        }
    }
    MVDB_TRY(quiesce(ix));
    // chunks of at most 64 MiB of rows (mvdb_cos8_add's staging): the row numbers travel with them
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / ((int64_t)ix->d * 4)));
    MVDB_TRY(ix->stage_rows.reserve((size_t)chunk));
    if (!x_on_device) {
        MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
        MVDB_TRY(ix->pin.reserve((size_t)chunk * ix->d * sizeof(float)));
    }
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        const size_t bytes = (size_t)rows * ix->d * sizeof(float);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        MVDB_HIP(hipMemcpyAsync(ix->stage_rows.p, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        const float* src = x + i0 * ix->d;
        if (!x_on_device) {
            memcpy(ix->pin.p, src, bytes);
            MVDB_HIP(hipMemcpyAsync(ix->stage.p, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
            src = ix->stage.p;
        }
        hipLaunchKernelGGL(cos8_quantize_list_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ix->ms, src,
                           (const int64_t*)ix->stage_rows.p, rows, ix->d, ix->stride, ix->codes, ix->a2);
        MVDB_HIP(hipGetLastError());
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}
}  // namespace

int mvdb_cos8_set_rows(mvdb_cos8* ix, const int64_t* rows_host, const float* x_host, int64_t m) {
    return set_rows_entry(ix, rows_host, x_host, false, m);
}

int mvdb_cos8_set_rows_device(mvdb_cos8* ix, const int64_t* rows_host, const float* x_dev, int64_t m) {
    return set_rows_entry(ix, rows_host, x_dev, true, m);
}

int mvdb_cos8_get_codes(const mvdb_cos8* ix, int64_t row0, int64_t n, int8_t* codes_host, int32_t* a2_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (codes_host)
        MVDB_HIP(hipMemcpy2D(codes_host, ix->d, ix->codes + row0 * ix->stride, ix->stride, ix->d, n,
                             hipMemcpyDeviceToHost));
    if (a2_host) MVDB_HIP(hipMemcpy(a2_host, ix->a2 + row0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_cos8_remove_rows(mvdb_cos8* ix, const int64_t* rows_host, int64_t m) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0 || (m > 0 && !rows_host)) return fail(MVDB_ERR_ARG, "bad row list");
    if (m == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::vector<int64_t> doomed(rows_host, rows_host + m);
    std::sort(doomed.begin(), doomed.end());
    for (int64_t i = 0; i < m; ++i) {
        if (doomed[i] < 0 || doomed[i] >= ix->n)
            return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)doomed[i], (long long)ix->n);
        if (i && doomed[i] == doomed[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)doomed[i]);
    }
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
        int64_t* keep_dev = nullptr;
        int8_t* tmp = nullptr;
        int32_t* tmp_a2 = nullptr;
        hipError_t e = hipMalloc((void**)&keep_dev, (size_t)kept * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void**)&tmp, (size_t)kept * ix->stride);
        if (e == hipSuccess) e = hipMalloc((void**)&tmp_a2, (size_t)kept * sizeof(int32_t));
        if (e == hipSuccess)
            e = hipMemcpyAsync(keep_dev, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms);
        if (e == hipSuccess) {
            const int64_t work = kept * ix->nchunk;
            hipLaunchKernelGGL(cos8_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, ix->codes,
                               ix->a2, keep_dev, kept, ix->nchunk, tmp, tmp_a2);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(ix->codes + r0 * ix->stride, tmp, (size_t)kept * ix->stride, hipMemcpyDeviceToDevice, ix->ms);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ix->a2 + r0, tmp_a2, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToDevice, ix->ms);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->ms);
        if (keep_dev) (void)hipFree(keep_dev);
        if (tmp) (void)hipFree(tmp);
        if (tmp_a2) (void)hipFree(tmp_a2);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? MVDB_ERR_OOM : MVDB_ERR_HIP, "cos8 remove_rows: %s",
                        hipGetErrorString(e));
    }
    ix->n -= m;
    ix->gen++;
    return 0;
}

int mvdb_cos8_search(const mvdb_cos8* ix, const float* q_host, int nq, int k, float* D_host, int64_t* I_host) {
    return search_host(ix, q_host, nq, k, nullptr, D_host, I_host);
}

int mvdb_cos8_search_device(const mvdb_cos8* ix, const float* q_dev, int nq, int k, int64_t label_offset,
                            float* D_dev, int64_t* I_dev, void* stream) {
    return search_dev(ix, q_dev, nq, k, nullptr, label_offset, D_dev, I_dev, stream);
}

int mvdb_cos8_rowset_create(const mvdb_cos8* ix, const int64_t* rows_host, int64_t m, int excluded,
                            mvdb_cos8_rowset** out) {
    if (!ix || !out) return fail(MVDB_ERR_ARG, "NULL argument");
    if (m < 0 || (m > 0 && !rows_host)) return fail(MVDB_ERR_ARG, "bad row list");
    *out = nullptr;
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    const int64_t n = ix->n;
    std::vector<int64_t> rows(rows_host, rows_host + m);
    std::sort(rows.begin(), rows.end());
    for (int64_t i = 0; i < m; ++i) {
        if (rows[i] < 0 || rows[i] >= n)
            return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)rows[i], (long long)n);
        if (i && rows[i] == rows[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)rows[i]);
    }
    mvdb_cos8_rowset* rs = new mvdb_cos8_rowset();
    rs->ix = ix;
    rs->device = ix->device;
    rs->gen = ix->gen;
    rs->n_base = n;
    rs->size = excluded ? n - m : m;
    rs->bitmap = excluded || m * 8 >= n;
    hipError_t e = hipSuccess;
    if (rs->bitmap) {
        const int64_t words = std::max<int64_t>(1, (n + 63) / 64);
        std::vector<uint64_t> bits((size_t)words, excluded ? 0ull : ~0ull);
        for (int64_t r : rows) {
            if (excluded) bits[r >> 6] |= 1ull << (r & 63);
            else bits[r >> 6] &= ~(1ull << (r & 63));
        }
        e = hipMalloc((void**)&rs->mask, (size_t)words * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemcpy(rs->mask, bits.data(), (size_t)words * sizeof(uint64_t), hipMemcpyHostToDevice);
    } else if (m > 0) {
        rs->m = m;
        e = hipMalloc((void**)&rs->rows, (size_t)m * sizeof(int64_t));
        if (e == hipSuccess) e = hipMemcpy(rs->rows, rows.data(), (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)mvdb_cos8_rowset_free(rs);
        return fail(e == hipErrorOutOfMemory ? MVDB_ERR_OOM : MVDB_ERR_HIP, "cos8 rowset: %s", hipGetErrorString(e));
    }
    *out = rs;
    return 0;
}

int64_t mvdb_cos8_rowset_size(const mvdb_cos8_rowset* rs) { return rs ? rs->size : -1; }
int mvdb_cos8_rowset_is_bitmap(const mvdb_cos8_rowset* rs) { return rs ? (int)rs->bitmap : -1; }

int mvdb_cos8_rowset_free(mvdb_cos8_rowset* rs) {
    if (!rs) return 0;
    DeviceGuard g(rs->device);
    // no device-wide wait here (as mvdb_rowset_free): hipFree itself does not release memory a queued kernel still reads
    if (rs->mask) (void)hipFree(rs->mask);
    if (rs->rows) (void)hipFree(rs->rows);
    delete rs;
    return 0;
}

int mvdb_cos8_search_rowset(const mvdb_cos8* ix, const float* q_host, int nq, int k, const mvdb_cos8_rowset* rs,
                            float* D_host, int64_t* I_host) {
    if (!rs) return fail(MVDB_ERR_ARG, "row set is NULL");
    return search_host(ix, q_host, nq, k, rs, D_host, I_host);
}

int mvdb_cos8_search_rowset_device(const mvdb_cos8* ix, const float* q_dev, int nq, int k, const mvdb_cos8_rowset* rs,
                                   int64_t label_offset, float* D_dev, int64_t* I_dev, void* stream) {
    if (!rs) return fail(MVDB_ERR_ARG, "row set is NULL");
    return search_dev(ix, q_dev, nq, k, rs, label_offset, D_dev, I_dev, stream);
}

}  // extern "C"
