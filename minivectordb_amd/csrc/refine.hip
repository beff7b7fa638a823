// refine.hip — C-ABI (include/mvdb.h "REFINE STORE") of the refine store: every row as IEEE binary16 on the device, and the
// re-rank that turns the candidates of a code index (binary, PQ, SQ4, RaBitQ, MX) into their exact top k.
//
// HBM layout: rows[cap, d] binary16, rows [0, n) live; d is a multiple of 8, so a row is whole 16-byte chunks.  The host shape
// is mx.hip's: workspaces per stream, exclusive mutators on a private stream, compacting removal through a staging copy.
#include <algorithm>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "refine_kernels.hpp"

using namespace mvdb;

namespace {

struct RefineWorkspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> qf;        // host API: the queries staged on the device
    DevBuf<int64_t> ids;     // host API: the lists of this call
    DevBuf<uint64_t> scored; // one key per list slot
    DevBuf<int64_t> out;     // host API results, packed [I | D]
    PinnedBuf pin, pin_out;
    std::mutex use_mu;       // one re-rank at a time per workspace
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
    ~RefineWorkspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_refine {
    int d = 0, device = 0;
    int64_t n = 0, cap = 0;
    uint16_t* rows = nullptr;
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add / set_rows on their way to the converter
    DevBuf<int64_t> stage_rows;
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, RefineWorkspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<RefineWorkspace*> pool, idle;           // host-API calls: private streams
    int chunks() const { return d / 8; }
    size_t row_bytes() const { return (size_t)d * 2; }
};

namespace {

// ---- workspaces (as mx.hip) ------------------------------------------------------------------------------------------------
RefineWorkspace* ws_for_stream(const mvdb_refine* st, hipStream_t s) {
    std::lock_guard<std::mutex> lk(st->ws_mu);
    auto it = st->by_stream.find(s);
    if (it != st->by_stream.end()) return it->second;
    RefineWorkspace* ws = new RefineWorkspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    st->by_stream[s] = ws;
    return ws;
}

RefineWorkspace* ws_acquire(const mvdb_refine* st) {
    std::lock_guard<std::mutex> lk(st->ws_mu);
    if (!st->idle.empty()) {
        RefineWorkspace* ws = st->idle.back();
        st->idle.pop_back();
        return ws;
    }
    RefineWorkspace* ws = new RefineWorkspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    st->pool.push_back(ws);
    return ws;
}

struct WsBack {
    const mvdb_refine* st;
    RefineWorkspace* ws;
    ~WsBack() {
        std::lock_guard<std::mutex> lk(st->ws_mu);
        st->idle.push_back(ws);
    }
};

// Mutators hold the store exclusively; they wait for every stream a re-rank of this store was enqueued on and for the private
// ones, and for nothing else (bits.hip: quiesce).
int quiesce(mvdb_refine* st) {
    std::lock_guard<std::mutex> lk(st->ws_mu);
    bool device_wide = false;
    for (auto it = st->by_stream.begin(); it != st->by_stream.end();) {
        const hipError_t e = hipStreamSynchronize(it->first);
        if (e == hipSuccess) {
            ++it;
            continue;
        }
        (void)hipGetLastError();
        if (e == hipErrorInvalidHandle || e == hipErrorInvalidResourceHandle || e == hipErrorContextIsDestroyed) {
            delete it->second;
            it = st->by_stream.erase(it);
        } else {
            device_wide = true;
            ++it;
        }
    }
    for (RefineWorkspace* ws : st->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(st->ms));
    return 0;
}

int grow(mvdb_refine* st, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "refine: at most %lld rows per store (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= st->cap) return 0;
    int64_t cap = std::max<int64_t>(need, st->cap + st->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    uint16_t* r = nullptr;
    if (hipMalloc((void**)&r, (size_t)cap * st->row_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVDB_ERR_OOM, "refine: cannot allocate %lld rows", (long long)cap);
    }
    if (st->n) {
        MVDB_HIP(hipMemcpyAsync(r, st->rows, (size_t)st->n * st->row_bytes(), hipMemcpyDeviceToDevice, st->ms));
        MVDB_HIP(hipStreamSynchronize(st->ms));
    }
    if (st->rows) (void)hipFree(st->rows);
    st->rows = r;
    st->cap = cap;
    return 0;
}

unsigned chunk_grid(int64_t work) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 1 << 20)); }

// fp32 [n, d] on the device -> binary16 rows (rows_dev == nullptr: consecutive from row `first`; else row rows_dev[i])
int convert_into(const mvdb_refine* st, const float* x_dev, int64_t n, const int64_t* rows_dev, int64_t first, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(refine_convert_kernel, dim3(chunk_grid(n * st->chunks())), dim3(256), 0, s, x_dev, n, st->chunks(), rows_dev,
                       (rf_u32x4*)(st->rows + first * st->d));
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_rows(const mvdb_refine* st, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= st->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)st->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

int check_mutation(const mvdb_refine* st, const void* x, int64_t n) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    if (n < 0 || (n > 0 && !x)) return fail(MVDB_ERR_ARG, "bad rows");
    return 0;
}

// ---- re-rank ---------------------------------------------------------------------------------------------------------------
template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "refine: the workspace of this stream is too small to capture this shape; run it once "
                                  "eagerly on the stream first");
    return b.reserve(n);
}

// Slots per block: enough blocks, with the call's other queries, for about four per CU, and no block with less than one round
// of its waves.  One query with 1024 candidates spreads over 64 blocks.  A first guess, not swept.
int rerank_per_block(int nq, int m, int device) {
    const int64_t want = std::max<int64_t>(1, (4ll * device_cus(device) + nq - 1) / nq);
    const int64_t slots = (m + want - 1) / want;
    return (int)((slots + kRefineSlots - 1) / kRefineSlots) * kRefineSlots;
}

// Everything on stream s, no synchronisation.  Exactly one of ids_dev (int64 [nq, m]) and keys_dev (keys [nq, m]) is given.
int rerank_core(const mvdb_refine* st, RefineWorkspace* ws, const float* q_dev, int nq, const int64_t* ids_dev,
                const uint64_t* keys_dev, int m, int k, float* D, int64_t* I, bool capturing, hipStream_t s) {
    MVDB_TRY(ws_reserve(ws->scored, (size_t)nq * m, capturing));
    const int per_block = rerank_per_block(nq, m, st->device);
    RefineRerankArgs a{st->rows, st->n, st->d, q_dev, ids_dev ? (const void*)ids_dev : (const void*)keys_dev, m, per_block,
                       ws->scored.p};
    const dim3 grid((unsigned)((m + per_block - 1) / per_block), (unsigned)nq);
    if (ids_dev) hipLaunchKernelGGL(refine_rerank_kernel<false>, grid, dim3(kRefineThreads), 0, s, a);
    else hipLaunchKernelGGL(refine_rerank_kernel<true>, grid, dim3(kRefineThreads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    hipLaunchKernelGGL(refine_merge_kernel, dim3(nq), dim3(kRefineThreads), 0, s, ws->scored.p, m, k, D, I);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_rerank(const mvdb_refine* st, const void* q, int nq, const void* list, int m, int k, const void* D, const void* I) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    if (!q || !list || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to rerank");
    if (nq <= 0 || nq > 65535) return fail(MVDB_ERR_ARG, "refine: nq must be in [1, 65535] (got %d)", nq);
    if (m <= 0 || m > kRefineMaxList) return fail(MVDB_ERR_ARG, "refine: m must be in [1, %d] (got %d)", kRefineMaxList, m);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "refine: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    return 0;
}

int rerank_on_stream(const mvdb_refine* st, const float* q_dev, int nq, const int64_t* ids_dev, const uint64_t* keys_dev, int m,
                     int k, float* D_dev, int64_t* I_dev, hipStream_t s) {
    DeviceGuard g(st->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", st->device);
    std::shared_lock<std::shared_mutex> lk(st->mu);
    RefineWorkspace* ws = ws_for_stream(st, s);
    if (!ws) return fail(MVDB_ERR_HIP, "refine: cannot create a workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    return rerank_core(st, ws, q_dev, nq, ids_dev, keys_dev, m, k, D_dev, I_dev, capturing, s);
}

}  // namespace

namespace mvdb {

int refine_rerank_keys(const mvdb_refine* st, const float* q_dev, int nq, const uint64_t* keys_dev, int m, int k, float* D_dev,
                       int64_t* I_dev, hipStream_t stream) {
    MVDB_TRY(check_rerank(st, q_dev, nq, keys_dev, m, k, D_dev, I_dev));
    return rerank_on_stream(st, q_dev, nq, nullptr, keys_dev, m, k, D_dev, I_dev, stream);
}

}  // namespace mvdb

extern "C" {

int mvdb_refine_create(int d, int device, mvdb_refine** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d < 8 || d > kRefineMaxDim || d % 8)
        return fail(MVDB_ERR_ARG, "refine: dimension %d is not a multiple of 8 in [8, %d]", d, kRefineMaxDim);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_refine* st = new mvdb_refine();
    st->d = d;
    st->device = device;
    if (hipStreamCreateWithFlags(&st->ms, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete st;
        return fail(MVDB_ERR_HIP, "refine: cannot create a stream");
    }
    *out = st;
    return 0;
}

int mvdb_refine_free(mvdb_refine* st) {
    if (!st) return 0;
    DeviceGuard g(st->device);
    {
        std::unique_lock<std::shared_mutex> lk(st->mu);
        if (quiesce(st) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : st->by_stream) delete kv.second;
        for (RefineWorkspace* ws : st->pool) delete ws;
        if (st->rows) (void)hipFree(st->rows);
        if (st->ms) (void)hipStreamDestroy(st->ms);
    }
    delete st;  // (the staging buffers it owns go here, still on the store's device)
    return 0;
}

int mvdb_refine_reset(mvdb_refine* st) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    MVDB_TRY(quiesce(st));
    st->n = 0;
    return 0;
}

int mvdb_refine_reserve(mvdb_refine* st, int64_t n) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    MVDB_TRY(quiesce(st));
    return grow(st, n);
}

int64_t mvdb_refine_ntotal(const mvdb_refine* st) { return st ? st->n : -1; }
int mvdb_refine_dim(const mvdb_refine* st) { return st ? st->d : -1; }

// rows appended from the host in chunks of at most 64 MiB, through the converter
int mvdb_refine_add(mvdb_refine* st, const float* x_host, int64_t n) {
    MVDB_TRY(check_mutation(st, x_host, n));
    if (n == 0) return 0;
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    MVDB_TRY(quiesce(st));
    MVDB_TRY(grow(st, st->n + n));
    const int64_t row_bytes = (int64_t)st->d * 4;
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(st->pin.reserve((size_t)(chunk * row_bytes)));
    MVDB_TRY(st->stage.reserve((size_t)chunk * st->d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        MVDB_HIP(hipStreamSynchronize(st->ms));  // the staging buffers are reused
        memcpy(st->pin.p, x_host + r0 * st->d, (size_t)(m * row_bytes));
        MVDB_HIP(hipMemcpyAsync(st->stage.p, st->pin.p, (size_t)(m * row_bytes), hipMemcpyHostToDevice, st->ms));
        MVDB_TRY(convert_into(st, st->stage.p, m, nullptr, st->n + r0, st->ms));
    }
    MVDB_HIP(hipStreamSynchronize(st->ms));
    st->n += n;
    return 0;
}

int mvdb_refine_add_device(mvdb_refine* st, const float* x_dev, int64_t n) {
    MVDB_TRY(check_mutation(st, x_dev, n));
    if (n == 0) return 0;
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    MVDB_TRY(quiesce(st));
    MVDB_TRY(grow(st, st->n + n));
    MVDB_TRY(convert_into(st, x_dev, n, nullptr, st->n, st->ms));
    MVDB_HIP(hipStreamSynchronize(st->ms));
    st->n += n;
    return 0;
}

int mvdb_refine_get_rows(const mvdb_refine* st, int64_t row0, int64_t n, uint16_t* rows_host) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    DeviceGuard g(st->device);
    std::shared_lock<std::shared_mutex> lk(st->mu);
    if (row0 < 0 || n < 0 || row0 + n > st->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)st->n);
    if (n == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows_host is NULL");
    MVDB_HIP(hipMemcpy(rows_host, st->rows + row0 * st->d, (size_t)n * st->row_bytes(), hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_refine_remove_rows(mvdb_refine* st, const int64_t* rows_host, int64_t m) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    if (m < 0 || (m > 0 && !rows_host)) return fail(MVDB_ERR_ARG, "bad row list");
    if (m == 0) return 0;
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    std::vector<int64_t> doomed;
    MVDB_TRY(check_rows(st, rows_host, m, &doomed));
    MVDB_TRY(quiesce(st));
    // the tail behind the first removed row, compacted through a staging copy of its survivors, then written back in place
    const int64_t r0 = doomed[0];
    std::vector<int64_t> keep;
    keep.reserve((size_t)(st->n - r0 - m));
    for (int64_t r = r0, j = 0; r < st->n; ++r) {
        if (j < m && doomed[j] == r) {
            ++j;
            continue;
        }
        keep.push_back(r);
    }
    const int64_t kept = (int64_t)keep.size();
    if (kept) {
        DevBuf<int64_t> keep_dev;
        DevBuf<uint16_t> tmp;
        MVDB_TRY(keep_dev.reserve((size_t)kept));
        MVDB_TRY(tmp.reserve((size_t)kept * st->d));
        MVDB_HIP(hipMemcpyAsync(keep_dev.p, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, st->ms));
        hipLaunchKernelGGL(refine_move_kernel, dim3(chunk_grid(kept * st->chunks())), dim3(256), 0, st->ms,
                           (const rf_u32x4*)st->rows, keep_dev.p, kept, st->chunks(), (rf_u32x4*)tmp.p);
        MVDB_HIP(hipGetLastError());
        MVDB_HIP(hipMemcpyAsync(st->rows + r0 * st->d, tmp.p, (size_t)kept * st->row_bytes(), hipMemcpyDeviceToDevice, st->ms));
        MVDB_HIP(hipStreamSynchronize(st->ms));
    }
    st->n -= m;
    return 0;
}

// the rows are staged on the device chunk by chunk, their row numbers with them, and go through the converter to their places
int mvdb_refine_set_rows(mvdb_refine* st, const int64_t* rows_host, const float* x_host, int64_t m) {
    if (!st) return fail(MVDB_ERR_ARG, "store is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host || !x_host) return fail(MVDB_ERR_ARG, "rows or x is NULL");
    DeviceGuard g(st->device);
    std::unique_lock<std::shared_mutex> lk(st->mu);
    {   // validate first, write after
        std::vector<int64_t> v;
        MVDB_TRY(check_rows(st, rows_host, m, &v));
    }
    MVDB_TRY(quiesce(st));
    const int64_t row_bytes = (int64_t)st->d * 4;
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(st->stage_rows.reserve((size_t)chunk));
    MVDB_TRY(st->pin.reserve((size_t)(chunk * row_bytes)));
    MVDB_TRY(st->stage.reserve((size_t)chunk * st->d));
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        MVDB_HIP(hipStreamSynchronize(st->ms));  // the staging buffers are reused
        MVDB_HIP(hipMemcpyAsync(st->stage_rows.p, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, st->ms));
        memcpy(st->pin.p, x_host + i0 * st->d, (size_t)(rows * row_bytes));
        MVDB_HIP(hipMemcpyAsync(st->stage.p, st->pin.p, (size_t)(rows * row_bytes), hipMemcpyHostToDevice, st->ms));
        MVDB_TRY(convert_into(st, st->stage.p, rows, st->stage_rows.p, 0, st->ms));
    }
    MVDB_HIP(hipStreamSynchronize(st->ms));
    return 0;
}

// host API: stage the queries and the lists, re-rank on a private stream, one packed D2H, wait
int mvdb_refine_rerank(const mvdb_refine* st, const float* q_host, int nq, const int64_t* cand_host, int m, int k, float* D_host,
                       int64_t* I_host) {
    MVDB_TRY(check_rerank(st, q_host, nq, cand_host, m, k, D_host, I_host));
    DeviceGuard g(st->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", st->device);
    std::shared_lock<std::shared_mutex> lk(st->mu);
    RefineWorkspace* ws = ws_acquire(st);
    if (!ws) return fail(MVDB_ERR_HIP, "refine: cannot create a workspace");
    WsBack back{st, ws};
    const size_t qbytes = (size_t)nq * st->d * sizeof(float), lbytes = (size_t)nq * m * sizeof(int64_t);
    MVDB_TRY(ws->pin.reserve(qbytes + lbytes));
    memcpy(ws->pin.p, q_host, qbytes);
    memcpy((char*)ws->pin.p + qbytes, cand_host, lbytes);
    MVDB_TRY(ws->qf.reserve((size_t)nq * st->d));
    MVDB_TRY(ws->ids.reserve((size_t)nq * m));
    MVDB_HIP(hipMemcpyAsync(ws->qf.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
    MVDB_HIP(hipMemcpyAsync(ws->ids.p, (char*)ws->pin.p + qbytes, lbytes, hipMemcpyHostToDevice, ws->stream));
    const size_t total = (size_t)nq * k;
    MVDB_TRY(ws->out.reserve(total + total / 2 + 1));  // I: total int64; D: total floats
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    MVDB_TRY(rerank_core(st, ws, ws->qf.p, nq, ws->ids.p, nullptr, m, k, Do, Io, false, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(float));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    memcpy(I_host, ws->pin_out.p, total * sizeof(int64_t));
    memcpy(D_host, (const char*)ws->pin_out.p + total * sizeof(int64_t), total * sizeof(float));
    return 0;
}

int mvdb_refine_rerank_device(const mvdb_refine* st, const float* q_dev, int nq, const int64_t* cand_dev, int m, int k,
                              float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_rerank(st, q_dev, nq, cand_dev, m, k, D_dev, I_dev));
    return rerank_on_stream(st, q_dev, nq, cand_dev, nullptr, m, k, D_dev, I_dev, (hipStream_t)stream);
}

}  // extern "C"
