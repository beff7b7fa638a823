// rabitq.hip — C-ABI (include/mvdb.h "RaBitQ index") of the 1-bit index behind RabitqVectorDatabase: the sign bits of the
// centred, rotated rows on the device, scored against a 4-bit query into an estimate of the inner product.  faiss.IndexRaBitQ's
// place in the flat family.
//
// HBM layout: codes[cap, d / 8] (d a multiple of 128: 1 to 32 whole 16-byte chunks), fg[cap] = (f, g) and B[cap], rows [0, n)
// live.  The centroid [d] and the rotation's sign bytes [4, d / 8] sit beside them.  No fp32 rows are kept.  The host shape is
// sq4.hip's: workspaces per stream, exclusive mutators on a private stream, compacting removal through a staging copy.
#include <algorithm>
#include <cmath>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "rabitq_kernels.hpp"

using namespace mvdb;

namespace {

struct RbqWorkspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> qf;        // host API: the queries staged on the device
    DevBuf<uint8_t> planes;  // [nq, 4, d / 8]
    DevBuf<uint8_t> u;       // [nq, d] in the matrix-core order
    DevBuf<float4> params;   // [nq]
    DevBuf<uint64_t> mask;   // host API: the bitmap of this call
    DevBuf<uint64_t> cand;   // partial top-k lists
    DevBuf<int64_t> out;     // host API results, packed [I | D]
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
    ~RbqWorkspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_rbq {
    int d = 0, rb = 0, nchunk = 0, device = 0;
    int P = 0;                 // the rotation's window: the largest power of two <= d
    int R = 0;                 // its rounds
    float scale = 1.0f;        // the fp32 nearest 1 / sqrt(P)
    int64_t n = 0, cap = 0;
    RbqStore st{nullptr, nullptr, nullptr};
    float* cen = nullptr;      // [d] on the device
    uint8_t* signs = nullptr;  // [4, d / 8] on the device
    std::vector<float> cen_h;
    std::vector<uint8_t> signs_h;
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add / set_rows on their way to the encoder
    DevBuf<int64_t> stage_rows;
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, RbqWorkspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<RbqWorkspace*> pool, idle;           // host-API calls: private streams
    RbqRotation rot() const { return RbqRotation{signs, R, scale}; }
};

namespace {

// ---- the shape table -------------------------------------------------------------------------------------------------------
// Per row width (16-byte chunks): G lanes per row — the power of two >= the chunk count —, U batches in flight per wave.
// kRbqBlocks is the most resident blocks per CU of the VALU form (the occupancy query may say fewer), kRbqMfmaMinNq the batch
// size from which the matrix-core form serves.  All of them are first guesses taken over from sq4.hip.
constexpr int kRbqBlocks = 8;
constexpr int kRbqMfmaMinNq = 5;
constexpr size_t kRbqLdsPerCu = 160 * 1024;

template <int G_, int U_>
struct RbqShape {
    static constexpr int G = G_, U = U_;
};
template <typename Launch>
int with_rbq_shape(int nchunk, Launch launch) {
    if (nchunk <= 1) return launch(RbqShape<1, 4>{});
    if (nchunk <= 2) return launch(RbqShape<2, 4>{});
    if (nchunk <= 4) return launch(RbqShape<4, 4>{});
    if (nchunk <= 8) return launch(RbqShape<8, 4>{});
    if (nchunk <= 16) return launch(RbqShape<16, 4>{});
    return launch(RbqShape<32, 4>{});
}

// the rotation's kernels by window registers per lane, NR = P / 64
template <int NR_>
struct RbqWindow {
    static constexpr int NR = NR_;
};
template <typename Launch>
int with_rbq_window(int P, Launch launch) {
    switch (P / kWave) {
        case 2: return launch(RbqWindow<2>{});
        case 4: return launch(RbqWindow<4>{});
        case 8: return launch(RbqWindow<8>{});
        case 16: return launch(RbqWindow<16>{});
        case 32: return launch(RbqWindow<32>{});
        default: return launch(RbqWindow<64>{});
    }
}

// the grid rule of the row scans: tiles -> waves -> blocks, at most per_cu resident blocks per CU
int rbq_grid(int64_t n, int rows_per_wave, int waves, int per_cu, int device) {
    const int64_t ntiles = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t want = (ntiles + waves - 1) / waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}

int queries_per_pass(int nq) { return nq >= 3 ? 4 : nq; }  // NQ in {1, 2, 4}

template <int G, int U>
const void* scan_kernel_for(int NQ) {
    void (*k1)(RbqScanArgs) = rbq_scan_kernel<G, U, 1>;
    void (*k2)(RbqScanArgs) = rbq_scan_kernel<G, U, 2>;
    void (*k4)(RbqScanArgs) = rbq_scan_kernel<G, U, 4>;
    return NQ == 1 ? (const void*)k1 : NQ == 2 ? (const void*)k2 : (const void*)k4;
}

template <int G, int U>
int scan_blocks(int64_t n, int NQ, int device) {
    const int per_cu = std::max(1, std::min(cached_occupancy(scan_kernel_for<G, U>(NQ), kRbqThreads, 0, 4), kRbqBlocks));
    return rbq_grid(n, (kWave / G) * U, kRbqThreads / kWave, per_cu, device);
}

template <int G, int U>
int launch_scan(const RbqScanArgs& a, int NQ, dim3 grid, hipStream_t s) {
    if (NQ == 1) hipLaunchKernelGGL((rbq_scan_kernel<G, U, 1>), grid, dim3(kRbqThreads), 0, s, a);
    else if (NQ == 2) hipLaunchKernelGGL((rbq_scan_kernel<G, U, 2>), grid, dim3(kRbqThreads), 0, s, a);
    else hipLaunchKernelGGL((rbq_scan_kernel<G, U, 4>), grid, dim3(kRbqThreads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// The block of the matrix-core form (sq4_mfma_block's rule): QB = 2 blocks of 32 queries per row read when the call has more
// than 32 queries and 64 queries fit the LDS beside one wave's lists; then as many waves, up to 8, as the lists leave room for,
// two blocks of 4 waves where two fit the CU's 160 KiB.
struct RbqMfmaPlan {
    int QB = 1, waves = 1, per_cu = 1;
    size_t lds = 0;
};
RbqMfmaPlan rbq_mfma_block(int d, int k, int nq) {
    RbqMfmaPlan p;
    p.QB = (nq > 32 && rbq_mfma_lds_bytes(d, k, 2, 1) <= kRbqLdsPerCu) ? 2 : 1;
    int nw = 8;
    while (nw > 1 && rbq_mfma_lds_bytes(d, k, p.QB, nw) > kRbqLdsPerCu) nw >>= 1;
    if (nw == 8 && rbq_mfma_lds_bytes(d, k, p.QB, 4) * 2 <= kRbqLdsPerCu) nw = 4;
    p.waves = nw;
    p.lds = rbq_mfma_lds_bytes(d, k, p.QB, nw);
    p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(8 / nw, kRbqLdsPerCu / p.lds));
    return p;
}

// form: 0 by the shape table, 1 the VALU form, 2 the matrix-core form (the benchmark times both)
bool mfma_serves(int nq, int form) { return form ? form == 2 : nq >= kRbqMfmaMinNq; }

// ---- workspaces (as sq4.hip) -----------------------------------------------------------------------------------------------
RbqWorkspace* ws_for_stream(const mvdb_rbq* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    RbqWorkspace* ws = new RbqWorkspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

RbqWorkspace* ws_acquire(const mvdb_rbq* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        RbqWorkspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    RbqWorkspace* ws = new RbqWorkspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

void ws_release(const mvdb_rbq* ix, RbqWorkspace* ws) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    ix->idle.push_back(ws);
}

struct WsBack {
    const mvdb_rbq* ix;
    RbqWorkspace* ws;
    ~WsBack() { ws_release(ix, ws); }
};

// Mutators hold the index exclusively; they wait for every stream a search of this index was enqueued on and for the private
// ones, and for nothing else (bits.hip: quiesce).
int quiesce(mvdb_rbq* ix) {
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
    for (RbqWorkspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "rbq search: the workspace of this stream is too small to capture this shape; run it once "
                                  "eagerly on the stream first");
    return b.reserve(n);
}

void free_store(RbqStore& st) {
    if (st.codes) (void)hipFree(st.codes);
    if (st.fg) (void)hipFree(st.fg);
    if (st.B) (void)hipFree(st.B);
    st = RbqStore{nullptr, nullptr, nullptr};
}

int alloc_store(RbqStore& st, int64_t rows, int rb) {
    if (hipMalloc((void**)&st.codes, (size_t)rows * rb) != hipSuccess || hipMalloc((void**)&st.fg, (size_t)rows * sizeof(float2)) != hipSuccess ||
        hipMalloc((void**)&st.B, (size_t)rows * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        free_store(st);
        return fail(MVDB_ERR_OOM, "rbq: cannot allocate %lld rows", (long long)rows);
    }
    return 0;
}

int grow(mvdb_rbq* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "rbq: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    RbqStore st{nullptr, nullptr, nullptr};
    MVDB_TRY(alloc_store(st, cap, ix->rb));
    if (ix->n) {
        MVDB_HIP(hipMemcpyAsync(st.codes, ix->st.codes, (size_t)ix->n * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipMemcpyAsync(st.fg, ix->st.fg, (size_t)ix->n * sizeof(float2), hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipMemcpyAsync(st.B, ix->st.B, (size_t)ix->n * sizeof(int32_t), hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    free_store(ix->st);
    ix->st = st;
    ix->cap = cap;
    return 0;
}

// fp32 [n, d] on the device -> code, (f, g), B (rows_dev == nullptr: stored rows row0 .. ; else stored row rows_dev[i])
int encode_into(const mvdb_rbq* ix, const float* x_dev, int64_t n, const int64_t* rows_dev, int64_t row0, hipStream_t s) {
    if (n <= 0) return 0;
    constexpr int per_block = kRbqThreads / kWave;
    RbqEncodeArgs a{x_dev, n, ix->d, ix->cen, ix->rot(), rows_dev, ix->st.codes + row0 * ix->rb, ix->st.fg + row0, ix->st.B + row0};
    const size_t lds = (size_t)per_block * ix->d * sizeof(float);
    return with_rbq_window(ix->P, [&](auto wn) {
        using W = decltype(wn);
        hipLaunchKernelGGL(rbq_encode_kernel<W::NR>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kRbqThreads), lds, s, a);
        MVDB_HIP(hipGetLastError());
        return 0;
    });
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// the call's 4-bit queries, one launch: q_dev [nq, d] -> ws->planes, ws->u, ws->params
int build_queries(const mvdb_rbq* ix, RbqWorkspace* ws, const float* q_dev, int nq, bool capturing, hipStream_t s) {
    MVDB_TRY(ws_reserve(ws->planes, (size_t)nq * 4 * ix->rb, capturing));
    MVDB_TRY(ws_reserve(ws->u, (size_t)nq * ix->d, capturing));
    MVDB_TRY(ws_reserve(ws->params, (size_t)nq, capturing));
    RbqQueryArgs a{q_dev, ix->d, ix->cen, ix->rot(), ws->planes.p, ws->u.p, ws->params.p};
    return with_rbq_window(ix->P, [&](auto wn) {
        using W = decltype(wn);
        hipLaunchKernelGGL(rbq_query_kernel<W::NR>, dim3((unsigned)nq), dim3(kWave), (size_t)ix->d * sizeof(float), s, a);
        MVDB_HIP(hipGetLastError());
        return 0;
    });
}

template <int QB>
int launch_mfma(const mvdb_rbq* ix, const RbqMfmaArgs& a, const RbqMfmaPlan& p, int nblocks, hipStream_t s) {
    MVDB_TRY(ensure_dynamic_lds((const void*)rbq_mfma_kernel<QB>, p.lds, ix->device));
    hipLaunchKernelGGL(rbq_mfma_kernel<QB>, dim3((unsigned)nblocks, (unsigned)((a.nq + 32 * QB - 1) / (32 * QB))),
                       dim3(p.waves * kWave), p.lds, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// Everything on stream s, no synchronisation.  q_dev: fp32 [nq, d]; mask_dev: nullptr or the bitmap, on the device.
int search_core(const mvdb_rbq* ix, RbqWorkspace* ws, const float* q_dev, int nq, int k, const uint64_t* mask_dev, int form,
                float* D, int64_t* I, bool capturing, hipStream_t s) {
    if (ix->n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(rbq_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    MVDB_TRY(build_queries(ix, ws, q_dev, nq, capturing, s));
    int nblocks = 0;
    if (mfma_serves(nq, form)) {
        const RbqMfmaPlan p = rbq_mfma_block(ix->d, k, nq);
        nblocks = rbq_grid(ix->n, 32, p.waves, p.per_cu, ix->device);
        MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
        RbqMfmaArgs a{ix->st.codes, ix->st.fg, ix->st.B, ix->nchunk, ix->d, ix->n, mask_dev, ws->u.p, ws->params.p, nq, k, ws->cand.p};
        MVDB_TRY(p.QB == 2 ? launch_mfma<2>(ix, a, p, nblocks, s) : launch_mfma<1>(ix, a, p, nblocks, s));
    } else {
        const int NQ = queries_per_pass(nq);
        MVDB_TRY(with_rbq_shape(ix->nchunk, [&](auto sh) {
            using Sh = decltype(sh);
            nblocks = scan_blocks<Sh::G, Sh::U>(ix->n, NQ, ix->device);
            MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
            RbqScanArgs a{ix->st.codes, ix->st.fg, ix->st.B, ix->nchunk, ix->n, mask_dev, ws->planes.p, ws->params.p, nq, k, ws->cand.p};
            return launch_scan<Sh::G, Sh::U>(a, NQ, dim3((unsigned)nblocks, (unsigned)((nq + NQ - 1) / NQ)), s);
        }));
    }
    hipLaunchKernelGGL(rbq_merge_kernel, dim3(nq), dim3(kRbqThreads), 0, s, ws->cand.p, nblocks, k, D, I);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_search(const mvdb_rbq* ix, const void* q, int nq, int k, int form, const void* D, const void* I) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "rbq: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    if (form < 0 || form > 2) return fail(MVDB_ERR_ARG, "rbq: form must be 0 (by the shape table), 1 (VALU) or 2 (matrix cores)");
    return 0;
}

// host queries -> ws->qf on the workspace's stream (and the bitmap -> ws->mask behind them in the same pinned buffer)
int stage_queries(const mvdb_rbq* ix, RbqWorkspace* ws, const float* q_host, int nq, const uint64_t* mask_host,
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
int search_host(const mvdb_rbq* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, int form, float* D_host,
                int64_t* I_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, form, D_host, I_host));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    RbqWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "rbq: cannot create a search workspace");
    WsBack back{ix, ws};
    const uint64_t* mask_dev = nullptr;
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, mask_host, &mask_dev));
    const size_t total = (size_t)nq * k;
    MVDB_TRY(ws->out.reserve(total + total / 2 + 1));  // I: total int64; D: total floats
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    MVDB_TRY(search_core(ix, ws, ws->qf.p, nq, k, mask_dev, form, Do, Io, false, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(float));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    const char* got = (const char*)ws->pin_out.p;
    memcpy(I_host, got, total * sizeof(int64_t));
    memcpy(D_host, got + total * sizeof(int64_t), total * sizeof(float));
    return 0;
}

// ---- ingest ----------------------------------------------------------------------------------------------------------------
int check_mutation(const mvdb_rbq* ix, const void* x, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x)) return fail(MVDB_ERR_ARG, "bad rows");
    return 0;
}

int check_rows(const mvdb_rbq* ix, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= ix->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)ix->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

// Host bytes -> device, through the pinned buffer in chunks of at most 64 MiB; after(offset_items, items) runs behind each chunk.
template <typename After>
int upload(mvdb_rbq* ix, const void* host, int64_t items, int64_t item_bytes, void* dev, bool advance, After after) {
    const int64_t chunk = std::min<int64_t>(items, std::max<int64_t>(1, (64ll << 20) / item_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * item_bytes)));
    for (int64_t i0 = 0; i0 < items; i0 += chunk) {
        const int64_t m = std::min(chunk, items - i0);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        memcpy(ix->pin.p, (const char*)host + i0 * item_bytes, (size_t)(m * item_bytes));
        MVDB_HIP(hipMemcpyAsync((char*)dev + (advance ? i0 * item_bytes : 0), ix->pin.p, (size_t)(m * item_bytes), hipMemcpyHostToDevice,
                                ix->ms));
        MVDB_TRY(after(i0, m));
    }
    return 0;
}

// set_rows: fp32 rows already on the device (staged or the caller's) through the encoder to their places
int set_rows_from(mvdb_rbq* ix, const int64_t* rows_host, const float* x, bool x_on_device, int64_t m) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    if (!x) return fail(MVDB_ERR_ARG, "x is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    {   // validate first, write after
        std::vector<int64_t> v;
        MVDB_TRY(check_rows(ix, rows_host, m, &v));
    }
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(ix->stage_rows.reserve((size_t)m));
    MVDB_HIP(hipMemcpyAsync(ix->stage_rows.p, rows_host, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
    if (x_on_device) {
        MVDB_TRY(encode_into(ix, x, m, ix->stage_rows.p, 0, ix->ms));
    } else {
        const int64_t row_bytes = (int64_t)ix->d * sizeof(float);
        MVDB_TRY(ix->stage.reserve((size_t)std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / row_bytes)) * ix->d));
        MVDB_TRY(upload(ix, x, m, row_bytes, ix->stage.p, false,
                        [&](int64_t i0, int64_t rows) { return encode_into(ix, ix->stage.p, rows, ix->stage_rows.p + i0, 0, ix->ms); }));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

int check_empty(const mvdb_rbq* ix, const char* what) {
    if (ix->n) return fail(MVDB_ERR_ARG, "rbq %s: the index holds %lld rows coded with the present one", what, (long long)ix->n);
    return 0;
}

}  // namespace

extern "C" {

int mvdb_rbq_create(int d, int device, mvdb_rbq** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d < 128 || d > 128 * kRbqMaxChunks || d % 128)
        return fail(MVDB_ERR_ARG, "rbq: dimension %d is not a multiple of 128 in [128, %d]", d, 128 * kRbqMaxChunks);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_rbq* ix = new mvdb_rbq();
    ix->d = d;
    ix->rb = d / 8;
    ix->nchunk = d / 128;
    ix->device = device;
    ix->P = 128;
    while (ix->P * 2 <= d) ix->P *= 2;
    ix->scale = (float)(1.0 / std::sqrt((double)ix->P));
    ix->cen_h.assign((size_t)d, 0.0f);
    ix->signs_h.assign((size_t)kRbqMaxRounds * ix->rb, 0);
    const size_t sbytes = (size_t)kRbqMaxRounds * ix->rb;
    if (hipMalloc((void**)&ix->cen, (size_t)d * sizeof(float)) != hipSuccess || hipMalloc((void**)&ix->signs, sbytes) != hipSuccess ||
        hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess ||
        hipMemcpy(ix->cen, ix->cen_h.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ix->signs, ix->signs_h.data(), sbytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (ix->cen) (void)hipFree(ix->cen);
        if (ix->signs) (void)hipFree(ix->signs);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
        delete ix;
        return fail(MVDB_ERR_HIP, "rbq: cannot create the centroid, the rotation or a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_rbq_free(mvdb_rbq* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (RbqWorkspace* ws : ix->pool) delete ws;
        free_store(ix->st);
        if (ix->cen) (void)hipFree(ix->cen);
        if (ix->signs) (void)hipFree(ix->signs);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_rbq_reset(mvdb_rbq* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    return 0;
}

int mvdb_rbq_reserve(mvdb_rbq* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_rbq_ntotal(const mvdb_rbq* ix) { return ix ? ix->n : -1; }
int mvdb_rbq_dim(const mvdb_rbq* ix) { return ix ? ix->d : -1; }

int mvdb_rbq_set_rotation(mvdb_rbq* ix, const uint8_t* signs_host, int rounds) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (rounds < 0 || rounds > kRbqMaxRounds) return fail(MVDB_ERR_ARG, "rbq: rounds must be in [0, %d] (got %d)", kRbqMaxRounds, rounds);
    if (rounds && !signs_host) return fail(MVDB_ERR_ARG, "signs is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(check_empty(ix, "set_rotation"));
    MVDB_TRY(quiesce(ix));
    std::fill(ix->signs_h.begin(), ix->signs_h.end(), (uint8_t)0);
    if (rounds) memcpy(ix->signs_h.data(), signs_host, (size_t)rounds * ix->rb);
    MVDB_HIP(hipMemcpy(ix->signs, ix->signs_h.data(), ix->signs_h.size(), hipMemcpyHostToDevice));
    ix->R = rounds;
    return 0;
}

int mvdb_rbq_get_rotation(const mvdb_rbq* ix, uint8_t* signs_host, int* rounds) {
    if (!ix || !rounds) return fail(MVDB_ERR_ARG, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *rounds = ix->R;
    if (signs_host && ix->R) memcpy(signs_host, ix->signs_h.data(), (size_t)ix->R * ix->rb);
    return 0;
}

int mvdb_rbq_set_centroid(mvdb_rbq* ix, const float* c_host) {
    if (!ix || !c_host) return fail(MVDB_ERR_ARG, "NULL argument");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(check_empty(ix, "set_centroid"));
    MVDB_TRY(quiesce(ix));
    ix->cen_h.assign(c_host, c_host + ix->d);
    MVDB_HIP(hipMemcpy(ix->cen, ix->cen_h.data(), (size_t)ix->d * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int mvdb_rbq_get_centroid(const mvdb_rbq* ix, float* c_host) {
    if (!ix || !c_host) return fail(MVDB_ERR_ARG, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    memcpy(c_host, ix->cen_h.data(), (size_t)ix->d * sizeof(float));
    return 0;
}

int mvdb_rbq_geometry(const mvdb_rbq* ix, int nq, int k, int* form, int64_t* stride_rows) {
    if (!ix || !form || !stride_rows) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0 || k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "rbq geometry: bad nq or k");
    DeviceGuard g(ix->device);
    if (mfma_serves(nq, 0)) {
        const RbqMfmaPlan p = rbq_mfma_block(ix->d, k, nq);
        *form = 2;
        *stride_rows = (int64_t)device_cus(ix->device) * p.per_cu * p.waves * 32;
        return 0;
    }
    *form = 1;
    return with_rbq_shape(ix->nchunk, [&](auto sh) {
        using Sh = decltype(sh);
        constexpr int tile = (kWave / Sh::G) * Sh::U;
        *stride_rows = (int64_t)scan_blocks<Sh::G, Sh::U>(INT64_MAX / 2, queries_per_pass(nq), ix->device) * (kRbqThreads / kWave) * tile;
        return 0;
    });
}

int mvdb_rbq_add(mvdb_rbq* ix, const float* x_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t row_bytes = (int64_t)ix->d * sizeof(float);
    MVDB_TRY(ix->stage.reserve((size_t)std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes)) * ix->d));
    MVDB_TRY(upload(ix, x_host, n, row_bytes, ix->stage.p, false,
                    [&](int64_t r0, int64_t m) { return encode_into(ix, ix->stage.p, m, nullptr, ix->n + r0, ix->ms); }));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_rbq_add_device(mvdb_rbq* ix, const float* x_dev, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_dev, n));
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(encode_into(ix, x_dev, n, nullptr, ix->n, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_rbq_add_codes(mvdb_rbq* ix, const uint8_t* codes_host, const float* factors_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, codes_host, n));
    if (n == 0) return 0;
    if (!factors_host) return fail(MVDB_ERR_ARG, "factors is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    auto nothing = [](int64_t, int64_t) { return 0; };
    MVDB_TRY(upload(ix, codes_host, n, ix->rb, ix->st.codes + ix->n * ix->rb, true, nothing));
    MVDB_TRY(upload(ix, factors_host, n, sizeof(float2), ix->st.fg + ix->n, true, nothing));
    hipLaunchKernelGGL(rbq_popcount_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->ms,
                       (const uint8_t*)(ix->st.codes + ix->n * ix->rb), n, ix->nchunk, ix->d, ix->st.B + ix->n);
    MVDB_HIP(hipGetLastError());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_rbq_get_rows(const mvdb_rbq* ix, int64_t row0, int64_t n, uint8_t* codes_host, float* factors_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (!codes_host || !factors_host) return fail(MVDB_ERR_ARG, "NULL output buffer");
    MVDB_HIP(hipMemcpy(codes_host, ix->st.codes + row0 * ix->rb, (size_t)n * ix->rb, hipMemcpyDeviceToHost));
    MVDB_HIP(hipMemcpy(factors_host, ix->st.fg + row0, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_rbq_remove_rows(mvdb_rbq* ix, const int64_t* rows_host, int64_t m) {
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
        MVDB_TRY(keep_dev.reserve((size_t)kept));
        RbqStore tmp{nullptr, nullptr, nullptr};
        MVDB_TRY(alloc_store(tmp, kept, ix->rb));
        int rc = 0;
        const int64_t work = kept * (ix->nchunk + 1);
        if (hipMemcpyAsync(keep_dev.p, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms) != hipSuccess) rc = 1;
        hipLaunchKernelGGL(rbq_move_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, ix->st, (const int64_t*)keep_dev.p,
                           (const int64_t*)nullptr, kept, ix->nchunk, tmp);
        if (hipGetLastError() != hipSuccess) rc = 1;
        if (hipMemcpyAsync(ix->st.codes + r0 * ix->rb, tmp.codes, (size_t)kept * ix->rb, hipMemcpyDeviceToDevice, ix->ms) != hipSuccess ||
            hipMemcpyAsync(ix->st.fg + r0, tmp.fg, (size_t)kept * sizeof(float2), hipMemcpyDeviceToDevice, ix->ms) != hipSuccess ||
            hipMemcpyAsync(ix->st.B + r0, tmp.B, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToDevice, ix->ms) != hipSuccess)
            rc = 1;
        if (hipStreamSynchronize(ix->ms) != hipSuccess) rc = 1;
        free_store(tmp);
        if (rc) {
            (void)hipGetLastError();
            return fail(MVDB_ERR_HIP, "rbq remove_rows: the compaction failed");
        }
    }
    ix->n -= m;
    return 0;
}

int mvdb_rbq_set_rows(mvdb_rbq* ix, const int64_t* rows_host, const float* x_host, int64_t m) {
    return set_rows_from(ix, rows_host, x_host, false, m);
}
int mvdb_rbq_set_rows_device(mvdb_rbq* ix, const int64_t* rows_host, const float* x_dev, int64_t m) {
    return set_rows_from(ix, rows_host, x_dev, true, m);
}

int mvdb_rbq_query(const mvdb_rbq* ix, const float* q_host, int nq, uint8_t* u_host, float* params_host) {
    if (!ix || !q_host || !u_host || !params_host) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    RbqWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "rbq: cannot create a search workspace");
    WsBack back{ix, ws};
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, nullptr, nullptr));
    MVDB_TRY(build_queries(ix, ws, ws->qf.p, nq, false, ws->stream));
    std::vector<uint8_t> slots((size_t)nq * ix->d);
    MVDB_HIP(hipMemcpyAsync(slots.data(), ws->u.p, slots.size(), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(params_host, ws->params.p, (size_t)nq * sizeof(float4), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    for (int qi = 0; qi < nq; ++qi)  // the scan's order -> natural dimension order
        for (int i = 0; i < ix->d; ++i) u_host[(size_t)qi * ix->d + i] = slots[(size_t)qi * ix->d + rbq_query_slot(i)];
    return 0;
}

int mvdb_rbq_search(const mvdb_rbq* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, float* D_host, int64_t* I_host) {
    return search_host(ix, q_host, nq, k, mask_host, 0, D_host, I_host);
}
int mvdb_rbq_search_form(const mvdb_rbq* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, int form, float* D_host,
                         int64_t* I_host) {
    return search_host(ix, q_host, nq, k, mask_host, form, D_host, I_host);
}

int mvdb_rbq_search_device(const mvdb_rbq* ix, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D_dev, int64_t* I_dev,
                           void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, 0, D_dev, I_dev));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    hipStream_t s = (hipStream_t)stream;
    RbqWorkspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "rbq: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    return search_core(ix, ws, q_dev, nq, k, mask_dev, 0, D_dev, I_dev, capturing, s);
}

}  // extern "C"
