// bits.hip — C-ABI (include/mvdb.h "binary index") of the binary index behind BinaryVectorDatabase: packed bit rows on the
// device, exact Hamming top-k.  faiss.IndexBinaryFlat restated: D int32 ascending, ties to the lower row.
//
// HBM layout: rows[cap, d_bits / 8], rows [0, n) live; d_bits is a multiple of 128, so a row is 1 to 32 whole 16-byte chunks and
// nothing is padded.  Searches take packed queries, or fp32 queries that the pack kernel turns into them (bit i = x[i] > 0).
#include <algorithm>
#include <map>
#include <shared_mutex>
#include <vector>

#include "bits_kernels.hpp"
#include "common.hpp"

using namespace mvdb;

namespace {

struct BitsWorkspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> qf;        // host fp32 queries staged on the device
    DevBuf<uint8_t> q;       // packed queries (staged from the host, or packed from fp32 ones)
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
    ~BitsWorkspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_bits {
    int d_bits = 0, rb = 0, nchunk = 0, device = 0;
    int64_t n = 0, cap = 0;
    uint8_t* rows = nullptr;
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add_float / set_rows_float on their way to the pack kernel
    DevBuf<uint8_t> stage_bits;  // set_rows: packed rows on their way to their places
    DevBuf<int64_t> stage_rows;
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, BitsWorkspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<BitsWorkspace*> pool, idle;           // host-API calls: private streams
};

namespace {

// ---- the shape table -------------------------------------------------------------------------------------------------------
// Per row width (16-byte chunks): G lanes per row — the power of two >= the chunk count —, U batches in flight per wave,
// BLOCKS the most resident blocks per CU of the VALU form (the occupancy query may say fewer), MFMA_MIN_NQ the batch size from
// which the matrix-core form serves.  MFMA_MIN_NQ = 9 is measured at 8 chunks (1024 bits) and 32 chunks (4096 bits):
// profiles/bits_bench.jsonl — the VALU form wins at 8 queries, the two are level at 9, the matrix-core form wins from 16
// (DESIGN.md 6u).  At every other width 9 is the UNMEASURED default, and U and BLOCKS are first guesses at every width.
template <int G_, int U_, int BLOCKS_, int MFMA_MIN_NQ_>
struct BitsShape {
    static constexpr int G = G_, U = U_, BLOCKS = BLOCKS_, MFMA_MIN_NQ = MFMA_MIN_NQ_;
};
template <typename Launch>
int with_bits_shape(int nchunk, Launch launch) {
    if (nchunk <= 1) return launch(BitsShape<1, 4, 8, 9>{});
    if (nchunk <= 2) return launch(BitsShape<2, 4, 8, 9>{});
    if (nchunk <= 4) return launch(BitsShape<4, 4, 8, 9>{});
    if (nchunk <= 8) return launch(BitsShape<8, 4, 8, 9>{});
    if (nchunk <= 16) return launch(BitsShape<16, 4, 8, 9>{});
    return launch(BitsShape<32, 4, 8, 9>{});
}

// the grid rule of the row scans: batches -> waves -> blocks, at most per_cu resident blocks per CU
int bits_grid(int64_t n, int rows_per_wave, int waves, int per_cu, int device) {
    const int64_t nbatches = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t want = (nbatches + waves - 1) / waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}

// The block of the matrix-core form: as many waves, up to 8, as the lists leave room for beside the expanded queries, and the
// blocks per CU that then fit (160 KiB of LDS per CU).  d_bits <= 2048 with short lists: two blocks of 4 waves; d_bits = 4096:
// one block of 8 waves while k <= 14, fewer waves beyond.
constexpr size_t kBitsLdsPerCu = 160 * 1024;
void bits_mfma_block(int d_bits, int k, int* waves, int* per_cu) {
    int nw = 8;
    while (nw > 1 && bits_mfma_lds_bytes(d_bits, k, nw) > kBitsLdsPerCu) nw >>= 1;
    if (nw == 8 && bits_mfma_lds_bytes(d_bits, k, 4) * 2 <= kBitsLdsPerCu) nw = 4;
    *waves = nw;
    *per_cu = (int)std::max<size_t>(1, std::min<size_t>(8 / nw, kBitsLdsPerCu / bits_mfma_lds_bytes(d_bits, k, nw)));
}

template <int G, int U, int BLOCKS>
int scan_blocks(int64_t n, int device) {
    void (*kern)(BitsScanArgs) = bits_scan_kernel<G, U, 1>;
    const int per_cu = std::max(1, std::min(cached_occupancy((const void*)kern, kBitsThreads, 0, 4), BLOCKS));
    return bits_grid(n, (kWave / G) * U, kBitsThreads / kWave, per_cu, device);
}

template <int G, int U>
int launch_scan(const BitsScanArgs& a, int NQ, dim3 grid, hipStream_t s) {
    if (NQ == 1) hipLaunchKernelGGL((bits_scan_kernel<G, U, 1>), grid, dim3(kBitsThreads), 0, s, a);
    else if (NQ == 2) hipLaunchKernelGGL((bits_scan_kernel<G, U, 2>), grid, dim3(kBitsThreads), 0, s, a);
    else if (NQ == 4) hipLaunchKernelGGL((bits_scan_kernel<G, U, 4>), grid, dim3(kBitsThreads), 0, s, a);
    else hipLaunchKernelGGL((bits_scan_kernel<G, U, 8>), grid, dim3(kBitsThreads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int queries_per_pass(int nq) { return nq >= 8 ? 8 : nq >= 3 ? 4 : nq; }  // NQ in {1, 2, 4, 8}

// form: 0 by the shape table, 1 the VALU form, 2 the matrix-core form (the benchmark times both where both can serve)
bool mfma_serves(const mvdb_bits* ix, int nq, int form) {
    if (form) return form == 2;
    int min_nq = 9;
    (void)with_bits_shape(ix->nchunk, [&](auto sh) {
        min_nq = decltype(sh)::MFMA_MIN_NQ;
        return 0;
    });
    return nq >= min_nq;
}

// ---- workspaces (as cos8.hip) ----------------------------------------------------------------------------------------------
BitsWorkspace* ws_for_stream(const mvdb_bits* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    BitsWorkspace* ws = new BitsWorkspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

BitsWorkspace* ws_acquire(const mvdb_bits* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        BitsWorkspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    BitsWorkspace* ws = new BitsWorkspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

void ws_release(const mvdb_bits* ix, BitsWorkspace* ws) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    ix->idle.push_back(ws);
}

// Mutators hold the index exclusively; they wait for every stream a search of this index was enqueued on and for the private
// ones, and for nothing else (cos8.hip: quiesce — the same rule for a stream that is gone or being captured).
int quiesce(mvdb_bits* ix) {
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
    for (BitsWorkspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "bits search: the workspace of this stream is too small to capture this shape; run it "
                                  "once eagerly on the stream first");
    return b.reserve(n);
}

int grow(mvdb_bits* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "bits: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    uint8_t* r = nullptr;
    if (hipMalloc((void**)&r, (size_t)cap * ix->rb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVDB_ERR_OOM, "bits: cannot allocate %lld rows", (long long)cap);
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

// fp32 [n, d_bits] on the device -> packed rows at out (rows_dev == nullptr: consecutive from out; else row rows_dev[i] of out)
int pack_into(const mvdb_bits* ix, const float* x_dev, int64_t n, const int64_t* rows_dev, uint8_t* out, hipStream_t s) {
    if (n <= 0) return 0;
    constexpr int per_block = kBitsThreads / kWave;
    hipLaunchKernelGGL(bits_pack_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBitsThreads), 0, s, x_dev, n,
                       ix->d_bits, rows_dev, out);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// Everything on stream s, no synchronisation.  q_dev: packed [nq, rb]; mask_dev: nullptr or the bitmap, on the device.
int search_core(const mvdb_bits* ix, BitsWorkspace* ws, const uint8_t* q_dev, int nq, int k, const uint64_t* mask_dev,
                int form, int32_t* D, int64_t* I, bool capturing, hipStream_t s) {
    if (ix->n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(bits_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    int nblocks = 0;
    if (mfma_serves(ix, nq, form)) {
        // 32 queries per row read; more than 32 queries: slabs over grid.y
        int waves = 0, per_cu = 0;
        bits_mfma_block(ix->d_bits, k, &waves, &per_cu);
        const size_t lds = bits_mfma_lds_bytes(ix->d_bits, k, waves);
        MVDB_TRY(ensure_dynamic_lds((const void*)bits_mfma_kernel, lds, ix->device));
        nblocks = bits_grid(ix->n, 32, waves, per_cu, ix->device);
        MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
        BitsMfmaArgs a{ix->rows, ix->nchunk, ix->d_bits, ix->n, mask_dev, q_dev, nq, k, ws->cand.p};
        hipLaunchKernelGGL(bits_mfma_kernel, dim3((unsigned)nblocks, (unsigned)((nq + kBitsMfmaQ - 1) / kBitsMfmaQ)),
                           dim3(waves * kWave), lds, s, a);
        MVDB_HIP(hipGetLastError());
    } else {
        const int NQ = queries_per_pass(nq);
        MVDB_TRY(with_bits_shape(ix->nchunk, [&](auto sh) {
            using S = decltype(sh);
            nblocks = scan_blocks<S::G, S::U, S::BLOCKS>(ix->n, ix->device);
            MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
            BitsScanArgs a{ix->rows, ix->nchunk, ix->d_bits, ix->n, mask_dev, q_dev, nq, k, ws->cand.p};
            return launch_scan<S::G, S::U>(a, NQ, dim3((unsigned)nblocks, (unsigned)((nq + NQ - 1) / NQ)), s);
        }));
    }
    hipLaunchKernelGGL(bits_merge_kernel, dim3(nq), dim3(kBitsThreads), 0, s, ws->cand.p, nblocks, k, D, I);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int check_search(const mvdb_bits* ix, const void* q, int nq, int k, const void* D, const void* I) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "bits: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    return 0;
}

// host API: stage queries (and the bitmap), search on a private stream, one packed D2H, wait.  is_float: q_host is fp32 [nq, d_bits].
int search_host(const mvdb_bits* ix, const void* q_host, bool is_float, int nq, int k, const uint64_t* mask_host, int form,
                int32_t* D_host, int64_t* I_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, D_host, I_host));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    BitsWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "bits: cannot create a search workspace");
    struct Back {
        const mvdb_bits* ix;
        BitsWorkspace* ws;
        ~Back() { ws_release(ix, ws); }
    } back{ix, ws};
    const size_t qbytes = (size_t)nq * (is_float ? (size_t)ix->d_bits * sizeof(float) : (size_t)ix->rb);
    const size_t words = mask_host ? (size_t)((ix->n + 63) / 64) : 0, total = (size_t)nq * k;
    MVDB_TRY(ws->pin.reserve(qbytes + words * sizeof(uint64_t)));
    memcpy(ws->pin.p, q_host, qbytes);
    MVDB_TRY(ws->q.reserve((size_t)nq * ix->rb));
    if (is_float) {
        MVDB_TRY(ws->qf.reserve((size_t)nq * ix->d_bits));
        MVDB_HIP(hipMemcpyAsync(ws->qf.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
        MVDB_TRY(pack_into(ix, ws->qf.p, nq, nullptr, ws->q.p, ws->stream));
    } else {
        MVDB_HIP(hipMemcpyAsync(ws->q.p, ws->pin.p, qbytes, hipMemcpyHostToDevice, ws->stream));
    }
    const uint64_t* mask_dev = nullptr;
    if (words) {
        MVDB_TRY(ws->mask.reserve(words));
        memcpy((char*)ws->pin.p + qbytes, mask_host, words * sizeof(uint64_t));
        MVDB_HIP(hipMemcpyAsync(ws->mask.p, (char*)ws->pin.p + qbytes, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
        mask_dev = ws->mask.p;
    }
    MVDB_TRY(ws->out.reserve(total + (total + 1) / 2));
    int64_t* Io = ws->out.p;
    int32_t* Do = (int32_t*)(ws->out.p + total);
    MVDB_TRY(search_core(ix, ws, ws->q.p, nq, k, mask_dev, form, Do, Io, false, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(int32_t));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    memcpy(I_host, ws->pin_out.p, total * sizeof(int64_t));
    memcpy(D_host, (const char*)ws->pin_out.p + total * sizeof(int64_t), total * sizeof(int32_t));
    return 0;
}

int search_dev(const mvdb_bits* ix, const void* q_dev, bool is_float, int nq, int k, const uint64_t* mask_dev, int32_t* D_dev,
               int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, D_dev, I_dev));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    hipStream_t s = (hipStream_t)stream;
    BitsWorkspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "bits: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    const uint8_t* q = (const uint8_t*)q_dev;
    if (is_float) {
        MVDB_TRY(ws_reserve(ws->q, (size_t)nq * ix->rb, capturing));
        MVDB_TRY(pack_into(ix, (const float*)q_dev, nq, nullptr, ws->q.p, s));
        q = ws->q.p;
    }
    return search_core(ix, ws, q, nq, k, mask_dev, 0, D_dev, I_dev, capturing, s);
}

// ---- ingest ----------------------------------------------------------------------------------------------------------------
// rows appended from the host in chunks of at most 64 MiB: packed bytes straight to their place, fp32 through the pack kernel
int add_host(mvdb_bits* ix, const void* x_host, bool is_float, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x_host)) return fail(MVDB_ERR_ARG, "bad rows");
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t row_bytes = is_float ? (int64_t)ix->d_bits * 4 : ix->rb;
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    if (is_float) MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d_bits));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        const size_t bytes = (size_t)(m * row_bytes);
        uint8_t* dst = ix->rows + (ix->n + r0) * ix->rb;
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        memcpy(ix->pin.p, (const char*)x_host + r0 * row_bytes, bytes);
        MVDB_HIP(hipMemcpyAsync(is_float ? (void*)ix->stage.p : (void*)dst, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
        if (is_float) MVDB_TRY(pack_into(ix, ix->stage.p, m, nullptr, dst, ix->ms));
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int add_dev(mvdb_bits* ix, const void* x_dev, bool is_float, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x_dev)) return fail(MVDB_ERR_ARG, "bad rows");
    if (n == 0) return 0;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    uint8_t* dst = ix->rows + ix->n * ix->rb;
    if (is_float) MVDB_TRY(pack_into(ix, (const float*)x_dev, n, nullptr, dst, ix->ms));
    else MVDB_HIP(hipMemcpyAsync(dst, x_dev, (size_t)n * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int check_rows(const mvdb_bits* ix, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= ix->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)ix->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

// set_rows: the rows are staged on the device chunk by chunk, their row numbers with them; fp32 rows then go through the pack
// kernel to their places, packed rows through the scatter
int set_rows_entry(mvdb_bits* ix, const int64_t* rows_host, const void* x, bool is_float, bool x_on_device, int64_t m) {
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
    const int64_t row_bytes = is_float ? (int64_t)ix->d_bits * 4 : ix->rb;
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->stage_rows.reserve((size_t)chunk));
    if (!x_on_device) {
        MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
        if (is_float) MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d_bits));
        else MVDB_TRY(ix->stage_bits.reserve((size_t)chunk * ix->rb));
    }
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        const size_t bytes = (size_t)(rows * row_bytes);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        MVDB_HIP(hipMemcpyAsync(ix->stage_rows.p, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        const void* src = (const char*)x + i0 * row_bytes;
        if (!x_on_device) {
            void* staged = is_float ? (void*)ix->stage.p : (void*)ix->stage_bits.p;
            memcpy(ix->pin.p, src, bytes);
            MVDB_HIP(hipMemcpyAsync(staged, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
            src = staged;
        }
        if (is_float) {
            MVDB_TRY(pack_into(ix, (const float*)src, rows, ix->stage_rows.p, ix->rows, ix->ms));
        } else {
            const int64_t work = rows * ix->nchunk;
            hipLaunchKernelGGL(bits_scatter_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms,
                               (const uint8_t*)src, (const int64_t*)ix->stage_rows.p, rows, ix->nchunk, ix->rows);
            MVDB_HIP(hipGetLastError());
        }
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

}  // namespace

extern "C" {

int mvdb_bits_create(int d_bits, int device, mvdb_bits** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d_bits < 128 || d_bits > 128 * kBitsMaxChunks || d_bits % 128)
        return fail(MVDB_ERR_ARG, "bits: dimension %d is not a multiple of 128 in [128, %d]", d_bits, 128 * kBitsMaxChunks);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_bits* ix = new mvdb_bits();
    ix->d_bits = d_bits;
    ix->rb = d_bits / 8;
    ix->nchunk = ix->rb / 16;
    ix->device = device;
    if (hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess) {
        delete ix;
        return fail(MVDB_ERR_HIP, "bits: cannot create a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_bits_free(mvdb_bits* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (BitsWorkspace* ws : ix->pool) delete ws;
        if (ix->rows) (void)hipFree(ix->rows);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_bits_reset(mvdb_bits* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    return 0;
}

int mvdb_bits_reserve(mvdb_bits* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_bits_ntotal(const mvdb_bits* ix) { return ix ? ix->n : -1; }
int mvdb_bits_dim(const mvdb_bits* ix) { return ix ? ix->d_bits : -1; }

int mvdb_bits_geometry(const mvdb_bits* ix, int nq, int k, int* form, int64_t* stride_rows) {
    if (!ix || !form || !stride_rows) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0 || k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "bits geometry: bad nq or k");
    DeviceGuard g(ix->device);
    if (mfma_serves(ix, nq, 0)) {
        int waves = 0, per_cu = 0;
        bits_mfma_block(ix->d_bits, k, &waves, &per_cu);
        *form = 2;
        *stride_rows = (int64_t)device_cus(ix->device) * per_cu * waves * 32;
        return 0;
    }
    *form = 1;
    return with_bits_shape(ix->nchunk, [&](auto sh) {
        using S = decltype(sh);
        constexpr int tile = (kWave / S::G) * S::U;
        *stride_rows = (int64_t)scan_blocks<S::G, S::U, S::BLOCKS>(INT64_MAX / 2, ix->device) * (kBitsThreads / kWave) * tile;
        return 0;
    });
}

int mvdb_bits_add(mvdb_bits* ix, const uint8_t* x_host, int64_t n) { return add_host(ix, x_host, false, n); }
int mvdb_bits_add_device(mvdb_bits* ix, const uint8_t* x_dev, int64_t n) { return add_dev(ix, x_dev, false, n); }
int mvdb_bits_add_float(mvdb_bits* ix, const float* x_host, int64_t n) { return add_host(ix, x_host, true, n); }
int mvdb_bits_add_float_device(mvdb_bits* ix, const float* x_dev, int64_t n) { return add_dev(ix, x_dev, true, n); }

int mvdb_bits_get_rows(const mvdb_bits* ix, int64_t row0, int64_t n, uint8_t* rows_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows_host is NULL");
    MVDB_HIP(hipMemcpy(rows_host, ix->rows + row0 * ix->rb, (size_t)n * ix->rb, hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_bits_remove_rows(mvdb_bits* ix, const int64_t* rows_host, int64_t m) {
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
        int64_t* keep_dev = nullptr;
        uint8_t* tmp = nullptr;
        hipError_t e = hipMalloc((void**)&keep_dev, (size_t)kept * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void**)&tmp, (size_t)kept * ix->rb);
        if (e == hipSuccess)
            e = hipMemcpyAsync(keep_dev, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms);
        if (e == hipSuccess) {
            const int64_t work = kept * ix->nchunk;
            hipLaunchKernelGGL(bits_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, ix->rows,
                               keep_dev, kept, ix->nchunk, tmp);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(ix->rows + r0 * ix->rb, tmp, (size_t)kept * ix->rb, hipMemcpyDeviceToDevice, ix->ms);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->ms);
        if (keep_dev) (void)hipFree(keep_dev);
        if (tmp) (void)hipFree(tmp);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? MVDB_ERR_OOM : MVDB_ERR_HIP, "bits remove_rows: %s", hipGetErrorString(e));
    }
    ix->n -= m;
    return 0;
}

int mvdb_bits_set_rows(mvdb_bits* ix, const int64_t* rows_host, const uint8_t* x_host, int64_t m) {
    return set_rows_entry(ix, rows_host, x_host, false, false, m);
}
int mvdb_bits_set_rows_device(mvdb_bits* ix, const int64_t* rows_host, const uint8_t* x_dev, int64_t m) {
    return set_rows_entry(ix, rows_host, x_dev, false, true, m);
}
int mvdb_bits_set_rows_float(mvdb_bits* ix, const int64_t* rows_host, const float* x_host, int64_t m) {
    return set_rows_entry(ix, rows_host, x_host, true, false, m);
}
int mvdb_bits_set_rows_float_device(mvdb_bits* ix, const int64_t* rows_host, const float* x_dev, int64_t m) {
    return set_rows_entry(ix, rows_host, x_dev, true, true, m);
}

int mvdb_bits_search(const mvdb_bits* ix, const uint8_t* q_host, int nq, int k, const uint64_t* mask_host, int32_t* D_host,
                     int64_t* I_host) {
    return search_host(ix, q_host, false, nq, k, mask_host, 0, D_host, I_host);
}
int mvdb_bits_search_float(const mvdb_bits* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, int32_t* D_host,
                           int64_t* I_host) {
    return search_host(ix, q_host, true, nq, k, mask_host, 0, D_host, I_host);
}
int mvdb_bits_search_form(const mvdb_bits* ix, const uint8_t* q_host, int nq, int k, const uint64_t* mask_host, int form,
                          int32_t* D_host, int64_t* I_host) {
    if (form < 0 || form > 2) return fail(MVDB_ERR_ARG, "bits: form must be 0 (by the shape table), 1 (VALU) or 2 (matrix cores)");
    return search_host(ix, q_host, false, nq, k, mask_host, form, D_host, I_host);
}
int mvdb_bits_search_device(const mvdb_bits* ix, const uint8_t* q_dev, int nq, int k, const uint64_t* mask_dev, int32_t* D_dev,
                            int64_t* I_dev, void* stream) {
    return search_dev(ix, q_dev, false, nq, k, mask_dev, D_dev, I_dev, stream);
}
int mvdb_bits_search_float_device(const mvdb_bits* ix, const float* q_dev, int nq, int k, const uint64_t* mask_dev,
                                  int32_t* D_dev, int64_t* I_dev, void* stream) {
    return search_dev(ix, q_dev, true, nq, k, mask_dev, D_dev, I_dev, stream);
}

}  // extern "C"
