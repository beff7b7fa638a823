// mx.hip — C-ABI (include/mvdb.h "MX INDEX") of the microscaling index behind MXVectorDatabase: MXFP4 or MXFP8 rows on the
// device, scored against MXFP8 queries by v_mfma_scale_f32_16x16x128_f8f6f4.
//
// HBM layout: codes[cap, d * format / 8] as the host gives them, scales[cap, 4, S4] transposed per row (mx_kernels.hpp), rows
// [0, n) live.  d is a multiple of 128, so a row is whole 16-byte chunks and nothing but the scale plane is padded.  No fp32
// rows are kept and nothing is trained.  The host shape is sq4.hip's: workspaces per stream, exclusive mutators on a private
// stream, compacting removal through a staging copy.
#include <algorithm>
#include <map>
#include <shared_mutex>
#include <vector>

#include "common.hpp"
#include "mx_kernels.hpp"

using namespace mvdb;

namespace {

struct MxWorkspace {
    OwnedStream owned;       // (first: the buffers below are freed before it)
    hipStream_t stream = nullptr;
    DevBuf<float> qf;        // host API: the queries staged on the device
    DevBuf<uint8_t> q8;      // the MXFP8 queries: E4M3 bytes [nq, d]
    DevBuf<uint8_t> qs;      // their scale planes [nq, 4, S4]
    DevBuf<int> valid;
    DevBuf<uint64_t> mask;   // host API: the bitmap of this call
    DevBuf<uint64_t> cand;   // partial top-k lists
    DevBuf<uint64_t> keys;   // refined search: the segments' merged lists, the re-rank's candidates
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
    ~MxWorkspace() {
        for (void* p : retired) (void)hipFree(p);
    }
};

}  // namespace

struct mvdb_mx {
    int d = 0, fmt = 0, rb = 0, s4 = 0, sb = 0, device = 0;  // rb: code bytes per row; sb = 4 S4: scale bytes per row
    int64_t n = 0, cap = 0;
    uint8_t* codes = nullptr;
    uint8_t* scales = nullptr;
    hipStream_t ms = nullptr;  // mutators' private stream
    DevBuf<float> stage;       // fp32 rows of add / set_rows on their way to the encoder
    DevBuf<uint8_t> stage_codes, stage_scales;  // set_rows_codes: rows on their way to their places
    DevBuf<int64_t> stage_rows;
    PinnedBuf pin;
    mutable std::shared_mutex mu;
    mutable std::mutex ws_mu;
    mutable std::map<hipStream_t, MxWorkspace*> by_stream;  // device-API calls: one workspace per caller stream
    mutable std::vector<MxWorkspace*> pool, idle;           // host-API calls: private streams
    int nblk() const { return d / 32; }
};

namespace {

constexpr size_t kMxLdsPerCu = 160 * 1024;

// the grid rule of the row scans: tiles -> waves -> blocks, at most per_cu resident blocks per CU
int mx_grid(int64_t n, int rows_per_wave, int waves, int per_cu, int device) {
    const int64_t ntiles = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t want = (ntiles + waves - 1) / waves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}

// The block of a scan (sq4_mfma_block's rule).  Up to 16 queries of d <= 1024 keep their B operands in registers.  Otherwise
// QB = 1, 2 or 4 groups of 16 queries per row read: as many as the call has queries for and as fit the LDS beside FOUR waves'
// lists — a block of one or two waves on a CU reads its rows too slowly for the wider B to pay (d = 4096, k = 64: QB = 1).
// Then as many waves, up to 8, as the lists leave room for, two blocks of 4 waves where two fit the CU's 160 KiB.  QB and the
// tiles in flight (mx_kernels.hpp) are first guesses, not swept.
struct MxPlan {
    int QB = 1, waves = 1, per_cu = 1;
    bool reg = false;
    size_t lds = 0;
};
MxPlan mx_plan(int d, int k, int nq) {
    MxPlan p;
    p.reg = nq <= 16 && d / 128 <= kMxRegSteps;
    p.QB = nq > 32 ? 4 : nq > 16 ? 2 : 1;
    while (p.QB > 1 && mx_lds_bytes(d, k, p.QB, 4, false) > kMxLdsPerCu) p.QB >>= 1;
    int nw = 8;
    while (nw > 1 && mx_lds_bytes(d, k, p.QB, nw, p.reg) > kMxLdsPerCu) nw >>= 1;
    if (nw == 8 && mx_lds_bytes(d, k, p.QB, 4, p.reg) * 2 <= kMxLdsPerCu) nw = 4;
    p.waves = nw;
    p.lds = mx_lds_bytes(d, k, p.QB, nw, p.reg);
    p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(8 / nw, kMxLdsPerCu / p.lds));
    return p;
}
int mx_tile_rows(int fmt) { return fmt == 4 ? 64 : 32; }  // 16 T

template <int FMT, int QB, bool REG>
int launch_scan_as(const mvdb_mx* ix, const MxScanArgs& a, const MxPlan& p, int nblocks, hipStream_t s) {
    MVDB_TRY(ensure_dynamic_lds((const void*)mx_scan_kernel<FMT, QB, REG>, p.lds, ix->device));
    hipLaunchKernelGGL((mx_scan_kernel<FMT, QB, REG>), dim3((unsigned)nblocks, (unsigned)((a.nq + 16 * QB - 1) / (16 * QB))),
                       dim3(p.waves * kWave), p.lds, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}
template <int FMT>
int launch_scan(const mvdb_mx* ix, const MxScanArgs& a, const MxPlan& p, int nblocks, hipStream_t s) {
    if (p.reg) return launch_scan_as<FMT, 1, true>(ix, a, p, nblocks, s);
    if (p.QB == 1) return launch_scan_as<FMT, 1, false>(ix, a, p, nblocks, s);
    if (p.QB == 2) return launch_scan_as<FMT, 2, false>(ix, a, p, nblocks, s);
    return launch_scan_as<FMT, 4, false>(ix, a, p, nblocks, s);
}

// ---- workspaces (as sq4.hip) -----------------------------------------------------------------------------------------------
MxWorkspace* ws_for_stream(const mvdb_mx* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    auto it = ix->by_stream.find(s);
    if (it != ix->by_stream.end()) return it->second;
    MxWorkspace* ws = new MxWorkspace();
    if (ws->init(s, false) != 0) {
        delete ws;
        return nullptr;
    }
    ix->by_stream[s] = ws;
    return ws;
}

MxWorkspace* ws_acquire(const mvdb_mx* ix) {
    std::lock_guard<std::mutex> lk(ix->ws_mu);
    if (!ix->idle.empty()) {
        MxWorkspace* ws = ix->idle.back();
        ix->idle.pop_back();
        return ws;
    }
    MxWorkspace* ws = new MxWorkspace();
    if (ws->init(nullptr, true) != 0) {
        delete ws;
        return nullptr;
    }
    ix->pool.push_back(ws);
    return ws;
}

struct WsBack {
    const mvdb_mx* ix;
    MxWorkspace* ws;
    ~WsBack() {
        std::lock_guard<std::mutex> lk(ix->ws_mu);
        ix->idle.push_back(ws);
    }
};

// Mutators hold the index exclusively; they wait for every stream a search of this index was enqueued on and for the private
// ones, and for nothing else (bits.hip: quiesce).
int quiesce(mvdb_mx* ix) {
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
    for (MxWorkspace* ws : ix->pool) MVDB_HIP(hipStreamSynchronize(ws->stream));
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

template <typename T>
int ws_reserve(DevBuf<T>& b, size_t n, bool capturing) {
    if (n <= b.cap) return 0;
    if (capturing)
        return fail(MVDB_ERR_ARG, "mx search: the workspace of this stream is too small to capture this shape; run it once "
                                  "eagerly on the stream first");
    return b.reserve(n);
}

int grow(mvdb_mx* ix, int64_t need) {
    if (need >= (int64_t)UINT32_MAX)
        return fail(MVDB_ERR_ARG, "mx: at most %lld rows per index (row numbers are 32-bit in the top-k keys)",
                    (long long)UINT32_MAX - 1);
    if (need <= ix->cap) return 0;
    int64_t cap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
    cap = std::max<int64_t>(cap, 1024);
    uint8_t *c = nullptr, *sc = nullptr;
    if (hipMalloc((void**)&c, (size_t)cap * ix->rb) != hipSuccess || hipMalloc((void**)&sc, (size_t)cap * ix->sb) != hipSuccess) {
        (void)hipGetLastError();
        if (c) (void)hipFree(c);
        return fail(MVDB_ERR_OOM, "mx: cannot allocate %lld rows", (long long)cap);
    }
    if (ix->n) {
        MVDB_HIP(hipMemcpyAsync(c, ix->codes, (size_t)ix->n * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipMemcpyAsync(sc, ix->scales, (size_t)ix->n * ix->sb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    if (ix->codes) (void)hipFree(ix->codes);
    if (ix->scales) (void)hipFree(ix->scales);
    ix->codes = c;
    ix->scales = sc;
    ix->cap = cap;
    return 0;
}

// fp32 [n, d] on the device -> codes and scales (rows_dev == nullptr: consecutive from row `first`; else row rows_dev[i])
template <int FMT>
int launch_encode(const MxEncodeArgs& a, hipStream_t s) {
    constexpr int per_block = kMxThreads / kWave;
    hipLaunchKernelGGL(mx_encode_kernel<FMT>, dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(kMxThreads), 0, s, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}
int encode_into(const mvdb_mx* ix, const float* x_dev, int64_t n, const int64_t* rows_dev, int64_t first, hipStream_t s) {
    if (n <= 0) return 0;
    MxEncodeArgs a{x_dev, n, ix->d, rows_dev, ix->codes + first * ix->rb, ix->scales + first * ix->sb, nullptr};
    return ix->fmt == 4 ? launch_encode<4>(a, s) : launch_encode<8>(a, s);
}

// host scale rows [m, d / 32] <-> transposed rows [m, 4, S4] (the pad is zero)
void transpose_scales(const mvdb_mx* ix, const uint8_t* nat, int64_t m, uint8_t* tr) {
    memset(tr, 0, (size_t)m * ix->sb);
    for (int64_t r = 0; r < m; ++r)
        for (int b = 0; b < ix->nblk(); ++b) tr[r * ix->sb + mx_scale_slot(b, ix->s4)] = nat[r * ix->nblk() + b];
}
void untranspose_scales(const mvdb_mx* ix, const uint8_t* tr, int64_t m, uint8_t* nat) {
    for (int64_t r = 0; r < m; ++r)
        for (int b = 0; b < ix->nblk(); ++b) nat[r * ix->nblk() + b] = tr[r * ix->sb + mx_scale_slot(b, ix->s4)];
}

// an E8M0 NaN scale, or an E4M3 NaN element, is no stored value
int check_codes(const mvdb_mx* ix, const uint8_t* codes, const uint8_t* scales, int64_t m) {
    for (int64_t i = 0; i < m * ix->nblk(); ++i)
        if (scales[i] == 0xFF)
            return fail(MVDB_ERR_ARG, "mx: the scale of block %lld of row %lld is 0xFF (E8M0 NaN)", (long long)(i % ix->nblk()),
                        (long long)(i / ix->nblk()));
    if (ix->fmt == 8)
        for (int64_t i = 0; i < m * ix->rb; ++i)
            if ((codes[i] & 0x7F) == 0x7F)
                return fail(MVDB_ERR_ARG, "mx: element %lld of row %lld is an E4M3 NaN", (long long)(i % ix->rb),
                            (long long)(i / ix->rb));
    return 0;
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// the call's MXFP8 queries, one launch of the rows' encoder: q_dev [nq, d] -> ws->q8, ws->qs, ws->valid
int build_queries(const mvdb_mx* ix, MxWorkspace* ws, const float* q_dev, int nq, bool capturing, hipStream_t s) {
    MVDB_TRY(ws_reserve(ws->q8, (size_t)nq * ix->d, capturing));
    MVDB_TRY(ws_reserve(ws->qs, (size_t)nq * ix->sb, capturing));
    MVDB_TRY(ws_reserve(ws->valid, (size_t)nq, capturing));
    return launch_encode<8>(MxEncodeArgs{q_dev, nq, ix->d, nullptr, ws->q8.p, ws->qs.p, ws->valid.p}, s);
}

// Everything on stream s, no synchronisation.  q_dev: fp32 [nq, d]; mask_dev: nullptr or the bitmap, on the device.
int search_core(const mvdb_mx* ix, MxWorkspace* ws, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D,
                int64_t* I, bool capturing, hipStream_t s) {
    if (ix->n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(mx_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D, I, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    MVDB_TRY(build_queries(ix, ws, q_dev, nq, capturing, s));
    const MxPlan p = mx_plan(ix->d, k, nq);
    const int nblocks = mx_grid(ix->n, mx_tile_rows(ix->fmt), p.waves, p.per_cu, ix->device);
    MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * k, capturing));
    MxScanArgs a{ix->codes, ix->scales, ix->d, ix->n, mask_dev, ws->q8.p, ws->qs.p, nq, k, ws->cand.p};
    MVDB_TRY(ix->fmt == 4 ? launch_scan<4>(ix, a, p, nblocks, s) : launch_scan<8>(ix, a, p, nblocks, s));
    hipLaunchKernelGGL(mx_merge_kernel, dim3(nq), dim3(kMxThreads), 0, s, ws->cand.p, nblocks, k, ws->valid.p, D, I);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// The refined search (include/mvdb.h: the candidate rule): the rows in S segments of L, a scan and a merge per segment through
// the one partial-list buffer — the stream orders them —, each merge leaving its f keys in the query's candidate list, then the
// refine store's re-rank over those lists where they lie.
int refined_core(const mvdb_mx* ix, const mvdb_refine* st, MxWorkspace* ws, const float* q_dev, int nq, int k, int fetch_k,
                 const uint64_t* mask_dev, float* D, int64_t* I, bool capturing, hipStream_t s) {
    if (ix->n == 0) return search_core(ix, ws, q_dev, nq, k, mask_dev, D, I, capturing, s);
    const int S = (fetch_k + 63) / 64, f = (fetch_k + S - 1) / S;
    const int64_t L = 64 * ((ix->n + 64ll * S - 1) / (64ll * S));
    MVDB_TRY(build_queries(ix, ws, q_dev, nq, capturing, s));
    const MxPlan p = mx_plan(ix->d, f, nq);
    const int nblocks = mx_grid(std::min(L, ix->n), mx_tile_rows(ix->fmt), p.waves, p.per_cu, ix->device);
    MVDB_TRY(ws_reserve(ws->cand, (size_t)nq * nblocks * f, capturing));
    MVDB_TRY(ws_reserve(ws->keys, (size_t)nq * S * f, capturing));
    for (int seg = 0; seg < S; ++seg) {
        const int64_t r0 = seg * L;
        const int64_t rows = std::min(ix->n, r0 + L) - r0;
        if (rows > 0) {
            MxScanArgs a{ix->codes + r0 * ix->rb, ix->scales + r0 * ix->sb, ix->d, rows, mask_dev ? mask_dev + r0 / 64 : nullptr,
                         ws->q8.p, ws->qs.p, nq, f, ws->cand.p, r0};
            MVDB_TRY(ix->fmt == 4 ? launch_scan<4>(ix, a, p, nblocks, s) : launch_scan<8>(ix, a, p, nblocks, s));
        }
        hipLaunchKernelGGL(mx_merge_keys_kernel, dim3(nq), dim3(kMxThreads), 0, s, ws->cand.p, rows > 0 ? nblocks : 0, f,
                           ws->valid.p, seg, S, ws->keys.p);
        MVDB_HIP(hipGetLastError());
    }
    return refine_rerank_keys(st, q_dev, nq, ws->keys.p, S * f, k, D, I, s);
}

int check_search(const mvdb_mx* ix, const void* q, int nq, int k, const void* D, const void* I) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "mx: k must be in [1, %d] (got %d)", kMaxFusedK, k);
    return 0;
}

int check_refined(const mvdb_mx* ix, const mvdb_refine* st, int k, int fetch_k) {
    if (!st) return fail(MVDB_ERR_ARG, "the refine store is NULL");
    if (fetch_k < k || fetch_k > 1024) return fail(MVDB_ERR_ARG, "mx: fetch_k must be in [k, 1024] (got %d, k = %d)", fetch_k, k);
    if (mvdb_refine_dim(st) != ix->d || mvdb_refine_ntotal(st) != ix->n)
        return fail(MVDB_ERR_ARG, "mx: the refine store holds %lld rows of %d dimensions, the index %lld of %d",
                    (long long)mvdb_refine_ntotal(st), mvdb_refine_dim(st), (long long)ix->n, ix->d);
    return 0;
}

// host queries -> ws->qf on the workspace's stream (and the bitmap -> ws->mask behind them in the same pinned buffer)
int stage_queries(const mvdb_mx* ix, MxWorkspace* ws, const float* q_host, int nq, const uint64_t* mask_host,
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

// ---- ingest ----------------------------------------------------------------------------------------------------------------
int check_mutation(const mvdb_mx* ix, const void* x, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || (n > 0 && !x)) return fail(MVDB_ERR_ARG, "bad rows");
    return 0;
}

// rows appended from the host in chunks of at most 64 MiB: fp32 through the encoder; codes straight to their place, their
// scales transposed in the pinned buffer on the way
int add_host(mvdb_mx* ix, const float* x_host, const uint8_t* codes_host, const uint8_t* scales_host, int64_t n) {
    const bool is_float = x_host != nullptr;
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (n == 0) return 0;
    if (!is_float) MVDB_TRY(check_codes(ix, codes_host, scales_host, n));
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    const int64_t row_bytes = is_float ? (int64_t)ix->d * 4 : ix->rb + ix->sb;
    const int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    if (is_float) MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        const int64_t at = ix->n + r0;
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        if (is_float) {
            const size_t bytes = (size_t)m * ix->d * 4;
            memcpy(ix->pin.p, x_host + r0 * ix->d, bytes);
            MVDB_HIP(hipMemcpyAsync(ix->stage.p, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
            MVDB_TRY(encode_into(ix, ix->stage.p, m, nullptr, at, ix->ms));
        } else {
            uint8_t* pc = (uint8_t*)ix->pin.p;
            uint8_t* ps = pc + m * ix->rb;
            memcpy(pc, codes_host + r0 * ix->rb, (size_t)m * ix->rb);
            transpose_scales(ix, scales_host + r0 * ix->nblk(), m, ps);
            MVDB_HIP(hipMemcpyAsync(ix->codes + at * ix->rb, pc, (size_t)m * ix->rb, hipMemcpyHostToDevice, ix->ms));
            MVDB_HIP(hipMemcpyAsync(ix->scales + at * ix->sb, ps, (size_t)m * ix->sb, hipMemcpyHostToDevice, ix->ms));
        }
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int check_rows(const mvdb_mx* ix, const int64_t* rows_host, int64_t m, std::vector<int64_t>* sorted) {
    sorted->assign(rows_host, rows_host + m);
    std::sort(sorted->begin(), sorted->end());
    for (int64_t i = 0; i < m; ++i) {
        const int64_t r = (*sorted)[i];
        if (r < 0 || r >= ix->n) return fail(MVDB_ERR_ARG, "row %lld out of range [0, %lld)", (long long)r, (long long)ix->n);
        if (i && r == (*sorted)[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)r);
    }
    return 0;
}

int launch_move(const mvdb_mx* ix, const uint8_t* src_codes, const uint8_t* src_scales, const int64_t* from, const int64_t* to,
                int64_t m, uint8_t* dst_codes, uint8_t* dst_scales) {
    const int cchunk = ix->rb / 16, schunk = ix->sb / 16;
    const int64_t work = m * (cchunk + schunk);
    hipLaunchKernelGGL(mx_move_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ix->ms, src_codes, src_scales, from, to,
                       m, cchunk, schunk, dst_codes, dst_scales);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// set_rows: the rows are staged on the device chunk by chunk, their row numbers with them; fp32 rows then go through the
// encoder to their places, coded rows through the scatter
int set_rows_host(mvdb_mx* ix, const int64_t* rows_host, const float* x_host, const uint8_t* codes_host,
                  const uint8_t* scales_host, int64_t m) {
    const bool is_float = x_host != nullptr;
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    if (!x_host && !(codes_host && scales_host)) return fail(MVDB_ERR_ARG, "the new rows are NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    {   // validate first, write after
        std::vector<int64_t> v;
        MVDB_TRY(check_rows(ix, rows_host, m, &v));
        if (!is_float) MVDB_TRY(check_codes(ix, codes_host, scales_host, m));
    }
    MVDB_TRY(quiesce(ix));
    const int64_t row_bytes = is_float ? (int64_t)ix->d * 4 : ix->rb + ix->sb;
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (64ll << 20) / row_bytes));
    MVDB_TRY(ix->stage_rows.reserve((size_t)chunk));
    MVDB_TRY(ix->pin.reserve((size_t)(chunk * row_bytes)));
    if (is_float) {
        MVDB_TRY(ix->stage.reserve((size_t)chunk * ix->d));
    } else {
        MVDB_TRY(ix->stage_codes.reserve((size_t)chunk * ix->rb));
        MVDB_TRY(ix->stage_scales.reserve((size_t)chunk * ix->sb));
    }
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        MVDB_HIP(hipStreamSynchronize(ix->ms));  // the staging buffers are reused
        MVDB_HIP(hipMemcpyAsync(ix->stage_rows.p, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        if (is_float) {
            const size_t bytes = (size_t)rows * ix->d * 4;
            memcpy(ix->pin.p, x_host + i0 * ix->d, bytes);
            MVDB_HIP(hipMemcpyAsync(ix->stage.p, ix->pin.p, bytes, hipMemcpyHostToDevice, ix->ms));
            MVDB_TRY(encode_into(ix, ix->stage.p, rows, ix->stage_rows.p, 0, ix->ms));
        } else {
            uint8_t* pc = (uint8_t*)ix->pin.p;
            uint8_t* ps = pc + rows * ix->rb;
            memcpy(pc, codes_host + i0 * ix->rb, (size_t)rows * ix->rb);
            transpose_scales(ix, scales_host + i0 * ix->nblk(), rows, ps);
            MVDB_HIP(hipMemcpyAsync(ix->stage_codes.p, pc, (size_t)rows * ix->rb, hipMemcpyHostToDevice, ix->ms));
            MVDB_HIP(hipMemcpyAsync(ix->stage_scales.p, ps, (size_t)rows * ix->sb, hipMemcpyHostToDevice, ix->ms));
            MVDB_TRY(launch_move(ix, ix->stage_codes.p, ix->stage_scales.p, nullptr, ix->stage_rows.p, rows, ix->codes, ix->scales));
        }
    }
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    return 0;
}

}  // namespace

extern "C" {

int mvdb_mx_create(int d, int format, int device, mvdb_mx** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (format != 4 && format != 8) return fail(MVDB_ERR_ARG, "mx: format %d is neither 4 (MXFP4) nor 8 (MXFP8)", format);
    if (d < 128 || d > kMxMaxDim || d % 128)
        return fail(MVDB_ERR_ARG, "mx: dimension %d is not a multiple of 128 in [128, %d]", d, kMxMaxDim);
    MVDB_TRY(ensure_device(device));
    DeviceGuard g(device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", device);
    mvdb_mx* ix = new mvdb_mx();
    ix->d = d;
    ix->fmt = format;
    ix->rb = mx_row_bytes(d, format);
    ix->s4 = mx_s4(d);
    ix->sb = 4 * ix->s4;
    ix->device = device;
    if (hipStreamCreateWithFlags(&ix->ms, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        delete ix;
        return fail(MVDB_ERR_HIP, "mx: cannot create a stream");
    }
    *out = ix;
    return 0;
}

int mvdb_mx_free(mvdb_mx* ix) {
    if (!ix) return 0;
    DeviceGuard g(ix->device);
    {
        std::unique_lock<std::shared_mutex> lk(ix->mu);
        if (quiesce(ix) != 0) (void)hipDeviceSynchronize();
        for (auto& kv : ix->by_stream) delete kv.second;
        for (MxWorkspace* ws : ix->pool) delete ws;
        if (ix->codes) (void)hipFree(ix->codes);
        if (ix->scales) (void)hipFree(ix->scales);
        if (ix->ms) (void)hipStreamDestroy(ix->ms);
    }
    delete ix;  // (the staging buffers it owns go here, still on the index's device)
    return 0;
}

int mvdb_mx_reset(mvdb_mx* ix) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    ix->n = 0;
    return 0;
}

int mvdb_mx_reserve(mvdb_mx* ix, int64_t n) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    MVDB_TRY(quiesce(ix));
    return grow(ix, n);
}

int64_t mvdb_mx_ntotal(const mvdb_mx* ix) { return ix ? ix->n : -1; }
int mvdb_mx_dim(const mvdb_mx* ix) { return ix ? ix->d : -1; }
int mvdb_mx_format(const mvdb_mx* ix) { return ix ? ix->fmt : -1; }

int mvdb_mx_geometry(const mvdb_mx* ix, int nq, int k, int* queries_per_read, int64_t* stride_rows) {
    if (!ix || !queries_per_read || !stride_rows) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0 || k <= 0 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "mx geometry: bad nq or k");
    DeviceGuard g(ix->device);
    const MxPlan p = mx_plan(ix->d, k, nq);
    *queries_per_read = 16 * p.QB;
    *stride_rows = (int64_t)device_cus(ix->device) * p.per_cu * p.waves * mx_tile_rows(ix->fmt);
    return 0;
}

int mvdb_mx_add(mvdb_mx* ix, const float* x_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_host, n));
    return n ? add_host(ix, x_host, nullptr, nullptr, n) : 0;
}

int mvdb_mx_add_codes(mvdb_mx* ix, const uint8_t* codes_host, const uint8_t* scales_host, int64_t n) {
    MVDB_TRY(check_mutation(ix, codes_host, n));
    MVDB_TRY(check_mutation(ix, scales_host, n));
    return n ? add_host(ix, nullptr, codes_host, scales_host, n) : 0;
}

int mvdb_mx_add_device(mvdb_mx* ix, const float* x_dev, int64_t n) {
    MVDB_TRY(check_mutation(ix, x_dev, n));
    DeviceGuard g(ix->device);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (n == 0) return 0;
    MVDB_TRY(quiesce(ix));
    MVDB_TRY(grow(ix, ix->n + n));
    MVDB_TRY(encode_into(ix, x_dev, n, nullptr, ix->n, ix->ms));
    MVDB_HIP(hipStreamSynchronize(ix->ms));
    ix->n += n;
    return 0;
}

int mvdb_mx_get_codes(const mvdb_mx* ix, int64_t row0, int64_t n, uint8_t* codes_host, uint8_t* scales_host) {
    if (!ix) return fail(MVDB_ERR_ARG, "index is NULL");
    DeviceGuard g(ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (row0 < 0 || n < 0 || row0 + n > ix->n)
        return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0, %lld)", (long long)row0, (long long)(row0 + n),
                    (long long)ix->n);
    if (n == 0) return 0;
    if (!codes_host || !scales_host) return fail(MVDB_ERR_ARG, "codes_host or scales_host is NULL");
    std::vector<uint8_t> tr((size_t)n * ix->sb);
    MVDB_HIP(hipMemcpy(codes_host, ix->codes + row0 * ix->rb, (size_t)n * ix->rb, hipMemcpyDeviceToHost));
    MVDB_HIP(hipMemcpy(tr.data(), ix->scales + row0 * ix->sb, tr.size(), hipMemcpyDeviceToHost));
    untranspose_scales(ix, tr.data(), n, scales_host);
    return 0;
}

int mvdb_mx_remove_rows(mvdb_mx* ix, const int64_t* rows_host, int64_t m) {
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
        DevBuf<uint8_t> tc, ts;
        MVDB_TRY(keep_dev.reserve((size_t)kept));
        MVDB_TRY(tc.reserve((size_t)kept * ix->rb));
        MVDB_TRY(ts.reserve((size_t)kept * ix->sb));
        MVDB_HIP(hipMemcpyAsync(keep_dev.p, keep.data(), (size_t)kept * sizeof(int64_t), hipMemcpyHostToDevice, ix->ms));
        MVDB_TRY(launch_move(ix, ix->codes, ix->scales, keep_dev.p, nullptr, kept, tc.p, ts.p));
        MVDB_HIP(hipMemcpyAsync(ix->codes + r0 * ix->rb, tc.p, (size_t)kept * ix->rb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipMemcpyAsync(ix->scales + r0 * ix->sb, ts.p, (size_t)kept * ix->sb, hipMemcpyDeviceToDevice, ix->ms));
        MVDB_HIP(hipStreamSynchronize(ix->ms));
    }
    ix->n -= m;
    return 0;
}

int mvdb_mx_set_rows(mvdb_mx* ix, const int64_t* rows_host, const float* x_host, int64_t m) {
    if (m > 0 && !x_host) return fail(MVDB_ERR_ARG, "x is NULL");
    return set_rows_host(ix, rows_host, x_host, nullptr, nullptr, m);
}
int mvdb_mx_set_rows_codes(mvdb_mx* ix, const int64_t* rows_host, const uint8_t* codes_host, const uint8_t* scales_host,
                           int64_t m) {
    if (m > 0 && !(codes_host && scales_host)) return fail(MVDB_ERR_ARG, "codes or scales is NULL");
    return set_rows_host(ix, rows_host, nullptr, codes_host, scales_host, m);
}

int mvdb_mx_query(const mvdb_mx* ix, const float* q_host, int nq, uint8_t* q8_host, uint8_t* scales_host) {
    if (!ix || !q_host || !q8_host || !scales_host) return fail(MVDB_ERR_ARG, "NULL argument");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    MxWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "mx: cannot create a search workspace");
    WsBack back{ix, ws};
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, nullptr, nullptr));
    MVDB_TRY(build_queries(ix, ws, ws->qf.p, nq, false, ws->stream));
    std::vector<uint8_t> tr((size_t)nq * ix->sb);
    MVDB_HIP(hipMemcpyAsync(q8_host, ws->q8.p, (size_t)nq * ix->d, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipMemcpyAsync(tr.data(), ws->qs.p, tr.size(), hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    untranspose_scales(ix, tr.data(), nq, scales_host);  // the scan's order -> natural block order
    return 0;
}

}  // extern "C"

namespace {

// host API: stage the queries (and the bitmap), search on a private stream, one packed D2H, wait.  st: nullptr, or the refine
// store of a refined search.
int search_host(const mvdb_mx* ix, const mvdb_refine* st, const float* q_host, int nq, int k, int fetch_k,
                const uint64_t* mask_host, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_search(ix, q_host, nq, k, D_host, I_host));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (fetch_k) MVDB_TRY(check_refined(ix, st, k, fetch_k));
    MxWorkspace* ws = ws_acquire(ix);
    if (!ws) return fail(MVDB_ERR_HIP, "mx: cannot create a search workspace");
    WsBack back{ix, ws};
    const uint64_t* mask_dev = nullptr;
    MVDB_TRY(stage_queries(ix, ws, q_host, nq, mask_host, &mask_dev));
    const size_t total = (size_t)nq * k;
    MVDB_TRY(ws->out.reserve(total + total / 2 + 1));  // I: total int64; D: total floats
    int64_t* Io = ws->out.p;
    float* Do = (float*)(ws->out.p + total);
    if (fetch_k) MVDB_TRY(refined_core(ix, st, ws, ws->qf.p, nq, k, fetch_k, mask_dev, Do, Io, false, ws->stream));
    else MVDB_TRY(search_core(ix, ws, ws->qf.p, nq, k, mask_dev, Do, Io, false, ws->stream));
    const size_t bytes = total * (sizeof(int64_t) + sizeof(float));
    MVDB_TRY(ws->pin_out.reserve(bytes));
    MVDB_HIP(hipMemcpyAsync(ws->pin_out.p, ws->out.p, bytes, hipMemcpyDeviceToHost, ws->stream));
    MVDB_HIP(hipStreamSynchronize(ws->stream));
    memcpy(I_host, ws->pin_out.p, total * sizeof(int64_t));
    memcpy(D_host, (const char*)ws->pin_out.p + total * sizeof(int64_t), total * sizeof(float));
    return 0;
}

int search_device(const mvdb_mx* ix, const mvdb_refine* st, const float* q_dev, int nq, int k, int fetch_k,
                  const uint64_t* mask_dev, float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search(ix, q_dev, nq, k, D_dev, I_dev));
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(MVDB_ERR_HIP, "cannot select device %d", ix->device);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (fetch_k) MVDB_TRY(check_refined(ix, st, k, fetch_k));
    hipStream_t s = (hipStream_t)stream;
    MxWorkspace* ws = ws_for_stream(ix, s);
    if (!ws) return fail(MVDB_ERR_HIP, "mx: cannot create a search workspace");
    std::lock_guard<std::mutex> use(ws->use_mu);
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    const bool capturing = s && hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive;
    if (capturing) ws->captured = true;
    RetireScope keep_old(ws->captured ? &ws->retired : nullptr);
    if (fetch_k) return refined_core(ix, st, ws, q_dev, nq, k, fetch_k, mask_dev, D_dev, I_dev, capturing, s);
    return search_core(ix, ws, q_dev, nq, k, mask_dev, D_dev, I_dev, capturing, s);
}

}  // namespace

extern "C" {

int mvdb_mx_search(const mvdb_mx* ix, const float* q_host, int nq, int k, const uint64_t* mask_host, float* D_host,
                   int64_t* I_host) {
    return search_host(ix, nullptr, q_host, nq, k, 0, mask_host, D_host, I_host);
}

int mvdb_mx_search_device(const mvdb_mx* ix, const float* q_dev, int nq, int k, const uint64_t* mask_dev, float* D_dev,
                          int64_t* I_dev, void* stream) {
    return search_device(ix, nullptr, q_dev, nq, k, 0, mask_dev, D_dev, I_dev, stream);
}

int mvdb_mx_search_refined(const mvdb_mx* ix, const mvdb_refine* st, const float* q_host, int nq, int k, int fetch_k,
                           const uint64_t* mask_host, float* D_host, int64_t* I_host) {
    if (fetch_k <= 0) return fail(MVDB_ERR_ARG, "mx: fetch_k must be in [k, 1024] (got %d)", fetch_k);
    return search_host(ix, st, q_host, nq, k, fetch_k, mask_host, D_host, I_host);
}

int mvdb_mx_search_refined_device(const mvdb_mx* ix, const mvdb_refine* st, const float* q_dev, int nq, int k, int fetch_k,
                                  const uint64_t* mask_dev, float* D_dev, int64_t* I_dev, void* stream) {
    if (fetch_k <= 0) return fail(MVDB_ERR_ARG, "mx: fetch_k must be in [k, 1024] (got %d)", fetch_k);
    return search_device(ix, st, q_dev, nq, k, fetch_k, mask_dev, D_dev, I_dev, stream);
}

}  // extern "C"
