// mvdb.hip — C-ABI (include/mvdb.h) of the flat index: host orchestration + kernel launches.
//
// HBM layout of an index: ONE row-major fp32 matrix X[cap, ld], ld = d rounded up to a multiple
// of 4 floats so that every row starts on a 16-byte boundary and is read as whole dwordx4 chunks;
// the padding is zero.  Rows [0, n) are live.  Nothing else of the corpus lives on the device
// (ids / metadata stay in the Python host layer, as in the reference).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <tuple>
#include <vector>
#include <shared_mutex>

#include "common.hpp"
#include "index_state.hpp"
#include "scan_kernels.hpp"
#include "grouped_scan.hpp"
#include "range_scan.hpp"
#include "join_scan.hpp"
#include "mmr_select.hpp"
#include "distinct_select.hpp"
#include "group_hits.hpp"
#include "maxsim_scan.hpp"
#include "assign_scan.hpp"
#include "examples_scan.hpp"
#include "boost_scan.hpp"
#include "sparse_scan.hpp"
#include "sparse_postings.hpp"
#include "probe_scan.hpp"
#include "code8_scan.hpp"
#include "scan_mfma_kernels.hpp"
#include "select_kernels.hpp"
#include "half_scan.hpp"
#include "util_kernels.hpp"

using namespace mvdb;

// ================================================================================================
// errors / device helpers / profiling
// ================================================================================================
namespace mvdb {

int launch_merge_di_sort(int metric, int nlists, int nq, int k, const float* D, int64_t strideD, const int64_t* I,
                         int64_t strideI, float* Dout, int64_t* Iout, int device, hipStream_t stream);  // collective.hip

static thread_local char g_err[512] = "";
thread_local std::vector<void*>* tls_retire = nullptr;

Knobs read_knobs() {
    Knobs k;
    k.scan_blocks_per_cu = env_int("MVDB_SCAN_BLOCKS_PER_CU", 0);
    k.mfma_blocks_per_cu = env_int("MVDB_MFMA_BLOCKS_PER_CU", 0);
    k.mfma_stage = env_int("MVDB_MFMA_STAGE", 16);
    k.mfma_ng2 = env_int("MVDB_MFMA_NG2", -1);
    k.gemm_scan_min_nq = env_int("MVDB_GEMM_SCAN_MIN_NQ", 104);
    k.gemm_scan_blocks_per_cu = env_int("MVDB_GEMM_SCAN_BLOCKS_PER_CU", 2);
    k.split_scan_min_nq = env_int("MVDB_SPLIT_SCAN_MIN_NQ", -1);
    k.half_phase_growth = env_int("MVDB_HALF_PHASE_GROWTH", 0);   // 0: by the pass width (launch_half_pass)
    k.half_last_growth = env_int("MVDB_HALF_LAST_GROWTH", 0);
    k.split_stats = env_int("MVDB_SPLIT_STATS", 0) != 0;
    k.disable_mfma_scan = env_int("MVDB_DISABLE_MFMA_SCAN", 0) != 0;
    k.disable_l2_mfma = env_int("MVDB_DISABLE_L2_MFMA", 0) != 0;
    k.disable_gemm_scan = env_int("MVDB_DISABLE_GEMM_SCAN", 0) != 0;
    k.disable_split_scan = env_int("MVDB_DISABLE_SPLIT_SCAN", 0) != 0;
    k.disable_half_scan = env_int("MVDB_DISABLE_HALF_SCAN", 0) != 0;
    k.disable_rerun_floor = env_int("MVDB_DISABLE_RERUN_FLOOR", 0) != 0;
    k.disable_rescue = env_int("MVDB_DISABLE_RESCUE", 0) != 0;
    k.disable_tile_skip = env_int("MVDB_DISABLE_TILE_SKIP", 0) != 0;
    k.tile_flag_min_tiles = env_int("MVDB_TILE_FLAG_MIN_TILES", 12288);
    k.tile_flags_mode = env_int("MVDB_TILE_FLAGS", -1);
    k.disable_masked_batch = env_int("MVDB_DISABLE_MASKED_BATCH", 0) != 0;
    k.disable_l2_cert = env_int("MVDB_DISABLE_L2_CERT", 0) != 0;
    k.disable_half_shadow = env_int("MVDB_DISABLE_HALF_SHADOW", 0) != 0;
    k.shadow_single_query = env_int("MVDB_SHADOW_SINGLE_QUERY", 0) != 0;
    k.grouped_items_per_cu = env_int("MVDB_GROUPED_ITEMS_PER_CU", 0);
    k.grouped_min_batches = std::max(1, env_int("MVDB_GROUPED_MIN_BATCHES", 4));
    if (const char* v = getenv("MVDB_COMPACT_BYTES"))
        if (*v) k.compact_bytes = std::max(1ll, atoll(v));
    k.compact_inplace = env_int("MVDB_COMPACT_INPLACE", 1) != 0;
    k.code8_seed_blocks = env_int("MVDB_CODE8_SEED_BLOCKS", 0);
    k.code8_seed_threads = env_int("MVDB_CODE8_SEED_THREADS", 0);
    k.code8_rescore_rows = env_int("MVDB_CODE8_RESCORE_ROWS", 0);
    k.code8_front_u = env_int("MVDB_CODE8_FRONT_U", 0);
    k.code8_handoff = env_int("MVDB_CODE8_HANDOFF", 0);
    k.code8_ring = env_int("MVDB_CODE8_RING", 0);
    return k;
}

int cached_occupancy(const void* kern, int threads, size_t lds, int dflt) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, size_t, int, int>, int> cache;  // (kernel, dynamic LDS, threads, current device)
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(kern, lds, threads, dev);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess || nb <= 0) nb = dflt;
    cache[key] = nb;
    return nb;
}

// Raises a kernel's dynamic-LDS limit once per (kernel, device): the attribute is per device, and one process may
// hold indexes on several GPUs.  No size is exempt: kernels with 32 KiB of static lists on top of a 32 - 48 KiB ring
// (half_scan.hip) have always had it set.
int ensure_dynamic_lds(const void* kern, size_t lds, int device) {
    if (lds == 0) return 0;
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> done;
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = done[{kern, device}];
    if (lds > have) {
        MVDB_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        have = lds;
    }
    return 0;
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int ensure_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MVDB_ERR_NODEVICE, "no HIP device available (%s); libmvdb has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n)
        return fail(MVDB_ERR_ARG, "device ordinal %d out of range [0,%d)", device, n);
    return 0;
}

int device_cus(int device) {
    static std::mutex mu;
    static std::map<int, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(device);
    if (it != cache.end()) return it->second;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        cus <= 0)
        cus = 256;
    cache[device] = cus;
    return cus;
}

// The profiler's events and pairs live in pools that only grow: a launch takes a free pair and free events (created on first
// use only), and mvdb_prof_read or an off -> on of mvdb_prof_enable gives them back — no event, map node or string is made per
// launch.  A pair's index is the bracket's ticket.  An event is counted: a bracket of a ProfChain begins at the stop event of
// the bracket before it, which must outlive that bracket's own pair.
struct ProfEvent {
    hipEvent_t ev = nullptr;
    int device = 0;  // the device that was current when it was created: the launching object's
    int refs = 0;
};
struct ProfPair {
    int a = -1, b = -1;                      // indices into g_prof_ev
    int label = -1;                          // index into g_prof_labels
    enum { kFree, kOpen, kClosed } state = kFree;
};
struct ProfLabel {
    std::string name;
    int held = 0;  // pairs of this label that are open or unread
};
constexpr int kProfLabelCap = MVDB_PROF_LABEL_CAP;
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfEvent> g_prof_ev;
static std::vector<ProfPair> g_prof;
static std::vector<int> g_prof_ev_free, g_prof_free;
static std::vector<ProfLabel> g_prof_labels;  // every label seen so far: a few dozen, searched linearly
static thread_local ProfChain* tls_prof_chain = nullptr;

static std::map<std::string, std::string> g_prof_sym;  // label -> the kernel instantiation last launched under it
void prof_symbol(const char* label, const char* fmt, ...) {
    if (!g_prof_on) return;
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_sym[label] = buf;
}
bool prof_enabled() { return g_prof_on; }
// (g_prof_mu held, all four)
static int prof_event_take() {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return -1;
    for (size_t i = g_prof_ev_free.size(); i-- > 0;) {  // an event serves the device it was created on: the newest free one of it
        const int e = g_prof_ev_free[i];
        if (g_prof_ev[e].device != device) continue;
        g_prof_ev_free.erase(g_prof_ev_free.begin() + (long)i);
        g_prof_ev[e].refs = 1;
        return e;
    }
    ProfEvent pe;
    if (hipEventCreate(&pe.ev) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    pe.device = device;
    pe.refs = 1;
    g_prof_ev.push_back(pe);
    g_prof_ev_free.reserve(g_prof_ev.capacity());  // prof_event_drop never allocates
    return (int)g_prof_ev.size() - 1;
}
static void prof_event_drop(int e) {
    if (e >= 0 && --g_prof_ev[e].refs == 0) g_prof_ev_free.push_back(e);
}
static ProfChain* prof_chain_on(hipStream_t stream) {
    return tls_prof_chain && tls_prof_chain->stream == stream ? tls_prof_chain : nullptr;
}
static void prof_release(int slot) {
    ProfPair& p = g_prof[slot];
    prof_event_drop(p.a);
    prof_event_drop(p.b);
    g_prof_labels[p.label].held--;
    p.state = ProfPair::kFree;
    g_prof_free.push_back(slot);
}
// chained: the bracket may begin at the stop event of the one before it (the single-kernel form; the recorded form records
// both of its events)
static int prof_open_pair(const char* name, hipStream_t stream, bool chained, hipEvent_t* start, hipEvent_t* stop) {
    *start = *stop = nullptr;
    if (!g_prof_on) return -1;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (cs != hipStreamCaptureStatusNone) return -1;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfChain* chain = prof_chain_on(stream);
    int label = 0;
    while (label < (int)g_prof_labels.size() && g_prof_labels[label].name != name) ++label;
    if (label == (int)g_prof_labels.size()) g_prof_labels.push_back({name, 0});
    const bool shared = chained && chain && chain->last >= 0;
    const int a = g_prof_labels[label].held >= kProfLabelCap ? -1 : shared ? chain->last : prof_event_take();
    const int b = a >= 0 ? prof_event_take() : -1;
    if (b < 0) {  // not timed: the bracket after it has no boundary to share
        if (a >= 0 && !shared) prof_event_drop(a);
        if (chain) {
            prof_event_drop(chain->last);
            chain->last = -1;
        }
        return -1;
    }
    if (shared) g_prof_ev[a].refs++;
    int slot;
    if (!g_prof_free.empty()) {
        slot = g_prof_free.back();
        g_prof_free.pop_back();
    } else {
        slot = (int)g_prof.size();
        g_prof.push_back(ProfPair());
        g_prof_free.reserve(g_prof.capacity());  // prof_release never allocates
    }
    ProfPair& p = g_prof[slot];
    p.a = a;
    p.b = b;
    p.label = label;
    p.state = ProfPair::kOpen;
    g_prof_labels[label].held++;
    if (!shared) *start = g_prof_ev[a].ev;
    *stop = g_prof_ev[b].ev;
    return slot;
}
int prof_open(const char* name, hipStream_t stream, hipEvent_t* start, hipEvent_t* stop) {
    return prof_open_pair(name, stream, true, start, stop);
}
void prof_close(int slot, hipStream_t stream) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof[slot].state = ProfPair::kClosed;
    if (ProfChain* chain = prof_chain_on(stream)) {  // the next bracket of the chain begins here
        prof_event_drop(chain->last);
        chain->last = g_prof[slot].b;
        g_prof_ev[chain->last].refs++;
    }
}
int prof_begin(const char* name, hipStream_t stream) {
    hipEvent_t a, b;
    const int slot = prof_open_pair(name, stream, false, &a, &b);
    if (slot >= 0) (void)hipEventRecord(a, stream);
    return slot;
}
void prof_end(int slot, hipStream_t stream) {
    if (slot < 0) return;
    hipEvent_t b;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        b = g_prof_ev[g_prof[slot].b].ev;
    }
    (void)hipEventRecord(b, stream);
    prof_close(slot, stream);
}
ProfChain::ProfChain(hipStream_t s) : stream(s), prev(tls_prof_chain) { tls_prof_chain = this; }
ProfChain::~ProfChain() {
    tls_prof_chain = prev;
    if (last < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    prof_event_drop(last);
}

}  // namespace mvdb

// ================================================================================================
// index object
// ================================================================================================
namespace {

// The one capture test: nothing allocates or synchronises while it holds.
bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return s && hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}

// A device allocation of EXACTLY the bytes asked for (the matrix and the stores derived from it: DevBuf's padding of a
// quarter would be gigabytes), freed at once when it is replaced or goes — never parked on tls_retire: nothing captured
// names these through a workspace.
template <typename T>
struct DevMem {
    T* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { release(); }
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

// `words` device words that kernels count in, plus a 64-byte host-mapped mirror they copy the counts to, which host code
// reads without a sync.  Both or neither: a failed ensure leaves the counter empty, which is no error — the kernels take
// NULL for "do not count" and the readers see zeros.
struct MirroredCounter {
    DevMem<unsigned int> words;
    PinnedBuf host;
    // Never called while a stream is capturing (it allocates).  zero_on: the stream whose later work counts here, the zeroing
    // is enqueued on it; none: zeroed before ensure returns.
    bool ensure(int n, const hipStream_t* zero_on = nullptr) {
        if (words.p) return true;
        const size_t bytes = (size_t)n * sizeof(unsigned int);
        if (words.alloc(bytes) != hipSuccess ||
            (zero_on ? hipMemsetAsync(words.p, 0, bytes, *zero_on) : hipMemset(words.p, 0, bytes)) != hipSuccess || host.reserve(64) != 0) {
            (void)hipGetLastError();
            words.release();
            return false;
        }
        memset(host.p, 0, 64);
        return true;
    }
    unsigned int* dev() const { return words.p; }
    template <typename W = unsigned int>
    volatile W* mirror() const { return words.p ? reinterpret_cast<volatile W*>(host.p) : nullptr; }
    template <typename W = unsigned int>
    W read(int i) const { return words.p ? mirror<W>()[i] : W(0); }
};

struct Workspace {
    OwnedStream owned;  // (first: every buffer below is freed before the stream this workspace created for itself)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf<float> q;
    DevBuf<float> qn;  // normalised copy of the queries for the multi-query pass
    DevBuf<uint64_t> cand;
    DevBuf<int64_t> out;  // packed results of the host API: [I: total int64 | D: total fp32] -> ONE D2H copy
    PinnedBuf pin_out;
    DevBuf<float> scores;
    DevBuf<uint64_t> selkeys;
    DevBuf<int64_t> rows;
    DevBuf<__bf16> qsplit;  // the fp16 image of one chunk of queries (certified pass; 2-byte elements)
    DevBuf<float> qnorm;
    DevBuf<int> flags;      // per-chunk count of uncertified queries
    DevBuf<int> qfail;      // per query: 1 = failed certification; behind them the compact list of those queries
    DevBuf<float> requery;  // the failed queries, gathered, and their exact results [D | I]
    DevBuf<int64_t> relabel;
    DevBuf<int> nfail;      // number of uncertified queries of the call (device-side gate of the exact re-run)
    DevBuf<int> need;       // one word per 32-query exact re-run pass: raised by the rescue pass where a query stays unanswered
    DevBuf<float> qfloor;   // per query: the admission floor of its exact re-run (half_certify_kernel), behind them the compact copy
    DevBuf<uint32_t> tflags;  // certified pass: one bit per (query of the call, 32-row tile) that may matter to the rescue pass
    DevBuf<int> tlist;        // the rescue launches' tile lists
    SelectState* st = nullptr;
    PinnedBuf pin;
    std::mutex use_mu;  // stream workspaces are shared by every host thread that names the stream: one search at a time
    bool captured = false;         // a search on this workspace has been captured into a hipGraph: its buffers are never freed
    std::vector<void*> retired;    // ... outgrown ones wait here until the workspace goes (common.hpp, RetireScope)
    // grouped search (mvdb_index_search_grouped): the item table on the device, its pinned staging copy, and the event recorded
    // behind the upload — the staging copy is rewritten only once the upload that reads it has run
    DevBuf<uint64_t> rkeys;             // range search: [nq, segment] appended keys (range_scan.hpp)
    DevBuf<unsigned long long> rcounts;  // ... and the host entry point's per-query counters
    DevBuf<uint32_t> rcand;              // range search, shared pass: [nq, capacity] candidate rows ...
    DevBuf<unsigned long long> rccount;  // ... and their per-query counters
    DevBuf<float> rthr;                  // per-query thresholds on the device (host entry point; L2: negated)
    DevBuf<int64_t> jrows;               // range join: the query rows' numbers = their bounds, one launch group
    DevBuf<float> mmrD;                  // MMR search: stage 1's candidates of one tile of queries, [min(nq, kCoreTile), fetch_k] ...
    DevBuf<int64_t> mmrI;                // ... scores and row numbers (mmr_select.hpp)
    DevBuf<int> dneed;                   // distinct search: kCoreTile need words of one tile of queries, then the collapse launch's ticket
    DevBuf<uint64_t> dtab;               // ... the table of tier 2, [T slots, n_groups] (distinct_select.hpp)
    DevBuf<int32_t> dG;                  // ... the host entry point's group codes, [nq, k]
    DevBuf<float> ghD;                   // group hits search: distinct search's scores of the call, [nq, k] (group_hits.hpp) ...
    DevBuf<int64_t> ghI;                 // ... its rows ...
    DevBuf<int32_t> ghG;                 // ... its group codes, where the caller takes none ...
    DevBuf<uint64_t> ghpart;             // ... and the block lists of the member pass, [T slots, grid.x, k * group_size + 1]
    DevBuf<uint64_t> mxtab;              // MaxSim search: the table of one call, [n_groups, T] (maxsim_scan.hpp) ...
    DevBuf<uint64_t> mxpart;             // ... the block lists of its top-k launch, [lists, 64] ...
    DevBuf<char> mxout;                  // ... the host entry point's results, packed: I_tok | D_tok | D | G
    DevBuf<uint64_t> asbest;             // assignment: the running best of every stored row, one word each (assign_scan.hpp)
    DevBuf<uint64_t> exbest;             // search by examples: the running (best positive, best negative) of every stored row (examples_scan.hpp) ...
    DevBuf<uint64_t> expart;             // ... the block lists of its top-k launch, [lists, 64] ...
    DevBuf<int64_t> exskip;              // ... the host entry point's skip rows
    DevBuf<float> bsT;                   // boosted search: the combined term column of one call, [n] (boost_scan.hpp) ...
    DevBuf<int64_t> bsrows;              // ... the sparse entries' rows ...
    DevBuf<float> bsvals;                // ... and their values
    DevBuf<uint64_t> spq;                // sparse search: the queries of one call, [nq + 1] term offsets then the (index, value) terms (sparse_scan.hpp) ...
    DevBuf<uint64_t> spmask;             // ... a row list as a bitmap over the stored rows ...
    DevBuf<int32_t> spmatched;           // ... and mvdb_index_sparse_scores' matched counts, [n]
    DevBuf<float> kmc;                   // k-means: the centres, [C, ld] ...
    DevBuf<int32_t> kmlab[2];            // ... the labels of this iteration and of the one before, [n] each ...
    DevBuf<uint32_t> kmmem;              // ... the member lists, label after label, [n] ...
    DevBuf<uint32_t> kmhist;             // ... the list build's counts, [C, slices] ...
    DevBuf<int64_t> kmcount;             // ... members per label, [C], then the changed-label count ...
    DevBuf<uint32_t> kmoff;              // ... the lists' bases [C + 1], then the work items' bases [C + 1] ...
    DevBuf<double> kmpart;               // ... the chunk partials, [n / 256 + C, d]
    DevBuf<ProbeItem> pitems;            // probed search: the work items of one chunk of queries, [queries, max_items] (probe_scan.hpp) ...
    DevBuf<int> pcount;                  // ... and their item counts, [queries]
    DevBuf<char> gtab;
    DevBuf<char> c8;        // int8 prefilter of a single query (code8_search): planes, terms, counter and active lists, gate, floor, candidates
    struct GroupedStage {   // one pinned copy of a table + the event recorded behind its upload
        PinnedBuf buf;
        hipEvent_t ev = nullptr;
        bool busy = false;
    };
    std::vector<GroupedStage*> gstage;  // a ring: a call takes a copy whose upload has run, or adds one (stage_grouped_table)
    std::vector<void*> gpin_captured;  // a captured call's upload re-reads its staging copy at every replay: kept, never rewritten
    PinnedBuf gpin_spare;              // ... allocated by the eager calls (nothing may be allocated while a stream is capturing)

    int init(int dev, hipStream_t s) {
        device = dev;
        if (s) {
            stream = s;
        } else {
            MVDB_HIP(hipStreamCreateWithFlags(&owned.h, hipStreamNonBlocking));
            stream = owned.h;
            own_stream = true;
        }
        MVDB_HIP(hipMalloc((void**)&st, sizeof(SelectState)));
        return 0;
    }
    // what is not a buffer (the buffers free themselves); also of a workspace whose init() failed half-way
    ~Workspace() {
        for (GroupedStage* g : gstage) {
            if (g->ev) (void)hipEventDestroy(g->ev);
            delete g;
        }
        for (void* p : gpin_captured) (void)hipHostFree(p);
        for (void* old : retired) (void)hipFree(old);
        if (st) (void)hipFree(st);
    }
};

}  // namespace

static std::atomic<uint64_t> g_index_serial{0};

// ---- the two stores derived from the matrix ------------------------------------------------------------------------------
// Searches (index held shared) build and read them under mvdb_index::shadow_mu; mutators (index held exclusively, searches
// quiesced) edit them directly.  What each event does to each store — the operations below are the only writers:
//
//   event                        | fp16 shadow (+ L2 offsets)                     | int8 code (+ floor sample)
//   -----------------------------+------------------------------------------------+------------------------------------------------
//   create                       | none; built by the first batch search that can | none; built by the first eligible single query
//                                | use it (ensure), offsets by the first L2 pass  | (ensure sets `wanted`), with the sample
//   add that fits                | extend: new rows converted; emptied instead if | extend: new rows coded and the sample gathered
//                                | incomplete or the bound moved the scale;       | again; left alone if incomplete (emptied by a
//                                | offsets catch up in ensure_offsets             | delete); nothing if none is held
//   add that reallocates (grow)  | drop, before the new matrix is allocated       | drop; wait restarts if wanted
//   reserve that reallocates     | as grow (nothing if the capacity suffices)     | as grow
//   set_rows                     | listed rows below `rows` converted in place    | listed rows below `rows` coded in place; the
//                                | (offsets: below `hn_rows`)                     | sample, if valid, gathered again per chunk
//   set_rows that moves the scale| invalidate, after the rows are written         | (as set_rows)
//   remove_rows                  | invalidate: emptied, allocation kept           | invalidate: emptied, sample stale, allocation
//                                |                                                | kept; wait restarts if wanted, held or not
//   reset                        | drop                                           | drop; wait restarts, `wanted` stays set
//   free                         | freed with the index                           | freed with the index
//   build failure                | drop, `failed` set: not tried again until a    | drop (wait untouched), `failed` set: NOTHING
//                                | drop, an invalidate or an add without a shadow | clears it, the route is off for this index
//                                | clears it                                      |
//   capture                      | ensure builds nothing: a complete shadow is    | ensure builds nothing: a complete code with a
//                                | used, else the fp32 passes serve               | valid sample is used, else the exact scan serves
//
// The code's FRONT plane (Code8Store::F5, the top 5 bits of every code: code8_scan.hpp) is part of the code in every row of
// this table: allocated (index option code8_front_plane; an allocation that fails leaves the code without it, nothing else),
// written by the same launch of code8_build_kernel, emptied, dropped and freed with the two planes.  Setting the option to 0
// frees it alone; setting it again drops a code that lacks it, and the next eligible query builds both.
//
// The code's BIT plane (Code8Store::B2, bit 2 of every code: code8_scan.hpp) — one more row of the table, the same in every
// column:
//   event                        | B2
//   ensure (first build)         | allocated where the front plane was (index option code8_bit_plane = 1); an allocation that
//                                | fails leaves the front form on its gathers, nothing else
//   build / add / set_rows       | written by the same launch of code8_build_kernel, range and list form
//   add beyond capacity, reserve | dropped with the code
//   remove_rows                  | emptied with the code, allocation kept
//   reset, build failure, free   | dropped / freed with the code
//   code8_bit_plane = 0          | freed alone; = 1 again drops a code that holds the front plane without it
//   code8_front_plane = 0        | KEPT (and kept current by the builds): only the front plane is freed
// (`failed` of both is read by routing code that holds only the shared lock and written under shadow_mu: atomic.)
namespace {

struct ShadowStore {   // half_scan.hip: flat_scan_h16_kernel
    DevMem<_Float16> Xh;
    int64_t cap = 0, rows = 0;  // rows allocated (+ kRowSlack behind them) / rows converted
    float scale = 0.f;
    std::atomic<bool> failed{false};
    DevMem<float> Hn;  // L2 over rows of mixed norms: |x_r|^2 / 2 of rows [0, hn_rows) (+ zeroed slack), dies with Xh
    int64_t hn_rows = 0;

    void drop();
    void invalidate();
    int extend(mvdb_index* idx, int64_t n_new);
    const _Float16* ensure(const mvdb_index* idx, hipStream_t s, float xscale);
    const float* ensure_offsets(const mvdb_index* idx, hipStream_t s);
};

struct Code8Store {   // code8_scan.hpp; DESIGN.md section 4.1b: d codes + (scale, residual bound) per row, the operand of the single-query prefilter
    DevMem<uint8_t> C8;  // two planes: [cap, 3 d / 4] high, then [cap, d / 4] low (low())
    DevMem<uint8_t> F5;  // the front plane: [cap rounded up to whole tiles, 5 d / 8], tiled (code8_front_wide_offset); may be absent
    DevMem<uint8_t> B2;  // the bit plane: [cap, d / 8], bit 2 of every code (code8_bit2_pack_chunk); held only beside F5, may be absent
    DevMem<float2> ar;
    DevMem<int8_t> samp;  // the stored copy of the floor's sample (code8_sample_kernel; the rule: gather_sample): codes, then (a, r) entries
    int64_t cap = 0, rows = 0;
    int64_t samp_n = 0;   // the row count the copy was gathered for, after the last write to the code; 0 = stale
    std::atomic<bool> wanted{false};  // an eligible single query has asked for the code since the index was created
    std::atomic<bool> failed{false};
    std::atomic<int> wait{0};  // single queries the exact scan still answers before a dropped code is rebuilt

    void drop(bool count_rebuild = true);
    void invalidate();
    int extend(mvdb_index* idx, int64_t n_new);
    bool ensure(const mvdb_index* idx, hipStream_t s);
    // the low plane lies behind the high plane of the whole CAPACITY: add into reserved space moves nothing
    uint8_t* low(int d) const { return C8.p + code8_low_offset(cap, d); }
    int build(const mvdb_index* idx, int64_t row0, int64_t n, hipStream_t s, const int64_t* list_dev = nullptr);
    int gather_sample(const mvdb_index* idx, int64_t n, hipStream_t s);
    bool sample_valid(int64_t n) const { return samp.p && rows == n && samp_n == n; }
};

}  // namespace

struct mvdb_index {
    const uint64_t serial = ++g_index_serial;  // unique per index object of the process: resident row sets name their index by it
    int d = 0, d4 = 0, metric = 0, device = 0;
    int64_t ld = 0;
    DevMem<float> X;
    int64_t n = 0, cap = 0;
    float row_norm_bound = 0.f;  // upper bound of |row| over the stored rows (INFINITY: unknown, raw adds)
    float norm2_lo = INFINITY, norm2_hi = 0.f;  // L2 metric only: bounds of |row|^2 over the stored rows (true values inside)
    uint64_t renumbered = 0;     // bumped whenever stored rows change their numbers (remove_rows, reset): resident row sets
                                 // built before are stale
    Knobs kn;                    // the MVDB_* hooks as read at creation (mvdb_index_reload_env re-reads)
    hipStream_t mut = nullptr;   // the mutators' own non-blocking stream: add / remove_rows never touch the legacy stream,
                                 // so work other libraries have in flight on the device (an encoder forward) is not stalled
    DevMem<unsigned int> normmax;     // 8-byte scratch of note_row_norms (raw adds)
    DevMem<float> ctmp;               // bounded staging buffer of mvdb_index_remove_rows (kept once a delete has run)
    size_t ctmp_bytes = 0;
    DevBuf<float> set_stage;          // bounded staging of mvdb_index_set_rows (kept once an update has run): one chunk of new
    DevBuf<int64_t> set_list;         // rows at the matrix' stride, and the row numbers they go to
    mutable std::mutex shadow_mu;     // (the event x store table above)
    mutable ShadowStore shadow;
    mutable Code8Store code;
    // the opt-in single-query route over the shadow (index_state.hpp: RouteWindow): refused single-query certificates,
    // counted from the first opted-in single query on (search_core)
    mutable MirroredCounter sq_fail;
    mutable RouteWindow sq_route;
    // adaptive tile flags (search_core): a running count of refused certificates of ANY certified call, created with the
    // shadow; the certified pass keeps tile flags only while that count has been moving
    mutable MirroredCounter rf;
    mutable std::atomic<unsigned int> rf_seen{0};
    mutable std::atomic<int> rf_calls_left{0};
    // the int8 route, created with the code.  Device words: [0] fallbacks, [1] calls, [2..3] one 64-bit word: rows refined
    // (code8_scan_kernel), [4..5] one 64-bit word: rows stage 0 of its front form could not reject, [6] calls of the front form;
    // mirror: fallbacks, candidates of the latest call, calls, then (64-bit, at byte 16) the survivors of stage 0 and, word 6,
    // the front form's calls, as block 0 of the latest front launch found them.  c8_front: the front form's own window over
    // the mean share of survivors (index_state.hpp: RouteWindow::suspended_mean) — suspended, the other form of the kernel runs
    mutable MirroredCounter c8_ctr;
    mutable RouteWindow c8_route;
    mutable RouteWindow c8_front;
    // range search, shared pass (range_shared_phase), created by the first call that takes it: a running count of queries its
    // fallback answered, mirrored with the candidates of the latest launch group as 64-bit words; calls that took the route
    // are counted on the host
    mutable MirroredCounter rg_ctr;
    mutable std::atomic<unsigned long long> rg_shared_calls{0};
    // the range join (range_shared_phase with bounds): the same pair of counters, of its own
    mutable MirroredCounter jn_ctr;
    mutable std::atomic<unsigned long long> jn_shared_calls{0};
    // distinct search, created by the first call: a running count of the queries tier 2 answered (one device word and its
    // mirror, written by distinct_collapse_kernel); the calls are counted on the host
    mutable MirroredCounter ds_ctr;
    mutable std::atomic<unsigned long long> ds_calls{0};
    // group hits search, created by the first call: a running count of the member rows met (one 64-bit device word and its
    // mirror, written by group_members_select_kernel); the calls are counted on the host
    mutable MirroredCounter gh_ctr;
    mutable std::atomic<unsigned long long> gh_calls{0};
    // MaxSim search: calls served and corpus passes enqueued, both counted on the host
    mutable std::atomic<unsigned long long> mx_calls{0}, mx_passes{0};
    // assignment (and the assignments of k-means): calls served and corpus passes enqueued, both counted on the host
    mutable std::atomic<unsigned long long> as_calls{0}, as_passes{0};
    // search by examples: calls served and corpus passes enqueued, both counted on the host
    mutable std::atomic<unsigned long long> ex_calls{0}, ex_passes{0};
    // boosted search: searches served and boost_scan_kernel launches enqueued, both counted on the host
    mutable std::atomic<unsigned long long> bs_calls{0}, bs_launches{0};
    // sparse and hybrid search: searches served and sparse_scan_kernel launches enqueued, both counted on the host
    mutable std::atomic<unsigned long long> sp_calls{0}, sp_launches{0};
    // ... served through the posting lists: searches, sparse_postings_kernel launches, and list entries of the queries' terms
    mutable std::atomic<unsigned long long> pp_calls{0}, pp_launches{0}, pp_entries{0};
    // probed search: calls served and launches enqueued, both counted on the host
    mutable std::atomic<unsigned long long> pb_calls{0}, pb_launches{0};
    mutable std::shared_mutex mu;  // search: shared; add/reset/remove/free: exclusive
    mutable std::mutex ws_mu;
    mutable std::vector<Workspace*> free_ws;           // synchronous searches
    mutable std::map<void*, Workspace*> stream_ws;     // async searches, one per caller stream
    mutable Workspace* default_stream_ws = nullptr;

    Workspace* acquire() const {
        {
            std::lock_guard<std::mutex> lk(ws_mu);
            if (!free_ws.empty()) {
                Workspace* w = free_ws.back();
                free_ws.pop_back();
                return w;
            }
        }
        Workspace* w = new Workspace();
        if (w->init(device, nullptr)) {
            delete w;
            return nullptr;
        }
        return w;
    }
    void release(Workspace* w) const {
        std::lock_guard<std::mutex> lk(ws_mu);
        free_ws.push_back(w);
    }
    Workspace* for_stream(hipStream_t s) const {
        std::lock_guard<std::mutex> lk(ws_mu);
        if (!s) {
            if (!default_stream_ws) {
                // legacy default stream: work is enqueued on stream 0 itself (the workspace owns no stream: stream 0 is never destroyed)
                Workspace* w = new Workspace();
                w->device = device;
                if (hipMalloc((void**)&w->st, sizeof(SelectState)) != hipSuccess) {
                    delete w;
                    return nullptr;
                }
                default_stream_ws = w;
            }
            return default_stream_ws;
        }
        auto it = stream_ws.find((void*)s);
        if (it != stream_ws.end()) return it->second;
        Workspace* w = new Workspace();
        if (w->init(device, s)) {
            delete w;
            return nullptr;
        }
        stream_ws[(void*)s] = w;
        return w;
    }
};

namespace {

// The launchers below read the hooks of the index being searched through a thread-local pointer (search_core installs it).
const Knobs g_default_knobs;
thread_local const Knobs* tls_kn = &g_default_knobs;
struct KnobScope {
    const Knobs* prev;
    explicit KnobScope(const Knobs* k) : prev(tls_kn) { tls_kn = k; }
    ~KnobScope() { tls_kn = prev; }
};
inline const Knobs& kn() { return *tls_kn; }

// ---- shape selection: G lanes per row, C chunks per lane, U rows in flight ----------------------
struct Shape {
    int G, C;
};
constexpr Shape choose_shape(int d4) {
    // one chunk per lane, 16 / 32 / 64 lanes per row (rows of up to 64 / 128 / 256 floats; the 1-, 2-, 4- and 8-lane
    // shapes of rounds 1 - 4 served rows of <= 4, 8 and 32 floats only: 84 instantiations for toy widths)
    if (d4 <= 64) return {d4 <= 16 ? 16 : d4 <= 32 ? 32 : 64, 1};  // (rows of <= 16 floats ride the 16-lane shape, lanes masked)
    if (d4 % 64 == 0 && d4 / 64 <= 8) return {64, d4 / 64};
    if (d4 == 96) return {32, 3};  // d = 384 (e5-small, config 5): three exact chunks on 32 lanes, two rows per wave-instruction
    // more than eight chunks per lane (d > 2048): ONE shape, sixteen chunks with the lanes beyond the row masked off — the
    // seven shapes in between (nine to fifteen chunks: 224 kernel instantiations, 30 % of this code object) went in round 5;
    // a masked chunk issues no load, the scan stays bound by the bytes of the row
    const int c = (d4 + 63) / 64;
    return {64, c > 8 ? 16 : c};
}
constexpr int kMaxC = 16;  // d <= 4096

// The exact scans are instantiated for the twelve shapes choose_shape returns.  launch(ScanShape<G, C>{}) for rows of d4 chunks:
// this is the one table of them (flat_scan_kernel, range_scan_kernel, range_rescore_kernel, grouped_scan_kernel and the
// candidate re-score of the int8 route all take their (G, C) from here).
template <int G_, int C_>
struct ScanShape {
    static constexpr int G = G_, C = C_;
};
int unsupported_shape(int d4) { return fail(MVDB_ERR_ARG, "dimension with %d 16-byte chunks per row is not supported (d <= 4096)", d4); }
template <typename Launch>
int with_scan_shape(int d4, Launch launch) {
    const Shape sh = choose_shape(d4);
    if (sh.G == 16 && sh.C == 1) return launch(ScanShape<16, 1>{});
    if (sh.G == 32 && sh.C == 1) return launch(ScanShape<32, 1>{});
    if (sh.G == 32 && sh.C == 3) return launch(ScanShape<32, 3>{});
    if (sh.G == 64) switch (sh.C) {
            case 1: return launch(ScanShape<64, 1>{});
            case 2: return launch(ScanShape<64, 2>{});
            case 3: return launch(ScanShape<64, 3>{});
            case 4: return launch(ScanShape<64, 4>{});
            case 5: return launch(ScanShape<64, 5>{});
            case 6: return launch(ScanShape<64, 6>{});
            case 7: return launch(ScanShape<64, 7>{});
            case 8: return launch(ScanShape<64, 8>{});
            case 16: return launch(ScanShape<64, 16>{});
            default: break;
        }
    return unsupported_shape(d4);
}

// ---- rows in flight per wave, U: three policies over the table (a score does not depend on U) ---------------------------------
// (Rounds 1 - 2 carried run-time tuning hooks here — MVDB_SCAN_VARIANT, MVDB_SCAN_U: other rows-in-flight counts per shape,
//  17 more shapes x 24 kernels each; the sweeps they served are in profiles/r01_sweep_scan_variants.txt.  Removed in round 3:
//  they were 40 % of this code object, which a process loads whole before its first search.)
// Streaming scans (every row, or the rows of a bitmap): about four independent 16-B loads per lane (scan_resident_blocks has the
// measurement), so 4 rows of one chunk, 2 of two or three, 1 beyond; the three exact chunks on 32 lanes keep 4.
constexpr int stream_u(int G, int C) { return C == 1 || G == 32 ? 4 : C <= 3 ? 2 : 1; }
// Row-list (gather) scans of two- and three-chunk rows keep FOUR rows in flight per wave (the streaming scan: two): a
// gathered row is a fresh DRAM page, so more rows must be outstanding to cover its latency — 10M x 512 rows resident,
// ids on the device: 10 % of the rows 5.74 -> 6.23 TB/s of rows touched, 50 % 6.37 -> 6.78, 99 % 6.54 -> 6.95.
// The grouped launch gathers too: its rows in flight are these (plan_grouped sizes its work items by them).
constexpr int gather_u(int G, int C) { return C <= 3 ? 4 : 1; }
// The exact re-scores of candidate rows (a range batch's shared pass, the int8 route): gathers too, 4 rows up to three
// chunks, 2 up to eight, 1 at sixteen.  (No sweep of these is on record: they are the values both re-score launchers were written with.)
constexpr int rescore_u(int G, int C) { return C <= 3 ? 4 : C <= 8 ? 2 : 1; }

// ---- runtime -> compile-time switches of a shape's kernels: subset indirection, lane masking ----------------------------------
// launch(ScanForm<SEL, MASKED>{}): SEL 0 every row, 1 a row list, 2 a bitmap; MASKED where the row does not fill G x C chunks.
template <int SEL_, bool MASKED_>
struct ScanForm {
    static constexpr int SEL = SEL_;
    static constexpr bool MASKED = MASKED_;
};
template <int G, int C, typename Launch>
int with_scan_form(int d4, bool row_list, bool bitmap, Launch launch) {
    auto sel = [&](auto masked) {
        constexpr bool M = decltype(masked)::value;
        if (bitmap) return launch(ScanForm<2, M>{});  // bitmap-selected rows (mvdb_index_search_masked)
        if (row_list) return launch(ScanForm<1, M>{});
        return launch(ScanForm<0, M>{});
    };
    // (32 lanes x 3 / 5 / 7 chunks are chosen for rows that fill them exactly: their lane-masked forms are never instantiated)
    constexpr bool kAlwaysFull = G == 32 && C > 1;
    if constexpr (!kAlwaysFull) {
        if (d4 != G * C) return sel(std::true_type{});
    }
    return sel(std::false_type{});
}

// ---- grids ------------------------------------------------------------------------------------------------------------------
// A row scan: RB = (64 / G) U rows per wave-batch, batches -> waves -> blocks, at most per_cu resident blocks per CU.
int scan_grid(int64_t n, int RB, int per_cu, int device) {
    const int64_t nbatches = (n + RB - 1) / RB;
    const int64_t want = (nbatches + kScanWaves - 1) / kScanWaves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}
// The fp32-MFMA passes: one 16-row tile per wave at a time.
int mfma_tile_grid(int64_t n, int per_cu, int device) {
    const int64_t ntiles = (n + 15) / 16;
    const int64_t want = (ntiles + kScanWaves - 1) / kScanWaves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
}
// Resident blocks per CU of the exact row scans (flat_scan_kernel, range_scan_kernel) at C chunks per lane; knob: the launch
// honours MVDB_SCAN_BLOCKS_PER_CU.
int scan_resident_blocks(const void* kern, int C, bool knob = true) {
    const int occ_hw = cached_occupancy(kern, kScanThreads, 0, 4);  // blocks per CU this instantiation sustains
    // measured on MI355X (round-1 sweep, profiles/r01_sweep_scan_variants.txt, 10M x 512): with ~4
    // independent 16-B loads per lane, 2 resident blocks (8 waves) per CU reach 7.21-7.24 TB/s; more
    // waves or more loads in flight per lane are 2-4 % slower, 1 block per CU is latency-starved
    // (gpurun_out/sweep_dims.log: the one- and three-chunk shapes — d = 64 / 256 / 384 — prefer U = 4 with
    //  3 resident blocks: 7.0-7.1 TB/s vs 6.5-6.9 at 2)
    const int cap_env = knob ? kn().scan_blocks_per_cu : 0;  // tuning hook
    return std::min(occ_hw, cap_env > 0 ? cap_env : (C == 1 || C == 3) ? 3 : 2);
}

// the widths of the int8 prefilter (code8_scan.hpp) and the exact-scan shapes they have
constexpr int kCode8Dims[] = {384, 512, 1024};
static_assert(kCode8Dims[2] <= kCode8MaxDim, "code8_seed_kernel holds the query's planes in LDS");
bool code8_dim(int d) { return std::find(std::begin(kCode8Dims), std::end(kCode8Dims), d) != std::end(kCode8Dims); }
constexpr bool code8_shape(int G, int C) {
    for (int d : kCode8Dims)
        if (choose_shape(d / 4).G == G && choose_shape(d / 4).C == C) return true;
    return false;
}

// label: the profiling label where the launch has one of its own (the int8 route's fallback scan)
template <int G, int C, int U, int METRIC, int MODE, int SEL, bool MASKED>
int launch_scan_kern(const ScanArgs& a, int nq, int device, hipStream_t stream, int* nblocks_out, const char* label = nullptr,
                     bool knob = true) {
    void (*kern)(ScanArgs) = flat_scan_kernel<G, C, U, METRIC, MODE, true, SEL, MASKED>;
    bool gated = false;
    // device-gated exact re-run of an L2 batch's queries: over the whole index (SEL 0) and under a bitmap (SEL 2 — round-4
    // advisor finding: without the gated instantiation every query of a certified masked L2 batch paid a full masked scan);
    // and the int8 route's fallback: the headline kernel's shape with GATED set, at that route's widths
    if constexpr ((METRIC == 1 && MODE == kModeTopK && (SEL == 0 || SEL == 2)) ||
                  (METRIC == 0 && MODE == kModeTopK && SEL == 0 && !MASKED && code8_shape(G, C))) {
        if (a.gate) {
            kern = flat_scan_kernel<G, C, U, METRIC, MODE, true, SEL, MASKED, true>;
            gated = true;
        }
    }
    if (a.gate && !gated) return fail(MVDB_ERR_ARG, "internal: a device-gated scan was requested for a kernel form that has no gated instantiation");
    const int nblocks = scan_grid(a.n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C, knob), device);
    if (nblocks_out) *nblocks_out = nblocks;
    return profiled_launch(label ? label : MODE == kModeTopK ? "ip_scan" : "ip_scan_scores", stream,
                           [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, nq), dim3(kScanThreads), 0, stream, done, a); },
                           "flat_scan_kernel<%d, %d, %d, %d, %d, %s, %d, %s, %s>", G, C, U, METRIC, MODE, "true", SEL, MASKED ? "true" : "false",
                           gated ? "true" : "false");
}

// Grid size the scan will use for (shape, n): needed up front to size the candidate buffer.
int scan_grid_upper_bound(int device) { return device_cus(device) * 8; }

int launch_scan(int metric, int mode, const ScanArgs& a, int nq, int device, hipStream_t s, int* nblocks) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);  // a row list: the gather policy
            if (metric == MVDB_METRIC_IP)
                return mode == kModeTopK ? launch_scan_kern<S::G, S::C, U, 0, kModeTopK, F::SEL, F::MASKED>(a, nq, device, s, nblocks)
                                         : launch_scan_kern<S::G, S::C, U, 0, kModeScores, F::SEL, F::MASKED>(a, nq, device, s, nblocks);
            return mode == kModeTopK ? launch_scan_kern<S::G, S::C, U, 1, kModeTopK, F::SEL, F::MASKED>(a, nq, device, s, nblocks)
                                     : launch_scan_kern<S::G, S::C, U, 1, kModeScores, F::SEL, F::MASKED>(a, nq, device, s, nblocks);
        });
    });
}

__global__ void fill_missing_kernel(float* D, int64_t* I, int64_t total, int metric) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = metric == 0 ? -3.402823466e+38f : 3.402823466e+38f;
        I[i] = -1;
    }
}

int64_t pow2ceil(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

int normalize_range(const mvdb_index* idx, float* base, int64_t n, hipStream_t s);

// Mutators (add / remove_rows / reset / reserve) hold the index exclusively, which only excludes HOST calls: scans enqueued
// earlier by mvdb_index_search_device on caller streams may still be reading the matrix.  Wait for THIS index's searches —
// every stream that ever searched it has a workspace here (the synchronous API's own workspaces are idle once a call has
// returned) — and for nothing else: no hipDeviceSynchronize, so an encoder forward or another index on the same device
// keeps running.  The mutators then work on the index's own non-blocking stream (idx->mut) and wait for that stream only.
int quiesce(mvdb_index* idx) {
    std::lock_guard<std::mutex> lk(idx->ws_mu);
    // A caller may have destroyed a stream it once searched on (hipStreamDestroy completes the stream's work first), or be
    // capturing one: neither may wedge the index (round-4 advisor finding: the error made every later add / remove_rows /
    // reset / reserve fail).  A dead handle is forgotten with its workspace; any other failure falls back to the device-wide
    // wait the mutators used before round 4.
    bool device_wide = false;
    for (auto it = idx->stream_ws.begin(); it != idx->stream_ws.end();) {
        const hipError_t e = hipStreamSynchronize((hipStream_t)it->first);
        if (e == hipSuccess) {
            ++it;
            continue;
        }
        (void)hipGetLastError();
        if (e == hipErrorInvalidHandle || e == hipErrorInvalidResourceHandle || e == hipErrorContextIsDestroyed) {
            delete it->second;
            it = idx->stream_ws.erase(it);
        } else {
            device_wide = true;
            ++it;
        }
    }
    if (device_wide) MVDB_HIP(hipDeviceSynchronize());
    if (idx->default_stream_ws) MVDB_HIP(hipStreamSynchronize(nullptr));
    if (!idx->mut) MVDB_HIP(hipStreamCreateWithFlags(&idx->mut, hipStreamNonBlocking));
    return 0;
}

template <int KB, int NG>
int launch_mfma_inst(const MfmaScanArgs& a, int device, hipStream_t stream, int* nblocks_out) {
    auto kern = flat_scan_mfma_kernel<KB, NG>;
    const size_t lds = (size_t)NG * KB * 4 * 64 * 4 + (size_t)kScanWaves * NG * 16 * a.k * 8;
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    int nb = cached_occupancy((const void*)kern, kScanThreads, lds, 1);
    nb = std::min(nb, kn().mfma_blocks_per_cu > 0 ? kn().mfma_blocks_per_cu : 4);
    const int nblocks = *nblocks_out = mfma_tile_grid(a.n, nb, device);
    return profiled_launch("ip_scan_mfma", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kScanThreads), lds, stream, done, a); });
}

template <int KB, int NG, int SKB>
int launch_mfma2_gated_inst(const MfmaScanArgs& a, int device, hipStream_t stream, int* nblocks_out, const int* gate, int gate_lo,
                            const int* need, int npasses, int per_pass, int rtot, int64_t cand_stride) {
    auto kern = a.mask ? flat_scan_mfma2_gated_kernel<KB, NG, SKB, true> : flat_scan_mfma2_gated_kernel<KB, NG, SKB, false>;
    const size_t lds = (size_t)kScanWaves * mfma2_wave_lds_bytes(SKB) + (size_t)kScanWaves * NG * 16 * a.k * 8;
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    int nb = cached_occupancy((const void*)kern, kScanThreads, lds, 1);
    nb = std::min(nb, kn().mfma_blocks_per_cu > 0 ? kn().mfma_blocks_per_cu : 2);
    const int nblocks = *nblocks_out = mfma_tile_grid(a.n, nb, device);
    return profiled_launch(
        "ip_scan_rerun", stream,
        [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kScanThreads), lds, stream, done, a, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride); },
        "flat_scan_mfma2_gated_kernel<%d, %d, %d, %s>", KB, NG, SKB, a.mask ? "true" : "false");
}

template <int KB, int NG, int SKB>
int launch_mfma2_inst(const MfmaScanArgs& a, int device, hipStream_t stream, int* nblocks_out, int metric = MVDB_METRIC_IP) {
    // the L2 form exists where it fits the registers (mfma_path_ok / two_groups route L2 batches accordingly)
    // (d = 768 with 1-KiB stages: the L2 epilogue's non-finite cases do not fit beside 192 registers of query fragments and
    //  64 of staged row — launch_mfma2 gives L2 the 512-B stages there)
    constexpr bool kL2Form = KB <= 48 && !(KB == 32 && NG == 2) && !(KB == 48 && SKB == 16);
    auto kern = flat_scan_mfma2_kernel<KB, NG, SKB, 0>;
    if (metric == MVDB_METRIC_L2) {
        if constexpr (kL2Form)
            kern = flat_scan_mfma2_kernel<KB, NG, SKB, 1>;
        else
            return fail(MVDB_ERR_ARG, "no L2 form of the staged multi-query kernel for d = %d with %d query group(s)", KB * 16, NG);
    }
    const size_t lds = (size_t)kScanWaves * mfma2_wave_lds_bytes(SKB) + (size_t)kScanWaves * NG * 16 * a.k * 8;
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    int nb = cached_occupancy((const void*)kern, kScanThreads, lds, 1);
    nb = std::min(nb, kn().mfma_blocks_per_cu > 0 ? kn().mfma_blocks_per_cu : 2);
    const int nblocks = *nblocks_out = mfma_tile_grid(a.n, nb, device);
    return profiled_launch("ip_scan_mfma", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kScanThreads), lds, stream, done, a); },
                           "flat_scan_mfma2_kernel<%d, %d, %d, %d>", KB, NG, SKB, metric == MVDB_METRIC_L2 ? 1 : 0);
}

template <int NG>
int launch_mfma2(int KB, const MfmaScanArgs& a, int device, hipStream_t s, int* nb, int metric = MVDB_METRIC_IP) {
    // 1-KiB-per-row stages (one contiguous KiB per DMA instruction) measured 2-5 % faster than 512-B
    // stages at 10M x 512; they need 32 KiB of LDS per wave, so fall back when the k-lists do not fit
    const size_t lds_deep = (size_t)kScanWaves * mfma2_wave_lds_bytes(16) + (size_t)kScanWaves * NG * 16 * a.k * 8;
    const bool deep = kn().mfma_stage == 16 && lds_deep <= 160 * 1024;
    switch (KB) {
        case 8: return launch_mfma2_inst<8, NG, 8>(a, device, s, nb, metric);
        case 16: return deep ? launch_mfma2_inst<16, NG, 16>(a, device, s, nb, metric)
                             : launch_mfma2_inst<16, NG, 8>(a, device, s, nb, metric);
        case 24: return launch_mfma2_inst<24, NG, 8>(a, device, s, nb, metric);
        case 32: return deep ? launch_mfma2_inst<32, NG, 16>(a, device, s, nb, metric)
                             : launch_mfma2_inst<32, NG, 8>(a, device, s, nb, metric);
        // d = 768 / 1024 (e5-large, bge-m3 widths): one query group only — the 192 / 256 registers of
        // query fragments leave one wave per SIMD, like two groups at d = 512
        case 40: if (NG == 1) return launch_mfma2_inst<40, 1, 8>(a, device, s, nb, metric);   // (d = 640 / 896: round 6 — the exact pass
                 break;                                                                      //  behind the rescue tier at those widths)
        case 48: if (NG == 1) return deep && metric != MVDB_METRIC_L2 ? launch_mfma2_inst<48, 1, 16>(a, device, s, nb, metric)
                                                                      : launch_mfma2_inst<48, 1, 8>(a, device, s, nb, metric);
                 break;
        case 56: if (NG == 1) return launch_mfma2_inst<56, 1, 8>(a, device, s, nb, metric);
                 break;
        case 64: if (NG == 1) return deep ? launch_mfma2_inst<64, 1, 16>(a, device, s, nb, metric)
                                          : launch_mfma2_inst<64, 1, 8>(a, device, s, nb, metric);
                 break;
        default: break;
    }
    return fail(MVDB_ERR_ARG, "no staged multi-query kernel for d = %d with %d query group(s)", KB * 16, NG);
}

// The exact re-run of uncertified queries (search_core): the same pass, enabled on the device by `*gate > gate_lo`.
// Returns the queries one launch takes (32 at d <= 512, 16 at d = 640 .. 1024), 0 when there is no kernel for d.
int mfma_gated_queries(const mvdb_index* idx) {
    const int KB = idx->d / 16;
    if (idx->d % 128 != 0) return 0;  // the staged kernel only
    return KB <= 32 ? 32 : KB <= 64 ? 16 : 0;
}
int launch_mfma2_gated(int KB, const MfmaScanArgs& a, int device, hipStream_t s, int* nb, const int* gate, int gate_lo,
                       const int* need = nullptr, int npasses = 1, int per_pass = 0, int rtot = 0, int64_t cand_stride = 0) {
    if (per_pass <= 0) per_pass = a.nq;   // one pass of a.nq queries
    if (rtot <= 0) rtot = a.nq;
    if (a.nq <= 16) {
        // one query group: with two, a pass of <= 16 queries issues twice the MFMAs it needs and is bound by them (8 queries
        // under a bitmap at 10M x 512: 3.67 ms against 3.0 unfiltered)
        switch (KB) {
            case 8: return launch_mfma2_gated_inst<8, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
            case 16: return launch_mfma2_gated_inst<16, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
            case 24: return launch_mfma2_gated_inst<24, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
            case 32: return launch_mfma2_gated_inst<32, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
            default: break;
        }
    }
    switch (KB) {
        case 8: return launch_mfma2_gated_inst<8, 2, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 16: return launch_mfma2_gated_inst<16, 2, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 24: return launch_mfma2_gated_inst<24, 2, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 32: return launch_mfma2_gated_inst<32, 2, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 40: return launch_mfma2_gated_inst<40, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 48: return launch_mfma2_gated_inst<48, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 56: return launch_mfma2_gated_inst<56, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        case 64: return launch_mfma2_gated_inst<64, 1, 8>(a, device, s, nb, gate, gate_lo, need, npasses, per_pass, rtot, cand_stride);
        default: break;
    }
    return fail(MVDB_ERR_ARG, "no gated multi-query kernel for d = %d", KB * 16);
}

template <int NG>
int launch_mfma_ng(int KB, const MfmaScanArgs& a, int device, hipStream_t s, int* nb) {
    switch (KB) {
        case 4: return launch_mfma_inst<4, NG>(a, device, s, nb);   // (d = 64: the one width the staged kernel — d % 128 == 0 — does not serve)
        default: return fail(MVDB_ERR_ARG, "no multi-query kernel for d = %d", KB * 16);
    }
}

// nq >= 64, k <= 16: compute-bound tiled GEMM + top-k (scan_mfma_kernels.hpp, last section)
bool mfma_path_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev);
// Fewest queries of a call for the GEMM-tiled exact scan (128 queries per launch, compute-bound: one launch costs ~4.7 single
// scans at 10M x 512): 104 where the fp32-MFMA passes exist (32 queries per HBM-bound pass), 6 at the widths that have neither
// those nor the certified pass (d % 16 == 0 outside 64 / 128 / ... / 1024: the retired bf16-split generation served them).
int gemm_min_nq(const mvdb_index* idx, int k) {
    return mfma_path_ok(idx, 2, k, nullptr) ? idx->kn.gemm_scan_min_nq : std::min(idx->kn.gemm_scan_min_nq, 6);
}
bool gemm_path_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev) {
    if (idx->kn.disable_gemm_scan) return false;
    if (k > kGemmScanMaxK || rows_dev || idx->metric != MVDB_METRIC_IP || nq < gemm_min_nq(idx, k)) return false;
    return idx->d % 16 == 0 && idx->ld == idx->d;
}

int launch_gemm_scan(const mvdb_index* idx, const float* q, int nq, int k, int64_t n, uint64_t* cand,
                     hipStream_t stream, int* nblocks_out, const int* gate = nullptr, int gate_lo = 0) {
    GemmScanArgs a;
    a.X = idx->X.p;
    a.n = n;
    a.ld = idx->ld;
    a.K = idx->d;
    a.q = q;
    a.nq = nq;
    a.k = k;
    a.cand = cand;
    const size_t lds = (size_t)2 * 2 * 16 * 132 * 4 + (size_t)4 * 64 * k * 8;
    MVDB_TRY(ensure_dynamic_lds((const void*)flat_scan_gemm_kernel, lds, idx->device));
    int nb = cached_occupancy((const void*)flat_scan_gemm_kernel, 256, lds, 1);
    nb = std::min(nb, std::max(1, kn().gemm_scan_blocks_per_cu));
    const int qtiles = (nq + 127) / 128;
    const int64_t ntiles = (n + 127) / 128;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)device_cus(idx->device) * nb / qtiles));
    *nblocks_out = gx;
    if (gate) {
        MVDB_TRY(ensure_dynamic_lds((const void*)flat_scan_gemm_gated_kernel, lds, idx->device));
        hipLaunchKernelGGL(flat_scan_gemm_gated_kernel, dim3(gx, qtiles), dim3(256), lds, stream, a, gate, gate_lo);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    return profiled_launch("ip_scan_gemm", stream, [&](hipEvent_t done) { launch_kernel(flat_scan_gemm_kernel, dim3(gx, qtiles), dim3(256), lds, stream, done, a); });
}

// Chunks that held an uncertified query, counted ON THE DEVICE (split_plan_kernel): the host never reads a certification
// flag on the search path.  One counter per device, read (with a device synchronise) by mvdb_split_rerun_count().
std::mutex g_rerun_mu;
std::map<int, unsigned long long*> g_rerun_ctr;
unsigned long long* rerun_counter(int device) {
    std::lock_guard<std::mutex> lk(g_rerun_mu);
    auto it = g_rerun_ctr.find(device);
    if (it != g_rerun_ctr.end()) return it->second;
    unsigned long long* p = nullptr;
    // [0] refused chunks, [1] tiles the rescue launches were handed, [2] tiles they would have scanned without the tile flags
    if (hipMalloc((void**)&p, 3 * sizeof(*p)) != hipSuccess || hipMemset(p, 0, 3 * sizeof(*p)) != hipSuccess) return nullptr;
    g_rerun_ctr[device] = p;
    return p;
}

// k the certified pass serves: it re-scores 64 nominees, so its certificate compares the k-th exact score with the ~64th
// approximate one: at k = 32 the gap is still ~6 eps on
// exchangeable data (10M x 512 random rows: 32nd to 64th score 6.1e-3, eps 1.04e-3; 1.6e-2 at k = 10)
constexpr int kHalfMaxK = 32;
bool half_path_ok(const mvdb_index* idx);
int mfma_gated_queries(const mvdb_index* idx);

// L2 metric on the certified passes: they nominate by inner product, which ranks like the distance when the stored rows have
// (nearly) one norm — every row of the drop-in classes is normalised.  The certificate (topk_device.hpp: l2_certified) is
// exact for ANY spread, but a wide one would make most queries fail it; beyond 2^-10 relative the exact kernels serve.
bool l2_cert_ok(const mvdb_index* idx) {
    return idx->metric == MVDB_METRIC_L2 && idx->norm2_hi > 0.f && std::isfinite(idx->norm2_hi) &&
           idx->norm2_hi - idx->norm2_lo <= idx->norm2_hi * (1.0f / 1024.0f) && !idx->kn.disable_l2_cert;
}
// ... and rows of ANY norms where the nomination pass runs over the fp16 shadow: it then nominates by q.x - |x|^2 / 2 with
// per-row offsets kept beside the shadow (launch_half_pass: l2off).  True when a batch of nq queries over n rows would take
// that pass.
bool half_path_ok(const mvdb_index* idx);
int half_min_nq(const mvdb_index* idx, int64_t n);
bool l2_offsets_ok(const mvdb_index* idx, int nq, int64_t n) {
    return idx->metric == MVDB_METRIC_L2 && !idx->kn.disable_l2_cert && half_shadow_dim(idx->d) && idx->ld == idx->d &&
           !idx->kn.disable_half_shadow && !idx->shadow.failed && half_path_ok(idx) && nq >= half_min_nq(idx, n);
}

// Fewest queries of a call that go to the certified passes.  Where the fp16 nomination pass streams the SHADOW of the rows
// (d = 256 / 384 / 512), one pass over n rows costs about what 0.55 n rows cost the exact scans, whatever the number of
// queries up to 128 — it beats the fp32-MFMA pass from TWO queries on once the corpus is big enough to bury its fixed cost
// (seed launch, phase merges, certification: ~0.1 ms).  Measured, device time per call, default / certified
// (profiles/r04_small_batch_crossover.jsonl): 10M x 512: 2 queries 2.93 / 1.61 ms, 32 queries 3.06 / 1.63; 1M rows: 2 queries
// 0.33 / 0.26, 13 queries 0.44 / 0.27; 100k rows: 2 queries 0.068 / 0.114, 8 queries 0.123 / 0.122, 13 queries 0.170 / 0.126.
// MVDB_SPLIT_SCAN_MIN_NQ overrides (the name dates from the retired split-precision passes).
// Tile flags cost a call that refuses nothing ~0.8 % (one compare + ballot per tile and wave, the flags' memset), so they are kept
// adaptively: split_plan_kernel mirrors a running count of refused certificates into a host-mapped word; when the word has moved
// since this index last looked, the next kTileFlagCalls certified calls keep flags (the call that FIRST meets refusals pays a
// whole-shadow rescue launch, the following ones walk tile lists).  MVDB_TILE_FLAGS=1: always, 0 (or MVDB_DISABLE_TILE_SKIP=1): never.
constexpr int kTileFlagCalls = 1024;
bool tile_flags_wanted(const mvdb_index* idx) {
    if (idx->kn.disable_tile_skip || idx->kn.tile_flags_mode == 0) return false;
    if (idx->kn.tile_flags_mode == 1) return true;
    if (!idx->rf.dev()) return false;
    const unsigned int v = idx->rf.read(0);
    if (v != idx->rf_seen.load(std::memory_order_relaxed)) {
        idx->rf_seen.store(v, std::memory_order_relaxed);
        idx->rf_calls_left.store(kTileFlagCalls, std::memory_order_relaxed);
    }
    if (idx->rf_calls_left.load(std::memory_order_relaxed) <= 0) return false;
    idx->rf_calls_left.fetch_sub(1, std::memory_order_relaxed);
    return true;
}

thread_local bool tls_single_suspended = false;  // decided once per search (search_core), read by every routing question of that call

int half_min_nq(const mvdb_index* idx, int64_t n) {
    if (idx->kn.split_scan_min_nq >= 0) return idx->kn.split_scan_min_nq;
    if (half_shadow_dim(idx->d) && idx->ld == idx->d && !idx->kn.disable_half_shadow && !idx->shadow.failed) {
        // (opt-in, MVDB_SHADOW_SINGLE_QUERY=1: ONE query too — 10M x 512: 2.86 -> ~1.6 ms per query, certified like any batch; off
        //  by default: the single-query scan is the headline's exact fp32 kernel and its roofline is defined on the fp32 bytes)
        if (n >= 500000) return idx->kn.shadow_single_query && !tls_single_suspended ? 1 : 2;
        if (n >= 100000) return 8;
    }
    return 33;
}

// Does a call of nq queries over n rows go through the CERTIFIED pass (fp16 nomination over the shadow, half_scan.hip)?
// (Until round 6 a second certified generation — bf16 (hi, lo) split products over the fp32 rows, scan_split_kernels.hpp —
//  served the widths without an fp16 kernel; it is retired: those widths take the exact passes below.)
bool split_path_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev, int64_t n) {
    if (idx->kn.disable_split_scan || !half_path_ok(idx)) return false;
    if (nq < half_min_nq(idx, n) || (nq == 1 && !(idx->kn.shadow_single_query && !tls_single_suspended))) return false;
    if (rows_dev || (idx->metric != MVDB_METRIC_IP && !l2_cert_ok(idx) && !l2_offsets_ok(idx, nq, n))) return false;
    // (k > 16 also needs the gated fp32-MFMA pass for the exact re-runs: the GEMM-tiled scan keeps 16 results per query)
    if (k > kHalfMaxK || (k > kGemmScanMaxK && mfma_gated_queries(idx) <= 0)) return false;
    // rows of known, sane norm only: the bound scales with max|x|
    if (!(idx->row_norm_bound > 0.f) || !(idx->row_norm_bound < 1.0e30f)) return false;
    return true;
}

// Between the launches of a certified pass: merge the per-block lists of a launch (the seed launch: one tile per block) — and
// the running nominees of the launches before it — into each query's 16
// best approximate keys, and publish the 16th score as the admission floor of the main launch — every row of the
// global approximate top-16 scores at least that much, so the main pass only has to insert the few rows above it
// (without the floor each wave re-learns its threshold from scratch: ~7,000 LDS list inserts per wave at 10M rows,
// more time than the MFMAs).
__global__ __launch_bounds__(1024) void phase_fold_kernel(const uint64_t* __restrict__ keys, int nlists,
                                                          const uint64_t* prev, uint64_t* seed, float* __restrict__ thr0) {
    // prev: NULL, or the [nq][16] running nominees of the earlier phases (may alias `seed`: read before written)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const int64_t total = (int64_t)nlists * kHalfKeep;
    const uint64_t* src = keys + (int64_t)qi * total;
    WaveTopK tk;
    tk.init(kHalfKeep);
    for (int64_t base = (int64_t)wave * 64; base < total; base += 1024) {
        const int64_t i = base + lane;
        tk.offer(i < total ? src[i] : 0ull);
    }
    if (prev && wave == 0) tk.offer(lane < kHalfKeep ? prev[(int64_t)qi * kHalfKeep + lane] : 0ull);
    __shared__ uint64_t sh[15 * 64];
    block_merge_topk(tk, sh, 16);
    if (wave == 0) {
        if (lane < kHalfKeep) seed[(int64_t)qi * kHalfKeep + lane] = tk.key;
        const uint64_t last = readlane_u64(tk.key, kHalfKeep - 1);
        if (lane == 0) thr0[qi] = last ? key_score(last) : -INFINITY;
    }
}

// ---- fp16 single-product nomination pass (half_scan.hip): 33+ queries per corpus pass where a kernel exists ----------
// (the pass streams the fp16 SHADOW of the rows: an index that may not keep one — option half_shadow = 0, or the shadow's
//  allocation failed — answers its batches on the exact fp32 passes)
bool half_path_ok(const mvdb_index* idx) {
    if (idx->kn.disable_half_scan || idx->kn.disable_half_shadow || idx->shadow.failed) return false;
    return half_max_queries(idx->d) > 0 && half_shadow_dim(idx->d) && idx->ld == idx->d && half_xscale(idx->row_norm_bound) > 0.f;
}

bool code8_route_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev, const uint64_t* mask_dev, int64_t n);
bool code8_front_wanted(int option, int d);   // whether an index of width d keeps the front plane under this value of code8_front_plane
int code8_search(const mvdb_index* idx, Workspace* ws, const ScanArgs& a, int k, int64_t label_offset, float* D_dev, int64_t* I_dev,
                 bool* served);

int launch_half_pass(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int nqpad, int k, int64_t n,
                     int64_t label_offset, float* D, int64_t* I, int* flag, int* failed, const uint32_t* mask = nullptr,
                     float* floor_out = nullptr, uint32_t* tflags = nullptr, int twords = 0, bool* flags_written = nullptr) {
    hipStream_t stream = ws->stream;
    if (flags_written) *flags_written = false;
    _Float16* qf = reinterpret_cast<_Float16*>(ws->qsplit.p);
    float* qnorm = ws->qnorm.p;
    float* floors = qnorm + nqpad;
    float* qinv = qnorm + 2 * nqpad;
    const float xscale = half_xscale(idx->row_norm_bound);
    MVDB_TRY(launch_half_queries(q, idx->ld, idx->d, nq, nqpad, xscale, qf, qnorm, qinv, stream));
    HalfScanArgs a;
    a.X = idx->X.p;
    a.n = n;
    a.ld = idx->ld;
    a.qf = qf;
    a.qinv = qinv;
    a.xscale = xscale;
    a.nq = nq;
    a.mask = mask;
    a.Xh = idx->shadow.ensure(idx, stream, xscale);
    a.stats = idx->kn.split_stats ? reinterpret_cast<unsigned int*>(ws->flags.p) + (ws->flags.cap - 32) : nullptr;
    if (a.stats) MVDB_HIP(hipMemsetAsync(a.stats, 0, 8, stream));
    const int64_t ntiles = (n + 31) / 32;
    const int cus = device_cus(idx->device);
    uint64_t* seed_keys = ws->cand.p;                           // [nqpad][16] running nominees
    uint64_t* cand = ws->cand.p + (size_t)nqpad * kHalfKeep;   // [nq][lists][16]
    a.cand = cand;
    // SEED launch: the first min(tiles, CUs) tiles, one per block, every score dumped (32 keys per block and query);
    // phase_fold_kernel keeps each query's 16 best and publishes the 16th score as the first admission floor.
    const int64_t seed_tiles = std::min<int64_t>(ntiles, cus);
    int gx = 0;
    a.tile0 = 0;
    a.tile1 = seed_tiles;
    a.thr0 = nullptr;
    // L2 metric over rows of MIXED norms (round 4; rows of one norm keep the cheaper inner-product nomination with the norm-range
    // certificate): rows are nominated by q.x - |x|^2 / 2 with the per-row offsets kept beside the shadow (section 4.3e); the
    // seed is then the shadow kernel itself without a floor — one tile per block, its 16 best per query — because the fp32
    // seed kernel knows no offsets.
    const float* hn = idx->metric == MVDB_METRIC_L2 && a.Xh && !l2_cert_ok(idx) && !idx->kn.disable_l2_cert ? idx->shadow.ensure_offsets(idx, stream)
                                                                                                          : nullptr;
    const bool l2off = hn != nullptr;
    if (l2off) {
        a.hn = hn;
        MVDB_TRY(launch_half_scan(idx->d, nqpad, false, a, idx->device, stream, &gx));
        hipLaunchKernelGGL(phase_fold_kernel, dim3(nq), dim3(1024), 0, stream, cand, gx, (const uint64_t*)nullptr, seed_keys, floors);
    } else {
        MVDB_TRY(launch_half_scan(idx->d, nqpad, true, a, idx->device, stream, &gx));
        hipLaunchKernelGGL(phase_fold_kernel, dim3(nq), dim3(1024), 0, stream, cand, 2 * gx, (const uint64_t*)nullptr,
                           seed_keys, floors);
    }
    MVDB_HIP(hipGetLastError());
    a.thr0 = floors;
    // The rest of the corpus is scanned in PHASES of growing size; between phases phase_fold_kernel folds the
    // per-block lists into the running 16 best and raises the floors (a block alone sees n / CUs rows: without the
    // refreshed floors its lists take hundreds of serial LDS inserts per wave).  Planned backwards: the LAST phase
    // covers at most `last_growth` times the rows before it — that leaves ~16 x last_growth candidates above its
    // floor for the 64-nominee certificate —, the earlier ones up to `growth` times.
    // Growth 16 / 6 (three main launches at 10M rows) up to 128 queries per pass; 6 / 4 (four) at 256, where a wave's insert
    // path stalls eight waves at the tile barrier and the rounds it takes scale with the sum of the growth factors
    // (profiles/r05_h16_phase_sweep.txt: 256 queries +3 - 5 % at 10M rows, +1 % at 1M; 128 / 32 queries lose 0.5 - 8 % to the extra
    // launch and merge, and keep 16 / 6).
    // (k <= 16 only: the floor the last phase starts from is the 16th best of the rows before it, and the k-th result has to
    //  beat it — with a quarter of the corpus before the last phase and k = 32, 16 of the 32 best fall into that quarter once
    //  in ~500 queries and the query is refused and re-run; a sixth: once in 1e5)
    const bool wide_pass = nqpad == 256 && k <= kHalfKeep;
    const int growth = std::max(2, idx->kn.half_phase_growth ? idx->kn.half_phase_growth : wide_pass ? 6 : 16);
    const int last_growth = std::max(2, idx->kn.half_last_growth ? idx->kn.half_last_growth : wide_pass ? 4 : 6);
    std::vector<int64_t> ends;
    for (int64_t b = ntiles, g = last_growth; b > seed_tiles; g = growth) {
        ends.push_back(b);
        b = (b + g - 1) / g;
        if (b <= 2 * seed_tiles) break;
    }
    int last_lists = 0;
    int64_t covered = seed_tiles;
    // Tile flags for the rescue pass (inner product, k <= 16; search_core decides).  With B = max|x| and e = half_eps(d) B: a
    // refused query's rescue launch admits rows with a(x) >= F = fl - e |q|, fl = t - m |q| (one ulp down), t the k-th fp32
    // re-score among the 64 nominees R, m = floor_margin = 2 d 2^-24 B.  At ANY moment of ANY main launch the threshold `thr` a
    // wave holds for the query (the larger of the phase's floor — the 16th best a() of the rows before the phase — and the 16th
    // of its list) is reached by at least 16 >= k candidates that are folded into R's pool, so R's k-th best a() is >= thr; a
    // nominee's re-score is >= a(x) - (e + m / 2) |q|; hence t >= thr - (e + m / 2) |q| and F >= thr - (2 e + 3 m / 2) |q| - ulp.
    // A tile whose best score stays below thr - flag_coef |q|, flag_coef = 2.25 e + 2 m, cannot hold an admitted row.
    if (tflags && !l2off && idx->metric == MVDB_METRIC_IP && k <= kHalfKeep) {
        a.tflags = tflags;
        a.twords = twords;
        a.flag_qn = qnorm;
        const double B = (double)idx->row_norm_bound;
        a.flag_coef = (float)((2.25 * half_eps(idx->d) + 4.0 * idx->d * std::ldexp(1.0, -24)) * B * (1.0 + 1e-6));
        if (flags_written) *flags_written = true;  // (the caller hands the rescue pass tile lists only if EVERY chunk's launches wrote flags)
    }
    for (size_t p = ends.size(); p-- > 0;) {
        a.tile0 = covered;
        a.tile1 = ends[p];
        MVDB_TRY(launch_half_scan(idx->d, nqpad, false, a, idx->device, stream, &gx));
        covered = ends[p];
        if (p > 0) {
            hipLaunchKernelGGL(phase_fold_kernel, dim3(nq), dim3(1024), 0, stream, cand, gx, seed_keys, seed_keys, floors);
            MVDB_HIP(hipGetLastError());
        } else {
            last_lists = gx;
        }
    }
    HalfCertifyArgs c;
    c.keys = cand;
    c.nlists = last_lists;
    c.base = seed_keys;
    c.thr0 = floors;
    c.X = idx->X.p;
    c.ld = idx->ld;
    c.d4 = idx->d4;
    c.q = q;
    c.qnorm = qnorm;
    c.eps = (float)(half_eps(idx->d) * (double)idx->row_norm_bound * (1.0 + 1e-6));  // rounded up
    c.k = k;
    c.label_offset = label_offset;
    c.D = D;
    c.I = I;
    c.uncertified = flag;
    c.failed = failed;
    c.l2 = l2off ? 2 : idx->metric == MVDB_METRIC_L2 ? 1 : 0;
    c.n2lo = idx->norm2_lo;
    c.floor_out = floor_out;
    c.floor_margin = (float)(2.0 * idx->d * std::ldexp(1.0, -24) * (double)idx->row_norm_bound * (1.0 + 1e-6));
    if (l2off) {
        // the stored |x|^2 / 2 (relative error < 2^-18, half_norms_kernel) and the fp32 subtraction a(x) - h (2^-23 of the larger)
        const double B = (double)idx->row_norm_bound;
        c.eps_h = (float)((std::ldexp(1.0, -18) + std::ldexp(1.0, -22)) * 0.5 * B * B * (1.0 + 1e-6));
        c.eps = (float)((double)c.eps + std::ldexp(1.0, -22) * B * (1.0 + 1e-6));
    }
    MVDB_TRY(launch_half_certify(c, nq, stream));
    if (a.stats) {
        unsigned int st[2] = {0, 0};
        MVDB_HIP(hipMemcpyAsync(st, a.stats, sizeof(st), hipMemcpyDeviceToHost, stream));
        MVDB_HIP(hipStreamSynchronize(stream));
        fprintf(stderr, "[mvdb half] list inserts %u, slow-path wave-rounds %u, %zu main launches\n", st[0], st[1], ends.size());
    }
    return 0;
}

bool mfma_path_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev) {
    if (idx->kn.disable_mfma_scan) return false;
    if (nq < 2 || k > kMaxFusedK || rows_dev) return false;
    if (idx->d % 16 || idx->ld != idx->d) return false;
    // squared L2 as |q|^2 + |x|^2 - 2 q.x: the staged kernel only (it sees whole rows go by)
    // (d <= 768: at d = 1024 the L2 form of the kernel spills; two 16-query groups only up to d = 384, same reason)
    if (idx->metric != MVDB_METRIC_IP && !(idx->d % 128 == 0 && idx->d <= 768 && !idx->kn.disable_l2_mfma)) return false;
    const int KB = idx->d / 16;
    return KB == 4 || KB == 8 || KB == 16 || KB == 24 || KB == 32 || KB == 40 || KB == 48 || KB == 56 || KB == 64;
}

// Core: queries already on the device (padded to ld), outputs on the device.  Enqueues on ws.stream.
// (Round 2 had an opt-in "dense subset" route here — score every row, pick the subset's scores out, radix-select over
// them — measured slower than the gather; round 3 replaced it by the bitmap-selected scan, mvdb_index_search_masked.)
// label of result = position p with rows = the ascending list of the mask's set bits: p = number of set bits below the row
__global__ __launch_bounds__(256) void mask_rank_kernel(int64_t* __restrict__ I, const uint64_t* __restrict__ mask) {
    __shared__ int part[256];
    const int64_t row = I[blockIdx.x];
    if (row < 0) return;  // block-uniform
    const int64_t words = row >> 6;
    int c = 0;
    for (int64_t w = threadIdx.x; w < words; w += 256) c += __popcll(mask[w]);
    if (threadIdx.x == 0 && (row & 63)) c += __popcll(mask[words] & ((1ull << (row & 63)) - 1ull));
    part[threadIdx.x] = c;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) part[threadIdx.x] += part[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) I[blockIdx.x] = part[0];
}

// The queries a multi-query pass reads: the caller's, or their normalised copy in ws->qn.
int normalized_queries(const mvdb_index* idx, Workspace* ws, const float* q_dev, int nq, int normalize_q, const float** qsrc) {
    *qsrc = q_dev;
    if (!normalize_q) return 0;
    MVDB_TRY(ws->qn.reserve((size_t)nq * idx->ld));
    MVDB_HIP(hipMemcpyAsync(ws->qn.p, q_dev, (size_t)nq * idx->ld * sizeof(float), hipMemcpyDeviceToDevice, ws->stream));
    MVDB_TRY(normalize_range(idx, ws->qn.p, nq, ws->stream));
    *qsrc = ws->qn.p;
    return 0;
}

// Merge the per-block lists a scan left in ws->cand into the k results of `nq` queries (one block per query).  gate / gate_lo:
// the device-side enable of an exact re-run (query b is merged iff *gate > gate_lo + b); need / per_pass / pass_stride: the
// second enable, one word per pass of per_pass queries whose lists start pass_stride keys apart (scan_kernels.hpp: MergeArgs).
int launch_merge(const mvdb_index* idx, Workspace* ws, int nq, int nlists, int k, int64_t label_offset, float* D, int64_t* I,
                 const int* gate = nullptr, int gate_lo = 0, const int* need = nullptr, int per_pass = 0, int64_t pass_stride = 0) {
    MergeArgs mg;
    mg.keys = ws->cand.p;
    mg.nlists = nlists;
    mg.k = k;
    mg.metric = idx->metric;
    mg.label_offset = label_offset;
    mg.D = D;
    mg.I = I;
    mg.gate = gate;
    mg.gate_lo = gate_lo;
    mg.need = need;
    mg.per_pass = per_pass;
    mg.pass_stride = pass_stride;
    hipLaunchKernelGGL(merge_keys_kernel, dim3(nq), dim3(kMergeThreads), 0, ws->stream, mg);
    MVDB_HIP(hipGetLastError());
    return 0;
}

constexpr int kCoreTile = 1024;      // queries search_core answers per pass over its workspace
constexpr int64_t kShiftMaxRows = 8;           // most scattered deleted rows of a call the one-pass compaction takes (a run of any length qualifies)
constexpr size_t kShiftSideBytes = 64u << 20;   // ... and the most its side copies may occupy
constexpr size_t kTileFlagMaxBytes = 512u << 20;  // the most the certified pass's tile flags may occupy (queries of the call x tiles / 8)
constexpr int kGatedPassGroup = 8;   // exact re-run passes (of 16 / 32 compact queries) one gated launch walks: one list buffer of that many

// The certified batch pass (search_core's route for batches; half_scan.hip): ONE fp16 product over the shadow nominates, fp32
// re-scores decide, a worst-case bound certifies; queries whose certificate is refused are re-run on the exact kernels,
// enabled on the device.  `a`: the scan arguments of the call (the L2 re-run launches the single-query scan with them).
// *answered: the leading queries of the call the pass took — the rest (fewer than the pass is worth) is the caller's;
// *qsrc_out: the queries as the pass read them (normalised where the call asks for it).
int certified_batch(const mvdb_index* idx, Workspace* ws, const ScanArgs& a, const float* q_dev, int nq, int k, int normalize_q, int64_t n,
                    int64_t label_offset, float* D_dev, int64_t* I_dev, const uint64_t* mask_dev, int* answered, const float** qsrc_out) {
    hipStream_t s = ws->stream;
    const uint32_t* mask32 = reinterpret_cast<const uint32_t*>(mask_dev);
    const float* qsrc = nullptr;
    MVDB_TRY(normalized_queries(idx, ws, q_dev, nq, normalize_q, &qsrc));
    *qsrc_out = qsrc;
    // chunk plan: 128 / 256 queries per pass while at least min_nq remain; what is left takes the exact passes
    const int min_nq = half_min_nq(idx, n);
    const int chunk = half_max_queries(idx->d);
    std::vector<std::pair<int, int>> plan;  // (first query, count)
    int q0 = 0;
    // (L2 over rows of mixed norms: the pass nominates by q.x - |x|^2 / 2 with per-row offsets beside the shadow; rows of one
    //  norm by inner product, which ranks like the distance then)
    const bool ip_ranks = idx->metric == MVDB_METRIC_IP || l2_cert_ok(idx);
    while (nq - q0 >= min_nq && (ip_ranks || l2_offsets_ok(idx, nq - q0, n))) {
        plan.emplace_back(q0, std::min(nq - q0, chunk));
        q0 += plan.back().second;
    }
    const int nchunks = (int)plan.size();
    if (nchunks > 0) {
        MVDB_TRY(ws->qsplit.reserve((size_t)std::max(2 * 128, chunk) * idx->d));
        MVDB_TRY(ws->qnorm.reserve((size_t)std::max(256, 3 * chunk)));  // |q|, admission floors, 1 / scale
        MVDB_TRY(ws->flags.reserve((size_t)std::max(nchunks, 64) + 32));  // + diagnostics counters in the last 32 slots
        MVDB_TRY(ws->cand.reserve((size_t)std::max(128, chunk) * (scan_grid_upper_bound(idx->device) + 1) * kHalfKeep));
        MVDB_TRY(ws->qfail.reserve((size_t)q0));
        MVDB_TRY(ws->qfloor.reserve((size_t)2 * q0 + 128));  // [q0] per query | [q0 + 128] per compact slot
        MVDB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws->qfloor.p), 0xff800000u, (size_t)q0, s));  // -inf: no floor
        MVDB_HIP(hipMemsetAsync(ws->flags.p, 0, (size_t)nchunks * sizeof(int), s));
        MVDB_HIP(hipMemsetAsync(ws->qfail.p, 0, (size_t)q0 * sizeof(int), s));
        // Tile flags (round 6): the main launches note, per query, which 32-row tiles came near its running threshold; should the
        // query be refused, its rescue launch walks those tiles only (clustered 10M x 512, 256 per call: 2.6 % of the shadow).  Inner product, k <= 16 (the floors are 16th-best scores), from ~400k rows on (below, the rescue launch is
        // short and the flags' memset is not), at most 512 MiB of flags — and only while the index has been refusing
        // certificates (tile_flags_wanted): a corpus that certifies everything never pays for them.
        const int64_t ntiles_all = (n + 31) / 32;
        const int twords = (int)((ntiles_all + 31) / 32);
        const bool tile_flags = idx->metric == MVDB_METRIC_IP && k <= kHalfKeep && ntiles_all >= idx->kn.tile_flag_min_tiles && tile_flags_wanted(idx) &&
                                !idx->kn.disable_rescue && !idx->kn.disable_rerun_floor && half_rescue_dim(idx->d) &&
                                (size_t)q0 * twords * sizeof(uint32_t) <= kTileFlagMaxBytes;
        if (tile_flags) {
            MVDB_TRY(ws->tflags.reserve((size_t)q0 * twords));
            MVDB_HIP(hipMemsetAsync(ws->tflags.p, 0, (size_t)q0 * twords * sizeof(uint32_t), s));
        }
        bool flags_ok = tile_flags;  // ... and every chunk's main launches did write them (launch_half_pass decides per chunk)
        for (int c = 0; c < nchunks; ++c) {
            const int c0 = plan[c].first, take = plan[c].second;
            bool wrote = false;
            MVDB_TRY(launch_half_pass(idx, ws, qsrc + (int64_t)c0 * idx->ld, take, half_chunk_queries(idx->d, take), k, n, label_offset,
                                      D_dev + (int64_t)c0 * k, I_dev + (int64_t)c0 * k, ws->flags.p + c, ws->qfail.p + c0, mask32,
                                      ws->qfloor.p + c0, tile_flags ? ws->tflags.p + (size_t)c0 * twords : nullptr, twords, &wrote));
            flags_ok = flags_ok && wrote;
        }
        // ---- uncertified queries: re-run on the exact kernels WITHOUT the host ever learning which they were ----------
        // split_plan_kernel compacts the failed queries (ascending) and publishes their number nb; the exact passes below
        // are launched unconditionally over the compact batch and enabled on the device: a launch whose query range
        // starts at or beyond nb returns at once (a few microseconds each when every query certified — the usual case).
        //   compact queries [0, 64): two 32-query fp32-MFMA passes (one corpus pass each: a handful of duplicate-heavy
        //                            neighbourhoods in a batch cost about one pass);
        //   the rest, in 128s:       the GEMM-tiled exact scan (a whole chunk failing: duplicate-heavy data).
        // No stream synchronise, no device-to-host copy: the call can be captured into a hipGraph (after one eager call
        // has sized the workspace) and an encoder -> search chain stays one enqueue.
        unsigned long long* ctr = rerun_counter(idx->device);
        if (!ctr) return fail(MVDB_ERR_OOM, "device allocation for the re-run counter failed");
        const int R = q0;  // most queries that can fail
        MVDB_TRY(ws->nfail.reserve(1));
        MVDB_TRY(ws->relabel.reserve((size_t)R * (1 + k)));
        MVDB_TRY(ws->requery.reserve((size_t)(R + 128) * idx->ld + (size_t)R * k));  // + one query tile of slack for the scans
        int64_t* map = ws->relabel.p;
        int64_t* It = map + R;
        float* qc = ws->requery.p;
        float* Dt = qc + (size_t)(R + 128) * idx->ld;
        unsigned int* sq_dev = nullptr;
        volatile unsigned int* sq_host = nullptr;
        if (nq == 1 && idx->kn.shadow_single_query) {  // the opt-in single-query route reports its refusals (sq_route)
            std::lock_guard<std::mutex> lk(idx->shadow_mu);
            if (idx->sq_fail.dev() || (!stream_capturing(s) && idx->sq_fail.ensure(1, &s))) {
                sq_dev = idx->sq_fail.dev();
                sq_host = idx->sq_fail.mirror();
            }
            (void)hipGetLastError();  // (unconditional, as the clear behind rf's creation: ShadowStore::ensure)
        }
        hipLaunchKernelGGL(split_plan_kernel, dim3(1), dim3(64), 0, s, (const int*)ws->flags.p, nchunks, (const int*)ws->qfail.p, q0,
                           map, ws->nfail.p, ctr, sq_dev, sq_host, idx->rf.dev(), idx->rf.mirror());
        {
            const int64_t rows = R + 128, gtotal = rows * (idx->ld / 4);
            const int ggrid = (int)std::min<int64_t>((gtotal + 255) / 256, (int64_t)device_cus(idx->device) * 8);
            hipLaunchKernelGGL(gather_failed_kernel, dim3(ggrid), dim3(256), 0, s, qc, qsrc, (const int64_t*)map,
                               (const int*)ws->nfail.p, rows, idx->ld, (const float*)ws->qfloor.p, ws->qfloor.p + q0);
        }
        MVDB_HIP(hipGetLastError());
        const int per_pass = mfma_gated_queries(idx);
        const int KB = idx->d / 16;
        int off = 0;
        // ---- the RESCUE pass (half_scan.hip): refused queries once more over the shadow, 128 at a time, every row above
        // the query's floor — what the k-th exact score (L2: distance) of its nominees admits, less the nomination error —
        // kept and re-scored in fp32; what it answers the exact passes skip.  need_per = compact queries per `need` word:
        // the queries of one exact pass (inner product: a gated fp32-MFMA pass of 32 / 16), or 1 (L2: one gated scan each).
        auto rescue = [&](int need_per, const int** need_out) -> int {
            *need_out = nullptr;
            const float xs = half_xscale(idx->row_norm_bound);
            if (need_per <= 0 || kRescueQueries % need_per != 0 || !half_rescue_dim(idx->d) || idx->ld != idx->d || k > kRescueKeep ||
                idx->kn.disable_rescue || idx->kn.disable_rerun_floor || !(xs > 0.f))
                return 0;
            const _Float16* Xh = idx->shadow.ensure(idx, s, xs);
            if (!Xh) return 0;
            // (L2: the same nomination form the certified pass used — per-row offsets where the rows' norms differ)
            const bool l2 = idx->metric == MVDB_METRIC_L2;
            const float* hn = l2 && !l2_cert_ok(idx) && !idx->kn.disable_l2_cert ? idx->shadow.ensure_offsets(idx, s) : nullptr;
            if (l2 && !l2_cert_ok(idx) && !hn) return 0;
            const int grid_ub = device_cus(idx->device) * kRescueBlocksPerCu;  // the rescue launch: one or two workgroups per CU
            const int slots = (R + kRescueQueries - 1) / kRescueQueries;
            const size_t nneed = (size_t)(R + kRescueQueries) / need_per + 8;
            const size_t nwords = nneed + slots;  // ... and the tile lists' lengths behind the need words (one memset)
            MVDB_TRY(ws->need.reserve(nwords));
            MVDB_TRY(ws->tlist.reserve((size_t)slots * ntiles_all));
            MVDB_TRY(ws->cand.reserve((size_t)kRescueQueries * (grid_ub + 1) * kRescueKeep));
            MVDB_TRY(ws->qsplit.reserve((size_t)2 * kRescueQueries * idx->d));
            MVDB_TRY(ws->qnorm.reserve((size_t)3 * kRescueQueries));
            MVDB_HIP(hipMemsetAsync(ws->need.p, 0, nwords * sizeof(int), s));
            _Float16* qf = reinterpret_cast<_Float16*>(ws->qsplit.p);
            float* qn2 = ws->qnorm.p;
            float* qinv = qn2 + 2 * kRescueQueries;
            float eps = (float)(half_eps(idx->d) * (double)idx->row_norm_bound * (1.0 + 1e-6));
            if (hn) eps = (float)((double)eps + std::ldexp(1.0, -22) * (double)idx->row_norm_bound * (1.0 + 1e-6));  // (launch_half_pass: the subtraction)
            {   // the launches' tile lists: what the refused queries' flags name (no flags: every tile)
                RescueTilesArgs ta;
                ta.tflags = flags_ok ? ws->tflags.p : nullptr;
                ta.twords = twords;
                ta.map = map;
                ta.nfail = ws->nfail.p;
                ta.seed_tiles = std::min<int64_t>(ntiles_all, device_cus(idx->device));  // (launch_half_pass: the seed launch's tiles)
                ta.ntiles = ntiles_all;
                ta.lists = ws->tlist.p;
                ta.counts = ws->need.p + nneed;
                ta.stats = ctr + 1;
                MVDB_TRY(launch_rescue_tiles(ta, slots, s));
            }
            for (int off2 = 0; off2 < R; off2 += kRescueQueries) {
                MVDB_TRY(launch_half_queries(qc + (int64_t)off2 * idx->ld, idx->ld, idx->d, kRescueQueries, kRescueQueries, xs, qf, qn2,
                                             qinv, s));
                HalfScanArgs ra;
                ra.X = idx->X.p;
                ra.n = n;
                ra.ld = idx->ld;
                ra.qf = qf;
                ra.qinv = qinv;
                ra.xscale = xs;
                ra.nq = std::min(kRescueQueries, R - off2);  // (slots past the call's queries can never be live)
                ra.mask = mask32;
                ra.Xh = Xh;
                ra.hn = hn;
                ra.stats = nullptr;
                ra.cand = ws->cand.p;
                ra.tile0 = 0;
                ra.tile1 = (n + 31) / 32;
                ra.thr0 = ws->qfloor.p + q0 + off2;
                ra.thr_eps = eps;
                ra.thr_qn = qn2;
                ra.gate = ws->nfail.p;
                ra.gate_lo = off2;
                ra.tile_list = ws->tlist.p + (size_t)(off2 / kRescueQueries) * ntiles_all;
                ra.tile_count = ws->need.p + nneed + off2 / kRescueQueries;
                int gx = 0;
                MVDB_TRY(launch_half_rescue_scan(idx->d, ra, idx->device, s, &gx));
                HalfRescueArgs rc;
                rc.keys = ws->cand.p;
                rc.nlists = gx;
                rc.X = idx->X.p;
                rc.ld = idx->ld;
                rc.d4 = idx->d4;
                rc.q = qc + (int64_t)off2 * idx->ld;
                rc.k = k;
                rc.label_offset = label_offset;
                rc.D = Dt + (int64_t)off2 * k;
                rc.I = It + (int64_t)off2 * k;
                rc.gate = ws->nfail.p;
                rc.gate_lo = off2;
                rc.need = ws->need.p + off2 / need_per;
                rc.per_pass = need_per;
                rc.l2 = l2 ? 1 : 0;
                MVDB_TRY(launch_half_rescue_certify(rc, s));
            }
            *need_out = ws->need.p;
            return 0;
        };
        if (idx->metric == MVDB_METRIC_L2) {
            // L2: the rescue pass, then — for what it could not hold — the exact single-query scan (sum (q - x)^2 directly),
            // 32 compact queries per launch, each query's blocks enabled on the device (refused count and `need` word)
            const int* need = nullptr;
            MVDB_TRY(rescue(1, &need));
            const int per = 32;
            MVDB_TRY(ws->cand.reserve((size_t)per * scan_grid_upper_bound(idx->device) * k));
            for (; off < R; off += per) {
                const int take = std::min(per, R - off);
                ScanArgs ga = a;
                ga.q = qc + (int64_t)off * idx->ld;
                ga.normalize_q = 0;
                ga.cand = ws->cand.p;
                ga.gate = ws->nfail.p;
                ga.gate_lo = off;
                ga.need = need ? need + off : nullptr;
                int nblocks = 0;
                MVDB_TRY(launch_scan(idx->metric, kModeTopK, ga, take, idx->device, s, &nblocks));
                // (one `need` word per query: "pass" = query, its lists nblocks * k keys after the query before)
                MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, Dt + (int64_t)off * k, It + (int64_t)off * k, ws->nfail.p, off,
                                      need ? need + off : nullptr, need ? 1 : 0, need ? (int64_t)nblocks * k : 0));
            }
            off = R;
        } else if (per_pass > 0 && !idx->kn.disable_mfma_scan) {
            const int* need = nullptr;
            MVDB_TRY(rescue(per_pass, &need));
            MVDB_TRY(ws->cand.reserve((size_t)32 * scan_grid_upper_bound(idx->device) * k));
            // (the GEMM scan keeps k <= 16 and takes no bitmap: those re-runs are all fp32-MFMA passes)
            // every refused query through the gated fp32-MFMA pass, 32 at a time (launches beyond the refused count return at
            // once).  Until round 5 the batch went to the 128-query GEMM-tiled scan after two such passes — 20-25 ms per 128
            // queries at 10M x 512 where four MFMA passes take 14.
            const int max_passes = (R + per_pass - 1) / per_pass;
            {
                // ONE launch walks up to kGatedPassGroup passes on the device (pass p: compact queries [p per_pass, ...); each
                // enabled by the refused count and its `need` word), ONE merge launch covers the group's compact queries; the
                // groups share one list buffer in stream order (so the lists are O(1) in the batch: 8 passes x 5 MB at k = 10)
                const int64_t cand_stride = (int64_t)per_pass * scan_grid_upper_bound(idx->device) * k;
                MVDB_TRY(ws->cand.reserve((size_t)std::min(max_passes, kGatedPassGroup) * cand_stride));
                for (int p0 = 0; p0 < max_passes; p0 += kGatedPassGroup) {
                    const int np = std::min(kGatedPassGroup, max_passes - p0), qoff = p0 * per_pass;
                    MfmaScanArgs ma;
                    ma.X = idx->X.p;
                    ma.n = n;
                    ma.ld = idx->ld;
                    ma.q = qc + (int64_t)qoff * idx->ld;
                    ma.nq = std::min(per_pass, R - qoff);
                    ma.k = k;
                    ma.cand = ws->cand.p;
                    ma.mask = mask32;
                    ma.thr0 = idx->kn.disable_rerun_floor ? nullptr : ws->qfloor.p + q0 + qoff;
                    int nblocks = 0;
                    MVDB_TRY(launch_mfma2_gated(KB, ma, idx->device, s, &nblocks, ws->nfail.p, qoff, need ? need + p0 : nullptr, np, per_pass,
                                                R - qoff, cand_stride));
                    MVDB_TRY(launch_merge(idx, ws, std::min(np * per_pass, R - qoff), nblocks, k, label_offset, Dt + (int64_t)qoff * k,
                                          It + (int64_t)qoff * k, ws->nfail.p, qoff, need ? need + p0 : nullptr, per_pass, cand_stride));
                }
                off = R;
            }
        }
        if (off < R && mask_dev) return fail(MVDB_ERR_ARG, "internal: bitmap re-run left to the GEMM scan");
        if (off < R) MVDB_TRY(ws->cand.reserve((size_t)128 * scan_grid_upper_bound(idx->device) * k));
        while (off < R) {
            const int take = std::min(128, R - off);
            int nblocks = 0;
            MVDB_TRY(launch_gemm_scan(idx, qc + (int64_t)off * idx->ld, take, k, n, ws->cand.p, s, &nblocks, ws->nfail.p, off));
            MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, Dt + (int64_t)off * k, It + (int64_t)off * k, ws->nfail.p, off));
            off += take;
        }
        hipLaunchKernelGGL(scatter_failed_kernel, dim3((unsigned)(((int64_t)R * k + 255) / 256)), dim3(256), 0, s, (const float*)Dt,
                           (const int64_t*)It, (const int64_t*)map, (const int*)ws->nfail.p, (int64_t)R, k, D_dev, I_dev);
        MVDB_HIP(hipGetLastError());
    }
    *answered = q0;
    return 0;
}

int search_core(const mvdb_index* idx, Workspace* ws, const float* q_dev, int nq, int k,
                int normalize_q, const int64_t* rows_dev, int64_t m, int64_t label_offset,
                float* D_dev, int64_t* I_dev, bool allow_split = true, const uint64_t* mask_dev = nullptr) {
    KnobScope knobs(&idx->kn);
    hipStream_t s = ws->stream;
    // Workspace O(1) in nq: a call of more queries is answered kCoreTile at a time on the same stream-ordered workspace (the
    // compact re-run buffers, per-query floors and flags below are sized by the queries of ONE tile; a tile is a whole number of
    // every pass's chunk: 32 / 128 / 256).  [round-5 advisor: the re-run workspace grew with the batch — 4 GB at 16k queries]
    if (nq > kCoreTile) {
        for (int t0 = 0; t0 < nq; t0 += kCoreTile)
            MVDB_TRY(search_core(idx, ws, q_dev + (int64_t)t0 * idx->ld, std::min(kCoreTile, nq - t0), k, normalize_q, rows_dev, m, label_offset,
                                 D_dev + (int64_t)t0 * k, I_dev + (int64_t)t0 * k, allow_split, mask_dev));
        return 0;
    }
    if (allow_split) tls_single_suspended = nq == 1 && idx->kn.shadow_single_query && idx->sq_route.suspended(idx->sq_fail.mirror());
    // row list: its m entries; bitmap: the first m rows when the caller says how many rows the bitmap covers (a resident
    // row set built before later appends), else every row
    const int64_t n = rows_dev ? m : (mask_dev && m > 0 ? std::min<int64_t>(m, idx->n) : idx->n);
    // Bitmap-selected rows, several queries: the passes that take a bitmap are the fp16 nomination pass (33+ queries; the
    // bit is looked at where a row is about to be nominated) and the staged fp32-MFMA pass (2..32 queries, and the exact
    // re-runs of uncertified queries); everything else answers a bitmap one query at a time.
    const uint32_t* mask32 = reinterpret_cast<const uint32_t*>(mask_dev);
    const bool masked_batch = mask_dev && nq >= 2 && k <= kMaxFusedK && idx->metric == MVDB_METRIC_IP && idx->ld == idx->d &&
                              mfma_gated_queries(idx) > 0 && !idx->kn.disable_masked_batch;
    // L2 under a bitmap (round 4): only through the fp16 nomination pass (its gate looks the bit up; the uncertified queries'
    // re-run is the single-query scan, which takes the bitmap too); smaller batches answer one query at a time
    const bool l2_masked_half = mask_dev && nq >= 2 && k <= kMaxFusedK && idx->metric == MVDB_METRIC_L2 && idx->ld == idx->d &&
                                !idx->kn.disable_masked_batch && (l2_cert_ok(idx) || l2_offsets_ok(idx, nq, n));
    if (mask_dev) {
        rows_dev = nullptr;
        if (!(masked_batch || l2_masked_half) || !half_path_ok(idx) || nq < half_min_nq(idx, n)) allow_split = false;
    }
    // the other multi-query passes take neither a row list nor a bitmap
    const int64_t* restricted = mask_dev ? reinterpret_cast<const int64_t*>(mask_dev) : rows_dev;
    if (n == 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           s, D_dev, I_dev, total, idx->metric);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    ScanArgs a;
    a.X = idx->X.p;
    a.n = n;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.q = q_dev;
    a.normalize_q = normalize_q;
    a.k = k;
    a.rows = rows_dev;
    a.mask = mask_dev;
    a.cand = nullptr;
    a.scores = nullptr;

    // ONE query over a large inner-product index: the int8 prefilter names the rows that can reach the top k, the exact kernel
    // scores those (code8_search).  Not served (no code yet and the stream is capturing, allocation failed, suspended): below.
    if (allow_split && code8_route_ok(idx, nq, k, rows_dev, mask_dev, n)) {
        bool served = false;
        MVDB_TRY(code8_search(idx, ws, a, k, label_offset, D_dev, I_dev, &served));
        if (served) return 0;
    }

    // Batches (2+ queries where the corpus buries the pass's fixed cost, half_min_nq), k <= 32, rows of known norm, a width the
    // fp16 kernels serve: ONE fp16 product over the shadow nominates, fp32 re-scores decide, a worst-case bound certifies
    // (certified_batch); what it leaves — fewer queries than the pass is worth — takes the exact passes below.
    if (allow_split && split_path_ok(idx, nq, k, rows_dev, n) && idx->shadow.ensure(idx, s, half_xscale(idx->row_norm_bound))) {
        int q0 = 0;
        const float* qsrc = nullptr;
        MVDB_TRY(certified_batch(idx, ws, a, q_dev, nq, k, normalize_q, n, label_offset, D_dev, I_dev, mask_dev, &q0, &qsrc));
        if (q0 == nq) return 0;
        return search_core(idx, ws, qsrc + (int64_t)q0 * idx->ld, nq - q0, k, 0, rows_dev, m, label_offset,
                           D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k, false, mask_dev);
    }

    if (masked_batch) {
        // ---- bitmap-selected rows, 2+ queries: staged fp32-MFMA passes of up to 32 (d <= 512) / 16 queries, exact ----------
        const float* qsrc = nullptr;
        MVDB_TRY(normalized_queries(idx, ws, q_dev, nq, normalize_q, &qsrc));
        const int per_pass = mfma_gated_queries(idx);
        MVDB_TRY(ws->cand.reserve((size_t)32 * scan_grid_upper_bound(idx->device) * k));
        for (int q0 = 0; q0 < nq; q0 += per_pass) {
            const int take = std::min(per_pass, nq - q0);
            MfmaScanArgs ma;
            ma.X = idx->X.p;
            ma.n = n;
            ma.ld = idx->ld;
            ma.q = qsrc + (int64_t)q0 * idx->ld;
            ma.nq = take;
            ma.k = k;
            ma.cand = ws->cand.p;
            ma.mask = mask32;
            int nblocks = 0;
            MVDB_TRY(profiled_launch("ip_scan_mfma_masked", s, [&] { return launch_mfma2_gated(idx->d / 16, ma, idx->device, s, &nblocks, nullptr, 0); }));
            MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k));
        }
        return 0;
    }

    // Large batches are cut into chunks: >= 104 queries left -> one 128-query GEMM-tiled launch (compute-
    // bound, 13.7 ms at 10M x 512), fewer -> 32-query MFMA passes (4.0 ms each); measured crossover ~100.
    if (gemm_path_ok(idx, nq, k, restricted)) {
        const float* qsrc = nullptr;
        MVDB_TRY(normalized_queries(idx, ws, q_dev, nq, normalize_q, &qsrc));
        MVDB_TRY(ws->cand.reserve((size_t)128 * scan_grid_upper_bound(idx->device) * k));
        const int min_nq = gemm_min_nq(idx, k);
        int q0 = 0;
        while (nq - q0 >= min_nq) {
            const int take = std::min(nq - q0, 128);
            int nblocks = 0;
            MVDB_TRY(launch_gemm_scan(idx, qsrc + (int64_t)q0 * idx->ld, take, k, n, ws->cand.p, s, &nblocks));
            MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k));
            q0 += take;
        }
        if (q0 == nq) return 0;
        // remainder: already-normalised queries through the paths below (a re-run of uncertified queries stays exact)
        return search_core(idx, ws, qsrc + (int64_t)q0 * idx->ld, nq - q0, k, 0, rows_dev, m, label_offset,
                           D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k, allow_split);
    }

    if (mfma_path_ok(idx, nq, k, restricted)) {
        // ---- several queries per corpus pass on the fp32 matrix cores ---------------------------
        const float* qsrc = nullptr;
        MVDB_TRY(normalized_queries(idx, ws, q_dev, nq, normalize_q, &qsrc));
        const int grid_ub = scan_grid_upper_bound(idx->device);
        MVDB_TRY(ws->cand.reserve((size_t)32 * grid_ub * k));
        for (int q0 = 0; q0 < nq;) {
            const int left = nq - q0;
            // staged kernel: 32 queries per pass (two query groups share each B fragment); the v1
            // kernel with two groups runs at one wave per SIMD and loses to two 16-query passes
            const bool staged = idx->d % 128 == 0;
            const bool two_groups = left > 16 && idx->d <= (idx->metric == MVDB_METRIC_IP ? 512 : 384) && (idx->kn.mfma_ng2 >= 0 ? idx->kn.mfma_ng2 != 0 : staged);
            const int take = two_groups ? std::min(left, 32) : std::min(left, 16);
            MfmaScanArgs ma;
            ma.X = idx->X.p;
            ma.n = n;
            ma.ld = idx->ld;
            ma.q = qsrc + (int64_t)q0 * idx->ld;
            ma.nq = take;
            ma.k = k;
            ma.cand = ws->cand.p;
            int nblocks = 0;
            const int KB = idx->d / 16;
            if (take > 16 && staged)
                MVDB_TRY(launch_mfma2<2>(KB, ma, idx->device, s, &nblocks, idx->metric));
            else if (take > 16)
                MVDB_TRY(launch_mfma_ng<2>(KB, ma, idx->device, s, &nblocks));
            else if (staged)
                MVDB_TRY(launch_mfma2<1>(KB, ma, idx->device, s, &nblocks, idx->metric));  // LDS-DMA staged, coalesced
            else
                MVDB_TRY(launch_mfma_ng<1>(KB, ma, idx->device, s, &nblocks));
            MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k));
            q0 += take;
        }
        return 0;
    }

    if (k <= kMaxFusedK) {
        MVDB_TRY(ws->cand.reserve((size_t)nq * scan_grid_upper_bound(idx->device) * k));
        a.cand = ws->cand.p;
        int nblocks = 0;
        MVDB_TRY(launch_scan(idx->metric, kModeTopK, a, nq, idx->device, s, &nblocks));
        return launch_merge(idx, ws, nq, nblocks, k, label_offset, D_dev, I_dev);
    }

    // ---- large k: scores -> radix select -> sort ------------------------------------------------------
    int nblocks = 0;
    MVDB_TRY(ws->scores.reserve((size_t)nq * n));
    a.scores = ws->scores.p;
    MVDB_TRY(launch_scan(idx->metric, kModeScores, a, nq, idx->device, s, &nblocks));
    const float* sc_base = ws->scores.p;
    const int64_t k_eff = std::min<int64_t>(k, n);
    const int64_t P = pow2ceil(std::max<int64_t>(k, 2));
    MVDB_TRY(ws->selkeys.reserve((size_t)P));
    const int cus = device_cus(idx->device);
    const int sel_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cus * 8));
    for (int qi = 0; qi < nq; ++qi) {
        const float* sc = sc_base + (int64_t)qi * n;
        hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, s, ws->st, (uint64_t)k_eff);
        for (int shift = 56; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(radix_hist_kernel, dim3(sel_grid), dim3(256), 0, s, sc, n, shift,
                               ws->st);
            hipLaunchKernelGGL(radix_pick_kernel, dim3(1), dim3(256), 0, s, shift, ws->st);
        }
        hipLaunchKernelGGL(radix_compact_kernel, dim3(sel_grid), dim3(256), 0, s, sc, n, ws->st,
                           ws->selkeys.p);
        if (P > k_eff)
            hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)((P - k_eff + 255) / 256)), dim3(256),
                               0, s, ws->selkeys.p, k_eff, P);
        if (P <= 4096) {
            hipLaunchKernelGGL(bitonic_sort_lds_kernel, dim3(1), dim3(1024), 0, s, ws->selkeys.p,
                               (int)P);
        } else {
            for (int64_t size = 2; size <= P; size <<= 1)
                for (int64_t stride = size >> 1; stride > 0; stride >>= 1)
                    hipLaunchKernelGGL(bitonic_step_kernel, dim3((unsigned)((P / 2 + 255) / 256)),
                                       dim3(256), 0, s, ws->selkeys.p, P, size, stride);
        }
        hipLaunchKernelGGL(emit_sorted_kernel, dim3((k + 255) / 256), dim3(256), 0, s,
                           ws->selkeys.p, k, idx->metric, label_offset, D_dev + (int64_t)qi * k,
                           I_dev + (int64_t)qi * k, 0);
        MVDB_HIP(hipGetLastError());
    }
    return 0;
}

// Copy `bytes` from the device to ws->pin_out on the workspace's stream and wait for them ("<what> failed: ..." otherwise).
int copy_back(Workspace* ws, const void* src, size_t bytes, const char* what) {
    MVDB_TRY(ws->pin_out.reserve(bytes));
    hipError_t e = hipMemcpyAsync(ws->pin_out.p, src, bytes, hipMemcpyDeviceToHost, ws->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ws->stream);
    if (e != hipSuccess) return fail(MVDB_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// A host-pointer entry point's workspace: one of the index's own (private stream), given back on every path.  The caller
// holds idx->mu shared, has made the index's device current and checks `ws` (NULL: mvdb_index::acquire failed).
struct HostCall {
    const mvdb_index* const idx;
    Workspace* const ws;
    explicit HostCall(const mvdb_index* i) : idx(i), ws(i->acquire()) {}
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    ~HostCall() {
        if (ws) idx->release(ws);
    }
    // host queries [nq, d] into ws->q (padded to ld) on ws->stream
    int stage(const float* q_host, int nq) {
        const size_t elems = (size_t)nq * idx->ld;
        MVDB_TRY(ws->q.reserve(elems));
        MVDB_TRY(ws->pin.reserve(elems * sizeof(float)));
        float* st = (float*)ws->pin.p;
        if (idx->ld == idx->d) {
            memcpy(st, q_host, elems * sizeof(float));
        } else {
            memset(st, 0, elems * sizeof(float));
            for (int i = 0; i < nq; ++i)
                memcpy(st + (size_t)i * idx->ld, q_host + (size_t)i * idx->d, idx->d * sizeof(float));
        }
        MVDB_HIP(hipMemcpyAsync(ws->q.p, st, elems * sizeof(float), hipMemcpyHostToDevice, ws->stream));
        return 0;
    }
    // the call's results on the device, packed in ws->out: [I: total int64 | D: total fp32] -> ONE copy back
    int results(size_t total, float** D_dev, int64_t** I_dev) {
        MVDB_TRY(ws->out.reserve(total + (total + 1) / 2));
        *I_dev = ws->out.p;
        *D_dev = reinterpret_cast<float*>(ws->out.p + total);
        return 0;
    }
    // epilogue: one async D2H into pinned staging, sync, unpack
    int fetch(size_t total, float* D_host, int64_t* I_host) {
        MVDB_TRY(copy_back(ws, ws->out.p, total * (sizeof(int64_t) + sizeof(float)), "search"));
        memcpy(I_host, ws->pin_out.p, total * sizeof(int64_t));
        memcpy(D_host, (const char*)ws->pin_out.p + total * sizeof(int64_t), total * sizeof(float));
        return 0;
    }
};

// A search being captured into a hipGraph: from now on this workspace keeps every buffer it outgrows (RetireScope), so a
// later, larger eager call on the same stream cannot free memory the graph still names.  Returns ws->captured.
bool note_capture(Workspace* ws) {
    if (!ws->captured && stream_capturing(ws->stream)) ws->captured = true;
    return ws->captured;
}

// A device-pointer entry point's prologue (the caller holds idx->mu shared and has made the index's device current): the
// stream's workspace, held for the call (one search at a time per stream workspace), the capture rule, and the queries
// padded to the row stride.  `rc` is checked before `ws` / `q` are used.
// Nothing a device entry point does behind this synchronises the stream or reads from the device: the call may be captured
// into a hipGraph once an eager call of the same shape has sized the stream's workspace (allocation is not capturable).
struct StreamCall {
    Workspace* const ws;
    std::unique_lock<std::mutex> use;
    RetireScope keep;
    const float* q;  // the queries at stride ld
    int rc;
    StreamCall(const mvdb_index* idx, void* stream, const float* q_dev, int nq)
        : ws(idx->for_stream((hipStream_t)stream)),
          use(ws ? std::unique_lock<std::mutex>(ws->use_mu) : std::unique_lock<std::mutex>()),
          keep(ws && note_capture(ws) ? &ws->retired : nullptr),
          q(q_dev),
          rc(ws ? pad(idx, q_dev, nq) : fail(MVDB_ERR_HIP, "workspace allocation failed")) {}

  private:
    int pad(const mvdb_index* idx, const float* q_dev, int nq) {
        if (idx->ld == idx->d) return 0;
        MVDB_TRY(ws->q.reserve((size_t)nq * idx->ld));
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)(((int64_t)nq * idx->ld + 255) / 256)), dim3(256), 0, ws->stream, ws->q.p, q_dev,
                           (int64_t)nq, idx->d, idx->ld);
        MVDB_HIP(hipGetLastError());
        q = ws->q.p;
        return 0;
    }
};

// Branch-free min / max (and strict ascent) of a host row list: vectorises; a list can hold millions of rows.
struct RowRange {
    int64_t lo = 0, hi = -1;
    bool sorted = true;  // strictly ascending
};
RowRange row_range(const int64_t* rows, int64_t m) {
    RowRange r;
    if (m <= 0) return r;
    r.lo = r.hi = rows[0];
    for (int64_t i = 1; i < m; ++i) {
        r.lo = rows[i] < r.lo ? rows[i] : r.lo;
        r.hi = rows[i] > r.hi ? rows[i] : r.hi;
        r.sorted &= rows[i] > rows[i - 1];
    }
    return r;
}

int check_search_args(const mvdb_index* idx, const void* q, int nq, int k, const void* D,
                      const void* I) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (k <= 0) return fail(MVDB_ERR_ARG, "k must be positive (got %d)", k);
    return 0;
}

// Rows of readable slack allocated behind the matrix: the tiled batch kernels fetch whole 32-row tiles (rows past n - 1
// are read, scored and never nominated) so that their DMA issue needs no per-lane bounds handling.
constexpr int64_t kRowSlack = 32;

// Grid of the utility kernels that give a wave to a row (four waves per block), at most per_cu blocks per CU.
int row_grid(int device, int64_t rows, int per_cu = 16) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, (int64_t)device_cus(device) * per_cu));
}

// ---- the fp16 shadow (the event x store table: above mvdb_index) ------------------------------------------------------------
void ShadowStore::drop() {
    Xh.release();
    Hn.release();
    cap = rows = hn_rows = 0;
    scale = 0.f;
    failed = false;
}

// The rows changed their numbers or their scale but the allocation still fits: the shadow is emptied, not freed — hipFree waits
// for the whole device and the next batch search would allocate the same bytes again — and rebuilt in place on demand.
void ShadowStore::invalidate() {
    rows = hn_rows = 0;
    failed = false;
}

// The shadow for a batch search on stream s (caller holds the index shared): the existing one if it covers the rows at
// this scale, else built here — once: 10M x 512 convert in ~5 ms — and published after a wait for s, so that searches on
// other streams find complete data.  NULL (the fp32 path serves): no kernel for d, switched off, allocation failed, or the
// stream is being captured (a build allocates and synchronises).
const _Float16* ShadowStore::ensure(const mvdb_index* idx, hipStream_t s, float xscale) {
    if (!half_shadow_dim(idx->d) || idx->ld != idx->d || idx->kn.disable_half_shadow || !(xscale > 0.f)) return nullptr;
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    if (Xh.p && scale == xscale && rows == idx->n) return Xh.p;
    if (failed || stream_capturing(s)) return nullptr;
    // (a stale shadow can only be one whose rows are a prefix at another scale or count: mutators drop or extend it while no
    //  search is in flight, so nobody else is reading what is rebuilt here)
    if (Xh.p && cap < idx->n) drop();
    if (Xh.p && scale != xscale) {   // another scale: every row is converted again, into the same allocation
        invalidate();
        scale = xscale;
    }
    if (!Xh.p) {
        const int64_t want = std::max<int64_t>(idx->cap, idx->n);
        if (Xh.alloc((size_t)(want + kRowSlack) * idx->d * sizeof(_Float16)) != hipSuccess) {
            (void)hipGetLastError();
            failed = true;
            return nullptr;
        }
        cap = want;
        rows = 0;
        scale = xscale;
        (void)idx->rf.ensure(1);  // (with the shadow — never inside a capture, once per index —: the refusal count of tile_flags_wanted)
        (void)hipGetLastError();  // (unconditional on purpose: without it the GPU suite, run in order, met a stale HIP error at a later launch check)
    }
    if (launch_half_shadow(idx->X.p + rows * idx->ld, idx->ld, idx->d, idx->n - rows, xscale, Xh.p + rows * idx->d, idx->device, s) != 0 ||
        hipStreamSynchronize(s) != hipSuccess) {
        drop();
        failed = true;
        return nullptr;
    }
    rows = idx->n;
    return Xh.p;
}

// L2 over rows of mixed norms (launch_half_pass: l2off): |x_r|^2 / 2 of the shadow's rows, 4 bytes per row beside it (+ zeroed
// slack: the kernel fetches a whole tile's offsets), built on first use and caught up after appends here; dropped with the
// shadow.  NULL: no complete shadow, allocation failed, or the stream is being captured before the array exists (the pass
// then nominates by inner product and the norm-range certificate sends what it cannot certify to the exact kernels).
const float* ShadowStore::ensure_offsets(const mvdb_index* idx, hipStream_t s) {
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    if (!Xh.p || rows != idx->n) return nullptr;
    if (Hn.p && hn_rows == idx->n) return Hn.p;
    if (stream_capturing(s)) return nullptr;
    if (!Hn.p) {
        const size_t bytes = (size_t)(cap + kRowSlack) * sizeof(float);
        if (Hn.alloc(bytes) != hipSuccess || hipMemsetAsync(Hn.p, 0, bytes, s) != hipSuccess) {
            (void)hipGetLastError();
            Hn.release();
            return nullptr;
        }
        hn_rows = 0;
    }
    if (launch_half_norms(idx->X.p + hn_rows * idx->ld, idx->ld, idx->d, idx->n - hn_rows, Hn.p + hn_rows, idx->device, s) != 0 ||
        hipStreamSynchronize(s) != hipSuccess) {
        Hn.release();
        hn_rows = 0;
        return nullptr;
    }
    hn_rows = idx->n;
    return Hn.p;
}

// add: the shadow follows when it is there, still fits and the scale the new norm bound asks for is the one it was built with
int ShadowStore::extend(mvdb_index* idx, int64_t n_new) {
    if (!Xh.p) {
        failed = false;
        return 0;
    }
    const float xscale = half_xscale(idx->row_norm_bound);
    if (cap < idx->n + n_new) {
        drop();
        return 0;
    }
    if (rows != idx->n || xscale != scale) {   // (the next batch search converts every row again, in place)
        invalidate();
        return 0;
    }
    MVDB_TRY(launch_half_shadow(idx->X.p + idx->n * idx->ld, idx->ld, idx->d, n_new, xscale, Xh.p + idx->n * idx->d, idx->device, idx->mut));
    MVDB_HIP(hipStreamSynchronize(idx->mut));
    rows = idx->n + n_new;
    return 0;
}

// ---- the int8 code of the rows and the single-query prefilter route (code8_scan.hpp) -------------------
constexpr int64_t kCode8MinRows = 500000;      // (>= kCode8Seed, code8_scan.hpp: the rows of the floor's sample are distinct)
static_assert(kCode8MinRows >= kCode8Seed, "the seed sample takes distinct rows");
// the most candidates a call may hand to the re-score: code8_rescore_kernel's grid is sized for it (kCode8RescoreRows per
// block), and a query that keeps more than this of the index is better served by the exact scan anyway
constexpr int64_t kCode8MaxCapacity = 65536;
// A dropped code is rebuilt once the exact scan has answered this many single queries since the drop: the build moves about
// 1.25 scans' worth of bytes (the matrix read once, a quarter of it written), a served query saves about 0.75 — two queries
// pay for it, so a workload that alternates one delete and one query never builds.
constexpr int kCode8RebuildAfter = 2;

// (count_rebuild: the rows changed under a code that was held or wanted — the wait starts again, whether or not a code is
//  held right now: every delete of a delete / query alternation restarts it, so such a workload never builds)
void Code8Store::drop(bool count_rebuild) {
    C8.release();
    F5.release();
    B2.release();
    ar.release();
    samp.release();
    cap = rows = samp_n = 0;
    if (count_rebuild && wanted.load()) wait.store(kCode8RebuildAfter);
}
// rows were renumbered: emptied, the allocation kept (ShadowStore::invalidate)
void Code8Store::invalidate() {
    if (wanted.load()) wait.store(kCode8RebuildAfter);
    rows = samp_n = 0;
}

// The one launch of code8_build_kernel: stored rows [row0, row0 + n) coded from the matrix, or — list_dev — the n stored rows
// it names, those below `rows` (set_rows: what the code does not cover yet is coded by the next build anyway).
int Code8Store::build(const mvdb_index* idx, int64_t row0, int64_t n, hipStream_t s, const int64_t* list_dev) {
    if (n > 0)
        hipLaunchKernelGGL(code8_build_kernel, dim3(row_grid(idx->device, n)), dim3(256), 0, s, (const float*)(idx->X.p + row0 * idx->ld), idx->ld,
                           idx->d, n, C8.p + row0 * code8_high_stride(idx->d), low(idx->d) + row0 * code8_low_stride(idx->d), ar.p + row0,
                           list_dev, list_dev ? rows : (int64_t)0, F5.p, row0,
                           B2.p ? B2.p + row0 * code8_bit2_stride(idx->d) : (uint8_t*)nullptr);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// The stored copy of the floor's sample.  It is VALID iff the code is complete (rows == n) and the copy was gathered for
// this n after the last write to the code (samp_n == n): sample_valid is the only test, this function the only
// writer.  Every writer of the code calls it behind its build, on the same stream, with the row count the
// index will have (ensure: a build; extend: add, where n moves and with it every slot; set_rows_core: rows
// rewritten in place — a captured graph of the route stays valid across that, so the copy follows eagerly); the paths that
// empty or free the code (invalidate, drop) mark it stale or free it with the code.  Nothing here runs inside a
// stream capture: ensure refuses before it gets here, the mutators run on idx->mut.
int Code8Store::gather_sample(const mvdb_index* idx, int64_t n, hipStream_t s) {
    samp_n = 0;
    const int64_t chunks = kCode8Seed * (idx->d / 16);
    const int grid = (int)std::min<int64_t>((chunks + 255) / 256, (int64_t)device_cus(idx->device) * 16);
    hipLaunchKernelGGL(code8_sample_kernel, dim3(grid), dim3(256), 0, s, (const uint8_t*)C8.p, (const uint8_t*)low(idx->d), (const float2*)ar.p, n, idx->d,
                       samp.p, reinterpret_cast<float2*>(samp.p + kCode8Seed * idx->d));
    MVDB_HIP(hipGetLastError());
    samp_n = n;
    return 0;
}

// The code for a single query on stream s (caller holds the index shared).  false: the exact scan serves this call.
bool Code8Store::ensure(const mvdb_index* idx, hipStream_t s) {
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    if (C8.p && sample_valid(idx->n)) return true;   // (complete code AND a current copy of the floor's sample)
    if (failed || stream_capturing(s)) return false;
    wanted.store(true);
    if (wait.load(std::memory_order_relaxed) > 0) {
        wait.fetch_sub(1, std::memory_order_relaxed);
        return false;
    }
    if (C8.p && cap < idx->n) drop(false);
    if (!C8.p) {
        const int64_t want = std::max<int64_t>(idx->cap, idx->n);
        if (C8.alloc((size_t)want * idx->d) != hipSuccess || ar.alloc((size_t)want * sizeof(float2)) != hipSuccess ||
            samp.alloc(code8_sample_bytes(idx->d)) != hipSuccess || !idx->c8_ctr.ensure(8)) {
            (void)hipGetLastError();
            drop(false);
            failed = true;
            return false;
        }
        // (the front plane never fails a search: without it the prefilter streams the high plane)
        if (code8_front_wanted(idx->kn.code8_front_plane, idx->d) && F5.alloc(code8_front_bytes(want, idx->d)) != hipSuccess) {
            (void)hipGetLastError();
            F5.release();
        }
        // (nor does the bit plane: without it the front form gathers the high plane for its survivors)
        if (F5.p && idx->kn.code8_bit_plane && B2.alloc(code8_bit2_bytes(want, idx->d)) != hipSuccess) {
            (void)hipGetLastError();
            B2.release();
        }
        cap = want;
        rows = 0;
    }
    if (build(idx, rows, idx->n - rows, s) != 0 || gather_sample(idx, idx->n, s) != 0 || hipStreamSynchronize(s) != hipSuccess) {
        drop(false);
        failed = true;
        return false;
    }
    rows = idx->n;
    return true;
}

// add: the code follows when it is there, complete and still fits (the rows are coded from the matrix, on the mutators' stream)
int Code8Store::extend(mvdb_index* idx, int64_t n_new) {
    if (!C8.p) return 0;
    if (cap < idx->n + n_new) {
        drop();
        return 0;
    }
    if (rows != idx->n) return 0;  // emptied by a delete: the next eligible query codes every row again
    MVDB_TRY(build(idx, idx->n, n_new, idx->mut));
    MVDB_TRY(gather_sample(idx, idx->n + n_new, idx->mut));   // n moves: every slot of the floor's sample does
    MVDB_HIP(hipStreamSynchronize(idx->mut));
    rows = idx->n + n_new;
    return 0;
}

bool code8_route_ok(const mvdb_index* idx, int nq, int k, const int64_t* rows_dev, const uint64_t* mask_dev, int64_t n) {
    if (nq != 1 || !idx->kn.code8_single_query || idx->kn.shadow_single_query) return false;
    if (idx->metric != MVDB_METRIC_IP || rows_dev || mask_dev || k > kMaxFusedK) return false;
    if (n != idx->n || n < kCode8MinRows || !code8_dim(idx->d) || idx->ld != idx->d) return false;
    if (!(idx->row_norm_bound > 0.f) || !(idx->row_norm_bound < 1.0e30f) || idx->code.failed) return false;
    return true;
}

// What is specific to the codes: (G, U, MASKED) of code8_seed_kernel per width, and for code8_scan_kernel — whose loads are
// 12 bytes per lane, not 16 — its own U and blocks per CU (SCAN_U, SCAN_BLOCKS).  All measured per shape: DESIGN.md section
// 4.1b.  launch(Code8Shape<...>{}) for d; the exact-scan shapes of the route come from with_scan_shape.
// The front form of code8_scan_kernel (it streams the front plane, a 32-code chunk per lane): FRONT_G lanes per row
// (code8_front_lanes: the plane's tiles are 64 / FRONT_G rows), FRONT_U tiles per batch, FRONT_BLOCKS per CU.  At d = 512 the
// plane has the quad layout (code8_front_quad): FRONT_G = 4, a lane holds four chunks of its row.
// FRONT_DEFAULT: whether option code8_front_plane = 1 keeps and streams the plane at this width (measured: DESIGN.md section
// 4.1b — at d = 1024 the front form loses on the zero-mean corpus, whose stage 0 leaves 11 % of the rows; the diagnostic
// values 2 and 3 of the option still build the plane there).
template <int G_, int U_, bool MASKED_, int SCAN_U_, int SCAN_BLOCKS_, int FRONT_G_, int FRONT_U_, int FRONT_BLOCKS_, bool FRONT_DEFAULT_>
struct Code8Shape {
    static constexpr bool FRONT_DEFAULT = FRONT_DEFAULT_;
    static constexpr int G = G_, U = U_, SCAN_U = SCAN_U_, SCAN_BLOCKS = SCAN_BLOCKS_;
    static constexpr int FRONT_G = FRONT_G_, FRONT_U = FRONT_U_, FRONT_BLOCKS = FRONT_BLOCKS_;
    static constexpr bool MASKED = MASKED_;
};
template <typename Launch>
int with_code8_shape(int d, Launch launch) {
    switch (d) {
        case 384: return launch(Code8Shape<32, 8, true, 8, 4, 16, 8, 2, true>{});
        // (the quad layout of the front plane, code8_front_quad: a lane quad per row, FRONT_U tiles of 16 rows per batch.
        // Two tiles — 10 KiB of loads per wave — on ONE block per CU: the sweep's best cell, profiles/code8_front_sweep.jsonl)
        case 512: return launch(Code8Shape<32, 4, false, 8, 2, code8_front_lanes(512), code8_front_quad(512) ? 2 : 4, code8_front_quad(512) ? 1 : 2, true>{});
        case 1024: return launch(Code8Shape<64, 4, false, 8, 2, 32, 4, 2, false>{});
        default: return fail(MVDB_ERR_ARG, "internal: no int8 prefilter kernel for d = %d", d);
    }
}
// launch(ScanShape<G, C>{}) for the exact-scan shape of one of the route's widths: nothing is instantiated for the other shapes
template <typename Launch>
int with_code8_exact_shape(int d4, Launch launch) {
    return with_scan_shape(d4, [&](auto shape) {
        if constexpr (code8_shape(decltype(shape)::G, decltype(shape)::C)) return launch(shape);
        else return fail(MVDB_ERR_ARG, "internal: no int8 prefilter kernel for rows of %d 16-byte chunks", d4);
    });
}

bool code8_front_wanted(int option, int d) {
    if (option == 0 || !code8_dim(d) || !code8_front_dim(d)) return false;
    bool dflt = false;
    (void)with_code8_shape(d, [&](auto cs) {
        dflt = decltype(cs)::FRONT_DEFAULT;
        return 0;
    });
    return option >= 2 || dflt;
}

// the prefilter's grid: CUs x BLOCKS blocks, BLOCKS per shape from the sweep of this kernel (Code8Shape::SCAN_BLOCKS;
// profiles/code8_planes_sweep.jsonl: U = 8 with 2 blocks per CU at d = 512 and 1024, with 4 at d = 384)
// (GF, UF > 0: the front form — its batches are (64 / GF) UF rows)
// (LIFT: the front form's survivors are lifted from the bit plane — code8_scan.hpp; the label keeps its five arguments)
// (HANDOFF: a fifth wave per block takes them; one block per CU as without it)
template <int G, int U, bool MASKED, int BLOCKS, int GF = 0, int UF = 0, bool LIFT = false, bool HANDOFF = false>
int code8_scan_blocks(int64_t n, int device) {
    void (*kern)(Code8ScanArgs) = code8_scan_kernel<G, U, MASKED, GF, UF, LIFT, HANDOFF>;
    constexpr int threads = kScanThreads + (HANDOFF ? kWave : 0);
    int per_cu = std::min(cached_occupancy((const void*)kern, threads, 0, 4), BLOCKS);
    if (kn().scan_blocks_per_cu > 0) per_cu = kn().scan_blocks_per_cu;
    return scan_grid(n, GF > 0 ? (kWave / GF) * UF : (kWave / G) * U, per_cu, device);
}
template <int G, int U, bool MASKED, int BLOCKS, int GF = 0, int UF = 0, bool LIFT = false, bool HANDOFF = false>
int launch_code8_scan(const Code8ScanArgs& a, int device, hipStream_t stream) {
    void (*kern)(Code8ScanArgs) = code8_scan_kernel<G, U, MASKED, GF, UF, LIFT, HANDOFF>;
    constexpr int threads = kScanThreads + (HANDOFF ? kWave : 0);
    const int nblocks = code8_scan_blocks<G, U, MASKED, BLOCKS, GF, UF, LIFT, HANDOFF>(a.n, device);
    if constexpr (GF > 0)
        return profiled_launch("ip_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(threads), 0, stream, done, a); },
                               "code8_scan_kernel<%d, %d, %s, %d, %d>", G, U, MASKED ? "true" : "false", GF, UF);
    else
        return profiled_launch("ip_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(threads), 0, stream, done, a); },
                               "code8_scan_kernel<%d, %d, %s>", G, U, MASKED ? "true" : "false");
}
// Whether the hand-off form serves where the lift serves (MVDB_CODE8_HANDOFF: 1 never, 2 always, 0 the measured default —
// DESIGN.md section 4.1b, "The survivor wave"), and its ring (MVDB_CODE8_RING: a power of two, 0 or anything else the default)
constexpr bool kCode8HandoffDefault = true;
bool code8_handoff_serves() { return kn().code8_handoff == 2 || (kn().code8_handoff != 1 && kCode8HandoffDefault); }
int code8_ring_entries() {
    const int r = kn().code8_ring;
    return r >= kCode8RingMin && r <= kCode8RingMax && (r & (r - 1)) == 0 ? r : kCode8RingDefault;
}
// Which form of the prefilter serves this call: the front form where the code holds the plane, unless its window has
// suspended it (the survivors of stage 0 pay three gathered lines each: past kCode8FrontShare of the rows the other form is
// faster) — option value 2 keeps it on.  One decision per call; no synchronisation (the mirrored words lag).
// The quad form runs one block per CU: fewer gathers are in flight, a survivor costs more and the lines cross earlier
// (measured again on the three 10M x 512 corpora: DESIGN.md section 4.1b).
constexpr double kCode8FrontShare = 0.12, kCode8FrontShareQuad = 0.08;
bool code8_front_serves(const mvdb_index* idx) {
    if (!idx->code.F5.p || !code8_front_wanted(idx->kn.code8_front_plane, idx->d)) return false;
    if (idx->kn.code8_front_plane >= 2) return idx->kn.code8_front_plane == 2;   // (diagnostic values: always / never)
    const volatile unsigned long long* sum = idx->c8_ctr.mirror<unsigned long long>();
    return !idx->c8_front.suspended_mean(sum ? sum + 2 : nullptr, idx->c8_ctr.mirror() ? idx->c8_ctr.mirror() + 6 : nullptr,
                                         (code8_front_quad(idx->d) ? kCode8FrontShareQuad : kCode8FrontShare) * (double)idx->n);
}

// The floor's launch.  The stored sample streams; every block leaves one list, which every block of the prefilter merges.
// (grid shapes measured: DESIGN.md section 4.1b)  *nlists: the lists the launch leaves — its grid.
template <int G, int U, bool MASKED>
int launch_code8_seed(const Code8SeedArgs& a, int device, hipStream_t stream, int* nlists) {
    void (*kern)(Code8SeedArgs) = code8_seed_kernel<G, U, MASKED>;
    int threads = kn().code8_seed_threads;   // (tuning hooks, as scan_blocks_per_cu: 0 = the measured defaults)
    if (threads != 256 && threads != 512 && threads != 1024) threads = kCode8SeedThreads;
    constexpr int64_t nbatches = kCode8Seed / ((kWave / G) * U);
    const int64_t want = (nbatches + threads / kWave - 1) / (threads / kWave);
    int64_t blocks = kn().code8_seed_blocks > 0 ? kn().code8_seed_blocks : device_cus(device);
    blocks = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(blocks, want), scan_grid_upper_bound(device)));
    *nlists = (int)blocks;
    return profiled_launch("ip_scan_code8_seed", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3((unsigned)blocks), dim3(threads), 0, stream, done, a); },
                           "code8_seed_kernel<%d, %d, %s>", G, U, MASKED ? "true" : "false");
}

// The re-score's launch: a grid for the whole capacity, of which the kernel uses what the count asks for.
template <int G, int C, int U, bool MASKED>
int launch_code8_rescore(const Code8RescoreArgs& a, int device, hipStream_t stream) {
    void (*kern)(Code8RescoreArgs) = code8_rescore_kernel<G, C, U, MASKED>;
    const int64_t want = (a.cap + a.rows_per_block - 1) / a.rows_per_block;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * 4));
    return profiled_launch("ip_scan_code8_rescore", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3((unsigned)blocks), dim3(kScanThreads), 0, stream, done, a); },
                           "code8_rescore_kernel<%d, %d, %d, %s>", G, C, U, MASKED ? "true" : "false");
}

int code8_search(const mvdb_index* idx, Workspace* ws, const ScanArgs& a0, int k, int64_t label_offset, float* D_dev, int64_t* I_dev,
                 bool* served) {
    *served = false;
    hipStream_t s = ws->stream;
    const int d = idx->d;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(idx->kn.code8_capacity, kCode8MaxCapacity));
    // workspace layout (bytes): planes [2 d] | terms [16 floats] | counter, active lists [2 x 8] | gate | floor | candidates
    // (the block lists of the seed and re-score launches, and of the gated fallback scan, go through ws->cand in turn)
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    const size_t o_planes = take((size_t)2 * d), o_par = take(16 * sizeof(float)), o_ctr = take(2 * sizeof(unsigned long long)),
                 o_gate = take(sizeof(int)), o_floor = take(sizeof(float)), o_cand = take((size_t)cap * sizeof(uint32_t));
    const size_t cand_keys = (size_t)scan_grid_upper_bound(idx->device) * k;
    const bool capturing = stream_capturing(s);
    if (capturing && (ws->c8.cap < off || ws->cand.cap < cand_keys)) return 0;  // nothing is allocated inside a capture
    if (idx->c8_route.suspended(idx->c8_ctr.mirror())) return 0;
    if (!idx->code.ensure(idx, s)) return 0;
    MVDB_TRY(ws->c8.reserve(off));
    MVDB_TRY(ws->cand.reserve(cand_keys));
    char* base = ws->c8.p;
    int8_t* qhi = reinterpret_cast<int8_t*>(base + o_planes);
    int8_t* qlo = qhi + d;
    float* par = reinterpret_cast<float*>(base + o_par);
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(base + o_ctr);
    int* active = reinterpret_cast<int*>(counter + 1);   // the lists the re-score launch of this call stored
    int* gate = reinterpret_cast<int*>(base + o_gate);
    float* floor = reinterpret_cast<float*>(base + o_floor);
    uint32_t* cand = reinterpret_cast<uint32_t*>(base + o_cand);

    // launches 1 to 4 follow one another with nothing in between: while they are timed, each bracket begins where the one
    // before it ended, and the call puts one marker on the stream (in front of the first) where it used to put eight
    ProfChain chain(s);
    // 1. the query's planes and margin terms (every block; block 0 leaves them here and zeroes the candidate counter), and
    //    per block the k best LOWER bounds of its share of the seed sample, from its stored copy
    Code8SeedArgs sd;
    sd.scodes = idx->code.samp.p;
    sd.sar = reinterpret_cast<const float2*>(idx->code.samp.p + kCode8Seed * d);
    sd.d = d;
    sd.q = a0.q;
    sd.normalize_q = a0.normalize_q;
    sd.row_norm_bound = idx->row_norm_bound;
    sd.qhi = qhi;
    sd.qlo = qlo;
    sd.par = par;
    sd.counter = counter;
    sd.k = k;
    sd.lists = ws->cand.p;
    int seed_lists = 0;
    MVDB_TRY(with_code8_shape(d, [&](auto cs) {
        using K = decltype(cs);
        return launch_code8_seed<K::G, K::U, K::MASKED>(sd, idx->device, s, &seed_lists);
    }));
    // 2. the floor — the k-th best of those lower bounds, merged by every block at its head — and the prefilter over the codes
    Code8ScanArgs c;
    c.high = idx->code.C8.p;
    c.low = idx->code.low(d);
    c.ar = idx->code.ar.p;
    c.n = idx->n;
    c.d = d;
    c.hstride = code8_high_stride(d);
    c.qhi = qhi;
    c.qlo = qlo;
    c.par = par;
    c.lists = ws->cand.p;
    c.nlists = seed_lists;
    c.k = k;
    c.floor = floor;
    c.cand = cand;
    c.cap = cap;
    c.counter = counter;
    c.survivors = reinterpret_cast<unsigned long long*>(idx->c8_ctr.dev() + 2);
    c.front = idx->code.F5.p;
    c.front_survivors = reinterpret_cast<unsigned long long*>(idx->c8_ctr.dev() + 4);
    c.front_calls = idx->c8_ctr.dev() + 6;
    c.front_msum = idx->c8_ctr.mirror<unsigned long long>() + 2;
    c.front_mcalls = idx->c8_ctr.mirror() + 6;
    c.bit2 = idx->code.B2.p;
    c.ring = code8_ring_entries();
    const bool front = code8_front_serves(idx);
    // the lift serves where the plane is held and wanted, at the measured tiles per batch (the tuning hook keeps the gathers)
    const bool lift = front && idx->code.B2.p && idx->kn.code8_bit_plane && kn().code8_front_u == 0;
    MVDB_TRY(with_code8_shape(d, [&](auto cs) {
        using K = decltype(cs);
        if (!front) return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::SCAN_BLOCKS>(c, idx->device, s);
        if constexpr (code8_front_quad(K::G * 16) && !K::MASKED) {
            if (lift && code8_handoff_serves())
                return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, K::FRONT_U, true, true>(c, idx->device, s);
        }
        if (lift) return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, K::FRONT_U, true>(c, idx->device, s);
        const int hook = kn().code8_front_u;   // (tuning hook)
        if constexpr (code8_front_quad(K::G * 16) && !K::MASKED) {
            // the quad layout: a batch is 16 UF rows and must divide the stage of 64
            const int fu = hook == 1 || hook == 2 || hook == 4 ? hook : K::FRONT_U;
            if (fu == 1) return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, 1>(c, idx->device, s);
            if (fu == 2) return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, 2>(c, idx->device, s);
            return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, 4>(c, idx->device, s);
        } else {
            const int fu = hook == 4 || hook == 8 ? hook : K::FRONT_U;
            if (fu == 4) return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, 4>(c, idx->device, s);
            return launch_code8_scan<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, 8>(c, idx->device, s);
        }
    }));
    // 3. the fallback decision and the exact scores of the candidates, ties by row: one sorted k-list per active block
    Code8RescoreArgs r;
    r.X = a0.X;
    r.ld = a0.ld;
    r.d4 = a0.d4;
    r.q = a0.q;
    r.normalize_q = a0.normalize_q;
    r.k = k;
    r.cand = cand;
    r.counter = counter;
    r.cap = cap;
    r.par = par;
    r.rows_per_block = kn().code8_rescore_rows > 0 ? kn().code8_rescore_rows : kCode8RescoreRows;   // (tuning hook)
    r.lists = ws->cand.p;
    r.active = active;
    r.gate = gate;
    r.ctr_dev = idx->c8_ctr.dev();
    r.stats = idx->c8_ctr.mirror();
    // (the exact scan's shape: the arithmetic is restated for exactly that; the route serves unpadded rows that fill it)
    MVDB_TRY(with_code8_exact_shape(a0.d4, [&](auto shape) {
        using S = decltype(shape);
        return launch_code8_rescore<S::G, S::C, rescore_u(S::G, S::C), false>(r, idx->device, s);
    }));
    // 4. fallback, enabled on the device: the full exact scan leaves its block lists where the re-score's would be
    ScanArgs a = a0;
    a.cand = ws->cand.p;
    int nblocks = 0;
    a.rows = nullptr;
    a.n = idx->n;
    a.gate = gate;
    a.gate_lo = 0;
    MVDB_TRY(with_code8_exact_shape(a.d4, [&](auto shape) {   // (the fallback has never honoured MVDB_SCAN_BLOCKS_PER_CU)
        using S = decltype(shape);
        return launch_scan_kern<S::G, S::C, stream_u(S::G, S::C), 0, kModeTopK, 0, false>(a, 1, idx->device, s, &nblocks, "ip_scan_code8_fallback",
                                                                                            /*knob=*/false);
    }));
    // 5. (D, I) from the lists of this call: the exact scan's where the gate is set, else the re-score's
    Code8FinishArgs f;
    f.lists = ws->cand.p;
    f.gate = gate;
    f.active = active;
    f.fallback_lists = nblocks;
    f.k = k;
    f.label_offset = label_offset;
    f.D = D_dev;
    f.I = I_dev;
    hipLaunchKernelGGL(code8_finish_kernel, dim3(1), dim3(kCode8FinishThreads), 0, s, f);
    MVDB_HIP(hipGetLastError());
    *served = true;
    return 0;
}

// The only place the matrix is reallocated (caller: index held exclusively, searches quiesced): room for `need` rows, with
// half as much again unless `exact` (reserve: the caller knows the final size).
int grow(mvdb_index* idx, int64_t need, bool exact) {
    if (need <= idx->cap) return 0;
    const int64_t cap = exact ? need : std::max<int64_t>(std::max<int64_t>(need, idx->cap + idx->cap / 2), 1024);
    // the fp16 shadow (50 % of the matrix's bytes) goes first: it is sized for the old capacity anyway (rebuilt by the next
    // batch search), and an add on a nearly full device must not fail for a copy that is about to be dropped
    idx->shadow.drop();
    idx->code.drop();
    DevMem<float> nx;
    MVDB_HIP(nx.alloc((size_t)(cap + kRowSlack) * idx->ld * sizeof(float)));
    if (idx->n > 0) {
        hipError_t e = hipMemcpyAsync(nx.p, idx->X.p, (size_t)idx->n * idx->ld * sizeof(float), hipMemcpyDeviceToDevice, idx->mut);
        if (e == hipSuccess) e = hipStreamSynchronize(idx->mut);
        if (e != hipSuccess)
            return fail(MVDB_ERR_HIP, "device copy while %s failed: %s", exact ? "reserving" : "growing index", hipGetErrorString(e));
    }
    std::swap(idx->X.p, nx.p);  // (the old matrix goes with nx)
    idx->cap = cap;
    return 0;
}

int normalize_range(const mvdb_index* idx, float* base, int64_t n, hipStream_t s) {
    if (n <= 0) return 0;
    const Shape sh = choose_shape(idx->d4);
    const int rpi = 64 / sh.G;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3(row_grid(idx->device, (n + rpi - 1) / rpi, 8)), dim3(256), 0, s, base, n, idx->ld, idx->d4,
                       sh.G);
    MVDB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* mvdb_last_error(void) { return g_err; }
int mvdb_abi_version(void) { return 1; }

int mvdb_device_count(int* count) {
    if (!count) return fail(MVDB_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        return fail(MVDB_ERR_NODEVICE, "no HIP device available (%s)",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    }
    *count = n;
    return 0;
}

int mvdb_index_create(int d, int metric, int device, mvdb_index** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (d <= 0) return fail(MVDB_ERR_ARG, "dimension must be positive (got %d)", d);
    if (d > kMaxC * 64 * 4) return fail(MVDB_ERR_ARG, "dimension %d > 4096 is not supported", d);
    if (metric != MVDB_METRIC_IP && metric != MVDB_METRIC_L2)
        return fail(MVDB_ERR_ARG, "unknown metric %d", metric);
    MVDB_TRY(ensure_device(device));
    mvdb_index* idx = new mvdb_index();
    idx->d = d;
    idx->ld = ((int64_t)d + 3) / 4 * 4;
    idx->d4 = (int)(idx->ld / 4);
    idx->metric = metric;
    idx->device = device;
    idx->kn = read_knobs();
    *out = idx;
    return 0;
}

int mvdb_index_reload_env(mvdb_index* idx) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    const bool code8 = idx->kn.code8_single_query;   // (options without an environment switch: kept)
    const long long code8_cap = idx->kn.code8_capacity;
    const int code8_front = idx->kn.code8_front_plane;
    const int code8_bit = idx->kn.code8_bit_plane;
    const int range_shared = idx->kn.range_shared;
    const long long range_cand = idx->kn.range_candidates;
    const int join_shared = idx->kn.join_shared;
    const long long distinct_table = idx->kn.distinct_table_bytes;
    const long long maxsim_table = idx->kn.maxsim_table_bytes;
    const long long groups_partials = idx->kn.groups_partials_bytes;
    const int maxsim_tokens = idx->kn.maxsim_tokens_per_pass;
    const int assign_vectors = idx->kn.assign_vectors_per_pass;
    const int examples_vectors = idx->kn.examples_vectors_per_pass;
    const long long probe_table = idx->kn.probe_table_bytes;
    const int sparse_postings = idx->kn.sparse_postings;
    idx->kn = read_knobs();
    idx->kn.sparse_postings = sparse_postings;
    idx->kn.distinct_table_bytes = distinct_table;
    idx->kn.maxsim_table_bytes = maxsim_table;
    idx->kn.groups_partials_bytes = groups_partials;
    idx->kn.maxsim_tokens_per_pass = maxsim_tokens;
    idx->kn.assign_vectors_per_pass = assign_vectors;
    idx->kn.examples_vectors_per_pass = examples_vectors;
    idx->kn.probe_table_bytes = probe_table;
    idx->kn.code8_single_query = code8;
    idx->kn.code8_capacity = code8_cap;
    idx->kn.code8_front_plane = code8_front;
    idx->kn.code8_bit_plane = code8_bit;
    idx->kn.range_shared = range_shared;
    idx->kn.range_candidates = range_cand;
    idx->kn.join_shared = join_shared;
    return 0;
}

int mvdb_index_set_option(mvdb_index* idx, const char* name, long long value) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!name) return fail(MVDB_ERR_ARG, "option name is NULL");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    const std::string n(name);
    if (n == "shadow_single_query") {
        idx->kn.shadow_single_query = value != 0;
        idx->sq_route.restart(idx->sq_fail.mirror());
    } else if (n == "code8_single_query") {
        idx->kn.code8_single_query = value != 0;
        idx->c8_route.restart(idx->c8_ctr.mirror());
    } else if (n == "code8_capacity") {  // diagnostic: a small candidate capacity makes calls take the fallback
        if (value <= 0 || value > kCode8MaxCapacity) return fail(MVDB_ERR_ARG, "code8_capacity must lie in [1, %lld]", (long long)kCode8MaxCapacity);
        idx->kn.code8_capacity = value;
    } else if (n == "code8_front_plane") {
        if (value < 0 || value > 3) return fail(MVDB_ERR_ARG, "code8_front_plane must be 0, 1, 2 or 3");
        DeviceGuard dg(idx->device);
        MVDB_TRY(quiesce(idx));
        idx->kn.code8_front_plane = (int)value;
        if (!code8_front_wanted((int)value, idx->d))
            idx->code.F5.release();
        else if (idx->code.C8.p && !idx->code.F5.p && code8_front_wanted((int)value, idx->d))
            idx->code.drop(false);   // (a code without the plane: the next eligible query builds both)
        const volatile unsigned long long* sum = idx->c8_ctr.mirror<unsigned long long>();
        idx->c8_front.restart_mean(sum ? sum + 2 : nullptr, idx->c8_ctr.mirror() ? idx->c8_ctr.mirror() + 6 : nullptr);
    } else if (n == "code8_bit_plane") {  // the plane of bit 2 beside the front plane: 0 frees it alone, 1 drops a code that holds the front plane without it
        if (value < 0 || value > 1) return fail(MVDB_ERR_ARG, "code8_bit_plane must be 0 or 1");
        DeviceGuard dg(idx->device);
        MVDB_TRY(quiesce(idx));
        idx->kn.code8_bit_plane = (int)value;
        if (value == 0)
            idx->code.B2.release();
        else if (idx->code.C8.p && idx->code.F5.p && !idx->code.B2.p)
            idx->code.drop(false);   // (the next eligible query builds the code with the plane)
    } else if (n == "range_shared") {  // batches of a range search on the shared fp16 pass: 0 never, 1 by size, 2 wherever eligible
        if (value < 0 || value > 2) return fail(MVDB_ERR_ARG, "range_shared must be 0, 1 or 2");
        idx->kn.range_shared = (int)value;
    } else if (n == "join_shared") {  // the range join on the shared fp16 pass: 0 never, 1 by size, 2 wherever eligible
        if (value < 0 || value > 2) return fail(MVDB_ERR_ARG, "join_shared must be 0, 1 or 2");
        idx->kn.join_shared = (int)value;
    } else if (n == "range_candidates") {  // candidates per query the shared pass holds (0: by cap); a small value forces the fallback
        if (value != 0 && (value < 64 || value > (1ll << 20))) return fail(MVDB_ERR_ARG, "range_candidates must be 0 or lie in [64, 2^20]");
        idx->kn.range_candidates = value;
    } else if (n == "distinct_table_bytes") {  // budget of the distinct search's tier-2 table (T slots of 8 n_groups bytes; T >= 1 whatever it is)
        if (value <= 0) return fail(MVDB_ERR_ARG, "distinct_table_bytes must be positive");
        idx->kn.distinct_table_bytes = value;
    } else if (n == "groups_partials_bytes") {  // budget of the group hits search's block lists (T slots of grid.x k group_size 8 bytes; T >= 1 whatever it is)
        if (value <= 0) return fail(MVDB_ERR_ARG, "groups_partials_bytes must be positive");
        idx->kn.groups_partials_bytes = value;
    } else if (n == "maxsim_table_bytes") {  // most bytes of the MaxSim search's table (T x n_groups x 8 of one call): a call above it is refused
        if (value <= 0) return fail(MVDB_ERR_ARG, "maxsim_table_bytes must be positive");
        idx->kn.maxsim_table_bytes = value;
    } else if (n == "maxsim_tokens_per_pass") {  // query vectors one corpus pass of a MaxSim search scores (0: as many as the rule allows)
        if (value < 0 || value > kMaxsimPassTokens) return fail(MVDB_ERR_ARG, "maxsim_tokens_per_pass must lie in [0, %d]", kMaxsimPassTokens);
        idx->kn.maxsim_tokens_per_pass = (int)value;
    } else if (n == "assign_vectors_per_pass") {  // vectors one corpus pass of an assignment scores (0: as many as the rule allows)
        if (value < 0 || value > kMaxsimPassTokens) return fail(MVDB_ERR_ARG, "assign_vectors_per_pass must lie in [0, %d]", kMaxsimPassTokens);
        idx->kn.assign_vectors_per_pass = (int)value;
    } else if (n == "examples_vectors_per_pass") {  // vectors one corpus pass of a search by examples scores (0: as many as the rule allows)
        if (value < 0 || value > kMaxsimPassTokens) return fail(MVDB_ERR_ARG, "examples_vectors_per_pass must lie in [0, %d]", kMaxsimPassTokens);
        idx->kn.examples_vectors_per_pass = (int)value;
    } else if (n == "probe_table_bytes") {  // budget of a probed search's item and candidate tables: a call above it runs its queries in chunks
        if (value <= 0) return fail(MVDB_ERR_ARG, "probe_table_bytes must be positive");
        idx->kn.probe_table_bytes = value;
    } else if (n == "sparse_postings") {  // 1: a sparse store that has postings is scored through them, 0: always the CSR pass
        if (value < 0 || value > 1) return fail(MVDB_ERR_ARG, "sparse_postings must be 0 or 1");
        idx->kn.sparse_postings = (int)value;
    } else if (n == "half_shadow")
        idx->kn.disable_half_shadow = value == 0;
    else if (n == "compact_bytes") {
        if (value <= 0) return fail(MVDB_ERR_ARG, "compact_bytes must be positive");
        idx->kn.compact_bytes = value;
    } else
        return fail(MVDB_ERR_ARG, "unknown index option '%s' (shadow_single_query, code8_single_query, code8_capacity, code8_front_plane, code8_bit_plane, range_shared, join_shared, range_candidates, distinct_table_bytes, groups_partials_bytes, maxsim_table_bytes, maxsim_tokens_per_pass, assign_vectors_per_pass, examples_vectors_per_pass, probe_table_bytes, sparse_postings, half_shadow, compact_bytes)", name);
    return 0;
}

long long mvdb_index_single_route_suspensions(const mvdb_index* idx) {
    return idx ? (long long)idx->sq_route.suspensions.load() : -1;
}

int mvdb_index_free(mvdb_index* idx) {
    if (!idx) return 0;
    DeviceGuard dg(idx->device);  // every free below, the members' own included, runs on the index's device
    {
        std::unique_lock<std::shared_mutex> lk(idx->mu);
        (void)quiesce(idx);
        if (idx->mut) (void)hipStreamDestroy(idx->mut);
        for (Workspace* w : idx->free_ws) delete w;
        for (auto& kv : idx->stream_ws) delete kv.second;
        delete idx->default_stream_ws;
    }
    delete idx;  // (the matrix, the stores, the counters and their mirrors: every member frees what it holds)
    return 0;
}

int mvdb_index_reset(mvdb_index* idx) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    MVDB_TRY(quiesce(idx));
    idx->n = 0;
    idx->shadow.drop();
    idx->code.drop();
    idx->row_norm_bound = 0.f;
    idx->norm2_lo = INFINITY;
    idx->norm2_hi = 0.f;
    ++idx->renumbered;
    return 0;
}

int64_t mvdb_index_ntotal(const mvdb_index* idx) { return idx ? idx->n : -1; }
int64_t mvdb_index_shadow_rows(const mvdb_index* idx) {
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    return idx->shadow.Xh.p ? idx->shadow.rows : 0;
}
int64_t mvdb_index_code8_rows(const mvdb_index* idx) {
    if (!idx) return -1;
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    return idx->code.C8.p ? idx->code.rows : 0;
}
int mvdb_index_code8_counters(const mvdb_index* idx, long long* fallbacks, long long* last_candidates, long long* calls) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (fallbacks) *fallbacks = (long long)idx->c8_ctr.read(0);
    if (last_candidates) *last_candidates = (long long)idx->c8_ctr.read(1);
    if (calls) *calls = (long long)idx->c8_ctr.read(2);
    return 0;
}
int mvdb_index_range_counters(const mvdb_index* idx, long long* shared_calls, long long* fallback_queries, long long* last_candidates) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (shared_calls) *shared_calls = (long long)idx->rg_shared_calls.load();
    if (fallback_queries) *fallback_queries = (long long)idx->rg_ctr.read<unsigned long long>(0);
    if (last_candidates) *last_candidates = (long long)idx->rg_ctr.read<unsigned long long>(1);
    return 0;
}
int mvdb_index_join_counters(const mvdb_index* idx, long long* shared_calls, long long* fallback_queries) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (shared_calls) *shared_calls = (long long)idx->jn_shared_calls.load();
    if (fallback_queries) *fallback_queries = (long long)idx->jn_ctr.read<unsigned long long>(0);
    return 0;
}
int mvdb_index_distinct_counters(const mvdb_index* idx, long long* calls, long long* fallback_queries) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->ds_calls.load();
    if (fallback_queries) *fallback_queries = (long long)idx->ds_ctr.read(0);
    return 0;
}
int mvdb_index_groups_counters(const mvdb_index* idx, long long* calls, long long* member_rows) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->gh_calls.load();
    if (member_rows) *member_rows = (long long)idx->gh_ctr.read<unsigned long long>(0);
    return 0;
}
int mvdb_index_maxsim_counters(const mvdb_index* idx, long long* calls, long long* passes) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->mx_calls.load();
    if (passes) *passes = (long long)idx->mx_passes.load();
    return 0;
}
int mvdb_index_assign_counters(const mvdb_index* idx, long long* calls, long long* passes) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->as_calls.load();
    if (passes) *passes = (long long)idx->as_passes.load();
    return 0;
}
int mvdb_index_examples_counters(const mvdb_index* idx, long long* calls, long long* passes) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->ex_calls.load();
    if (passes) *passes = (long long)idx->ex_passes.load();
    return 0;
}
double mvdb_range_band(int d, float qnorm, float row_norm_bound) {
    if (d <= 0 || !(qnorm >= 0.f) || !(row_norm_bound >= 0.f)) return INFINITY;
    return half_range_eps(d) * (double)qnorm * (double)row_norm_bound;
}
int mvdb_index_code8_refined(const mvdb_index* idx, long long* rows) {
    if (!idx || !rows) return fail(MVDB_ERR_ARG, "mvdb_index_code8_refined: bad arguments");
    *rows = 0;
    if (!idx->c8_ctr.dev()) return 0;
    DeviceGuard dg(idx->device);
    unsigned long long v = 0;
    MVDB_HIP(hipMemcpy(&v, idx->c8_ctr.dev() + 2, sizeof(v), hipMemcpyDeviceToHost));
    *rows = (long long)v;
    return 0;
}
int mvdb_code8_scan_geometry(int d, int64_t n, int device, int* rows_per_batch, int* waves) {
    if (!code8_dim(d) || n <= 0 || !rows_per_batch || !waves) return fail(MVDB_ERR_ARG, "mvdb_code8_scan_geometry: bad arguments");
    DeviceGuard dg(device);
    return with_code8_shape(d, [&](auto cs) {
        using K = decltype(cs);
        *rows_per_batch = (kWave / K::G) * K::SCAN_U;
        *waves = code8_scan_blocks<K::G, K::SCAN_U, K::MASKED, K::SCAN_BLOCKS>(n, device) * kScanWaves;
        return 0;
    });
}
int mvdb_code8_pack(int d, const int8_t* codes, uint8_t* high, uint8_t* low) {
    if (d <= 0 || d % 16 || !codes || !high || !low) return fail(MVDB_ERR_ARG, "mvdb_code8_pack: bad arguments");
    code8_pack_row(d, codes, high, low);
    return 0;
}
int mvdb_code8_unpack(int d, const uint8_t* high, const uint8_t* low, int8_t* codes) {
    if (d <= 0 || d % 16 || !codes || !high || !low) return fail(MVDB_ERR_ARG, "mvdb_code8_unpack: bad arguments");
    code8_unpack_row(d, high, low, codes);
    return 0;
}
int mvdb_code8_front_pack(int d, const int8_t* codes, uint8_t* image) {
    if (!code8_front_dim(d) || !codes || !image) return fail(MVDB_ERR_ARG, "mvdb_code8_front_pack: bad arguments (d must be a multiple of 32, at most 2048)");
    code8_front_pack_row(d, codes, image);
    return 0;
}
int mvdb_code8_front_unpack(int d, const uint8_t* image, int8_t* codes) {
    if (!code8_front_dim(d) || !codes || !image) return fail(MVDB_ERR_ARG, "mvdb_code8_front_unpack: bad arguments (d must be a multiple of 32, at most 2048)");
    code8_front_unpack_row(d, image, codes);
    return 0;
}
int mvdb_code8_front_geometry(int d, int64_t n, int device, int* rows_per_batch, int* waves) {
    if (!code8_dim(d) || n <= 0 || !rows_per_batch || !waves) return fail(MVDB_ERR_ARG, "mvdb_code8_front_geometry: bad arguments");
    DeviceGuard dg(device);
    return with_code8_shape(d, [&](auto cs) {
        using K = decltype(cs);
        *rows_per_batch = (kWave / K::FRONT_G) * K::FRONT_U;
        *waves = code8_scan_blocks<K::G, K::SCAN_U, K::MASKED, K::FRONT_BLOCKS, K::FRONT_G, K::FRONT_U>(n, device) * kScanWaves;
        return 0;
    });
}
int mvdb_index_code8_front_counters(const mvdb_index* idx, long long* survivors, long long* calls, long long* suspensions, int* held) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (survivors) *survivors = 0;
    if (calls) *calls = 0;
    if (suspensions) *suspensions = (long long)idx->c8_front.suspensions.load();
    if (held) {
        std::lock_guard<std::mutex> lk(idx->shadow_mu);
        *held = idx->code.F5.p ? 1 : 0;
    }
    if (!idx->c8_ctr.dev()) return 0;
    DeviceGuard dg(idx->device);
    unsigned int w[3] = {0, 0, 0};
    MVDB_HIP(hipMemcpy(w, idx->c8_ctr.dev() + 4, sizeof(w), hipMemcpyDeviceToHost));
    if (survivors) *survivors = (long long)((unsigned long long)w[0] | ((unsigned long long)w[1] << 32));
    if (calls) *calls = (long long)w[2];
    return 0;
}
int mvdb_index_code8_read_row(const mvdb_index* idx, int64_t row, uint8_t* high, uint8_t* low, uint8_t* front) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    std::lock_guard<std::mutex> sk(idx->shadow_mu);
    const Code8Store& c = idx->code;
    if (!c.C8.p || row < 0 || row >= c.rows) return fail(MVDB_ERR_ARG, "mvdb_index_code8_read_row: row %lld is not in the code", (long long)row);
    if (front && !c.F5.p) return fail(MVDB_ERR_ARG, "mvdb_index_code8_read_row: the code holds no front plane");
    DeviceGuard dg(idx->device);
    const int d = idx->d;
    if (high) MVDB_HIP(hipMemcpy(high, c.C8.p + row * code8_high_stride(d), code8_high_stride(d), hipMemcpyDeviceToHost));
    if (low) MVDB_HIP(hipMemcpy(low, c.low(d) + row * code8_low_stride(d), code8_low_stride(d), hipMemcpyDeviceToHost));
    if (front) {
        // the row's tile in one copy; the image is put together chunk by chunk, by the offsets the writers use
        const int64_t R = code8_front_tile_rows(d);
        const size_t tile_bytes = (size_t)R * (size_t)code8_front_stride(d);
        const size_t tile_at = (size_t)(row / R * R) * (size_t)code8_front_stride(d);
        std::vector<uint8_t> tile(tile_bytes);
        MVDB_HIP(hipMemcpy(tile.data(), c.F5.p + tile_at, tile_bytes, hipMemcpyDeviceToHost));
        for (int t = 0; t < d / 32; ++t) {
            memcpy(front + 16 * t, tile.data() + (code8_front_wide_offset(row, t, d) - tile_at), 16);
            memcpy(front + d / 2 + 4 * t, tile.data() + (code8_front_narrow_offset(row, t, d) - tile_at), 4);
        }
    }
    return 0;
}
int mvdb_code8_bit2_pack(int d, const int8_t* codes, uint8_t* bits) {
    if (!code8_front_dim(d) || !codes || !bits) return fail(MVDB_ERR_ARG, "mvdb_code8_bit2_pack: bad arguments (d must be a multiple of 32, at most 2048)");
    code8_bit2_pack_row(d, codes, bits);
    return 0;
}
int mvdb_code8_bit2_unpack(int d, const uint8_t* bits, int8_t* codes) {
    if (!code8_front_dim(d) || !codes || !bits) return fail(MVDB_ERR_ARG, "mvdb_code8_bit2_unpack: bad arguments (d must be a multiple of 32, at most 2048)");
    code8_bit2_unpack_row(d, bits, codes);
    return 0;
}
int mvdb_index_code8_read_bit2(const mvdb_index* idx, int64_t row, uint8_t* bits, int* held) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    std::lock_guard<std::mutex> sk(idx->shadow_mu);
    const Code8Store& c = idx->code;
    if (held) *held = c.B2.p ? 1 : 0;
    if (!bits) return 0;
    if (!c.C8.p || row < 0 || row >= c.rows) return fail(MVDB_ERR_ARG, "mvdb_index_code8_read_bit2: row %lld is not in the code", (long long)row);
    if (!c.B2.p) return fail(MVDB_ERR_ARG, "mvdb_index_code8_read_bit2: the code holds no bit plane");
    DeviceGuard dg(idx->device);
    const int stride = code8_bit2_stride(idx->d);
    MVDB_HIP(hipMemcpy(bits, c.B2.p + row * stride, stride, hipMemcpyDeviceToHost));
    return 0;
}
int mvdb_code8_front_offset(int d, int64_t row, int chunk, int64_t* wide, int64_t* narrow) {
    if (!code8_front_dim(d) || row < 0 || chunk < 0 || chunk >= d / 32 || !wide || !narrow)
        return fail(MVDB_ERR_ARG, "mvdb_code8_front_offset: bad arguments (d a multiple of 32, at most 2048; chunk in [0, d / 32))");
    *wide = (int64_t)code8_front_wide_offset(row, chunk, d);
    *narrow = (int64_t)code8_front_narrow_offset(row, chunk, d);
    return 0;
}
int mvdb_code8_margin(int d, float qnorm, float qstep, float row_norm_bound, float* alpha, float* beta) {
    if (d <= 0 || !alpha || !beta) return fail(MVDB_ERR_ARG, "mvdb_code8_margin: bad arguments");
    const Code8Margin m = code8_margin(d, qnorm, qstep, row_norm_bound);
    *alpha = m.alpha;
    *beta = m.beta;
    return 0;
}
int mvdb_index_dim(const mvdb_index* idx) { return idx ? idx->d : -1; }
int mvdb_index_device(const mvdb_index* idx) { return idx ? idx->device : -1; }

int mvdb_index_reserve(mvdb_index* idx, int64_t n) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    if (n <= idx->cap) return 0;
    MVDB_TRY(quiesce(idx));
    return grow(idx, n, /*exact=*/true);
}

// Keeps idx->row_norm_bound >= |row| for every stored row: 1 for rows normalised on the device, one
// extra read of the new rows otherwise (non-finite rows leave the bound non-finite).  The new rows are [0, n) behind dst, or
// (set_rows) the n stored rows list_dev names, dst at row 0.  The bounds only ever widen.
static int note_row_norms(mvdb_index* idx, const float* dst, int64_t n, int normalize, const int64_t* list_dev = nullptr) {
    const bool l2 = idx->metric == MVDB_METRIC_L2;
    if (normalize && !l2) {
        // |row| after normalize_rows_kernel: |x| / sqrt(fl(|x|^2)) with an fp32 sum of depth <= 4 * 16 + 6 (d <= 4096),
        // one sqrt, one divide, one multiply: <= 1 + (70 / 2 + 3) * 2^-24 = 1 + 2.3e-6
        idx->row_norm_bound = std::max(idx->row_norm_bound, 1.000004f);
        return 0;
    }
    // raw rows — and every row of an L2 index, whose certified batch passes need BOTH ends of the norm range (a zero row
    // that normalisation left alone has norm 0): one extra read of the new rows
    if (!idx->normmax.p) MVDB_HIP(idx->normmax.alloc(2 * sizeof(unsigned int)));
    unsigned int* dmax = idx->normmax.p;
    unsigned int bits[2] = {0u, 0x7F800000u};  // max = 0, min = +inf
    hipError_t e = hipMemcpyAsync(dmax, bits, sizeof(bits), hipMemcpyHostToDevice, idx->mut);
    if (e == hipSuccess) e = hipStreamSynchronize(idx->mut);  // (bits is a stack buffer)
    if (e == hipSuccess) {
        const int grid = row_grid(idx->device, n);
        if (l2)
            hipLaunchKernelGGL(row_norm2_range_kernel, dim3(grid), dim3(256), 0, idx->mut, dst, n, idx->ld, idx->d4, dmax, list_dev);
        else
            hipLaunchKernelGGL(max_row_norm2_kernel, dim3(grid), dim3(256), 0, idx->mut, dst, n, idx->ld, idx->d4, dmax, list_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bits, dmax, sizeof(bits), hipMemcpyDeviceToHost, idx->mut);
    if (e == hipSuccess) e = hipStreamSynchronize(idx->mut);
    MVDB_HIP(e);
    float n2, lo2;
    memcpy(&n2, &bits[0], sizeof(n2));
    memcpy(&lo2, &bits[1], sizeof(lo2));
    const float bound = std::isfinite(n2) ? std::sqrt(n2) * 1.000001f : INFINITY;
    idx->row_norm_bound = std::max(idx->row_norm_bound, normalize ? std::max(bound, 1.000004f) : bound);
    if (l2) {
        // the kernel's fp32 sums carry <= (depth + 1) 2^-24 < 5e-6 relative error: widen to bounds of the TRUE squared norms
        if (std::isfinite(n2) && std::isfinite(lo2)) {
            idx->norm2_hi = std::max(idx->norm2_hi, n2 * 1.00001f);
            idx->norm2_lo = std::min(idx->norm2_lo, lo2 * 0.99999f);
        } else {
            idx->norm2_hi = INFINITY;
            idx->norm2_lo = 0.f;
        }
    }
    return 0;
}

// What the three add entry points share (they keep their argument checks): room for n more rows, then fill(dst) enqueues the
// rows behind dst on idx->mut.  The rows are not visible to searches until idx->n moves, at the end; everything runs on the
// index's own stream.
static int append_rows(mvdb_index* idx, int64_t n, int normalize, const std::function<int(float*)>& fill) {
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    if (idx->n + n > 0xFFFFFFFFll)
        return fail(MVDB_ERR_ARG, "more than 2^32-1 rows per device index are not supported");
    MVDB_TRY(quiesce(idx));
    MVDB_TRY(grow(idx, idx->n + n, /*exact=*/false));
    float* dst = idx->X.p + idx->n * idx->ld;
    MVDB_TRY(fill(dst));
    if (normalize) MVDB_TRY(normalize_range(idx, dst, n, idx->mut));
    MVDB_HIP(hipStreamSynchronize(idx->mut));  // the caller's buffer is free again, the rows are in place
    MVDB_TRY(note_row_norms(idx, dst, n, normalize));
    MVDB_TRY(idx->shadow.extend(idx, n));
    MVDB_TRY(idx->code.extend(idx, n));
    idx->n += n;
    return 0;
}

int mvdb_index_add(mvdb_index* idx, const float* x_host, int64_t n, int normalize) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (n == 0) return 0;
    if (!x_host) return fail(MVDB_ERR_ARG, "x is NULL");
    return append_rows(idx, n, normalize, [&](float* dst) {
        if (idx->ld == idx->d) {
            MVDB_HIP(hipMemcpyAsync(dst, x_host, (size_t)n * idx->d * sizeof(float), hipMemcpyHostToDevice, idx->mut));
        } else {
            MVDB_HIP(hipMemsetAsync(dst, 0, (size_t)n * idx->ld * sizeof(float), idx->mut));
            MVDB_HIP(hipMemcpy2DAsync(dst, idx->ld * sizeof(float), x_host, idx->d * sizeof(float),
                                      idx->d * sizeof(float), (size_t)n, hipMemcpyHostToDevice, idx->mut));
        }
        return 0;
    });
}

int mvdb_index_add_device(mvdb_index* idx, const float* x_dev, int64_t n, int normalize) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (n == 0) return 0;
    if (!x_dev) return fail(MVDB_ERR_ARG, "x is NULL");
    return append_rows(idx, n, normalize, [&](float* dst) {
        // x_dev is the caller's: whatever produced it must be complete (or ordered before the legacy stream) — as before, the
        // copy below waits for the legacy stream only when it is issued there, so it is issued on the mutators' stream after a
        // legacy-stream join
        MVDB_HIP(hipStreamSynchronize(nullptr));
        if (idx->ld == idx->d) {
            MVDB_HIP(hipMemcpyAsync(dst, x_dev, (size_t)n * idx->d * sizeof(float), hipMemcpyDeviceToDevice, idx->mut));
        } else {
            const int grid = (int)std::min<int64_t>((n * idx->ld + 255) / 256, (int64_t)device_cus(idx->device) * 16);
            hipLaunchKernelGGL(pad_rows_kernel, dim3(grid), dim3(256), 0, idx->mut, dst, x_dev, n, idx->d, idx->ld);
            MVDB_HIP(hipGetLastError());
        }
        return 0;
    });
}

int mvdb_index_add_synthetic(mvdb_index* idx, int64_t n, uint64_t seed, int64_t first_row,
                             int normalize) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0 || first_row < 0) return fail(MVDB_ERR_ARG, "negative row count / offset");
    if (n == 0) return 0;
    return append_rows(idx, n, normalize, [&](float* dst) {
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n * idx->d4 + 255) / 256, (int64_t)device_cus(idx->device) * 16));
        hipLaunchKernelGGL(synth_fill_kernel, dim3(grid), dim3(256), 0, idx->mut, dst, n, idx->ld, idx->d, seed, first_row);
        MVDB_HIP(hipGetLastError());
        return 0;
    });
}

// ---- set_rows: stored rows overwritten in place (contract: mvdb.h) -----------------------------------------------------------
constexpr size_t kSetStageBytes = 32u << 20;   // one chunk of staged rows: at most this many bytes (and at least one row)

// every row in [0, n), none twice; nothing is enqueued before this has passed.  sorted: takes the ascending copy.
static int check_row_list(const int64_t* rows_host, int64_t m, int64_t n, std::vector<int64_t>* sorted = nullptr) {
    std::vector<int64_t> v(rows_host, rows_host + m);
    std::sort(v.begin(), v.end());
    for (int64_t i = 0; i < m; ++i) {
        if (v[i] < 0 || v[i] >= n) return fail(MVDB_ERR_ARG, "row %lld out of range [0,%lld)", (long long)v[i], (long long)n);
        if (i && v[i] == v[i - 1]) return fail(MVDB_ERR_ARG, "row %lld listed twice", (long long)v[i]);
    }
    if (sorted) sorted->swap(v);
    return 0;
}

// Caller holds the index exclusively, searches quiesced.  Per chunk of at most kSetStageBytes: the row numbers and the new rows
// go to the staging buffers (at the matrix' stride, padding zero), scatter_rows_kernel writes them over the stored rows, and
// each derived store that covers a listed row is converted from the stored row by the kernel that add uses, in its list form.
// A fixed number of launches per chunk; nothing here is proportional to idx->n.
static int set_rows_core(mvdb_index* idx, const int64_t* rows_host, const float* x, bool x_on_device, int64_t m, int normalize) {
    const size_t row_bytes = (size_t)idx->ld * sizeof(float);
    const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(1, (int64_t)(kSetStageBytes / row_bytes)));
    MVDB_TRY(idx->set_stage.reserve((size_t)chunk * idx->ld));
    MVDB_TRY(idx->set_list.reserve((size_t)chunk));
    float* S = idx->set_stage.p;
    int64_t* L = idx->set_list.p;
    const Shape sh = choose_shape(idx->d4);
    const int rpi = 64 / sh.G;
    const bool padded = idx->ld != idx->d;
    ShadowStore& sh16 = idx->shadow;
    if (x_on_device) MVDB_HIP(hipStreamSynchronize(nullptr));  // (mvdb_index_add_device's join with the legacy stream)
    // the shadow at the scale it was built with: should the widened bound ask for another one, it is invalidated below
    const bool shadow = sh16.Xh.p && sh16.rows > 0;
    const bool offsets = sh16.Hn.p && sh16.hn_rows > 0;
    const bool code = idx->code.C8.p && idx->code.rows > 0;
    for (int64_t i0 = 0; i0 < m; i0 += chunk) {
        const int64_t rows = std::min(chunk, m - i0);
        const float* src = x + i0 * idx->d;
        MVDB_HIP(hipMemcpyAsync(L, rows_host + i0, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, idx->mut));
        if (!padded) {
            MVDB_HIP(hipMemcpyAsync(S, src, (size_t)rows * row_bytes, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, idx->mut));
        } else if (x_on_device) {
            const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((rows * idx->ld + 255) / 256, (int64_t)device_cus(idx->device) * 16));
            hipLaunchKernelGGL(pad_rows_kernel, dim3(grid), dim3(256), 0, idx->mut, S, src, rows, idx->d, idx->ld);
        } else {
            MVDB_HIP(hipMemsetAsync(S, 0, (size_t)rows * row_bytes, idx->mut));
            MVDB_HIP(hipMemcpy2DAsync(S, row_bytes, src, idx->d * sizeof(float), idx->d * sizeof(float), (size_t)rows, hipMemcpyHostToDevice,
                                      idx->mut));
        }
        hipLaunchKernelGGL(scatter_rows_kernel, dim3(row_grid(idx->device, (rows + rpi - 1) / rpi, 8)), dim3(256), 0, idx->mut, idx->X.p,
                           (const float*)S, (const int64_t*)L, rows, idx->ld, idx->d4, (int)(idx->ld / 4), sh.G, normalize);
        MVDB_HIP(hipGetLastError());
        if (shadow)
            MVDB_TRY(launch_half_shadow(idx->X.p, idx->ld, idx->d, rows, sh16.scale, sh16.Xh.p, idx->device, idx->mut, L, sh16.rows));
        if (offsets) MVDB_TRY(launch_half_norms(idx->X.p, idx->ld, idx->d, rows, sh16.Hn.p, idx->device, idx->mut, L, sh16.hn_rows));
        if (code) {
            MVDB_TRY(idx->code.build(idx, 0, rows, idx->mut, L));
            // a listed row may be one of the floor's sample: the whole copy is gathered again (a fixed 131,072 rows)
            if (idx->code.sample_valid(idx->n)) MVDB_TRY(idx->code.gather_sample(idx, idx->n, idx->mut));
        }
        // (waits for the chunk: the staging buffers are free again, and so is the caller's part of x)
        MVDB_TRY(note_row_norms(idx, idx->X.p, rows, normalize, L));
        MVDB_HIP(hipStreamSynchronize(idx->mut));
    }
    if (shadow && half_xscale(idx->row_norm_bound) != sh16.scale) sh16.invalidate();  // (ShadowStore::extend's rule)
    return 0;
}

static int set_rows_entry(mvdb_index* idx, const int64_t* rows_host, const float* x, bool x_on_device, int64_t m, int normalize) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    if (!x) return fail(MVDB_ERR_ARG, "x is NULL");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_row_list(rows_host, m, idx->n));
    DeviceGuard dg(idx->device);
    MVDB_TRY(quiesce(idx));
    return set_rows_core(idx, rows_host, x, x_on_device, m, normalize);
}

int mvdb_index_set_rows(mvdb_index* idx, const int64_t* rows_host, const float* x_host, int64_t m, int normalize) {
    return set_rows_entry(idx, rows_host, x_host, false, m, normalize);
}

int mvdb_index_set_rows_device(mvdb_index* idx, const int64_t* rows_host, const float* x_dev, int64_t m, int normalize) {
    return set_rows_entry(idx, rows_host, x_dev, true, m, normalize);
}

int mvdb_index_get_rows(const mvdb_index* idx, int64_t row0, int64_t n, float* out_host) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n == 0) return 0;
    if (!out_host) return fail(MVDB_ERR_ARG, "out is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (row0 < 0 || n < 0 || row0 + n > idx->n)
        return fail(MVDB_ERR_ARG, "rows [%lld,%lld) out of range [0,%lld)", (long long)row0,
                    (long long)(row0 + n), (long long)idx->n);
    DeviceGuard dg(idx->device);
    const float* src = idx->X.p + row0 * idx->ld;
    if (idx->ld == idx->d)
        MVDB_HIP(hipMemcpy(out_host, src, (size_t)n * idx->d * sizeof(float), hipMemcpyDeviceToHost));
    else
        MVDB_HIP(hipMemcpy2D(out_host, idx->d * sizeof(float), src, idx->ld * sizeof(float),
                             idx->d * sizeof(float), (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// ---- remove_rows: the tail behind the first deleted row is compacted in place, by one of two routes ----------------------------
// the staging buffer of both routes, kept between calls
static int reserve_ctmp(mvdb_index* idx, size_t bytes) {
    if (idx->ctmp_bytes >= bytes) return 0;
    idx->ctmp_bytes = 0;
    if (idx->ctmp.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MVDB_ERR_OOM, "device allocation for row compaction failed (%zu bytes)", bytes);
    }
    idx->ctmp_bytes = bytes;
    return 0;
}

// The sorted delete list, made relative to the tail's first row, goes to the device on idx->mut (stream-ordered allocation:
// hipFree would synchronise the device).  *e: the copy's status, which finish_compaction reports with the launches'.
static int upload_deletes(mvdb_index* idx, std::vector<int64_t>& del, int64_t** del_dev, hipError_t* e) {
    MVDB_HIP(hipMallocAsync((void**)del_dev, del.size() * sizeof(int64_t), idx->mut));
    const int64_t first = del[0];
    for (auto& v : del) v -= first;
    *e = hipMemcpyAsync(*del_dev, del.data(), del.size() * sizeof(int64_t), hipMemcpyHostToDevice, idx->mut);
    return 0;
}

static int finish_compaction(mvdb_index* idx, int64_t* del_dev, hipError_t e) {
    if (del_dev) (void)hipFreeAsync(del_dev, idx->mut);
    if (e == hipSuccess) e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(idx->mut);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(MVDB_ERR_HIP, "row compaction failed: %s", hipGetErrorString(e));
    return 0;
}

// A handful of rows (the reference deletes ONE per call, vector_database.py:119) or one run: the tail is shifted in place in one
// pass — every byte read once and written once — with a side copy of m rows per workgroup boundary (util_kernels.hpp:
// shift_rows_kernel); delete of an early row of 10M x 512: 14.5 -> 8.2 ms (profiles/r06_delete_probe.jsonl).  *done stays
// false where the side copies would outgrow their bound: the staged route serves.
static int compact_shift(mvdb_index* idx, std::vector<int64_t>& del, int64_t tail_new, bool* done) {
    const int64_t m = (int64_t)del.size(), first = del[0];
    const bool run = del[m - 1] - del[0] == m - 1;
    const int64_t rowunits = idx->ld / 4;  // 16-byte units per row (ld is a multiple of 4 floats)
    const int64_t new_units = tail_new * rowunits, old_units = (idx->n - first) * rowunits;
    const int64_t slice = 256 * kShiftUnits;
    const int64_t side_units = m * rowunits;
    const int64_t cus = device_cus(idx->device);
    // eight workgroups per CU; fewer (down to two) where the side copies of that many boundaries would outgrow their bound
    int64_t groups = std::min<int64_t>(cus * 8, (new_units + slice - 1) / slice);
    const int64_t fit = (int64_t)(kShiftSideBytes / ((size_t)side_units * 16)) + 1;
    const bool fits = fit >= std::min<int64_t>(groups, cus * 2);
    groups = std::min(groups, fit);
    const int64_t range = ((new_units + groups - 1) / groups + slice - 1) / slice * slice;
    groups = (new_units + range - 1) / range;
    const size_t side_bytes = (size_t)std::max<int64_t>(groups - 1, 1) * side_units * 16;
    if (!fits || side_bytes > kShiftSideBytes) return 0;
    MVDB_TRY(reserve_ctmp(idx, side_bytes));
    int64_t* del_dev = nullptr;
    hipError_t e = hipSuccess;
    if (!run) MVDB_TRY(upload_deletes(idx, del, &del_dev, &e));
    f32x4u* tail = reinterpret_cast<f32x4u*>(idx->X.p + first * idx->ld);
    f32x4u* side = reinterpret_cast<f32x4u*>(idx->ctmp.p);
    if (groups > 1) {
        const unsigned gx = (unsigned)std::min<int64_t>((side_units + 255) / 256, 64);
        hipLaunchKernelGGL(shift_save_kernel, dim3(gx, (unsigned)(groups - 1)), dim3(256), 0, idx->mut, side, tail, range, side_units,
                           old_units);
    }
    if (run)
        hipLaunchKernelGGL(shift_rows_kernel<true>, dim3((unsigned)groups), dim3(256), 0, idx->mut, tail, side, del_dev, m, new_units,
                           range, rowunits, side_units);
    else
        hipLaunchKernelGGL(shift_rows_kernel<false>, dim3((unsigned)groups), dim3(256), 0, idx->mut, tail, side, del_dev, m, new_units,
                           range, rowunits, side_units);
    *done = true;
    return finish_compaction(idx, del_dev, e);
}

// Every kept row moves UP, so the tail is compacted in place, in ascending chunks through a bounded staging buffer (512 MiB,
// MVDB_COMPACT_BYTES; kept by the index): chunk c gathers the sources of the new rows [r0, r0 + rows) — all at or above
// r0 + 1 — into the buffer, then copies the buffer over [r0, r0 + rows); stream order makes the next chunk's sources (all
// >= r0 + rows) untouched by that copy.  (Until round 4 the whole tail went through a temporary of its own size: one early
// delete in a 164 GB index needed another 164 GB.)  The source row of a new row is found by binary search in the sorted list
// of deleted rows.
static int compact_staged(mvdb_index* idx, std::vector<int64_t>& del, int64_t tail_new) {
    const int64_t m = (int64_t)del.size(), first = del[0];
    const size_t row_bytes = (size_t)idx->ld * sizeof(float);
    MVDB_TRY(reserve_ctmp(idx, std::min<size_t>((size_t)tail_new * row_bytes, std::max<size_t>((size_t)idx->kn.compact_bytes, row_bytes))));
    const int64_t chunk_rows = (int64_t)(idx->ctmp_bytes / row_bytes);
    int64_t* del_dev = nullptr;
    hipError_t e = hipSuccess;
    MVDB_TRY(upload_deletes(idx, del, &del_dev, &e));
    float* tail = idx->X.p + first * idx->ld;
    for (int64_t r0 = 0; r0 < tail_new && e == hipSuccess; r0 += chunk_rows) {
        const int64_t rows = std::min(chunk_rows, tail_new - r0);
        hipLaunchKernelGGL(gather_kept_rows_kernel, dim3(row_grid(idx->device, rows)), dim3(256), 0, idx->mut, idx->ctmp.p, tail, del_dev, m, r0,
                           rows, idx->ld);
        e = hipMemcpyAsync(tail + r0 * idx->ld, idx->ctmp.p, (size_t)rows * row_bytes, hipMemcpyDeviceToDevice, idx->mut);
    }
    return finish_compaction(idx, del_dev, e);
}

int mvdb_index_remove_rows(mvdb_index* idx, const int64_t* rows_host, int64_t m) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m == 0) return 0;
    if (!rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    std::vector<int64_t> del;
    MVDB_TRY(check_row_list(rows_host, m, idx->n, &del));
    DeviceGuard dg(idx->device);
    MVDB_TRY(quiesce(idx));
    ++idx->renumbered;
    idx->shadow.invalidate();  // rows are renumbered: the next batch search rebuilds the shadow in the allocation it already has
    idx->code.invalidate();
    const int64_t n_new = idx->n - m;
    // rows before the first deleted one do not move: compact only the tail [first, n)
    const int64_t tail_new = n_new - del[0];
    if (n_new > 0 && tail_new > 0) {
        bool done = false;  // MVDB_COMPACT_INPLACE=0: always the staged route
        if (idx->kn.compact_inplace && (m <= kShiftMaxRows || del[m - 1] - del[0] == m - 1)) MVDB_TRY(compact_shift(idx, del, tail_new, &done));
        if (!done) MVDB_TRY(compact_staged(idx, del, tail_new));
    }
    idx->n = n_new;
    return 0;
}

int mvdb_index_search(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                      float* D_host, int64_t* I_host) {
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(search_core(idx, call.ws, call.ws->q.p, nq, k, normalize_q, nullptr, 0, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_subset(const mvdb_index* idx, const float* q_host, int nq, int k,
                             int normalize_q, const int64_t* rows_host, int64_t m, float* D_host,
                             int64_t* I_host) {
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    if (m < 0) return fail(MVDB_ERR_ARG, "negative subset size");
    if (m > 0 && !rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const RowRange rr = row_range(rows_host, m);
    if (m > 0 && (rr.lo < 0 || rr.hi >= idx->n))
        return fail(MVDB_ERR_ARG, "subset row %lld out of range [0,%lld)", (long long)(rr.lo < 0 ? rr.lo : rr.hi),
                    (long long)idx->n);
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* ws = call.ws;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(ws->rows.reserve((size_t)std::max<int64_t>(m, 1)));
    if (m > 0) {
        hipError_t e = hipMemcpyAsync(ws->rows.p, rows_host, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, ws->stream);
        if (e != hipSuccess) return fail(MVDB_ERR_HIP, "subset upload failed: %s", hipGetErrorString(e));
    }
    MVDB_TRY(search_core(idx, ws, ws->q.p, nq, k, normalize_q, ws->rows.p, m, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_device(const mvdb_index* idx, const float* q_dev, int nq, int k,
                             int normalize_q, int64_t label_offset, float* D_dev, int64_t* I_dev,
                             void* stream) {
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    // (certification failures of the batch passes are re-run by device-gated launches: nothing here reads from the device)
    return search_core(idx, call.ws, call.q, nq, k, normalize_q, nullptr, 0, label_offset, D_dev, I_dev);
}

__global__ void map_subset_labels_kernel(int64_t* I, int64_t total, const int64_t* __restrict__ rows,
                                         int64_t label_offset) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const int64_t p = I[i];
        I[i] = p >= 0 ? rows[p] + label_offset : -1;
    }
}

int mvdb_index_search_subset_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const int64_t* rows_dev, int64_t m, int map_labels, int64_t label_offset,
                                    float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    if (m < 0) return fail(MVDB_ERR_ARG, "negative subset size");
    if (m > 0 && !rows_dev) return fail(MVDB_ERR_ARG, "rows is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    Workspace* ws = call.ws;
    // m == 0: search_core's empty-corpus branch needs a non-NULL row list to take the subset meaning
    const int64_t* rows = m > 0 ? rows_dev : reinterpret_cast<const int64_t*>(ws->st);
    MVDB_TRY(search_core(idx, ws, call.q, nq, k, normalize_q, rows, m, map_labels ? 0 : label_offset, D_dev, I_dev));
    if (map_labels && m > 0) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(map_subset_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ws->stream,
                           I_dev, total, rows_dev, label_offset);
        MVDB_HIP(hipGetLastError());
    }
    return 0;
}

static int finish_mask_labels(const mvdb_index* idx, Workspace* ws, int nq, int k, const uint64_t* mask_dev, int labels,
                              int64_t* I_dev) {
    if (labels == 0) {  // positions in the ascending list of the set rows (what mvdb_index_search_subset returns for that list)
        hipLaunchKernelGGL(mask_rank_kernel, dim3((unsigned)((int64_t)nq * k)), dim3(256), 0, ws->stream, I_dev, mask_dev);
        MVDB_HIP(hipGetLastError());
    }
    return 0;
}

int mvdb_index_search_masked_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const uint64_t* mask_dev, int labels, int64_t label_offset, float* D_dev,
                                    int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    if (!mask_dev) return fail(MVDB_ERR_ARG, "mask is NULL");
    if (labels != 0 && labels != 1) return fail(MVDB_ERR_ARG, "labels must be 0 (positions) or 1 (row numbers)");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    Workspace* ws = call.ws;
    MVDB_TRY(search_core(idx, ws, call.q, nq, k, normalize_q, nullptr, 0, labels == 1 ? label_offset : 0, D_dev, I_dev, true, mask_dev));
    return finish_mask_labels(idx, ws, nq, k, mask_dev, labels, I_dev);
}

int mvdb_index_search_masked(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                             const uint64_t* mask_host, int labels, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    if (!mask_host) return fail(MVDB_ERR_ARG, "mask is NULL");
    if (labels != 0 && labels != 1) return fail(MVDB_ERR_ARG, "labels must be 0 (positions) or 1 (row numbers)");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* ws = call.ws;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    const size_t words = (size_t)((idx->n + 63) / 64);
    MVDB_TRY(ws->rows.reserve(std::max<size_t>(words, 1)));  // 8-byte words: the row-list buffer serves
    uint64_t* mask_dev = reinterpret_cast<uint64_t*>(ws->rows.p);
    if (words) {
        hipError_t e = hipMemcpyAsync(mask_dev, mask_host, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream);
        if (e != hipSuccess) return fail(MVDB_ERR_HIP, "mask upload failed: %s", hipGetErrorString(e));
    }
    MVDB_TRY(search_core(idx, ws, ws->q.p, nq, k, normalize_q, nullptr, 0, 0, D_dev, I_dev, true, mask_dev));
    MVDB_TRY(finish_mask_labels(idx, ws, nq, k, mask_dev, labels, I_dev));
    return call.fetch(total, D_host, I_host);
}

// ---- resident row sets: a filter's rows uploaded ONCE, searched many times ---------------------------------------------
// Built on the host in one pass over the list (range check, sortedness, duplicates are the caller's business as in
// mvdb_index_search_subset): a SORTED list that keeps at least 90 % of the rows, and every "all rows but these" set,
// becomes a bitmap (n / 8 bytes up the wire instead of 8 per row, one full-rate pass per search); anything else stays a
// row list on the device.  Results carry ROW NUMBERS.
}  // extern "C"

// would search_core answer a bitmap-selected batch of nq queries on shared corpus passes? (its own conditions, restated)
static bool masked_batch_possible(const mvdb_index* idx, int nq, int k, int64_t n) {
    if (nq < 2 || k > kMaxFusedK || idx->ld != idx->d || idx->kn.disable_masked_batch) return false;
    if (idx->metric == MVDB_METRIC_IP) return mfma_gated_queries(idx) > 0;
    return (l2_cert_ok(idx) || l2_offsets_ok(idx, nq, n)) && half_path_ok(idx) && nq >= half_min_nq(idx, n);
}

struct mvdb_rowset {
    uint64_t owner = 0;       // serial number of the index the set was built on (never reused, unlike an address)
    int device = 0;
    int64_t n_at_create = 0;  // the index's row count the set was built against
    uint64_t renumbered = 0;  // ... and its renumbering generation
    int64_t count = 0;        // rows selected
    int64_t* rows = nullptr;  // list form (device), in the caller's order
    uint64_t* mask = nullptr; // bitmap form (device)
    uint64_t* twin = nullptr; // list form, sorted, n >= 4096: the same rows as a bitmap too (n / 8 bytes) — what a BATCH of queries
                              // is searched under when sharing corpus passes beats one gathered scan per query (rowset_search_core)
};

extern "C" {

int mvdb_rowset_create(const mvdb_index* idx, const int64_t* rows_host, int64_t m, int excluded, mvdb_rowset** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m > 0 && !rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int64_t n = idx->n;
    const RowRange rr = row_range(rows_host, m);
    if (m > 0 && (rr.lo < 0 || rr.hi >= n))
        return fail(MVDB_ERR_ARG, "row %lld out of range [0,%lld)", (long long)(rr.lo < 0 ? rr.lo : rr.hi), (long long)n);
    const bool sorted = rr.sorted;
    DeviceGuard dg(idx->device);
    mvdb_rowset* rs = new mvdb_rowset();
    rs->owner = idx->serial;
    rs->device = idx->device;
    rs->n_at_create = n;
    rs->renumbered = idx->renumbered;
    // bitmap: "all rows but these", and sorted lists that keep >= 90 % of the rows.  On the device a resident LIST is
    // gathered at 6.2-7.0 TB/s of rows touched (10M x 512: half the rows 1.50 ms, 90 % 2.65 ms, 99 % 2.89 ms) against
    // 2.87 ms for the bitmap's full pass at any density, so the bitmap only wins where the list is ~n long — there it
    // is 64x smaller in HBM and on the wire
    const bool as_mask = excluded || (sorted && m * 10 >= n * 9 && n >= 4096);
    hipError_t e = hipSuccess;
    if (as_mask) {
        const size_t words = (size_t)((n + 63) / 64);
        std::vector<uint64_t> w(std::max<size_t>(words, 1), excluded ? ~0ull : 0ull);
        if (excluded) {
            if (n == 0) w[0] = 0;                                   // an empty index: no row is selected
            else if (n & 63) w[words - 1] = (1ull << (n & 63)) - 1ull;  // bits at or beyond n stay clear
            int64_t removed = 0;
            for (int64_t i = 0; i < m; ++i) {
                uint64_t& word = w[rows_host[i] >> 6];
                const uint64_t bit = 1ull << (rows_host[i] & 63);
                removed += (word & bit) != 0;  // a row listed twice is removed once
                word &= ~bit;
            }
            rs->count = n - removed;
        } else {
            for (int64_t i = 0; i < m; ++i) w[rows_host[i] >> 6] |= 1ull << (rows_host[i] & 63);
            rs->count = m;  // sorted strictly ascending: no duplicates
        }
        e = hipMalloc((void**)&rs->mask, w.size() * sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemcpy(rs->mask, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    } else {
        rs->count = m;
        e = hipMalloc((void**)&rs->rows, (size_t)std::max<int64_t>(m, 1) * sizeof(int64_t));
        if (e == hipSuccess && m > 0) e = hipMemcpy(rs->rows, rows_host, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && sorted && n >= 4096 && m * 64 >= n) {   // (sparser than 1 row in 64: no batch is better off under a bitmap)
            const size_t words = (size_t)((n + 63) / 64);
            std::vector<uint64_t> w(words, 0ull);
            for (int64_t i = 0; i < m; ++i) w[rows_host[i] >> 6] |= 1ull << (rows_host[i] & 63);
            if (hipMalloc((void**)&rs->twin, words * sizeof(uint64_t)) != hipSuccess ||
                hipMemcpy(rs->twin, w.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipGetLastError();   // the twin is an optimisation: without it batches answer one query at a time
                if (rs->twin) (void)hipFree(rs->twin);
                rs->twin = nullptr;
            }
        }
    }
    if (e != hipSuccess) {
        if (rs->mask) (void)hipFree(rs->mask);
        if (rs->rows) (void)hipFree(rs->rows);
        if (rs->twin) (void)hipFree(rs->twin);
        delete rs;
        return fail(MVDB_ERR_HIP, "row set upload failed: %s", hipGetErrorString(e));
    }
    *out = rs;
    return 0;
}

int64_t mvdb_rowset_size(const mvdb_rowset* rs) { return rs ? rs->count : -1; }
int mvdb_rowset_is_bitmap(const mvdb_rowset* rs) { return rs && rs->mask ? 1 : 0; }

int mvdb_rowset_free(mvdb_rowset* rs) {
    if (!rs) return 0;
    {
        DeviceGuard dg(rs->device);
        if (rs->mask) (void)hipFree(rs->mask);
        if (rs->rows) (void)hipFree(rs->rows);
        if (rs->twin) (void)hipFree(rs->twin);
    }
    delete rs;
    return 0;
}

// the body shared by the host and the device entry points: queries on the device, results to device buffers
static int rowset_check(const mvdb_index* idx, const mvdb_rowset* rs) {
    if (!rs) return fail(MVDB_ERR_ARG, "row set is NULL");
    // rows appended since the set was built are simply not part of it (the filter was evaluated before they arrived);
    // a SHRUNK index has renumbered its rows: the set is stale
    if (rs->owner != idx->serial) return fail(MVDB_ERR_ARG, "the row set belongs to another index");
    if (rs->device != idx->device || rs->n_at_create > idx->n || rs->renumbered != idx->renumbered)
        return fail(MVDB_ERR_ARG, "the row set was built for another state of the index (%lld rows then, %lld now)",
                    (long long)rs->n_at_create, (long long)idx->n);
    return 0;
}
static int rowset_search_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int normalize_q,
                              const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    tls_single_suspended = false;  // (the routing questions asked here are about batches; search_core decides for its own call)
    const int64_t total = (int64_t)nq * k;
    if (rs->count == 0 || (rs->mask && rs->n_at_create == 0)) {  // nothing selected (search_core reads m == 0 as "every row")
        hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ws->stream, D_dev, I_dev,
                           total, idx->metric);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    if (rs->mask)
        return search_core(idx, ws, q, nq, k, normalize_q, nullptr, rs->n_at_create, label_offset, D_dev, I_dev, true, rs->mask);
    // A batch under a LIST: one gathered scan per query costs nq x (fraction of the rows) full passes; under the list's bitmap
    // twin the queries share corpus passes (the certified pass over the fp16 shadow: ~0.6 of a full pass per 128 / 256
    // queries; else the fp32-MFMA pass: one per 16 / 32 queries).  Same labels, same tie order (the list is sorted).
    if (rs->twin && masked_batch_possible(idx, nq, k, rs->n_at_create)) {
        const int64_t n = rs->n_at_create;
        const bool half = half_path_ok(idx) && nq >= half_min_nq(idx, n);
        const int per = half ? std::max(1, half_max_queries(idx->d)) : std::max(1, mfma_gated_queries(idx));
        const bool have_shadow = __atomic_load_n(&idx->shadow.Xh.p, __ATOMIC_RELAXED) != nullptr;  // a heuristic read: ShadowStore::ensure writes it under shadow_mu
        const double shared = (double)((nq + per - 1) / per) * (half && have_shadow ? 0.6 : 1.0);
        const double gathered = (double)nq * (double)rs->count / (double)n * 1.1;
        if (shared < gathered)
            return search_core(idx, ws, q, nq, k, normalize_q, nullptr, n, label_offset, D_dev, I_dev, true, rs->twin);
    }
    MVDB_TRY(search_core(idx, ws, q, nq, k, normalize_q, rs->rows, rs->count, 0, D_dev, I_dev));
    hipLaunchKernelGGL(map_subset_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ws->stream, I_dev, total,
                       (const int64_t*)rs->rows, label_offset);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int mvdb_index_search_rowset(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                             const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(rowset_search_core(idx, call.ws, call.ws->q.p, nq, k, normalize_q, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_rowset_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    Workspace* ws = call.ws;
    return rowset_search_core(idx, ws, call.q, nq, k, normalize_q, rs, label_offset, D_dev, I_dev);
}

}  // extern "C"

// ---- range search: every selected row at or above a threshold (range_scan.hpp) ------------------------------------------
namespace {

template <int G, int C, int U, int METRIC, int SEL, bool MASKED>
int launch_range_kern(const RangeScanArgs& a, int nq, int device, hipStream_t stream) {
    void (*kern)(RangeScanArgs) = range_scan_kernel<G, C, U, METRIC, SEL, MASKED>;
    // the grid of the single-query scan (launch_scan_kern): 2 resident blocks per CU, 3 for the one- and three-chunk shapes
    const int nblocks = scan_grid(a.n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C), device);
    // (the gated launch of the shared pass runs under a label of its own: a profile tells the scans that were asked for from
    //  the launches that return at once)
    return profiled_launch(a.gate_count ? "ip_scan_range_fallback" : "ip_scan_range", stream,
                           [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, nq), dim3(kScanThreads), 0, stream, done, a); },
                           "range_scan_kernel<%d, %d, %d, %d, %d, %s>", G, C, U, METRIC, SEL, MASKED ? "true" : "false");
}

// the shapes and rows in flight of launch_scan: a score depends on (G, C, MASKED, METRIC) only, U follows the measured best
int launch_range(int metric, const RangeScanArgs& a, int nq, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);
            return metric == MVDB_METRIC_IP ? launch_range_kern<S::G, S::C, U, 0, F::SEL, F::MASKED>(a, nq, device, s)
                                            : launch_range_kern<S::G, S::C, U, 1, F::SEL, F::MASKED>(a, nq, device, s);
        });
    });
}

// the range join's bounded scan (join_scan.hpp): the same shapes, forms and grid, labels of its own
template <int G, int C, int U, int METRIC, int SEL, bool MASKED>
int launch_join_kern(const JoinScanArgs& a, int nq, int device, hipStream_t stream) {
    void (*kern)(JoinScanArgs) = join_scan_kernel<G, C, U, METRIC, SEL, MASKED>;
    const int nblocks = scan_grid(a.n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C), device);
    return profiled_launch(a.gate_count ? "ip_scan_join_fallback" : "ip_scan_join", stream,
                           [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, nq), dim3(kScanThreads), 0, stream, done, a); },
                           "join_scan_kernel<%d, %d, %d, %d, %d, %s>", G, C, U, METRIC, SEL, MASKED ? "true" : "false");
}

int launch_join(int metric, const JoinScanArgs& a, int nq, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);
            return metric == MVDB_METRIC_IP ? launch_join_kern<S::G, S::C, U, 0, F::SEL, F::MASKED>(a, nq, device, s)
                                            : launch_join_kern<S::G, S::C, U, 1, F::SEL, F::MASKED>(a, nq, device, s);
        });
    });
}

constexpr int kRangeTile = 1024;  // queries of one range launch (a call of more is answered that many at a time)

// ---- the shared pass of a range batch (inner product): nomination over the fp16 shadow, exact re-score, gated fallback ----------
// Reached through range_shared_route only, which holds the index to the shadow's widths with unpadded rows (half_path_ok:
// d = 128, 256, ..., 1024): rows of 32 x 1, 64 x 1, 32 x 3 and 64 x 2 / 3 / 4 chunks.  No other shape has a re-score kernel.
constexpr bool rescore_shape(int G, int C) { return G >= 32 && C <= 4; }

int launch_rescore(const RangeRescoreArgs& a, int nq, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        if constexpr (!rescore_shape(S::G, S::C)) {
            return unsupported_shape(a.d4);
        } else {
            constexpr int U = rescore_u(S::G, S::C);
            return with_scan_form<S::G, S::C>(a.d4, false, false, [&](auto form) {
                constexpr bool MASKED = decltype(form)::MASKED;
                void (*kern)(RangeRescoreArgs) = range_rescore_kernel<S::G, S::C, U, MASKED>;
                // blocks per query: enough for a full candidate segment at a few batches per wave, no more than the device holds at once
                constexpr int RB = (kWave / S::G) * U;
                const int64_t want = (a.ccap + (int64_t)RB * kScanWaves * 4 - 1) / ((int64_t)RB * kScanWaves * 4);
                const int64_t room = std::max<int64_t>(1, (int64_t)device_cus(device) * 8 / nq);
                const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(want, room));
                return profiled_launch("ip_scan_range_rescore", s, [&](hipEvent_t done) { launch_kernel(kern, dim3(gx, nq), dim3(kScanThreads), 0, s, done, a); },
                                       "range_rescore_kernel<%d, %d, %d, %s>", S::G, S::C, U, MASKED ? "true" : "false");
            });
        }
    });
}

// floors[i] = threshold_i - coef |q_i|, rounded down (a NaN or -inf floor admits every row: the query overflows or is decided
// by the exact re-score)
__global__ void range_floor_kernel(const float* __restrict__ thrs, float thr, const float* __restrict__ qnorm, float coef, int nq,
                                   float* __restrict__ floors) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float t = thrs ? thrs[i] : thr;
    floors[i] = nextafterf(t - coef * qnorm[i], -INFINITY);
}

// diagnostics of one launch group: queries whose candidates overflowed (added to the running count), candidates held
__global__ __launch_bounds__(256) void range_stats_kernel(const unsigned long long* __restrict__ ccount, unsigned long long ccap, int nq,
                                                          unsigned int* ctr, volatile unsigned long long* host) {
    __shared__ unsigned long long sh[2][4];
    unsigned long long nf = 0, nc = 0;
    for (int i = threadIdx.x; i < nq; i += 256) {
        const unsigned long long c = ccount[i];
        nf += c > ccap;
        nc += c > ccap ? 0ull : c;
    }
    for (int off = 32; off; off >>= 1) {
        nf += __shfl_xor(nf, off);
        nc += __shfl_xor(nc, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = nf;
        sh[1][threadIdx.x >> 6] = nc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        nf = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        nc = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        const unsigned int total = atomicAdd(ctr, (unsigned int)nf) + (unsigned int)nf;
        host[0] = total;
        host[1] = nc;
    }
}

// the route's own zeroing and query copy: kernels, so that a captured call holds kernel nodes only
__global__ void range_zero_kernel(unsigned long long* __restrict__ a, unsigned long long* __restrict__ b, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        a[i] = 0ull;
        b[i] = 0ull;
    }
}
__global__ void range_copy_kernel(const float* __restrict__ src, int64_t n, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

__global__ void negate_kernel(const float* __restrict__ src, int n, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = -src[i];
}

// Fewest queries of a range call that take the shared pass (option range_shared = 1).  The certified top-k pass, whose cost
// structure this pass shares — one stream of the shadow per 128 / 256 queries against one stream of the fp32 rows per query —
// starts at 2 queries from 500k rows and at 8 from 100k (half_min_nq); those crossovers were measured for ANOTHER kernel, and
// the batch cells of benchmarks/bench_range.py have not been timed yet.  Until they are, the rule keeps to the batches where
// arithmetic alone decides: 33+ queries replace 33+ fp32 passes by one pass over half the bytes.
int range_shared_min_nq(int64_t n) {
    (void)n;
    return 33;
}

// the counters of the route: allocated with the first call that takes it, never inside a capture
bool ensure_range_stats(const mvdb_index* idx, MirroredCounter& ctr, hipStream_t s) {
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    return ctr.dev() || (!stream_capturing(s) && ctr.ensure(1));
}

// Does this launch group go through the shared pass?  Inner product, a batch, every row or a bitmap-form set, an index that
// meets the certified pass's shadow conditions (half_path_ok: a width with a shadow kernel, unpadded rows, rows of known finite
// norm), and a shadow that exists or may be built now (never while the stream is capturing).
// (mode, ctr: option range_shared and the range calls' counter, or the range join's pair)
const _Float16* range_shared_route(const mvdb_index* idx, Workspace* ws, int nq, const mvdb_rowset* rs, int64_t n, int mode,
                                   MirroredCounter& ctr) {
    if (mode == 0 || nq < 2 || n <= 0 || idx->metric != MVDB_METRIC_IP || (rs && !rs->mask) || !half_path_ok(idx)) return nullptr;
    if (mode == 1 && nq < range_shared_min_nq(n)) return nullptr;
    {   // the band (half_range_eps) bounds the scan's sum by its depth, 4 C + log2 G <= 4 ceil(d / 128) + 6: hold the shape to it
        const Shape sh = choose_shape(idx->d4);
        int lg = 0;
        while ((1 << lg) < sh.G) ++lg;
        if (4 * sh.C + lg > (idx->d + 127) / 128 * 4 + 6) return nullptr;
    }
    const _Float16* Xh = idx->shadow.ensure(idx, ws->stream, half_xscale(idx->row_norm_bound));
    if (!Xh || !ensure_range_stats(idx, ctr, ws->stream)) return nullptr;
    return Xh;
}

// The three stages on the call's stream, no host synchronisation: (a) per 128 / 256 queries one nomination launch over the
// shadow against the floors threshold_i - band_i; (b) the exact re-score of the candidates appends the passing keys; (c) the
// thresholded scan, enabled per query on the device, answers the queries whose candidates overflowed.  `a`: the arguments the
// per-query route would launch with.
// bounds_host (the range join; bounds_dev: the same on the device): query i admits rows below bounds_host[i] only — the nomination launch
// of a chunk covers the tiles below the chunk's largest bound (none: no launch), the gated fallback is the bounded scan, and
// the diagnostics go to the join's own counter.
int range_shared_phase(const mvdb_index* idx, Workspace* ws, const _Float16* Xh, RangeScanArgs a, int nq,
                       const int64_t* bounds_host = nullptr, const int64_t* bounds_dev = nullptr) {
    hipStream_t s = ws->stream;
    const int chunk = half_max_queries(idx->d);
    int64_t ccap = idx->kn.range_candidates > 0 ? idx->kn.range_candidates : std::max<int64_t>(pow2ceil(std::max<int64_t>(2 * a.cap, 2)), 4096);
    ccap = std::max<int64_t>(64, std::min<int64_t>(ccap, 1ll << 20));
    ccap = std::min<int64_t>(ccap, (256ll << 20) / 4 / nq);  // the candidate workspace stays at or below 256 MiB (nq <= 1024: >= 65536)
    MVDB_TRY(ws->rcand.reserve((size_t)nq * (size_t)ccap));
    MVDB_TRY(ws->rccount.reserve((size_t)nq));
    MVDB_TRY(ws->qsplit.reserve((size_t)std::max(2 * 128, chunk) * idx->d));
    MVDB_TRY(ws->qnorm.reserve((size_t)std::max(256, 3 * chunk)));
    hipLaunchKernelGGL(range_zero_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, a.counts, ws->rccount.p, nq);
    MVDB_HIP(hipGetLastError());
    // the nomination reads the queries as the certified pass does: normalised by the row normaliser where the call asks for
    // it.  The re-score normalises inside its prologue (the scan's own arithmetic).  Both sum the squares per lane and over a
    // butterfly — depth 4 C + log2 G <= 38 at the shadow widths — and multiply by 1 / sqrt: each image is within
    // ((depth + 1) / 2 + 3) 2^-24 of the real-number one, the two within (depth + 7) 2^-24 of each other, element by element.
    // The band carries (d + 8) 2^-24, which would cover sums of squares taken in ANY order
    // (tests/test_range_batch_cpu.py: test_allowance_for_the_two_normalised_query_images).
    const float* qsrc = a.q;
    double extra = 0.0;
    if (a.normalize_q) {
        MVDB_TRY(ws->qn.reserve((size_t)nq * idx->ld));
        const int64_t total = (int64_t)nq * idx->ld;
        hipLaunchKernelGGL(range_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.q, total, ws->qn.p);
        MVDB_HIP(hipGetLastError());
        MVDB_TRY(normalize_range(idx, ws->qn.p, nq, s));
        qsrc = ws->qn.p;
        extra = (idx->d + 8.0) * std::ldexp(1.0, -24);
    }
    const float coef = (float)((half_range_eps(idx->d) + extra) * (double)idx->row_norm_bound * (1.0 + 1e-6));
    const float xscale = half_xscale(idx->row_norm_bound);
    _Float16* qf = reinterpret_cast<_Float16*>(ws->qsplit.p);
    for (int c0 = 0; c0 < nq; c0 += chunk) {
        const int take = std::min(chunk, nq - c0);
        int64_t rows_below = a.n;
        if (bounds_host) rows_below = std::min(a.n, *std::max_element(bounds_host + c0, bounds_host + c0 + take));
        if (rows_below <= 0) continue;
        const int nqpad = half_chunk_queries(idx->d, take);
        float* qnorm = ws->qnorm.p;
        float* floors = qnorm + nqpad;
        float* qinv = qnorm + 2 * nqpad;
        MVDB_TRY(launch_half_queries(qsrc + (int64_t)c0 * idx->ld, idx->ld, idx->d, take, nqpad, xscale, qf, qnorm, qinv, s));
        hipLaunchKernelGGL(range_floor_kernel, dim3((take + 255) / 256), dim3(256), 0, s, a.thrs ? a.thrs + c0 : nullptr, a.thr, qnorm,
                           coef, take, floors);
        MVDB_HIP(hipGetLastError());
        HalfRangeArgs h;
        h.Xh = Xh;
        h.qf = qf;
        h.qinv = qinv;
        h.floors = floors;
        h.nq = take;
        h.n = rows_below;
        h.before = bounds_host ? bounds_dev + c0 : nullptr;
        h.mask = reinterpret_cast<const uint32_t*>(a.mask);
        h.cand = ws->rcand.p + (size_t)c0 * (size_t)ccap;
        h.ccap = ccap;
        h.ccount = ws->rccount.p + c0;
        MVDB_TRY(launch_half_range(idx->d, nqpad, h, idx->device, s));
    }
    RangeRescoreArgs r;
    r.X = a.X;
    r.ld = a.ld;
    r.d4 = a.d4;
    r.q = a.q;
    r.normalize_q = a.normalize_q;
    r.thr = a.thr;
    r.thrs = a.thrs;
    r.cand = ws->rcand.p;
    r.ccap = ccap;
    r.ccount = ws->rccount.p;
    r.keys = a.keys;
    r.seg = a.seg;
    r.cap = a.cap;
    r.counts = a.counts;
    MVDB_TRY(launch_rescore(r, nq, idx->device, s));
    MirroredCounter& ctr = bounds_host ? idx->jn_ctr : idx->rg_ctr;
    hipLaunchKernelGGL(range_stats_kernel, dim3(1), dim3(256), 0, s, ws->rccount.p, (unsigned long long)ccap, nq, ctr.dev(),
                       ctr.mirror<unsigned long long>());
    MVDB_HIP(hipGetLastError());
    a.gate_count = ws->rccount.p;
    a.gate_cap = (unsigned long long)ccap;
    if (!bounds_host) return launch_range(idx->metric, a, nq, idx->device, s);
    JoinScanArgs j;
    static_cast<RangeScanArgs&>(j) = a;
    j.before = bounds_dev;
    return launch_join(idx->metric, j, nq, idx->device, s);
}

int check_range_args(const mvdb_index* idx, const void* q, int nq, float threshold, int64_t cap, const void* counts, const void* D,
                     const void* I) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !counts) return fail(MVDB_ERR_ARG, "NULL buffer passed to range search");
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (threshold != threshold) return fail(MVDB_ERR_ARG, "the threshold is NaN");
    if (cap < 0) return fail(MVDB_ERR_ARG, "cap must not be negative (got %lld)", (long long)cap);
    if (cap > 0 && (!D || !I)) return fail(MVDB_ERR_ARG, "D / I may be NULL only with cap == 0");
    return 0;
}

// zero the counters and run the thresholded scan: counts[i] = passing rows of query i, keys[i * seg ...] the first `cap` of
// them in no defined order.  *rows_out: the row list the keys' positions refer to (NULL: they are row numbers).
// thrs: NULL, or the queries' own thresholds on the device in the units of the keys (L2: negated).  *shared: the launch group
// took the shared pass.
int range_scan_phase(const mvdb_index* idx, Workspace* ws, const float* q, int nq, float threshold, const float* thrs, int normalize_q,
                     const mvdb_rowset* rs, int64_t cap, int64_t seg, unsigned long long* counts, const int64_t** rows_out, bool* shared) {
    KnobScope knobs(&idx->kn);
    hipStream_t s = ws->stream;
    MVDB_TRY(ws->rkeys.reserve((size_t)nq * (size_t)seg));
    RangeScanArgs a;
    a.X = idx->X.p;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.q = q;
    a.normalize_q = normalize_q;
    a.thr = idx->metric == MVDB_METRIC_IP ? threshold : -threshold;  // the key's score of an L2 row is -distance
    a.thrs = thrs;
    a.rows = nullptr;
    a.mask = nullptr;
    a.n = idx->n;
    if (rs) {
        if (rs->mask) {
            a.mask = rs->mask;
            a.n = rs->count == 0 ? 0 : std::min<int64_t>(rs->n_at_create, idx->n);  // rows appended since are not part of the set
        } else {
            a.rows = rs->rows;
            a.n = rs->count;
        }
    }
    a.keys = ws->rkeys.p;
    a.seg = seg;
    a.cap = cap;
    a.counts = counts;
    *rows_out = a.rows;
    if (a.n > 0) {
        if (const _Float16* Xh = range_shared_route(idx, ws, nq, rs, a.n, idx->kn.range_shared, idx->rg_ctr)) {
            *shared = true;
            return range_shared_phase(idx, ws, Xh, a, nq);   // (zeroes the counters itself)
        }
    }
    MVDB_HIP(hipMemsetAsync(counts, 0, (size_t)nq * sizeof(unsigned long long), s));
    if (a.n == 0) return 0;
    return launch_range(idx->metric, a, nq, idx->device, s);
}

// sort the leading keys of every segment (descending) — P: a power of two >= every count that is to be sorted
int range_sort_phase(Workspace* ws, int nq, int64_t seg, int64_t cap, int64_t P, const unsigned long long* counts) {
    hipStream_t s = ws->stream;
    const int L = (int)std::min<int64_t>(P, kRangeSortTile);
    const dim3 tiles((unsigned)(P / L), (unsigned)nq);
    hipLaunchKernelGGL(range_sort_lds_kernel, tiles, dim3(kRangeSortThreads), 0, s, ws->rkeys.p, seg, counts, cap, L, (int64_t)2, (int64_t)L);
    for (int64_t size = 2 * (int64_t)L; size <= P; size <<= 1) {
        for (int64_t stride = size >> 1; stride >= L; stride >>= 1)
            hipLaunchKernelGGL(range_sort_step_kernel, dim3((unsigned)((P / 2 + 255) / 256), (unsigned)nq), dim3(256), 0, s, ws->rkeys.p, seg,
                               counts, cap, size, stride);
        hipLaunchKernelGGL(range_sort_lds_kernel, tiles, dim3(kRangeSortThreads), 0, s, ws->rkeys.p, seg, counts, cap, L, size, size);
    }
    MVDB_HIP(hipGetLastError());
    return 0;
}

int range_emit_phase(const mvdb_index* idx, Workspace* ws, int nq, int64_t seg, int64_t cap, int64_t width,
                     const unsigned long long* counts, const int64_t* rows, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)nq), dim3(256), 0, ws->stream, ws->rkeys.p, seg,
                       counts, cap, width, idx->metric, rows, label_offset, D_dev, I_dev);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// host entry points, behind the scan phase of one tile (counters in ws->rcounts, keys in ws->rkeys): counts, sort, emit, fill
int range_host_finish(const mvdb_index* idx, HostCall& call, int nq, int64_t cap, int64_t seg, const int64_t* rows, int64_t* counts_host,
                      float* D_host, int64_t* I_host) {
    Workspace* ws = call.ws;
    // the counts come back first: the sort and the copy are sized by what is there, not by the capacity
    MVDB_TRY(copy_back(ws, ws->rcounts.p, (size_t)nq * sizeof(unsigned long long), "range search"));
    int64_t width = 0;
    for (int i = 0; i < nq; ++i) {
        counts_host[i] = (int64_t)((const unsigned long long*)ws->pin_out.p)[i];
        if (counts_host[i] <= cap) width = std::max(width, counts_host[i]);
    }
    if (cap == 0) return 0;
    const size_t total = (size_t)nq * (size_t)width;
    if (width > 0) {
        float* D_dev = nullptr;
        int64_t* I_dev = nullptr;
        MVDB_TRY(call.results(total, &D_dev, &I_dev));
        MVDB_TRY(range_sort_phase(ws, nq, seg, cap, pow2ceil(std::max<int64_t>(width, 2)), ws->rcounts.p));
        MVDB_TRY(range_emit_phase(idx, ws, nq, seg, cap, width, ws->rcounts.p, rows, 0, D_dev, I_dev));
        MVDB_TRY(copy_back(ws, ws->out.p, total * (sizeof(int64_t) + sizeof(float)), "range search"));
    }
    const int64_t* I_st = (const int64_t*)ws->pin_out.p;
    const float* D_st = (const float*)((const char*)ws->pin_out.p + total * sizeof(int64_t));
    const float missing = idx->metric == MVDB_METRIC_IP ? -3.402823466e+38f : 3.402823466e+38f;
    for (int i = 0; i < nq; ++i) {
        const int64_t have = counts_host[i] <= cap ? counts_host[i] : 0;  // an overflowed query: missing markers only
        float* Dr = D_host + (size_t)i * cap;
        int64_t* Ir = I_host + (size_t)i * cap;
        if (have) {
            memcpy(Ir, I_st + (size_t)i * width, (size_t)have * sizeof(int64_t));
            memcpy(Dr, D_st + (size_t)i * width, (size_t)have * sizeof(float));
        }
        std::fill(Dr + have, Dr + cap, missing);
        std::fill(Ir + have, Ir + cap, (int64_t)-1);
    }
    return 0;
}

// host entry point, one tile of queries already staged in ws->q
int range_host_tile(const mvdb_index* idx, HostCall& call, int nq, float threshold, const float* thrs, int normalize_q, const mvdb_rowset* rs,
                    int64_t cap, int64_t* counts_host, float* D_host, int64_t* I_host, bool* shared) {
    Workspace* ws = call.ws;
    const int64_t seg = cap > 0 ? pow2ceil(std::max<int64_t>(cap, 2)) : 0;
    MVDB_TRY(ws->rcounts.reserve((size_t)nq));
    const int64_t* rows = nullptr;
    MVDB_TRY(range_scan_phase(idx, ws, ws->q.p, nq, threshold, thrs, normalize_q, rs, cap, seg, ws->rcounts.p, &rows, shared));
    return range_host_finish(idx, call, nq, cap, seg, rows, counts_host, D_host, I_host);
}

// ---- range join (join_scan.hpp): the queries are stored rows, each matched against the rows before it -----------------------
// The scan phase of one launch group of query rows: their numbers = their bounds go to the device (8 bytes per query — the rows
// themselves never leave it), the queries are read from the matrix in place where the group is a run of consecutive rows and
// gathered into the workspace otherwise.
int join_scan_phase(const mvdb_index* idx, Workspace* ws, const int64_t* qrows_host, int nq, float threshold, const mvdb_rowset* rs,
                    int64_t cap, int64_t seg, unsigned long long* counts, const int64_t** rows_out, bool* shared) {
    KnobScope knobs(&idx->kn);
    hipStream_t s = ws->stream;
    MVDB_TRY(ws->rkeys.reserve((size_t)nq * (size_t)seg));
    MVDB_TRY(ws->jrows.reserve((size_t)nq));
    // (pageable memory: the copy has left the host buffer when the call returns)
    if (hipMemcpyAsync(ws->jrows.p, qrows_host, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(MVDB_ERR_HIP, "range join: the row numbers' upload failed");
    bool consecutive = true;
    int64_t max_bound = qrows_host[0];
    for (int i = 1; i < nq; ++i) {
        consecutive = consecutive && qrows_host[i] == qrows_host[0] + i;
        max_bound = std::max(max_bound, qrows_host[i]);
    }
    const float* q = idx->X.p + qrows_host[0] * idx->ld;
    if (!consecutive) {
        MVDB_TRY(ws->q.reserve((size_t)nq * idx->ld));
        const int64_t units = (int64_t)nq * (idx->ld / 4);
        hipLaunchKernelGGL(join_gather_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, ws->q.p, idx->X.p, ws->jrows.p,
                           (int64_t)nq, idx->ld);
        MVDB_HIP(hipGetLastError());
        q = ws->q.p;
    }
    JoinScanArgs a;
    a.X = idx->X.p;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.q = q;
    a.normalize_q = 0;
    a.thr = idx->metric == MVDB_METRIC_IP ? threshold : -threshold;  // the key's score of an L2 row is -distance
    a.rows = nullptr;
    a.mask = nullptr;
    a.n = idx->n;
    if (rs) {
        if (rs->mask) {
            a.mask = rs->mask;
            a.n = rs->count == 0 ? 0 : std::min<int64_t>(rs->n_at_create, idx->n);  // rows appended since are not part of the set
        } else {
            a.rows = rs->rows;
            a.n = rs->count;
        }
    }
    if (!a.rows) a.n = std::min(a.n, max_bound);  // streamed forms: no query of the group looks at or beyond its largest bound
    a.keys = ws->rkeys.p;
    a.seg = seg;
    a.cap = cap;
    a.counts = counts;
    a.before = ws->jrows.p;
    *rows_out = a.rows;
    if (a.n > 0 && max_bound > 0) {
        if (const _Float16* Xh = range_shared_route(idx, ws, nq, rs, a.n, idx->kn.join_shared, idx->jn_ctr)) {
            *shared = true;
            return range_shared_phase(idx, ws, Xh, a, nq, qrows_host, a.before);   // (zeroes the counters itself)
        }
    }
    MVDB_HIP(hipMemsetAsync(counts, 0, (size_t)nq * sizeof(unsigned long long), s));
    if (a.n <= 0 || max_bound <= 0) return 0;
    return launch_join(idx->metric, a, nq, idx->device, s);
}

}  // namespace

extern "C" {

// thresholds_host: NULL (every query under `threshold`), or one per query
static int range_search_host(const mvdb_index* idx, const float* q_host, int nq, float threshold, const float* thresholds_host,
                             int normalize_q, const mvdb_rowset* rs, int64_t cap, int64_t* counts_host, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_range_args(idx, q_host, nq, threshold, cap, counts_host, D_host, I_host));
    if (thresholds_host)
        for (int i = 0; i < nq; ++i)
            if (thresholds_host[i] != thresholds_host[i]) return fail(MVDB_ERR_ARG, "threshold %d is NaN", i);
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* ws = call.ws;
    bool shared = false;
    std::vector<float> tkeys;  // the thresholds in the units of the keys
    auto tile = [&](int t0) -> int {
        const int take = std::min(kRangeTile, nq - t0);
        MVDB_TRY(call.stage(q_host + (size_t)t0 * idx->d, take));
        const float* thrs = nullptr;
        if (thresholds_host) {
            tkeys.assign(thresholds_host + t0, thresholds_host + t0 + take);
            if (idx->metric != MVDB_METRIC_IP)
                for (float& v : tkeys) v = -v;
            MVDB_TRY(ws->rthr.reserve((size_t)take));
            // (pageable memory: the copy has left the host buffer when the call returns)
            if (hipMemcpyAsync(ws->rthr.p, tkeys.data(), (size_t)take * sizeof(float), hipMemcpyHostToDevice, ws->stream) != hipSuccess)
                return fail(MVDB_ERR_HIP, "range search: the thresholds' upload failed");
            thrs = ws->rthr.p;
        }
        return range_host_tile(idx, call, take, threshold, thrs, normalize_q, rs, cap, counts_host + t0, cap ? D_host + (size_t)t0 * cap : nullptr,
                               cap ? I_host + (size_t)t0 * cap : nullptr, &shared);
    };
    int rc = 0;
    for (int t0 = 0; t0 < nq && !rc; t0 += kRangeTile) rc = tile(t0);
    if (shared) idx->rg_shared_calls.fetch_add(1);  // (a call that failed behind the shared pass counts too)
    return rc;
}

static int range_search_dev(const mvdb_index* idx, const float* q_dev, int nq, float threshold, const float* thresholds_dev,
                            int normalize_q, const mvdb_rowset* rs, int64_t cap, int64_t label_offset, int64_t* counts_dev, float* D_dev,
                            int64_t* I_dev, void* stream) {
    MVDB_TRY(check_range_args(idx, q_dev, nq, threshold, cap, counts_dev, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    Workspace* ws = call.ws;
    const float* q = call.q;
    const float* thrs = thresholds_dev;
    if (thrs && idx->metric != MVDB_METRIC_IP) {  // the key's score of an L2 row is -distance
        MVDB_TRY(ws->rthr.reserve((size_t)nq));
        hipLaunchKernelGGL(negate_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ws->stream, thresholds_dev, nq, ws->rthr.p);
        MVDB_HIP(hipGetLastError());
        thrs = ws->rthr.p;
    }
    // Nothing below reads from the device: the sort is sized by the capacity (each block looks its query's count up and
    // sorts no more than that), so the call may be captured once an eager call of the same shape has sized the workspace.
    const int64_t seg = cap > 0 ? pow2ceil(std::max<int64_t>(cap, 2)) : 0;
    bool shared = false;
    for (int t0 = 0; t0 < nq; t0 += kRangeTile) {
        const int take = std::min(kRangeTile, nq - t0);
        unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_dev) + t0;
        const int64_t* rows = nullptr;
        MVDB_TRY(range_scan_phase(idx, ws, q + (size_t)t0 * idx->ld, take, threshold, thrs ? thrs + t0 : nullptr, normalize_q, rs, cap, seg,
                                  counts, &rows, &shared));
        if (cap == 0) continue;
        MVDB_TRY(range_sort_phase(ws, take, seg, cap, seg, counts));
        MVDB_TRY(range_emit_phase(idx, ws, take, seg, cap, cap, counts, rows, label_offset, D_dev + (size_t)t0 * cap, I_dev + (size_t)t0 * cap));
    }
    if (shared) idx->rg_shared_calls.fetch_add(1);
    return 0;
}

int mvdb_index_range_join(const mvdb_index* idx, const int64_t* qrows_host, int nq, float threshold, const mvdb_rowset* rs, int64_t cap,
                          int64_t* counts_host, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_range_args(idx, qrows_host, nq, threshold, cap, counts_host, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const RowRange rr = row_range(qrows_host, nq);
    if (rr.lo < 0 || rr.hi >= idx->n)
        return fail(MVDB_ERR_ARG, "query row %lld out of range [0,%lld)", (long long)(rr.lo < 0 ? rr.lo : rr.hi), (long long)idx->n);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* ws = call.ws;
    const int64_t seg = cap > 0 ? pow2ceil(std::max<int64_t>(cap, 2)) : 0;
    bool shared = false;
    int rc = 0;
    for (int t0 = 0; t0 < nq && !rc; t0 += kRangeTile) {
        const int take = std::min(kRangeTile, nq - t0);
        const int64_t* rows = nullptr;
        rc = ws->rcounts.reserve((size_t)take);
        if (!rc) rc = join_scan_phase(idx, ws, qrows_host + t0, take, threshold, rs, cap, seg, ws->rcounts.p, &rows, &shared);
        if (!rc)
            rc = range_host_finish(idx, call, take, cap, seg, rows, counts_host + t0, cap ? D_host + (size_t)t0 * cap : nullptr,
                                   cap ? I_host + (size_t)t0 * cap : nullptr);
    }
    if (shared) idx->jn_shared_calls.fetch_add(1);  // (a call that failed behind the shared pass counts too)
    return rc;
}

int mvdb_index_range_search(const mvdb_index* idx, const float* q_host, int nq, float threshold, int normalize_q,
                            const mvdb_rowset* rs, int64_t cap, int64_t* counts_host, float* D_host, int64_t* I_host) {
    return range_search_host(idx, q_host, nq, threshold, nullptr, normalize_q, rs, cap, counts_host, D_host, I_host);
}

int mvdb_index_range_search_each(const mvdb_index* idx, const float* q_host, int nq, const float* thresholds_host, int normalize_q,
                                 const mvdb_rowset* rs, int64_t cap, int64_t* counts_host, float* D_host, int64_t* I_host) {
    if (!thresholds_host) return fail(MVDB_ERR_ARG, "NULL buffer passed to range search");
    return range_search_host(idx, q_host, nq, 0.f, thresholds_host, normalize_q, rs, cap, counts_host, D_host, I_host);
}

int mvdb_index_range_search_device(const mvdb_index* idx, const float* q_dev, int nq, float threshold, int normalize_q,
                                   const mvdb_rowset* rs, int64_t cap, int64_t label_offset, int64_t* counts_dev, float* D_dev,
                                   int64_t* I_dev, void* stream) {
    return range_search_dev(idx, q_dev, nq, threshold, nullptr, normalize_q, rs, cap, label_offset, counts_dev, D_dev, I_dev, stream);
}

int mvdb_index_range_search_each_device(const mvdb_index* idx, const float* q_dev, int nq, const float* thresholds_dev, int normalize_q,
                                        const mvdb_rowset* rs, int64_t cap, int64_t label_offset, int64_t* counts_dev, float* D_dev,
                                        int64_t* I_dev, void* stream) {
    if (!thresholds_dev) return fail(MVDB_ERR_ARG, "NULL buffer passed to range search");
    return range_search_dev(idx, q_dev, nq, 0.f, thresholds_dev, normalize_q, rs, cap, label_offset, counts_dev, D_dev, I_dev, stream);
}

}  // extern "C"

// ---- MMR search: k diverse rows picked on the device from the top fetch_k (mmr_select.hpp) --------------------------------
namespace {

// LDS one workgroup may ask for on `device` (remembered)
size_t device_lds_per_block(int device) {
    static std::mutex mu;
    static std::map<int, size_t> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(device);
    if (it != cache.end()) return it->second;
    int bytes = 0;
    if (hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || bytes <= 0) bytes = 64 << 10;
    return cache[device] = (size_t)bytes;
}

// THE rule of the two forms, from the row stride, fetch_k and the device's LDS alone: 0 where the candidates' rows and the
// per-candidate arrays fit the budget — seven eighths of the LDS a workgroup may have (140 of 160 KiB: 64 rows of 512 floats
// fit, 1024 rows of 32 do not; the selection then has the CU to itself) —, else 1; -1 where not even one row fits beside
// the arrays.
int mmr_form_rule(int64_t ld, int fetch_k, size_t lds_per_block) {
    const size_t budget = lds_per_block - lds_per_block / 8;
    if (mmr_lds_bytes(0, fetch_k, ld) + kMmrStaticLds <= budget) return 0;
    if (mmr_lds_bytes(1, fetch_k, ld) + kMmrStaticLds <= lds_per_block) return 1;
    return -1;
}

int check_mmr_args(const mvdb_index* idx, const void* q, int nq, int k, int fetch_k, float lambda, const void* D, const void* I) {
    MVDB_TRY(check_search_args(idx, q, nq, k, D, I));
    if (fetch_k < k || fetch_k > kMmrMaxFetch)
        return fail(MVDB_ERR_ARG, "MMR search needs k <= fetch_k <= %d (got k = %d, fetch_k = %d)", kMmrMaxFetch, k, fetch_k);
    if (!(lambda >= 0.f && lambda <= 1.f)) return fail(MVDB_ERR_ARG, "lambda must lie in [0, 1] (got %g)", (double)lambda);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "MMR search needs an inner-product index");
    return 0;
}

// Queries on the device at stride ld, results to device buffers: per tile of kCoreTile queries the candidate search
// (search_core / rowset_search_core with label_offset 0, into the workspace) and one launch of the selection behind it.
int mmr_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int fetch_k, float lambda, int normalize_q,
             const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    const int form = mmr_form_rule(idx->ld, fetch_k, device_lds_per_block(idx->device));
    if (form < 0) return fail(MVDB_ERR_ARG, "MMR search: a row of %d floats does not fit the device's LDS", idx->d);
    const size_t lds = mmr_lds_bytes(form, fetch_k, idx->ld);
    void (*kern)(MmrArgs) = form == 0 ? mmr_select_kernel<0> : mmr_select_kernel<1>;
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, idx->device));
    const size_t tile = (size_t)std::min(nq, kCoreTile);
    MVDB_TRY(ws->mmrD.reserve(tile * fetch_k));
    MVDB_TRY(ws->mmrI.reserve(tile * fetch_k));
    MmrArgs a;
    a.X = idx->X.p;
    a.ld = idx->ld;
    a.candD = ws->mmrD.p;
    a.candI = ws->mmrI.p;
    a.fetch_k = fetch_k;
    a.k = k;
    a.lambda = lambda;
    a.mu = 1.f - lambda;
    a.label_offset = label_offset;
    for (int t0 = 0; t0 < nq; t0 += kCoreTile) {
        const int take = std::min(kCoreTile, nq - t0);
        const float* qt = q + (int64_t)t0 * idx->ld;
        if (rs) MVDB_TRY(rowset_search_core(idx, ws, qt, take, fetch_k, normalize_q, rs, 0, ws->mmrD.p, ws->mmrI.p));
        else MVDB_TRY(search_core(idx, ws, qt, take, fetch_k, normalize_q, nullptr, 0, 0, ws->mmrD.p, ws->mmrI.p));
        a.D = D_dev + (int64_t)t0 * k;
        a.I = I_dev + (int64_t)t0 * k;
        MVDB_TRY(profiled_launch("mmr_select", ws->stream,
                                 [&](hipEvent_t done) { launch_kernel(kern, dim3((unsigned)take), dim3(kMmrThreads), lds, ws->stream, done, a); },
                                 "mmr_select_kernel<%d>", form));
    }
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_search_mmr(const mvdb_index* idx, const float* q_host, int nq, int k, int fetch_k, float lambda, int normalize_q,
                          const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_mmr_args(idx, q_host, nq, k, fetch_k, lambda, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(mmr_core(idx, call.ws, call.ws->q.p, nq, k, fetch_k, lambda, normalize_q, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_mmr_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int fetch_k, float lambda,
                                 int normalize_q, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                 void* stream) {
    MVDB_TRY(check_mmr_args(idx, q_dev, nq, k, fetch_k, lambda, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises: capturable once an eager call of the same shape has sized the workspace
    return mmr_core(idx, call.ws, call.q, nq, k, fetch_k, lambda, normalize_q, rs, label_offset, D_dev, I_dev);
}

int mvdb_mmr_form(int d, int fetch_k, int device) {
    if (d <= 0) return -fail(MVDB_ERR_ARG, "d must be positive (got %d)", d);
    if (fetch_k < 1 || fetch_k > kMmrMaxFetch) return -fail(MVDB_ERR_ARG, "fetch_k must lie in [1, %d] (got %d)", kMmrMaxFetch, fetch_k);
    if (const int rc = ensure_device(device)) return -rc;
    const int form = mmr_form_rule(((int64_t)d + 3) / 4 * 4, fetch_k, device_lds_per_block(device));
    if (form < 0) return -fail(MVDB_ERR_ARG, "MMR search: a row of %d floats does not fit the device's LDS", d);
    return form;
}

}  // extern "C"

// ---- distinct search: the best row of each group, the k best groups (distinct_select.hpp) ---------------------------------
struct mvdb_grouping {
    uint64_t owner = 0;       // serial number of the index the grouping was built on
    int device = 0;
    int64_t n = 0;            // the index's row count it was built against: one code per row
    uint64_t renumbered = 0;  // ... and its renumbering generation
    int64_t n_groups = 0;
    int32_t* codes = nullptr; // [n] on the device (none for an empty index)
};

namespace {

int grouping_check(const mvdb_index* idx, const mvdb_grouping* g) {
    if (!g) return fail(MVDB_ERR_ARG, "grouping is NULL");
    if (g->owner != idx->serial) return fail(MVDB_ERR_ARG, "the grouping belongs to another index");
    // one code per stored row: rows added since have none, rows removed since have renumbered the rest
    if (g->device != idx->device || g->n != idx->n || g->renumbered != idx->renumbered)
        return fail(MVDB_ERR_ARG, "the grouping was built for another state of the index (%lld rows then, %lld now)", (long long)g->n,
                    (long long)idx->n);
    return 0;
}

int check_distinct_args(const mvdb_index* idx, const void* q, int nq, int k, int fetch_k, const void* D, const void* I) {
    MVDB_TRY(check_search_args(idx, q, nq, k, D, I));
    if (k > kMaxFusedK) return fail(MVDB_ERR_ARG, "distinct search needs k <= %d (got %d)", kMaxFusedK, k);
    if (fetch_k < k || fetch_k > kDistinctMaxFetch)
        return fail(MVDB_ERR_ARG, "distinct search needs k <= fetch_k <= %d (got k = %d, fetch_k = %d)", kDistinctMaxFetch, k, fetch_k);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "distinct search needs an inner-product index");
    return 0;
}

__global__ void distinct_fill_missing_kernel(float* D, int64_t* I, int32_t* G, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        D[i] = -3.402823466e+38f;
        I[i] = -1;
        if (G) G[i] = -1;
    }
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_group_best_kern(const GroupBestArgs& a, int slots, int device, hipStream_t stream) {
    void (*kern)(GroupBestArgs) = group_best_scan_kernel<G, C, U, SEL, MASKED>;
    // the grid of the single-query scan (launch_scan_kern)
    const int nblocks = scan_grid(a.n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C), device);
    return profiled_launch("distinct_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, slots), dim3(kScanThreads), 0, stream, done, a); },
                           "group_best_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// the shapes and rows in flight of launch_scan: a score depends on (G, C, MASKED) only
int launch_group_best(const GroupBestArgs& a, int slots, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);
            return launch_group_best_kern<S::G, S::C, U, F::SEL, F::MASKED>(a, slots, device, s);
        });
    });
}

// the counter of tier 2: allocated with the first call, never inside a capture
bool ensure_distinct_stats(const mvdb_index* idx, hipStream_t s) {
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    return idx->ds_ctr.dev() || (!stream_capturing(s) && idx->ds_ctr.ensure(1));
}

// Queries on the device at stride ld, results to device buffers.  Per tile of kCoreTile queries: the candidate search
// (search_core / rowset_search_core with label_offset 0, into the workspace), the collapse launch behind it, and — unless
// the candidates cover the selection, which the host knows — per sub-tile of T slots the three gated launches of tier 2.
int distinct_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int fetch_k, int normalize_q,
                  const mvdb_grouping* grp, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev, int32_t* G_dev) {
    hipStream_t s = ws->stream;
    ++idx->ds_calls;
    const int64_t m = rs ? rs->count : idx->n;  // rows selected
    if (m == 0 || (rs && rs->mask && rs->n_at_create == 0)) {
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(distinct_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D_dev, I_dev, G_dev, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    const bool covers = fetch_k >= m;
    const size_t tile = (size_t)std::min(nq, kCoreTile);
    MVDB_TRY(ws->mmrD.reserve(tile * fetch_k));
    MVDB_TRY(ws->mmrI.reserve(tile * fetch_k));
    if (!ws->dneed.p) {  // (a fixed size: the ticket behind the need words is zeroed once and left zero by every launch)
        MVDB_TRY(ws->dneed.reserve((size_t)kCoreTile + 1));
        MVDB_HIP(hipMemsetAsync(ws->dneed.p, 0, ((size_t)kCoreTile + 1) * sizeof(int), s));
    }
    const bool counted = ensure_distinct_stats(idx, s);
    const int64_t ng = grp->n_groups;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)tile, idx->kn.distinct_table_bytes / (8 * ng)));
    if (!covers) MVDB_TRY(ws->dtab.reserve((size_t)T * (size_t)ng));

    DistinctCollapseArgs c;
    c.candD = ws->mmrD.p;
    c.candI = ws->mmrI.p;
    c.codes = grp->codes;
    c.fetch_k = fetch_k;
    c.k = k;
    c.covers = covers ? 1 : 0;
    c.label_offset = label_offset;
    c.need = ws->dneed.p;
    c.ticket = reinterpret_cast<unsigned int*>(ws->dneed.p + kCoreTile);
    c.ctr = counted ? idx->ds_ctr.dev() : nullptr;
    c.host = counted ? idx->ds_ctr.mirror() : nullptr;
    const int cthreads = (fetch_k + kWave - 1) / kWave * kWave;

    GroupBestArgs g;
    g.X = idx->X.p;
    g.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : idx->n;
    g.ld = idx->ld;
    g.d4 = idx->d4;
    g.normalize_q = normalize_q;
    g.rows = rs ? rs->rows : nullptr;
    g.mask = rs ? rs->mask : nullptr;
    g.codes = grp->codes;
    g.table = ws->dtab.p;
    g.n_groups = ng;
    DistinctTopkArgs t;
    t.table = ws->dtab.p;
    t.n_groups = ng;
    t.rows = g.rows;
    t.codes = grp->codes;
    t.k = k;
    t.label_offset = label_offset;
    const int clear_gx = (int)std::max<int64_t>(1, std::min<int64_t>((ng + 2047) / 2048, 1024));

    for (int t0 = 0; t0 < nq; t0 += kCoreTile) {
        const int take = std::min(kCoreTile, nq - t0);
        const float* qt = q + (int64_t)t0 * idx->ld;
        if (rs) MVDB_TRY(rowset_search_core(idx, ws, qt, take, fetch_k, normalize_q, rs, 0, ws->mmrD.p, ws->mmrI.p));
        else MVDB_TRY(search_core(idx, ws, qt, take, fetch_k, normalize_q, nullptr, 0, 0, ws->mmrD.p, ws->mmrI.p));
        c.D = D_dev + (int64_t)t0 * k;
        c.I = I_dev + (int64_t)t0 * k;
        c.G = G_dev ? G_dev + (int64_t)t0 * k : nullptr;
        MVDB_TRY(profiled_launch("distinct_collapse", s,
                                 [&](hipEvent_t done) { launch_kernel(distinct_collapse_kernel, dim3((unsigned)take), dim3(cthreads), 0, s, done, c); },
                                 "distinct_collapse_kernel"));
        if (covers) continue;
        for (int s0 = 0; s0 < take; s0 += T) {
            const int slots = std::min(T, take - s0);
            const int* need = ws->dneed.p + s0;
            // (the clear runs under the scan's label, as a record of its own: it names no symbol)
            MVDB_TRY(profiled_launch("distinct_scan", s, [&](hipEvent_t done) {
                launch_kernel(distinct_clear_kernel, dim3(clear_gx, slots), dim3(256), 0, s, done, ws->dtab.p, ng, need);
            }));
            g.q = qt + (int64_t)s0 * idx->ld;
            g.need = need;
            MVDB_TRY(launch_group_best(g, slots, idx->device, s));
            t.need = need;
            t.D = c.D + (int64_t)s0 * k;
            t.I = c.I + (int64_t)s0 * k;
            t.G = c.G ? c.G + (int64_t)s0 * k : nullptr;
            MVDB_TRY(profiled_launch("distinct_select", s,
                                     [&](hipEvent_t done) { launch_kernel(distinct_topk_kernel, dim3((unsigned)slots), dim3(kDistinctThreads), 0, s, done, t); },
                                     "distinct_topk_kernel"));
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int mvdb_grouping_create(const mvdb_index* idx, const int32_t* codes_host, int64_t n, int64_t n_groups, mvdb_grouping** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (n > 0 && !codes_host) return fail(MVDB_ERR_ARG, "codes is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (n != idx->n) return fail(MVDB_ERR_ARG, "a grouping needs one code per stored row (%lld codes, %lld rows)", (long long)n, (long long)idx->n);
    if (n > 0 && (n_groups < 1 || n_groups > n))
        return fail(MVDB_ERR_ARG, "n_groups must lie in [1, %lld] (got %lld)", (long long)n, (long long)n_groups);
    int32_t lo = 0, hi = -1;
    if (n > 0) lo = hi = codes_host[0];
    for (int64_t i = 1; i < n; ++i) {  // (branch-free: vectorises)
        lo = codes_host[i] < lo ? codes_host[i] : lo;
        hi = codes_host[i] > hi ? codes_host[i] : hi;
    }
    if (n > 0 && (lo < 0 || hi >= n_groups))
        return fail(MVDB_ERR_ARG, "group code %d out of range [0,%lld)", (int)(lo < 0 ? lo : hi), (long long)n_groups);
    DeviceGuard dg(idx->device);
    mvdb_grouping* g = new mvdb_grouping();
    g->owner = idx->serial;
    g->device = idx->device;
    g->n = n;
    g->renumbered = idx->renumbered;
    g->n_groups = n > 0 ? n_groups : 0;
    if (n > 0) {
        hipError_t e = hipMalloc((void**)&g->codes, (size_t)n * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemcpy(g->codes, codes_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (g->codes) (void)hipFree(g->codes);
            delete g;
            return fail(MVDB_ERR_HIP, "grouping upload failed: %s", hipGetErrorString(e));
        }
    }
    *out = g;
    return 0;
}

int64_t mvdb_grouping_rows(const mvdb_grouping* g) { return g ? g->n : -1; }
int64_t mvdb_grouping_groups(const mvdb_grouping* g) { return g ? g->n_groups : -1; }

int mvdb_grouping_free(mvdb_grouping* g) {
    if (!g) return 0;
    if (g->codes) {
        DeviceGuard dg(g->device);
        (void)hipFree(g->codes);
    }
    delete g;
    return 0;
}

int mvdb_index_search_distinct(const mvdb_index* idx, const float* q_host, int nq, int k, int fetch_k, int normalize_q,
                               const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_host, int64_t* I_host, int32_t* G_host) {
    MVDB_TRY(check_distinct_args(idx, q_host, nq, k, fetch_k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(grouping_check(idx, grp));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    if (G_host) MVDB_TRY(call.ws->dG.reserve(total));
    MVDB_TRY(distinct_core(idx, call.ws, call.ws->q.p, nq, k, fetch_k, normalize_q, grp, rs, 0, D_dev, I_dev, G_host ? call.ws->dG.p : nullptr));
    if (G_host) {
        MVDB_TRY(copy_back(call.ws, call.ws->dG.p, total * sizeof(int32_t), "distinct search"));
        memcpy(G_host, call.ws->pin_out.p, total * sizeof(int32_t));
    }
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_distinct_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int fetch_k, int normalize_q,
                                      const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_dev, int64_t* I_dev, int32_t* G_dev,
                                      int64_t label_offset, void* stream) {
    MVDB_TRY(check_distinct_args(idx, q_dev, nq, k, fetch_k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(grouping_check(idx, grp));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises: capturable once an eager call of the same shape has sized the workspace
    return distinct_core(idx, call.ws, call.q, nq, k, fetch_k, normalize_q, grp, rs, label_offset, D_dev, I_dev, G_dev);
}

}  // extern "C"

// ---- group hits search: the k best groups, each with its group_size best rows (group_hits.hpp) ----------------------------
namespace {

int check_groups_args(const mvdb_index* idx, const void* q, int nq, int k, int group_size, int fetch_k, const void* D, const void* I) {
    MVDB_TRY(check_distinct_args(idx, q, nq, k, fetch_k, D, I));
    if (group_size < 1 || group_size > kGroupsMaxSize)
        return fail(MVDB_ERR_ARG, "group hits search needs 1 <= group_size <= %d (got %d)", kGroupsMaxSize, group_size);
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int groups_scan_blocks(int64_t n, int device) {
    void (*kern)(GroupMembersArgs) = group_members_scan_kernel<G, C, U, SEL, MASKED>;
    return scan_grid(n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C), device);  // the grid of the single-query scan
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_group_members_kern(const GroupMembersArgs& a, int slots, int nblocks, hipStream_t stream) {
    void (*kern)(GroupMembersArgs) = group_members_scan_kernel<G, C, U, SEL, MASKED>;
    return profiled_launch("groups_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, slots), dim3(kScanThreads), 0, stream, done, a); },
                           "group_members_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// the shapes and rows in flight of launch_scan: a score depends on (G, C, MASKED) only.  slots == 0: the grid only.
int launch_group_members(const GroupMembersArgs& a, int slots, int device, hipStream_t s, int* nblocks) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);
            if (slots == 0) {
                *nblocks = groups_scan_blocks<S::G, S::C, U, F::SEL, F::MASKED>(a.n, device);
                return 0;
            }
            return launch_group_members_kern<S::G, S::C, U, F::SEL, F::MASKED>(a, slots, *nblocks, s);
        });
    });
}

// the counter of member rows: allocated with the first call, never inside a capture
bool ensure_groups_stats(const mvdb_index* idx, hipStream_t s) {
    std::lock_guard<std::mutex> lk(idx->shadow_mu);
    return idx->gh_ctr.dev() || (!stream_capturing(s) && idx->gh_ctr.ensure(2));
}

// Queries on the device at stride ld, results to device buffers.  distinct_core — unchanged, both tiers — picks the groups
// of every query into G_dev (its rows and scores go to the workspace); then, per tile of kCoreTile queries and per sub-tile
// of T slots, the member pass and its select.  The workspace is sized by the call's shape alone.
int groups_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int group_size, int fetch_k, int normalize_q,
                const mvdb_grouping* grp, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev, int32_t* G_dev) {
    hipStream_t s = ws->stream;
    ++idx->gh_calls;
    const size_t heads = (size_t)nq * k;
    MVDB_TRY(ws->ghD.reserve(heads));
    MVDB_TRY(ws->ghI.reserve(heads));
    if (!G_dev) {
        MVDB_TRY(ws->ghG.reserve(heads));
        G_dev = ws->ghG.p;
    }
    MVDB_TRY(distinct_core(idx, ws, q, nq, k, fetch_k, normalize_q, grp, rs, 0, ws->ghD.p, ws->ghI.p, G_dev));
    const int64_t m = rs ? rs->count : idx->n;  // rows selected
    if (m == 0 || (rs && rs->mask && rs->n_at_create == 0)) {
        const int64_t total = (int64_t)heads * group_size;
        hipLaunchKernelGGL(distinct_fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D_dev, I_dev, (int32_t*)nullptr, total);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    const bool counted = ensure_groups_stats(idx, s);

    GroupMembersArgs g;
    g.X = idx->X.p;
    g.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : idx->n;
    g.ld = idx->ld;
    g.d4 = idx->d4;
    g.normalize_q = normalize_q;
    g.rows = rs ? rs->rows : nullptr;
    g.mask = rs ? rs->mask : nullptr;
    g.codes = grp->codes;
    g.k = k;
    g.group_size = group_size;
    int gx = 0;
    MVDB_TRY(launch_group_members(g, 0, idx->device, s, &gx));
    const int64_t tile = std::min(nq, kCoreTile);
    const int64_t list_words = (int64_t)k * group_size;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(tile, idx->kn.groups_partials_bytes / ((int64_t)gx * list_words * 8)));
    // (by the call's shape, not the index: the largest grid of a scan, the budget in block lists — at least one slot's, at
    //  most the tile's)
    const int64_t gx_ub = std::max<int64_t>(scan_grid_upper_bound(idx->device), gx);
    const int64_t lists_ub = idx->kn.groups_partials_bytes / (list_words * 8);
    MVDB_TRY(ws->ghpart.reserve((size_t)std::min<int64_t>(tile * gx_ub, std::max<int64_t>(gx_ub, lists_ub)) * (size_t)(list_words + 1)));
    g.partials = ws->ghpart.p;

    GroupMembersSelectArgs t;
    t.partials = ws->ghpart.p;
    t.nblocks = gx;
    t.k = k;
    t.group_size = group_size;
    t.rows = g.rows;
    t.label_offset = label_offset;
    t.ticket = reinterpret_cast<unsigned int*>(ws->dneed.p + kCoreTile);  // (distinct_core's: zero between launches)
    t.ctr = counted ? reinterpret_cast<unsigned long long*>(idx->gh_ctr.dev()) : nullptr;
    t.host = counted ? idx->gh_ctr.mirror<unsigned long long>() : nullptr;

    for (int t0 = 0; t0 < nq; t0 += kCoreTile) {
        const int take = std::min(kCoreTile, nq - t0);
        for (int s0 = t0; s0 < t0 + take; s0 += T) {
            const int slots = std::min(T, t0 + take - s0);
            g.q = q + (int64_t)s0 * idx->ld;
            g.G = G_dev + (int64_t)s0 * k;
            MVDB_TRY(launch_group_members(g, slots, idx->device, s, &gx));
            t.D = D_dev + (int64_t)s0 * list_words;
            t.I = I_dev + (int64_t)s0 * list_words;
            MVDB_TRY(profiled_launch("groups_select", s,
                                     [&](hipEvent_t done) { launch_kernel(group_members_select_kernel, dim3((unsigned)slots), dim3(kGroupsSelectThreads), 0, s, done, t); },
                                     "group_members_select_kernel"));
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_search_groups(const mvdb_index* idx, const float* q_host, int nq, int k, int group_size, int fetch_k, int normalize_q,
                             const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_host, int64_t* I_host, int32_t* G_host) {
    MVDB_TRY(check_groups_args(idx, q_host, nq, k, group_size, fetch_k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(grouping_check(idx, grp));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t heads = (size_t)nq * k, total = heads * group_size;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(call.ws->dG.reserve(heads));
    MVDB_TRY(groups_core(idx, call.ws, call.ws->q.p, nq, k, group_size, fetch_k, normalize_q, grp, rs, 0, D_dev, I_dev, call.ws->dG.p));
    if (G_host) {
        MVDB_TRY(copy_back(call.ws, call.ws->dG.p, heads * sizeof(int32_t), "group hits search"));
        memcpy(G_host, call.ws->pin_out.p, heads * sizeof(int32_t));
    }
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_groups_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int group_size, int fetch_k, int normalize_q,
                                    const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_dev, int64_t* I_dev, int32_t* G_dev,
                                    int64_t label_offset, void* stream) {
    MVDB_TRY(check_groups_args(idx, q_dev, nq, k, group_size, fetch_k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(grouping_check(idx, grp));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises: capturable once an eager call of the same shape has sized the workspace
    return groups_core(idx, call.ws, call.q, nq, k, group_size, fetch_k, normalize_q, grp, rs, label_offset, D_dev, I_dev, G_dev);
}

}  // extern "C"

// ---- MaxSim search: one question of T vectors, a group scores the sum of its per-vector maxima (maxsim_scan.hpp) ----------
namespace {

int check_maxsim_args(const mvdb_index* idx, const void* q, int T, int k, const void* D, const void* G) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!q || !D || !G) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (T < 1 || T > kMaxsimMaxTokens) return fail(MVDB_ERR_ARG, "MaxSim search needs 1 <= T <= %d query vectors (got %d)", kMaxsimMaxTokens, T);
    if (k < 1 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "MaxSim search needs 1 <= k <= %d (got %d)", kMaxFusedK, k);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "MaxSim search needs an inner-product index");
    return 0;
}

// under the index's shared lock, before anything is enqueued: the grouping, the row set, the table against its bound
int check_maxsim_state(const mvdb_index* idx, int T, const mvdb_grouping* grp, const mvdb_rowset* rs) {
    MVDB_TRY(grouping_check(idx, grp));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    const long long bytes = (long long)T * (long long)grp->n_groups * 8;
    if (bytes > idx->kn.maxsim_table_bytes)
        return fail(MVDB_ERR_ARG, "MaxSim search: the table of %d vectors x %lld groups needs %lld bytes, above the index option maxsim_table_bytes (%lld)",
                    T, (long long)grp->n_groups, bytes, idx->kn.maxsim_table_bytes);
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_maxsim_kern(const MaxsimScanArgs& a, int device, hipStream_t stream) {
    void (*kern)(MaxsimScanArgs) = maxsim_scan_kernel<G, C, U, SEL, MASKED>;
    constexpr int RB = (kWave / G) * U;
    const size_t lds = maxsim_lds_bytes(a.Tp, a.ld, RB);
    if (lds > device_lds_per_block(device))
        return fail(MVDB_ERR_ARG, "MaxSim search: a pass needs %zu bytes of LDS, the device gives a workgroup %zu", lds, device_lds_per_block(device));
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    // two resident blocks of eight waves where the vectors leave room for them (the scan's eight waves per CU, twice)
    const int per_cu = std::min(cached_occupancy((const void*)kern, kMaxsimThreads, lds, 1), 2);
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t want = (nbatches + kMaxsimWaves - 1) / kMaxsimWaves;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
    return profiled_launch("maxsim_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kMaxsimThreads), lds, stream, done, a); },
                           "maxsim_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// the shapes of launch_scan: a score depends on (G, C, MASKED) only; the rows in flight are maxsim_u's
int launch_maxsim(const MaxsimScanArgs& a, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            return launch_maxsim_kern<S::G, S::C, maxsim_u(S::G, S::C), F::SEL, F::MASKED>(a, device, s);
        });
    });
}

// The T vectors on the device at stride ld, results to device buffers: the clear, ceil(T / Tp) passes over consecutive ranges
// of the vectors into their own columns of the table, the block lists, the merge that writes the outputs.
int maxsim_core(const mvdb_index* idx, Workspace* ws, const float* q, int T, int k, int normalize_q, const mvdb_grouping* grp,
                const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int32_t* G_dev, int64_t* I_tok_dev, float* D_tok_dev) {
    hipStream_t s = ws->stream;
    ++idx->mx_calls;
    const int64_t m = rs ? rs->count : idx->n;  // rows selected
    if (m == 0 || (rs && rs->mask && rs->n_at_create == 0)) {
        hipLaunchKernelGGL(maxsim_fill_missing_kernel, dim3((unsigned)((k * T + 255) / 256)), dim3(256), 0, s, D_dev, G_dev, I_tok_dev, D_tok_dev, k, T);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    const int64_t ng = grp->n_groups;
    const int64_t words = (int64_t)T * ng;
    const int nlists = (int)std::max<int64_t>(1, std::min<int64_t>((ng + kDistinctThreads - 1) / kDistinctThreads, kMaxsimLists));
    MVDB_TRY(ws->mxtab.reserve((size_t)words));
    MVDB_TRY(ws->mxpart.reserve((size_t)nlists * kWave));
    const int Tp = maxsim_tokens_per_pass(T, idx->ld, idx->kn.maxsim_tokens_per_pass);

    const int clear_gx = (int)std::max<int64_t>(1, std::min<int64_t>((words + 2047) / 2048, 2048));
    // (the clear runs under the scan's label, as a record of its own: it names no symbol)
    MVDB_TRY(profiled_launch("maxsim_scan", s, [&](hipEvent_t done) { launch_kernel(maxsim_clear_kernel, dim3(clear_gx), dim3(256), 0, s, done, ws->mxtab.p, words); }));

    MaxsimScanArgs a;
    a.X = idx->X.p;
    a.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : idx->n;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.normalize_q = normalize_q;
    a.rows = rs ? rs->rows : nullptr;
    a.mask = rs ? rs->mask : nullptr;
    a.codes = grp->codes;
    a.T = T;
    for (int v0 = 0; v0 < T; v0 += Tp) {
        a.q = q + (int64_t)v0 * idx->ld;
        a.Tp = std::min(Tp, T - v0);
        a.table = ws->mxtab.p + v0;
        MVDB_TRY(launch_maxsim(a, idx->device, s));
        ++idx->mx_passes;
    }

    MaxsimTopkArgs t;
    t.table = ws->mxtab.p;
    t.n_groups = ng;
    t.T = T;
    t.k = k;
    t.part = ws->mxpart.p;
    MVDB_TRY(profiled_launch("maxsim_select", s,
                             [&](hipEvent_t done) { launch_kernel(maxsim_topk_kernel, dim3((unsigned)nlists), dim3(kDistinctThreads), 0, s, done, t); },
                             "maxsim_topk_kernel"));
    MaxsimEmitArgs e;
    e.part = ws->mxpart.p;
    e.nlists = nlists;
    e.table = ws->mxtab.p;
    e.T = T;
    e.k = k;
    e.rows = a.rows;
    e.label_offset = label_offset;
    e.D = D_dev;
    e.G = G_dev;
    e.I_tok = I_tok_dev;
    e.D_tok = D_tok_dev;
    MVDB_TRY(profiled_launch("maxsim_select", s, [&](hipEvent_t done) { launch_kernel(maxsim_emit_kernel, dim3(1), dim3(kDistinctThreads), 0, s, done, e); }));
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_search_maxsim(const mvdb_index* idx, const float* q_host, int T, int k, int normalize_q, const mvdb_grouping* grp,
                             const mvdb_rowset* rs, float* D_host, int32_t* G_host, int64_t* I_tok_host, float* D_tok_host) {
    MVDB_TRY(check_maxsim_args(idx, q_host, T, k, D_host, G_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_maxsim_state(idx, T, grp, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, T));
    // packed: I_tok [k, T] int64 | D_tok [k, T] fp32 | D [k] fp32 | G [k] int32 -> ONE copy back
    const size_t kt = (size_t)k * T;
    const size_t bytes = kt * 12 + (size_t)k * 8;
    MVDB_TRY(call.ws->mxout.reserve(bytes));
    char* const out = call.ws->mxout.p;
    int64_t* I_tok = reinterpret_cast<int64_t*>(out);
    float* D_tok = reinterpret_cast<float*>(out + kt * 8);
    float* D = reinterpret_cast<float*>(out + kt * 12);
    int32_t* G = reinterpret_cast<int32_t*>(out + kt * 12 + (size_t)k * 4);
    MVDB_TRY(maxsim_core(idx, call.ws, call.ws->q.p, T, k, normalize_q, grp, rs, 0, D, G, I_tok, D_tok));
    MVDB_TRY(copy_back(call.ws, out, bytes, "MaxSim search"));
    const char* const pin = (const char*)call.ws->pin_out.p;
    if (I_tok_host) memcpy(I_tok_host, pin, kt * 8);
    if (D_tok_host) memcpy(D_tok_host, pin + kt * 8, kt * 4);
    memcpy(D_host, pin + kt * 12, (size_t)k * 4);
    memcpy(G_host, pin + kt * 12 + (size_t)k * 4, (size_t)k * 4);
    return 0;
}

int mvdb_index_search_maxsim_device(const mvdb_index* idx, const float* q_dev, int T, int k, int normalize_q, const mvdb_grouping* grp,
                                    const mvdb_rowset* rs, float* D_dev, int32_t* G_dev, int64_t* I_tok_dev, float* D_tok_dev,
                                    int64_t label_offset, void* stream) {
    MVDB_TRY(check_maxsim_args(idx, q_dev, T, k, D_dev, G_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_maxsim_state(idx, T, grp, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, T);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises: capturable once an eager call of the same shape has sized the workspace
    return maxsim_core(idx, call.ws, call.q, T, k, normalize_q, grp, rs, label_offset, D_dev, G_dev, I_tok_dev, D_tok_dev);
}

}  // extern "C"

// ---- assignment and k-means: every stored row labelled by the nearest of C vectors (assign_scan.hpp) -----------------------
namespace {

int check_assign_args(const mvdb_index* idx, const void* c, int C) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!c) return fail(MVDB_ERR_ARG, "NULL buffer passed to assign");
    if (C < 1 || C > kAssignMaxVectors) return fail(MVDB_ERR_ARG, "assignment needs 1 <= C <= %d vectors (got %d)", kAssignMaxVectors, C);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "assignment needs an inner-product index");
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_assign_kern(const AssignScanArgs& a, int device, hipStream_t stream) {
    void (*kern)(AssignScanArgs) = assign_scan_kernel<G, C, U, SEL, MASKED>;
    constexpr int RB = (kWave / G) * U;
    const size_t lds = 4 * (size_t)a.Vp * (size_t)a.ld;
    if (lds > device_lds_per_block(device))
        return fail(MVDB_ERR_ARG, "assignment: a pass needs %zu bytes of LDS, the device gives a workgroup %zu", lds, device_lds_per_block(device));
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    // MaxSim's grid: two resident blocks of eight waves where the vectors leave room for them
    const int per_cu = std::min(cached_occupancy((const void*)kern, kMaxsimThreads, lds, 1), 2);
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t want = (nbatches + kMaxsimWaves - 1) / kMaxsimWaves;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
    return profiled_launch("assign_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kMaxsimThreads), lds, stream, done, a); },
                           "assign_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// MaxSim's forms, from the one shape table
int launch_assign(const AssignScanArgs& a, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            return launch_assign_kern<S::G, S::C, maxsim_u(S::G, S::C), F::SEL, F::MASKED>(a, device, s);
        });
    });
}

int utility_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, 2048)); }

// The C vectors on the device at stride ld -> ws->asbest, a word per stored row: the clear, then ceil(C / Vp) passes over
// consecutive ranges of the vectors.
int assign_core(const mvdb_index* idx, Workspace* ws, const float* c, int C, int normalize_c, const mvdb_rowset* rs) {
    hipStream_t s = ws->stream;
    ++idx->as_calls;
    const int64_t n = idx->n;
    MVDB_TRY(ws->asbest.reserve((size_t)std::max<int64_t>(n, 1)));
    MVDB_TRY(profiled_launch("assign_scan", s, [&](hipEvent_t done) { launch_kernel(assign_clear_kernel, dim3(utility_grid(n)), dim3(256), 0, s, done, ws->asbest.p, n); }));
    const int64_t m = rs ? rs->count : n;  // rows selected
    if (m == 0 || (rs && rs->mask && rs->n_at_create == 0)) return 0;
    const int Vp = assign_vectors_per_pass(C, idx->ld, idx->kn.assign_vectors_per_pass);
    AssignScanArgs a;
    a.X = idx->X.p;
    a.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : n;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.normalize_q = normalize_c;
    a.rows = rs ? rs->rows : nullptr;
    a.mask = rs ? rs->mask : nullptr;
    a.best = ws->asbest.p;
    for (int v0 = 0; v0 < C; v0 += Vp) {
        a.q = c + (int64_t)v0 * idx->ld;
        a.Vp = std::min(Vp, C - v0);
        a.v0 = v0;
        MVDB_TRY(launch_assign(a, idx->device, s));
        ++idx->as_passes;
    }
    return 0;
}

// the words -> labels / scores (either may be NULL), or packed in place for the host entry points' one copy back
int assign_emit(const mvdb_index* idx, Workspace* ws, int32_t* labels, float* scores, bool pack) {
    AssignEmitArgs e;
    e.best = ws->asbest.p;
    e.n = idx->n;
    e.labels = labels;
    e.scores = scores;
    e.pack = pack ? 1 : 0;
    hipLaunchKernelGGL(assign_emit_kernel, dim3(utility_grid(idx->n)), dim3(256), 0, ws->stream, e);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// the packed words of every row to the host, unpacked
int assign_fetch(const mvdb_index* idx, Workspace* ws, int32_t* labels_host, float* scores_host, const char* what) {
    const int64_t n = idx->n;
    if (n == 0 || (!labels_host && !scores_host)) return 0;
    MVDB_TRY(copy_back(ws, ws->asbest.p, (size_t)n * 8, what));
    const uint64_t* const w = (const uint64_t*)ws->pin_out.p;
    for (int64_t i = 0; i < n; ++i) {
        if (labels_host) labels_host[i] = (int32_t)(uint32_t)w[i];
        if (scores_host) {
            const uint32_t bits = (uint32_t)(w[i] >> 32);
            memcpy(&scores_host[i], &bits, 4);
        }
    }
    return 0;
}

int launch_normalize(const mvdb_index* idx, const float* src, float* dst, int nv, hipStream_t s) {
    return with_scan_shape(idx->d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(idx->d4, false, false, [&](auto form) {
            using F = decltype(form);
            const int64_t threads = (int64_t)nv * S::G;
            hipLaunchKernelGGL((assign_normalize_kernel<S::G, S::C, F::MASKED>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, dst, nv,
                               idx->ld, idx->d4);
            MVDB_HIP(hipGetLastError());
            return 0;
        });
    });
}

// slices of the list build: about 2048 rows each, at most kKmeansSlices
struct KmeansSlices {
    int nb;
    int64_t per;
};
KmeansSlices kmeans_slices(int64_t n) {
    KmeansSlices k;
    k.nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048, kKmeansSlices));
    k.per = std::max<int64_t>(1, (n + k.nb - 1) / k.nb);
    return k;
}

// labels -> counts per label (ws->kmcount) and, with `lists`, the member lists and the work items' bases
int kmeans_lists(const mvdb_index* idx, Workspace* ws, const int32_t* labels, int C, bool lists) {
    hipStream_t s = ws->stream;
    const int64_t n = idx->n;
    const KmeansSlices sl = kmeans_slices(n);
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3(sl.nb), dim3(256), (size_t)C * 4, s, labels, n, sl.per, C, sl.nb, ws->kmhist.p);
    hipLaunchKernelGGL(kmeans_colscan_kernel, dim3(C), dim3(kWave), 0, s, ws->kmhist.p, sl.nb, ws->kmcount.p);
    if (lists) {
        uint32_t* const base = ws->kmoff.p;
        hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(1), dim3(kWave), 0, s, ws->kmcount.p, C, base, base + C + 1);
        hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(sl.nb), dim3(kWave), (size_t)C * 4, s, labels, n, sl.per, C, sl.nb, ws->kmhist.p, base, ws->kmmem.p);
    }
    MVDB_HIP(hipGetLastError());
    return 0;
}

// one update of the centres from the labels: the lists, the chunk sums, the finalise
int kmeans_update(const mvdb_index* idx, Workspace* ws, const int32_t* labels, int C) {
    hipStream_t s = ws->stream;
    MVDB_TRY(kmeans_lists(idx, ws, labels, C, true));
    const int64_t items = idx->n / kKmeansChunk + C;  // at most: a label's last chunk may be short
    KmeansSumArgs a;
    a.X = idx->X.p;
    a.ld = idx->ld;
    a.d = idx->d;
    a.C = C;
    a.members = ws->kmmem.p;
    a.base = ws->kmoff.p;
    a.ioff = ws->kmoff.p + C + 1;
    a.part = ws->kmpart.p;
    hipLaunchKernelGGL(kmeans_chunksum_kernel, dim3((unsigned)items), dim3(kKmeansChunk), 0, s, a);
    KmeansFinalArgs f;
    f.part = ws->kmpart.p;
    f.ioff = a.ioff;
    f.count = ws->kmcount.p;
    f.centres = ws->kmc.p;
    f.ld = idx->ld;
    f.d = idx->d;
    hipLaunchKernelGGL(kmeans_finalise_kernel, dim3(C), dim3(256), 0, s, f);
    MVDB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_assign(const mvdb_index* idx, const float* c_host, int C, int normalize_c, const mvdb_rowset* rs, int32_t* labels_host,
                      float* scores_host) {
    MVDB_TRY(check_assign_args(idx, c_host, C));
    if (!labels_host) return fail(MVDB_ERR_ARG, "NULL buffer passed to assign");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(c_host, C));
    MVDB_TRY(assign_core(idx, call.ws, call.ws->q.p, C, normalize_c, rs));
    MVDB_TRY(assign_emit(idx, call.ws, nullptr, nullptr, true));
    return assign_fetch(idx, call.ws, labels_host, scores_host, "assign");
}

int mvdb_index_assign_device(const mvdb_index* idx, const float* c_dev, int C, int normalize_c, const mvdb_rowset* rs, int32_t* labels_dev,
                             float* scores_dev, void* stream) {
    MVDB_TRY(check_assign_args(idx, c_dev, C));
    if (!labels_dev) return fail(MVDB_ERR_ARG, "NULL buffer passed to assign");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, c_dev, C);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises
    MVDB_TRY(assign_core(idx, call.ws, call.q, C, normalize_c, rs));
    return assign_emit(idx, call.ws, labels_dev, scores_dev, false);
}

int mvdb_index_kmeans(const mvdb_index* idx, float* centres_host, int C, int max_iter, const mvdb_rowset* rs, int32_t* labels_host,
                      float* scores_host, int64_t* counts_host, int* iterations) {
    MVDB_TRY(check_assign_args(idx, centres_host, C));
    if (!counts_host) return fail(MVDB_ERR_ARG, "NULL buffer passed to kmeans");
    if (max_iter < 1) return fail(MVDB_ERR_ARG, "k-means needs max_iter >= 1 (got %d)", max_iter);
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    hipStream_t s = ws->stream;
    const int64_t n = idx->n;
    const KmeansSlices sl = kmeans_slices(n);
    const size_t nrows = (size_t)std::max<int64_t>(n, 1);
    MVDB_TRY(ws->kmc.reserve((size_t)C * idx->ld));
    MVDB_TRY(ws->kmlab[0].reserve(nrows));
    MVDB_TRY(ws->kmlab[1].reserve(nrows));
    MVDB_TRY(ws->kmmem.reserve(nrows));
    MVDB_TRY(ws->kmhist.reserve((size_t)C * sl.nb));
    MVDB_TRY(ws->kmcount.reserve((size_t)C + 1));
    MVDB_TRY(ws->kmoff.reserve(2 * ((size_t)C + 1)));
    MVDB_TRY(ws->kmpart.reserve((size_t)(n / kKmeansChunk + C) * idx->d));
    unsigned long long* const changed_dev = reinterpret_cast<unsigned long long*>(ws->kmcount.p + C);

    // centres = initial, each normalised by the scan's prologue (the padding of a row stays zero: staged so)
    MVDB_TRY(call.stage(centres_host, C));
    MVDB_HIP(hipMemsetAsync(ws->kmc.p, 0, (size_t)C * idx->ld * sizeof(float), s));
    MVDB_TRY(launch_normalize(idx, ws->q.p, ws->kmc.p, C, s));

    int cur = 0, updates = 0;
    bool converged = false;
    for (int it = 1; it <= max_iter; ++it) {
        MVDB_TRY(assign_core(idx, ws, ws->kmc.p, C, 0, rs));
        MVDB_TRY(assign_emit(idx, ws, ws->kmlab[cur].p, nullptr, false));
        if (it > 1) {
            MVDB_HIP(hipMemsetAsync(changed_dev, 0, 8, s));
            hipLaunchKernelGGL(kmeans_changed_kernel, dim3(utility_grid(n)), dim3(256), 0, s, ws->kmlab[cur].p, ws->kmlab[cur ^ 1].p, n, changed_dev);
            MVDB_HIP(hipGetLastError());
            MVDB_TRY(copy_back(ws, changed_dev, 8, "k-means"));  // the one read of an iteration
            if (*(const unsigned long long*)ws->pin_out.p == 0ull) {
                converged = true;
                break;
            }
        }
        MVDB_TRY(kmeans_update(idx, ws, ws->kmlab[cur].p, C));
        ++updates;
        cur ^= 1;
    }
    if (!converged) {  // the loop ran out: the labels of the centres as they are now
        MVDB_TRY(assign_core(idx, ws, ws->kmc.p, C, 0, rs));
        MVDB_TRY(assign_emit(idx, ws, ws->kmlab[cur].p, nullptr, false));
    }
    // ws->asbest is the assignment of the returned centres in both cases, ws->kmlab[cur] its labels
    MVDB_TRY(kmeans_lists(idx, ws, ws->kmlab[cur].p, C, false));
    MVDB_TRY(copy_back(ws, ws->kmcount.p, (size_t)C * 8, "k-means"));
    memcpy(counts_host, ws->pin_out.p, (size_t)C * 8);
    MVDB_TRY(copy_back(ws, ws->kmc.p, (size_t)C * idx->ld * sizeof(float), "k-means"));
    for (int c = 0; c < C; ++c) memcpy(centres_host + (size_t)c * idx->d, (const float*)ws->pin_out.p + (size_t)c * idx->ld, (size_t)idx->d * sizeof(float));
    MVDB_TRY(assign_emit(idx, ws, nullptr, nullptr, true));
    MVDB_TRY(assign_fetch(idx, ws, labels_host, scores_host, "k-means"));
    if (iterations) *iterations = updates;
    return 0;
}

}  // extern "C"

// ---- probed search: a partition of the rows into C member lists, a query scans the lists of its nprobe best centres (probe_scan.hpp) ----
struct mvdb_partition {
    uint64_t owner = 0;       // serial number of the index the partition was built on
    int device = 0;
    int64_t n = 0;            // the index's row count it covers: one label per row
    uint64_t renumbered = 0;  // ... and the index's renumbering generation
    int C = 0, d = 0;
    int64_t ld = 0;
    int64_t cap = 0;            // rows the label and member arrays hold
    DevMem<float> centres;      // [C, ld] after their own normalisation, zero padded
    DevMem<int32_t> labels;     // [cap] -1: in no list
    DevMem<uint32_t> members;   // [cap] the lists, list after list, ascending rows inside each
    DevMem<uint32_t> offsets;   // [C + 1]
    std::vector<int64_t> sizes;  // [C] members per list (host copy)
    std::vector<int64_t> items;  // [C + 1] items[j]: work items of the j LARGEST lists — what a query of j probes needs at most
    mutable std::shared_mutex mu;  // search and the readers: shared; update: exclusive
};

namespace {

int partition_check(const mvdb_index* idx, const mvdb_partition* p, bool for_update) {
    if (p->owner != idx->serial) return fail(MVDB_ERR_ARG, "the partition belongs to another index");
    if (p->device != idx->device || p->renumbered != idx->renumbered)
        return fail(MVDB_ERR_ARG, "rows were removed since the partition was built: re-create it from its labels");
    if (for_update ? p->n > idx->n : p->n != idx->n)
        return fail(MVDB_ERR_ARG, "the partition covers %lld rows, the index holds %lld: mvdb_partition_update first", (long long)p->n, (long long)idx->n);
    return 0;
}

// labels -> member lists, offsets and the host's copy of the sizes (the stable counting sort of kmeans_lists); waits for the stream
int partition_lists(const mvdb_index* idx, Workspace* ws, mvdb_partition* p) {
    hipStream_t s = ws->stream;
    const int C = p->C;
    const int64_t n = p->n;
    const KmeansSlices sl = kmeans_slices(n);
    MVDB_TRY(ws->kmhist.reserve((size_t)C * sl.nb));
    MVDB_TRY(ws->kmcount.reserve((size_t)C + 1));
    MVDB_TRY(ws->kmoff.reserve(2 * ((size_t)C + 1)));
    uint32_t* const base = ws->kmoff.p;
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3(sl.nb), dim3(256), (size_t)C * 4, s, p->labels.p, n, sl.per, C, sl.nb, ws->kmhist.p);
    hipLaunchKernelGGL(kmeans_colscan_kernel, dim3(C), dim3(kWave), 0, s, ws->kmhist.p, sl.nb, ws->kmcount.p);
    hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(1), dim3(kWave), 0, s, ws->kmcount.p, C, base, base + C + 1);
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(sl.nb), dim3(kWave), (size_t)C * 4, s, p->labels.p, n, sl.per, C, sl.nb, ws->kmhist.p, base, p->members.p);
    MVDB_HIP(hipGetLastError());
    MVDB_HIP(hipMemcpyAsync(p->offsets.p, base, ((size_t)C + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    MVDB_TRY(copy_back(ws, ws->kmcount.p, (size_t)C * 8, "partition"));
    p->sizes.assign((const int64_t*)ws->pin_out.p, (const int64_t*)ws->pin_out.p + C);
    std::vector<int64_t> pieces(C);
    for (int c = 0; c < C; ++c) pieces[c] = (p->sizes[c] + kProbeSlice - 1) / kProbeSlice;
    std::sort(pieces.begin(), pieces.end(), std::greater<int64_t>());
    p->items.assign((size_t)C + 1, 0);
    for (int c = 0; c < C; ++c) p->items[c + 1] = p->items[c] + pieces[c];
    return 0;
}

// room for `rows` labels and members; the labels held so far are kept
int partition_reserve(mvdb_partition* p, int64_t rows) {
    if (rows <= p->cap && p->labels.p) return 0;
    const size_t want = (size_t)std::max<int64_t>(rows, 1);
    DevMem<int32_t> grown;
    if (grown.alloc(want * sizeof(int32_t)) != hipSuccess) return fail(MVDB_ERR_OOM, "partition: %zu bytes of labels could not be allocated", want * sizeof(int32_t));
    if (p->labels.p && p->n > 0) MVDB_HIP(hipMemcpy(grown.p, p->labels.p, (size_t)p->n * sizeof(int32_t), hipMemcpyDeviceToDevice));
    if (p->members.alloc(want * sizeof(uint32_t)) != hipSuccess) return fail(MVDB_ERR_OOM, "partition: %zu bytes of member lists could not be allocated", want * sizeof(uint32_t));
    std::swap(p->labels.p, grown.p);
    p->cap = (int64_t)want;
    return 0;
}

int check_probe_args(const mvdb_index* idx, const mvdb_partition* p, const void* q, int nq, int k, int nprobe, const void* D, const void* I) {
    MVDB_TRY(check_search_args(idx, q, nq, k, D, I));
    if (!p) return fail(MVDB_ERR_ARG, "partition is NULL");
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "probed search needs an inner-product index");
    if (k > kMaxFusedK) return fail(MVDB_ERR_ARG, "probed search needs k <= %d (got %d)", kMaxFusedK, k);
    if (nprobe < 1 || nprobe > p->C) return fail(MVDB_ERR_ARG, "probed search needs 1 <= nprobe <= %d lists (got %d)", p->C, nprobe);
    return 0;
}

// the partition and the row set against the index's state: refused before anything is enqueued (the caller holds both locks)
int check_probe_state(const mvdb_index* idx, const mvdb_partition* p, const mvdb_rowset* rs) {
    MVDB_TRY(partition_check(idx, p, false));
    if (rs) {
        MVDB_TRY(rowset_check(idx, rs));
        if (!rs->mask) return fail(MVDB_ERR_ARG, "probed search takes a bitmap-form row set; a list-form set is served by mvdb_index_search_rowset");
    }
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_probe_scan_kern(const ProbeScanArgs& a, int nq, hipStream_t stream) {
    void (*kern)(ProbeScanArgs) = probe_scan_kernel<G, C, U, SEL, MASKED>;
    return profiled_launch("probe_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3((unsigned)a.max_items, (unsigned)nq), dim3(kScanThreads), 0, stream, done, a); },
                           "probe_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// the shape of the single-query scan, the rows in flight of the gathered scans (U does not enter the arithmetic)
int launch_probe_scan(const ProbeScanArgs& a, int nq, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        constexpr int U = gather_u(S::G, S::C);
        static_assert(kProbeSlice % (kScanWaves * (kWave / S::G) * U) == 0, "an item is a whole number of block steps");
        return with_scan_form<S::G, S::C>(a.d4, false, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            if constexpr (F::SEL == 1) return fail(MVDB_ERR_ARG, "internal: the probe scan has no row-list form");
            else return launch_probe_scan_kern<S::G, S::C, U, F::SEL, F::MASKED>(a, nq, s);
        });
    });
}

// Queries on the device at stride ld, results to device buffers; everything has been checked.  Per chunk of queries four
// launches: the coarse scores (the single-query scan over the centre matrix, a grid row per query), the plan, the scan of
// the items, the merge.  Nothing is read back: the grid of the scan is sized from the nprobe LARGEST lists.
int probe_core(const mvdb_index* idx, Workspace* ws, const mvdb_partition* p, const float* q, int nq, int k, int nprobe, int normalize_q,
               const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    KnobScope knobs(&idx->kn);
    hipStream_t s = ws->stream;
    ++idx->pb_calls;
    const int64_t max_items = p->items[nprobe];
    if (max_items == 0 || (rs && (rs->count == 0 || rs->n_at_create == 0))) {  // no row in any list, or none selected
        const int64_t total = (int64_t)nq * k;
        hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D_dev, I_dev, total, idx->metric);
        MVDB_HIP(hipGetLastError());
        ++idx->pb_launches;
        return 0;
    }
    if (max_items > 0x7FFFFFFFll) return fail(MVDB_ERR_ARG, "probed search: %lld work items per query", (long long)max_items);
    const int C = p->C;
    // the tables of ONE query: its items, their candidate lists, its coarse scores
    const int64_t per_query = max_items * ((int64_t)sizeof(ProbeItem) + 8 * (int64_t)k) + 4 * (int64_t)C;
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nq, kCoreTile), idx->kn.probe_table_bytes / per_query));
    MVDB_TRY(ws->scores.reserve((size_t)chunk * C));
    MVDB_TRY(ws->pitems.reserve((size_t)chunk * max_items));
    MVDB_TRY(ws->pcount.reserve((size_t)chunk));
    MVDB_TRY(ws->cand.reserve((size_t)chunk * max_items * k));

    ScanArgs c;
    c.X = p->centres.p;
    c.n = C;
    c.ld = idx->ld;
    c.d4 = idx->d4;
    c.normalize_q = normalize_q;
    c.k = 0;
    c.rows = nullptr;
    c.mask = nullptr;
    c.cand = nullptr;
    c.scores = ws->scores.p;
    ProbePlanArgs pl;
    pl.scores = reinterpret_cast<const uint32_t*>(ws->scores.p);
    pl.C = C;
    pl.P = (int)pow2ceil(std::max(C, 2));
    pl.nprobe = nprobe;
    pl.off = p->offsets.p;
    pl.max_items = (int)max_items;
    pl.items = ws->pitems.p;
    pl.count = ws->pcount.p;
    ProbeScanArgs a;
    a.X = idx->X.p;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.normalize_q = normalize_q;
    a.k = k;
    a.members = p->members.p;
    a.items = ws->pitems.p;
    a.count = ws->pcount.p;
    a.max_items = (int)max_items;
    a.mask = rs ? rs->mask : nullptr;
    a.mask_n = rs ? rs->n_at_create : 0;
    a.cand = ws->cand.p;
    ProbeMergeArgs mg;
    mg.keys = ws->cand.p;
    mg.count = ws->pcount.p;
    mg.max_items = (int)max_items;
    mg.k = k;
    mg.label_offset = label_offset;

    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int take = std::min(chunk, nq - q0);
        c.q = a.q = q + (int64_t)q0 * idx->ld;
        MVDB_TRY(launch_scan(MVDB_METRIC_IP, kModeScores, c, take, idx->device, s, nullptr));
        MVDB_TRY(profiled_launch("probe_plan", s, [&](hipEvent_t done) { launch_kernel(probe_plan_kernel, dim3((unsigned)take), dim3(kProbePlanThreads), 0, s, done, pl); },
                                 "probe_plan_kernel"));
        MVDB_TRY(launch_probe_scan(a, take, s));
        mg.D = D_dev + (int64_t)q0 * k;
        mg.I = I_dev + (int64_t)q0 * k;
        MVDB_TRY(profiled_launch("probe_merge", s, [&](hipEvent_t done) { launch_kernel(probe_merge_kernel, dim3((unsigned)take), dim3(kMergeThreads), 0, s, done, mg); },
                                 "probe_merge_kernel"));
        idx->pb_launches += 4;
    }
    return 0;
}

}  // namespace

extern "C" {

int mvdb_partition_create(const mvdb_index* idx, const float* centres_host, int C, int normalize_c, const int32_t* labels_host,
                          mvdb_partition** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    MVDB_TRY(check_assign_args(idx, centres_host, C));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int64_t n = idx->n;
    if (labels_host) {
        int32_t lo = 0, hi = -1;
        for (int64_t i = 0; i < n; ++i) {  // (branch-free: vectorises)
            lo = labels_host[i] < lo ? labels_host[i] : lo;
            hi = labels_host[i] > hi ? labels_host[i] : hi;
        }
        if (lo < -1 || hi >= C) return fail(MVDB_ERR_ARG, "label %d out of range [-1,%d)", (int)(lo < -1 ? lo : hi), C);
    }
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    hipStream_t s = ws->stream;
    std::unique_ptr<mvdb_partition> p(new mvdb_partition());
    p->owner = idx->serial;
    p->device = idx->device;
    p->renumbered = idx->renumbered;
    p->C = C;
    p->d = idx->d;
    p->ld = idx->ld;
    const size_t cbytes = (size_t)C * idx->ld * sizeof(float);
    if (p->centres.alloc(cbytes) != hipSuccess || p->offsets.alloc(((size_t)C + 1) * sizeof(uint32_t)) != hipSuccess)
        return fail(MVDB_ERR_OOM, "partition: the centres could not be allocated");
    MVDB_TRY(partition_reserve(p.get(), n));
    p->n = n;
    // the centres as they are searched from now on: normalised by the scan's prologue where asked (the padding stays zero: staged so)
    MVDB_TRY(call.stage(centres_host, C));
    if (normalize_c) {
        MVDB_HIP(hipMemsetAsync(p->centres.p, 0, cbytes, s));
        MVDB_TRY(launch_normalize(idx, ws->q.p, p->centres.p, C, s));
    } else {
        MVDB_HIP(hipMemcpyAsync(p->centres.p, ws->q.p, cbytes, hipMemcpyDeviceToDevice, s));
    }
    if (labels_host) {
        if (n > 0) MVDB_HIP(hipMemcpyAsync(p->labels.p, labels_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    } else {  // assign's pass over every row: the labels of mvdb_index_assign(centres, normalize_c)
        MVDB_TRY(assign_core(idx, ws, p->centres.p, C, 0, nullptr));
        MVDB_TRY(assign_emit(idx, ws, p->labels.p, nullptr, false));
    }
    MVDB_TRY(partition_lists(idx, ws, p.get()));
    *out = p.release();
    return 0;
}

int mvdb_partition_update(mvdb_partition* p, const mvdb_index* idx, const int64_t* changed_rows_host, int64_t m) {
    if (!p) return fail(MVDB_ERR_ARG, "partition is NULL");
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (m < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (m > 0 && !changed_rows_host) return fail(MVDB_ERR_ARG, "rows is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    std::unique_lock<std::shared_mutex> pk(p->mu);
    MVDB_TRY(partition_check(idx, p, true));
    const int64_t n = idx->n;
    const RowRange rr = row_range(changed_rows_host, m);
    if (m > 0 && (rr.lo < 0 || rr.hi >= n))
        return fail(MVDB_ERR_ARG, "row %lld out of range [0,%lld)", (long long)(rr.lo < 0 ? rr.lo : rr.hi), (long long)n);
    // the rows to label again: the listed ones and those added since, ascending, each once
    std::vector<int64_t> rows(changed_rows_host, changed_rows_host + m);
    for (int64_t r = p->n; r < n; ++r) rows.push_back(r);
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    if (rows.empty()) return 0;
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    hipStream_t s = ws->stream;
    MVDB_TRY(partition_reserve(p, n));
    const int64_t cnt = (int64_t)rows.size();
    MVDB_TRY(ws->rows.reserve((size_t)cnt));
    MVDB_HIP(hipMemcpyAsync(ws->rows.p, rows.data(), (size_t)cnt * sizeof(int64_t), hipMemcpyHostToDevice, s));
    // one assign under a list-form selection of just those rows
    mvdb_rowset sel;
    sel.owner = idx->serial;
    sel.device = idx->device;
    sel.n_at_create = n;
    sel.renumbered = idx->renumbered;
    sel.count = cnt;
    sel.rows = ws->rows.p;
    MVDB_TRY(assign_core(idx, ws, p->centres.p, p->C, 0, &sel));
    hipLaunchKernelGGL(probe_relabel_kernel, dim3(utility_grid(cnt)), dim3(256), 0, s, (const int64_t*)ws->rows.p, cnt, (const uint64_t*)ws->asbest.p, p->labels.p);
    MVDB_HIP(hipGetLastError());
    p->n = n;
    return partition_lists(idx, ws, p);
}

int mvdb_partition_labels(const mvdb_partition* p, int64_t row0, int64_t n, int32_t* labels_host) {
    if (!p) return fail(MVDB_ERR_ARG, "partition is NULL");
    std::shared_lock<std::shared_mutex> pk(p->mu);
    if (row0 < 0 || n < 0 || row0 + n > p->n) return fail(MVDB_ERR_ARG, "rows [%lld, %lld) out of range [0,%lld)", (long long)row0, (long long)(row0 + n), (long long)p->n);
    if (n == 0) return 0;
    if (!labels_host) return fail(MVDB_ERR_ARG, "labels is NULL");
    DeviceGuard dg(p->device);
    MVDB_HIP(hipMemcpy(labels_host, p->labels.p + row0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mvdb_partition_centres(const mvdb_partition* p, float* centres_host) {
    if (!p) return fail(MVDB_ERR_ARG, "partition is NULL");
    if (!centres_host) return fail(MVDB_ERR_ARG, "centres is NULL");
    DeviceGuard dg(p->device);
    std::vector<float> padded((size_t)p->C * p->ld);
    MVDB_HIP(hipMemcpy(padded.data(), p->centres.p, padded.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int c = 0; c < p->C; ++c) memcpy(centres_host + (size_t)c * p->d, padded.data() + (size_t)c * p->ld, (size_t)p->d * sizeof(float));
    return 0;
}

int mvdb_partition_sizes(const mvdb_partition* p, int64_t* counts_host) {
    if (!p) return fail(MVDB_ERR_ARG, "partition is NULL");
    if (!counts_host) return fail(MVDB_ERR_ARG, "counts is NULL");
    std::shared_lock<std::shared_mutex> pk(p->mu);
    memcpy(counts_host, p->sizes.data(), (size_t)p->C * sizeof(int64_t));
    return 0;
}

int64_t mvdb_partition_rows(const mvdb_partition* p) {
    if (!p) return -1;
    std::shared_lock<std::shared_mutex> pk(p->mu);
    return p->n;
}
int mvdb_partition_lists(const mvdb_partition* p) { return p ? p->C : -1; }

int mvdb_partition_free(mvdb_partition* p) {
    if (!p) return 0;
    DeviceGuard dg(p->device);  // the arrays free themselves, on the partition's device
    delete p;
    return 0;
}

int mvdb_index_search_probe(const mvdb_index* idx, const mvdb_partition* p, const float* q_host, int nq, int k, int nprobe, int normalize_q,
                            const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_probe_args(idx, p, q_host, nq, k, nprobe, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    std::shared_lock<std::shared_mutex> pk(p->mu);
    MVDB_TRY(check_probe_state(idx, p, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(probe_core(idx, call.ws, p, call.ws->q.p, nq, k, nprobe, normalize_q, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_probe_device(const mvdb_index* idx, const mvdb_partition* p, const float* q_dev, int nq, int k, int nprobe, int normalize_q,
                                   const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_probe_args(idx, p, q_dev, nq, k, nprobe, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    std::shared_lock<std::shared_mutex> pk(p->mu);
    MVDB_TRY(check_probe_state(idx, p, rs));
    DeviceGuard dg(idx->device);
    if (stream_capturing((hipStream_t)stream)) return fail(MVDB_ERR_ARG, "probed search cannot be captured into a hipGraph");
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises
    return probe_core(idx, call.ws, p, call.q, nq, k, nprobe, normalize_q, rs, label_offset, D_dev, I_dev);
}

int mvdb_index_probe_counters(const mvdb_index* idx, long long* calls, long long* probe_launches) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->pb_calls.load();
    if (probe_launches) *probe_launches = (long long)idx->pb_launches.load();
    return 0;
}

}  // extern "C"

// ---- search by examples: P positives and N negatives, a row scores by its nearest positive (examples_scan.hpp) -------------
namespace {

int check_examples_args(const mvdb_index* idx, const void* v, int P, int N, int k, const void* skip, int n_skip, const void* D, const void* I) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (!v || !D || !I) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    if (P < 1) return fail(MVDB_ERR_ARG, "search by examples needs at least one positive (got P = %d)", P);
    if (N < 0) return fail(MVDB_ERR_ARG, "search by examples needs N >= 0 (got %d)", N);
    if ((long long)P + N > kExamplesMaxVectors)
        return fail(MVDB_ERR_ARG, "search by examples needs P + N <= %d vectors (got %d + %d)", kExamplesMaxVectors, P, N);
    if (k < 1 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "search by examples needs 1 <= k <= %d (got %d)", kMaxFusedK, k);
    if (n_skip < 0 || n_skip > kExamplesMaxSkip) return fail(MVDB_ERR_ARG, "search by examples needs 0 <= n_skip <= %d (got %d)", kExamplesMaxSkip, n_skip);
    if (n_skip > 0 && !skip) return fail(MVDB_ERR_ARG, "NULL skip rows passed to search by examples");
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "search by examples needs an inner-product index");
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_examples_kern(const ExamplesScanArgs& a, int device, hipStream_t stream) {
    void (*kern)(ExamplesScanArgs) = examples_scan_kernel<G, C, U, SEL, MASKED>;
    constexpr int RB = (kWave / G) * U;
    const size_t lds = 4 * (size_t)a.Vp * (size_t)a.ld;
    if (lds > device_lds_per_block(device))
        return fail(MVDB_ERR_ARG, "search by examples: a pass needs %zu bytes of LDS, the device gives a workgroup %zu", lds, device_lds_per_block(device));
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    // assign's grid: two resident blocks of eight waves where the vectors leave room for them
    const int per_cu = std::min(cached_occupancy((const void*)kern, kMaxsimThreads, lds, 1), 2);
    const int64_t nbatches = (a.n + RB - 1) / RB;
    const int64_t want = (nbatches + kMaxsimWaves - 1) / kMaxsimWaves;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
    return profiled_launch("examples_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kMaxsimThreads), lds, stream, done, a); },
                           "examples_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// assign's forms, from the one shape table
int launch_examples(const ExamplesScanArgs& a, int device, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            return launch_examples_kern<S::G, S::C, maxsim_u(S::G, S::C), F::SEL, F::MASKED>(a, device, s);
        });
    });
}

// The P + N vectors on the device at stride ld, the skip rows on the device, results to device buffers: the clear, ceil((P + N)
// / Vp) passes over consecutive ranges of the vectors, the skip rows' words zeroed, the block lists, the merge that writes.
int examples_core(const mvdb_index* idx, Workspace* ws, const float* v, int P, int N, int k, int normalize, const mvdb_rowset* rs,
                  const int64_t* skip_dev, int n_skip, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    hipStream_t s = ws->stream;
    ++idx->ex_calls;
    const int64_t n = idx->n;
    ExamplesEmitArgs e;
    e.part = nullptr;
    e.nlists = 0;
    e.k = k;
    e.label_offset = label_offset;
    e.D = D_dev;
    e.I = I_dev;
    const int64_t m = rs ? rs->count : n;  // rows selected
    if (m > 0 && !(rs && rs->mask && rs->n_at_create == 0)) {
        const int nlists = (int)std::max<int64_t>(1, std::min<int64_t>((n + kDistinctThreads - 1) / kDistinctThreads, kExamplesLists));
        MVDB_TRY(ws->exbest.reserve((size_t)n));
        MVDB_TRY(ws->expart.reserve((size_t)nlists * kWave));
        // (the clear runs under the scan's label, as a record of its own: it names no symbol)
        MVDB_TRY(profiled_launch("examples_scan", s, [&](hipEvent_t done) { launch_kernel(examples_clear_kernel, dim3(utility_grid(n)), dim3(256), 0, s, done, ws->exbest.p, n); }));
        const int V = P + N;
        const int Vp = examples_vectors_per_pass(V, idx->ld, idx->kn.examples_vectors_per_pass);
        ExamplesScanArgs a;
        a.X = idx->X.p;
        a.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : n;
        a.ld = idx->ld;
        a.d4 = idx->d4;
        a.P = P;
        a.normalize_q = normalize;
        a.rows = rs ? rs->rows : nullptr;
        a.mask = rs ? rs->mask : nullptr;
        a.best = ws->exbest.p;
        for (int v0 = 0; v0 < V; v0 += Vp) {
            a.q = v + (int64_t)v0 * idx->ld;
            a.Vp = std::min(Vp, V - v0);
            a.v0 = v0;
            MVDB_TRY(launch_examples(a, idx->device, s));
            ++idx->ex_passes;
        }
        if (n_skip > 0) {
            hipLaunchKernelGGL(examples_skip_kernel, dim3((unsigned)((n_skip + 255) / 256)), dim3(256), 0, s, ws->exbest.p, n, skip_dev, n_skip);
            MVDB_HIP(hipGetLastError());
        }
        ExamplesTopkArgs t;
        t.best = ws->exbest.p;
        t.n = n;
        t.k = k;
        t.part = ws->expart.p;
        MVDB_TRY(profiled_launch("examples_select", s,
                                 [&](hipEvent_t done) { launch_kernel(examples_topk_kernel, dim3((unsigned)nlists), dim3(kDistinctThreads), 0, s, done, t); },
                                 "examples_topk_kernel"));
        e.part = ws->expart.p;
        e.nlists = nlists;
    }
    // (an empty index or an empty set: no lists, every output is padding)
    MVDB_TRY(profiled_launch("examples_select", s, [&](hipEvent_t done) { launch_kernel(examples_emit_kernel, dim3(1), dim3(kDistinctThreads), 0, s, done, e); }));
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_search_examples(const mvdb_index* idx, const float* v_host, int P, int N, int k, int normalize, const mvdb_rowset* rs,
                               const int64_t* skip_rows_host, int n_skip, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_examples_args(idx, v_host, P, N, k, skip_rows_host, n_skip, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    for (int i = 0; i < n_skip; ++i)
        if (skip_rows_host[i] < 0 || skip_rows_host[i] >= idx->n)
            return fail(MVDB_ERR_ARG, "search by examples: skip row %lld is outside [0, %lld)", (long long)skip_rows_host[i], (long long)idx->n);
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    // the vectors and, behind them in the same pinned staging buffer, the skip rows
    const size_t vbytes = (size_t)(P + N) * idx->ld * sizeof(float);
    MVDB_TRY(ws->pin.reserve(vbytes + (size_t)n_skip * sizeof(int64_t)));
    MVDB_TRY(call.stage(v_host, P + N));
    if (n_skip > 0) {
        MVDB_TRY(ws->exskip.reserve((size_t)n_skip));
        char* const st = (char*)ws->pin.p + vbytes;
        memcpy(st, skip_rows_host, (size_t)n_skip * sizeof(int64_t));
        MVDB_HIP(hipMemcpyAsync(ws->exskip.p, st, (size_t)n_skip * sizeof(int64_t), hipMemcpyHostToDevice, ws->stream));
    }
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results((size_t)k, &D_dev, &I_dev));
    MVDB_TRY(examples_core(idx, ws, ws->q.p, P, N, k, normalize, rs, ws->exskip.p, n_skip, 0, D_dev, I_dev));
    return call.fetch((size_t)k, D_host, I_host);
}

int mvdb_index_search_examples_device(const mvdb_index* idx, const float* v_dev, int P, int N, int k, int normalize, const mvdb_rowset* rs,
                                      const int64_t* skip_rows_dev, int n_skip, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                      void* stream) {
    MVDB_TRY(check_examples_args(idx, v_dev, P, N, k, skip_rows_dev, n_skip, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    if (stream_capturing((hipStream_t)stream)) return fail(MVDB_ERR_ARG, "search by examples cannot be captured into a hipGraph");
    StreamCall call(idx, stream, v_dev, P + N);
    MVDB_TRY(call.rc);
    // nothing below reads from the device or synchronises (skip rows outside [0, ntotal) are ignored by the kernel)
    return examples_core(idx, call.ws, call.q, P, N, k, normalize, rs, skip_rows_dev, n_skip, label_offset, D_dev, I_dev);
}

}  // extern "C"

// ---- boosted search: S = w_s * s + T[row], T from resident term columns and sparse entries (boost_scan.hpp) -----------------
struct mvdb_rowterm {
    uint64_t owner = 0;       // serial number of the index the column was built on
    int device = 0;
    int64_t n = 0;            // the index's row count it was built against: one value per row
    uint64_t renumbered = 0;  // ... and its renumbering generation
    float* values = nullptr;  // [n] on the device (none for an empty index)
};

namespace {

int rowterm_check(const mvdb_index* idx, const mvdb_rowterm* t, int j) {
    if (!t) return fail(MVDB_ERR_ARG, "boosted search: term %d is NULL", j);
    if (t->owner != idx->serial || t->device != idx->device) return fail(MVDB_ERR_ARG, "boosted search: term %d belongs to another index", j);
    // one value per stored row: rows added since have none, rows removed since have renumbered the rest (set_rows keeps the numbers)
    if (t->n != idx->n)
        return fail(MVDB_ERR_ARG, "boosted search: term %d holds %lld rows, the index %lld", j, (long long)t->n, (long long)idx->n);
    if (t->renumbered != idx->renumbered)
        return fail(MVDB_ERR_ARG, "boosted search: term %d was built before rows were removed (%lld rows then, %lld now)", j, (long long)t->n,
                    (long long)idx->n);
    return 0;
}

// the term, weight and sparse arguments every boosted entry point takes (the caller holds idx->mu shared)
int check_boost_terms(const mvdb_index* idx, const mvdb_rowterm* const* terms, const float* weights, int nterms, const int64_t* sparse_rows,
                      const float* sparse_values, int64_t nsparse, int nq) {
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "boosted search needs an inner-product index");
    if (nterms < 0 || nterms > kBoostMaxTerms) return fail(MVDB_ERR_ARG, "boosted search takes 0 to %d terms (got %d)", kBoostMaxTerms, nterms);
    if (nsparse < 0) return fail(MVDB_ERR_ARG, "boosted search: negative sparse count");
    if (nterms == 0 && nsparse == 0) return fail(MVDB_ERR_ARG, "boosted search has nothing to boost by: no term and no sparse entry");
    if (nterms > 0 && (!terms || !weights)) return fail(MVDB_ERR_ARG, "NULL terms or weights passed to boosted search");
    if (nsparse > 0 && (!sparse_rows || !sparse_values)) return fail(MVDB_ERR_ARG, "NULL sparse rows or values passed to boosted search");
    if (nsparse > 0 && nq != 1) return fail(MVDB_ERR_ARG, "boosted search: sparse entries belong to a single query (got nq = %d)", nq);
    for (int j = 0; j < nterms; ++j) MVDB_TRY(rowterm_check(idx, terms[j], j));
    if (nsparse > 0) {
        std::vector<int64_t> sorted(sparse_rows, sparse_rows + nsparse);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.front() < 0 || sorted.back() >= idx->n)
            return fail(MVDB_ERR_ARG, "boosted search: sparse row %lld is outside [0, %lld)", (long long)(sorted.front() < 0 ? sorted.front() : sorted.back()),
                        (long long)idx->n);
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return fail(MVDB_ERR_ARG, "boosted search: sparse row %lld is listed twice", (long long)*dup);
    }
    return 0;
}

// The sparse entries to the device through the workspace's pinned staging, `pin_off` bytes in (behind what the caller staged
// there).  The staging bytes are read when the copies run: the host entry points wait for their results anyway; the device
// entry point waits for the copies before it returns (boost_search_device).
int stage_boost_sparse(Workspace* ws, size_t pin_off, const int64_t* rows, const float* values, int64_t m) {
    MVDB_TRY(ws->bsrows.reserve((size_t)m));
    MVDB_TRY(ws->bsvals.reserve((size_t)m));
    MVDB_TRY(ws->pin.reserve(pin_off + (size_t)m * (sizeof(int64_t) + sizeof(float))));
    char* const st = (char*)ws->pin.p + pin_off;
    memcpy(st, rows, (size_t)m * sizeof(int64_t));
    memcpy(st + (size_t)m * sizeof(int64_t), values, (size_t)m * sizeof(float));
    MVDB_HIP(hipMemcpyAsync(ws->bsrows.p, st, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, ws->stream));
    MVDB_HIP(hipMemcpyAsync(ws->bsvals.p, st + (size_t)m * sizeof(int64_t), (size_t)m * sizeof(float), hipMemcpyHostToDevice, ws->stream));
    return 0;
}

// T into ws->bsT: the combine launch, then the scatter of the sparse entries (already on the device)
int boost_combine_core(const mvdb_index* idx, Workspace* ws, const mvdb_rowterm* const* terms, const float* weights, int nterms, int64_t nsparse) {
    const int64_t n = idx->n;
    if (n == 0) return 0;
    hipStream_t s = ws->stream;
    MVDB_TRY(ws->bsT.reserve((size_t)n));
    BoostCombineArgs c;
    for (int j = 0; j < kBoostMaxTerms; ++j) {
        c.t[j] = j < nterms ? terms[j]->values : nullptr;
        c.w[j] = j < nterms ? weights[j] : 0.f;
    }
    c.nterms = nterms;
    c.n = n;
    c.T = ws->bsT.p;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + 255) / 256, (int64_t)device_cus(idx->device) * 8));
    MVDB_TRY(profiled_launch("boost_combine", s, [&](hipEvent_t done) { launch_kernel(boost_combine_kernel, dim3(grid), dim3(256), 0, s, done, c); },
                             "boost_combine_kernel"));
    if (nsparse > 0)
        MVDB_TRY(profiled_launch("boost_combine", s, [&](hipEvent_t done) {
            launch_kernel(boost_scatter_kernel, dim3((unsigned)((nsparse + 255) / 256)), dim3(256), 0, s, done, ws->bsT.p, n, (const int64_t*)ws->bsrows.p,
                          (const float*)ws->bsvals.p, nsparse);
        }, "boost_scatter_kernel"));
    return 0;
}

template <int G, int C, int U, int SEL, bool MASKED>
int launch_boost_kern(const BoostScanArgs& a, int nq, int device, hipStream_t stream, int* nblocks_out) {
    void (*kern)(BoostScanArgs) = boost_scan_kernel<G, C, U, SEL, MASKED>;
    // the grid of the single-query scan (launch_scan_kern)
    const int nblocks = scan_grid(a.n, (kWave / G) * U, scan_resident_blocks((const void*)kern, C), device);
    *nblocks_out = nblocks;
    return profiled_launch("boost_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks, nq), dim3(kScanThreads), 0, stream, done, a); },
                           "boost_scan_kernel<%d, %d, %d, %d, %s>", G, C, U, SEL, MASKED ? "true" : "false");
}

// the shapes, forms and rows in flight of launch_scan
int launch_boost(const BoostScanArgs& a, int nq, int device, hipStream_t s, int* nblocks) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        return with_scan_form<S::G, S::C>(a.d4, a.rows != nullptr, a.mask != nullptr, [&](auto form) {
            using F = decltype(form);
            constexpr int U = F::SEL == 1 ? gather_u(S::G, S::C) : stream_u(S::G, S::C);
            return launch_boost_kern<S::G, S::C, U, F::SEL, F::MASKED>(a, nq, device, s, nblocks);
        });
    });
}

// The scan over ws->bsT, whoever wrote it (the combine above; the sparse scoring launch of hybrid search): per tile of kCoreTile
// queries ONE scan launch — the queries are the grid's y dimension — and the merge.  Something is selected.
int boost_scan_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int normalize_q, float score_weight, const mvdb_rowset* rs,
                    int64_t label_offset, float* D_dev, int64_t* I_dev) {
    hipStream_t s = ws->stream;
    const int64_t n = idx->n;
    const int tile = std::min(nq, kCoreTile);
    MVDB_TRY(ws->cand.reserve((size_t)tile * scan_grid_upper_bound(idx->device) * k));
    BoostScanArgs a;
    a.X = idx->X.p;
    a.n = rs ? (rs->mask ? rs->n_at_create : rs->count) : n;
    a.ld = idx->ld;
    a.d4 = idx->d4;
    a.normalize_q = normalize_q;
    a.k = k;
    a.rows = rs ? rs->rows : nullptr;
    a.mask = rs ? rs->mask : nullptr;
    a.T = ws->bsT.p;
    a.score_weight = score_weight;
    a.cand = ws->cand.p;
    for (int q0 = 0; q0 < nq; q0 += tile) {
        const int take = std::min(tile, nq - q0);
        a.q = q + (int64_t)q0 * idx->ld;
        int nblocks = 0;
        MVDB_TRY(launch_boost(a, take, idx->device, s, &nblocks));
        ++idx->bs_launches;
        MVDB_TRY(launch_merge(idx, ws, take, nblocks, k, label_offset, D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k));
    }
    return 0;
}

// Queries on the device at stride ld, the sparse entries on the device, results to device buffers: the combine (shared by the
// queries of the call), then boost_scan_core.
int boost_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int normalize_q, float score_weight,
               const mvdb_rowterm* const* terms, const float* weights, int nterms, int64_t nsparse, const mvdb_rowset* rs, int64_t label_offset,
               float* D_dev, int64_t* I_dev) {
    hipStream_t s = ws->stream;
    ++idx->bs_calls;
    const int64_t n = idx->n;
    const int64_t m = rs ? rs->count : n;  // rows selected
    const int64_t total = (int64_t)nq * k;
    if (m == 0 || (rs && rs->mask && rs->n_at_create == 0)) {  // an empty index or an empty set: every output is padding
        hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, D_dev, I_dev, total, idx->metric);
        MVDB_HIP(hipGetLastError());
        return 0;
    }
    MVDB_TRY(boost_combine_core(idx, ws, terms, weights, nterms, nsparse));
    return boost_scan_core(idx, ws, q, nq, k, normalize_q, score_weight, rs, label_offset, D_dev, I_dev);
}

int check_boost_args(const mvdb_index* idx, const void* q, int nq, int k, const void* D, const void* I) {
    MVDB_TRY(check_search_args(idx, q, nq, k, D, I));
    if (k > kMaxFusedK) return fail(MVDB_ERR_ARG, "boosted search needs 1 <= k <= %d (got %d)", kMaxFusedK, k);
    return 0;
}

}  // namespace

extern "C" {

int mvdb_rowterm_create(const mvdb_index* idx, const float* values_host, int64_t n, mvdb_rowterm** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (n > 0 && !values_host) return fail(MVDB_ERR_ARG, "values is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (n != idx->n) return fail(MVDB_ERR_ARG, "a row term needs one value per stored row (%lld values, %lld rows)", (long long)n, (long long)idx->n);
    DeviceGuard dg(idx->device);
    mvdb_rowterm* t = new mvdb_rowterm();
    t->owner = idx->serial;
    t->device = idx->device;
    t->n = n;
    t->renumbered = idx->renumbered;
    if (n > 0) {
        hipError_t e = hipMalloc((void**)&t->values, (size_t)n * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(t->values, values_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (t->values) (void)hipFree(t->values);
            delete t;
            return fail(MVDB_ERR_HIP, "row term upload failed: %s", hipGetErrorString(e));
        }
    }
    *out = t;
    return 0;
}

int64_t mvdb_rowterm_rows(const mvdb_rowterm* t) { return t ? t->n : -1; }

int mvdb_rowterm_free(mvdb_rowterm* t) {
    if (!t) return 0;
    if (t->values) {
        DeviceGuard dg(t->device);
        (void)hipFree(t->values);
    }
    delete t;
    return 0;
}

int mvdb_index_search_boosted(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q, float score_weight,
                              const mvdb_rowterm* const* terms, const float* weights, int nterms, const int64_t* sparse_rows_host,
                              const float* sparse_values_host, int64_t nsparse, const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_boost_args(idx, q_host, nq, k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_boost_terms(idx, terms, weights, nterms, sparse_rows_host, sparse_values_host, nsparse, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    // the queries and, behind them in the same pinned staging buffer, the sparse entries
    const size_t qbytes = (size_t)nq * idx->ld * sizeof(float);
    MVDB_TRY(ws->pin.reserve(qbytes + (size_t)nsparse * (sizeof(int64_t) + sizeof(float))));
    MVDB_TRY(call.stage(q_host, nq));
    if (nsparse > 0) MVDB_TRY(stage_boost_sparse(ws, qbytes, sparse_rows_host, sparse_values_host, nsparse));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(boost_core(idx, ws, ws->q.p, nq, k, normalize_q, score_weight, terms, weights, nterms, nsparse, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_boosted_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q, float score_weight,
                                     const mvdb_rowterm* const* terms, const float* weights, int nterms, const int64_t* sparse_rows_host,
                                     const float* sparse_values_host, int64_t nsparse, const mvdb_rowset* rs, int64_t label_offset,
                                     float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_boost_args(idx, q_dev, nq, k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_boost_terms(idx, terms, weights, nterms, sparse_rows_host, sparse_values_host, nsparse, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    if (stream_capturing((hipStream_t)stream)) return fail(MVDB_ERR_ARG, "boosted search cannot be captured into a hipGraph");
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    if (nsparse > 0) {
        // the one host wait of this entry point: the staging copy of the sparse entries belongs to the workspace, and the next
        // call on this stream may rewrite it — so the uploads have run before this call returns.  nsparse == 0: no wait at all.
        MVDB_TRY(stage_boost_sparse(call.ws, 0, sparse_rows_host, sparse_values_host, nsparse));
        MVDB_HIP(hipStreamSynchronize(call.ws->stream));
    }
    return boost_core(idx, call.ws, call.q, nq, k, normalize_q, score_weight, terms, weights, nterms, nsparse, rs, label_offset, D_dev, I_dev);
}

int mvdb_index_boost_combine(const mvdb_index* idx, const mvdb_rowterm* const* terms, const float* weights, int nterms,
                             const int64_t* sparse_rows_host, const float* sparse_values_host, int64_t nsparse, float* T_host) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_boost_terms(idx, terms, weights, nterms, sparse_rows_host, sparse_values_host, nsparse, 1));
    if (idx->n == 0) return 0;
    if (!T_host) return fail(MVDB_ERR_ARG, "T is NULL");
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    if (nsparse > 0) MVDB_TRY(stage_boost_sparse(ws, 0, sparse_rows_host, sparse_values_host, nsparse));
    MVDB_TRY(boost_combine_core(idx, ws, terms, weights, nterms, nsparse));
    MVDB_TRY(copy_back(ws, ws->bsT.p, (size_t)idx->n * sizeof(float), "boost combine"));
    memcpy(T_host, ws->pin_out.p, (size_t)idx->n * sizeof(float));
    return 0;
}

int mvdb_index_boost_counters(const mvdb_index* idx, long long* calls, long long* scan_launches) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->bs_calls.load();
    if (scan_launches) *scan_launches = (long long)idx->bs_launches.load();
    return 0;
}

}  // extern "C"

// ---- sparse vectors: a CSR pass scores every stored sparse row against a sparse query; hybrid = that column, then the boosted scan (sparse_scan.hpp) ----
struct mvdb_sparse {
    uint64_t owner = 0;       // serial number of the index the store was built on
    int device = 0;
    int64_t n = 0;            // the index's row count it was built against: one sparse vector per row
    uint64_t renumbered = 0;  // ... and its renumbering generation
    int64_t dim = 0, nnz = 0, ntiles = 0;
    SparseEntry* entries = nullptr;  // [nnz + 2] on the device
    int64_t* indptr = nullptr;       // [n + 1]
    int64_t* tiles = nullptr;        // [2 (ntiles + 1)]: the tiles' first rows, then their first entries
    // the inverted form (sparse_postings.hpp), built on request: mvdb_sparse_build_postings
    bool has_post = false;
    PostEntry* post = nullptr;           // [nnz + 2] on the device
    int64_t* post_ptr = nullptr;         // [dim + 1]
    std::vector<int64_t> post_ptr_host;  // its host copy: absent terms are dropped and touched entries counted on the host
};

namespace {

int sparse_check(const mvdb_index* idx, const mvdb_sparse* sp) {
    if (!sp) return fail(MVDB_ERR_ARG, "sparse search: the sparse store is NULL");
    if (sp->owner != idx->serial || sp->device != idx->device) return fail(MVDB_ERR_ARG, "sparse search: the sparse store belongs to another index");
    if (sp->n != idx->n) return fail(MVDB_ERR_ARG, "sparse search: the sparse store holds %lld rows, the index %lld", (long long)sp->n, (long long)idx->n);
    if (sp->renumbered != idx->renumbered)
        return fail(MVDB_ERR_ARG, "sparse search: the sparse store was built before rows were removed (%lld rows then, %lld now)", (long long)sp->n,
                    (long long)idx->n);
    return 0;
}

// the queries of a call: offsets from 0, 1 .. kSparseMaxQuery distinct indices inside [0, dim) each
int check_sparse_queries(const mvdb_sparse* sp, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq) {
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (!q_indptr) return fail(MVDB_ERR_ARG, "NULL sparse query passed to sparse search");
    if (q_indptr[0] != 0) return fail(MVDB_ERR_ARG, "sparse query: the offsets start at %lld, not 0", (long long)q_indptr[0]);
    for (int i = 0; i < nq; ++i) {
        const int64_t m = q_indptr[i + 1] - q_indptr[i];
        if (m < 1 || m > kSparseMaxQuery)
            return fail(MVDB_ERR_ARG, "sparse query %d holds %lld terms: a query needs 1 to %d", i, (long long)m, kSparseMaxQuery);
    }
    if (!q_indices || !q_values) return fail(MVDB_ERR_ARG, "NULL sparse query passed to sparse search");
    std::vector<int32_t> sorted;
    for (int i = 0; i < nq; ++i) {
        sorted.assign(q_indices + q_indptr[i], q_indices + q_indptr[i + 1]);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.front() < 0 || sorted.back() >= sp->dim)
            return fail(MVDB_ERR_ARG, "sparse query %d: index %lld is outside [0, %lld)", i, (long long)(sorted.front() < 0 ? sorted.front() : sorted.back()),
                        (long long)sp->dim);
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return fail(MVDB_ERR_ARG, "sparse query %d: index %lld is listed twice", i, (long long)*dup);
    }
    return 0;
}

// The queries to ws->spq through the pinned staging, `pin_off` bytes in (a multiple of 8; the caller has reserved the staging
// buffer): [nq + 1] offsets, then the packed terms.  The staging bytes are read when the copy runs (stage_boost_sparse).
size_t sparse_query_bytes(const int64_t* q_indptr, int nq) { return (size_t)(nq + 1 + q_indptr[nq]) * sizeof(uint64_t); }
int stage_sparse_queries(Workspace* ws, size_t pin_off, const int64_t* q_indptr, const int32_t* q_indices, const float* q_values, int nq) {
    const int64_t M = q_indptr[nq];
    const size_t words = (size_t)(nq + 1 + M);
    MVDB_TRY(ws->spq.reserve(words));
    MVDB_TRY(ws->pin.reserve(pin_off + words * sizeof(uint64_t)));
    char* const st = (char*)ws->pin.p + pin_off;
    memcpy(st, q_indptr, (size_t)(nq + 1) * sizeof(int64_t));
    SparseEntry* const e = reinterpret_cast<SparseEntry*>(st + (size_t)(nq + 1) * sizeof(int64_t));
    for (int64_t i = 0; i < M; ++i) {
        e[i].index = (uint32_t)q_indices[i];
        memcpy(&e[i].value, q_values + i, sizeof(float));
    }
    MVDB_HIP(hipMemcpyAsync(ws->spq.p, st, words * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
    return 0;
}

// the rows a sparse launch may offer: NULL (every row) or a bitmap over the rows [0, *mask_rows) — the set's own, its twin, or
// the row list turned into one in the workspace
int sparse_selector(const mvdb_index* idx, Workspace* ws, const mvdb_rowset* rs, const uint64_t** mask, int64_t* mask_rows) {
    *mask = nullptr;
    *mask_rows = 0;
    if (!rs) return 0;
    *mask_rows = rs->n_at_create;
    if (rs->mask || rs->twin) {
        *mask = rs->mask ? rs->mask : rs->twin;
        return 0;
    }
    const size_t words = (size_t)((rs->n_at_create + 63) / 64);
    MVDB_TRY(ws->spmask.reserve(words));
    MVDB_HIP(hipMemsetAsync(ws->spmask.p, 0, words * sizeof(uint64_t), ws->stream));
    hipLaunchKernelGGL(rows_to_mask_kernel, dim3((unsigned)((rs->count + 255) / 256)), dim3(256), 0, ws->stream, (const int64_t*)rs->rows, rs->count,
                       rs->n_at_create, (unsigned long long*)ws->spmask.p);
    MVDB_HIP(hipGetLastError());
    *mask = ws->spmask.p;
    return 0;
}

SparseScanArgs sparse_args(const mvdb_sparse* sp, Workspace* ws, int nq) {
    SparseScanArgs a{};
    a.entries = sp->entries;
    a.indptr = sp->indptr;
    a.tile_row = sp->tiles;
    a.tile_ent = sp->tiles + sp->ntiles + 1;
    a.ntiles = sp->ntiles;
    a.q_indptr = reinterpret_cast<const int64_t*>(ws->spq.p);
    a.q_terms = reinterpret_cast<const SparseEntry*>(ws->spq.p + nq + 1);
    a.weight = 1.0f;
    return a;
}

int sparse_grid(const mvdb_index* idx, const mvdb_sparse* sp) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(sp->ntiles, (int64_t)device_cus(idx->device) * kSparseBlocksPerCu));
}

// ---- the posting route (sparse_postings.hpp): a store that has postings, unless the index option sparse_postings is 0 ----
bool by_postings(const mvdb_index* idx, const mvdb_sparse* sp) { return sp->has_post && idx->kn.sparse_postings != 0; }

// The queries in the posting route's form to ws->spq, through the pinned staging as stage_sparse_queries: [nq + 1] term offsets,
// then per query its terms in ascending index order as (list begin, list end, index, value) — a term whose list is empty is
// dropped here, from the host directory, so a query may keep no term at all.  Counts the list entries of the kept terms.
size_t posting_query_bytes(const int64_t* q_indptr, int nq) { return (size_t)(nq + 1 + 3 * q_indptr[nq]) * sizeof(uint64_t); }
int stage_posting_queries(const mvdb_index* idx, const mvdb_sparse* sp, Workspace* ws, size_t pin_off, const int64_t* q_indptr, const int32_t* q_indices,
                          const float* q_values, int nq) {
    const int64_t M = q_indptr[nq];
    const size_t words = (size_t)(nq + 1 + 3 * M);
    MVDB_TRY(ws->spq.reserve(words));
    MVDB_TRY(ws->pin.reserve(pin_off + words * sizeof(uint64_t)));
    char* const st = (char*)ws->pin.p + pin_off;
    int64_t* const off = reinterpret_cast<int64_t*>(st);
    PostTerm* const terms = reinterpret_cast<PostTerm*>(st + (size_t)(nq + 1) * sizeof(int64_t));
    std::vector<std::pair<int32_t, int64_t>> order;  // (index, position in the caller's arrays)
    int64_t kept = 0;
    unsigned long long entries = 0;
    off[0] = 0;
    for (int i = 0; i < nq; ++i) {
        order.clear();
        for (int64_t j = q_indptr[i]; j < q_indptr[i + 1]; ++j) order.emplace_back(q_indices[j], j);
        std::sort(order.begin(), order.end());
        for (const auto& o : order) {
            const int64_t b = sp->post_ptr_host[(size_t)o.first], e = sp->post_ptr_host[(size_t)o.first + 1];
            if (b == e) continue;
            PostTerm& t = terms[kept++];
            t.begin = b;
            t.end = e;
            t.index = (uint32_t)o.first;
            memcpy(&t.value, q_values + o.second, sizeof(float));
            entries += (unsigned long long)(e - b);
        }
        off[i + 1] = kept;
    }
    idx->pp_entries += entries;
    MVDB_HIP(hipMemcpyAsync(ws->spq.p, st, (size_t)(nq + 1 + 3 * kept) * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
    return 0;
}

// the queries of a call in the form of the route that will score them
size_t routed_query_bytes(const mvdb_index* idx, const mvdb_sparse* sp, const int64_t* q_indptr, int nq) {
    return by_postings(idx, sp) ? posting_query_bytes(q_indptr, nq) : sparse_query_bytes(q_indptr, nq);
}
int stage_routed_queries(const mvdb_index* idx, const mvdb_sparse* sp, Workspace* ws, size_t pin_off, const int64_t* q_indptr, const int32_t* q_indices,
                         const float* q_values, int nq) {
    if (by_postings(idx, sp)) return stage_posting_queries(idx, sp, ws, pin_off, q_indptr, q_indices, q_values, nq);
    return stage_sparse_queries(ws, pin_off, q_indptr, q_indices, q_values, nq);
}

PostingsArgs postings_args(const mvdb_sparse* sp, Workspace* ws, int nq) {
    PostingsArgs a{};
    a.post = sp->post;
    a.n = sp->n;
    a.nblocks = (sp->n + kPostBlockRows - 1) / kPostBlockRows;
    a.q_off = reinterpret_cast<const int64_t*>(ws->spq.p);
    a.q_terms = reinterpret_cast<const PostTerm*>(ws->spq.p + nq + 1);
    a.weight = 1.0f;
    return a;
}

int postings_grid(const mvdb_index* idx, const PostingsArgs& a) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(a.nblocks, (int64_t)device_cus(idx->device) * kPostBlocksPerCu));
}

// the scoring launch: T[r] = weight * sparse(r) of query `query` of the staged call, for every row (and matched[r], if asked)
int sparse_column(const mvdb_index* idx, const mvdb_sparse* sp, Workspace* ws, int nq_staged, int query, float weight, float* T, int32_t* matched) {
    if (by_postings(idx, sp)) {
        PostingsArgs a = postings_args(sp, ws, nq_staged);
        a.q_off += query;
        a.weight = weight;
        a.T = T;
        a.matched = matched;
        hipStream_t s = ws->stream;
        ++idx->pp_launches;
        return profiled_launch("sparse_postings", s, [&](hipEvent_t done) {
            launch_kernel(sparse_postings_kernel<0, 0>, dim3(postings_grid(idx, a)), dim3(kPostThreads), 0, s, done, a);
        }, "sparse_postings_kernel<0, 0>");
    }
    SparseScanArgs a = sparse_args(sp, ws, nq_staged);
    a.q_indptr += query;
    a.weight = weight;
    a.T = T;
    a.matched = matched;
    hipStream_t s = ws->stream;
    ++idx->sp_launches;
    return profiled_launch("sparse_scan", s, [&](hipEvent_t done) {
        launch_kernel(sparse_scan_kernel<0, 0>, dim3(sparse_grid(idx, sp)), dim3(kSparseThreads), 0, s, done, a);
    }, "sparse_scan_kernel<0, 0>");
}

bool nothing_selected(const mvdb_index* idx, const mvdb_rowset* rs) {
    return (rs ? rs->count : idx->n) == 0 || (rs && rs->mask && rs->n_at_create == 0);
}

int fill_padding(Workspace* ws, float* D_dev, int64_t* I_dev, int64_t total) {
    hipLaunchKernelGGL(fill_missing_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ws->stream, D_dev, I_dev, total, (int)MVDB_METRIC_IP);
    MVDB_HIP(hipGetLastError());
    return 0;
}

// the staged queries against the store: one top-k launch per kCoreTile queries (the grid's y) and the merge of its block lists
int sparse_search_core(const mvdb_index* idx, const mvdb_sparse* sp, Workspace* ws, int nq, int k, const mvdb_rowset* rs, int64_t label_offset,
                       float* D_dev, int64_t* I_dev) {
    ++idx->sp_calls;
    if (nothing_selected(idx, rs)) return fill_padding(ws, D_dev, I_dev, (int64_t)nq * k);
    hipStream_t s = ws->stream;
    if (by_postings(idx, sp)) {
        ++idx->pp_calls;
        PostingsArgs a = postings_args(sp, ws, nq);
        MVDB_TRY(sparse_selector(idx, ws, rs, &a.mask, &a.mask_rows));
        const int grid = postings_grid(idx, a);
        const int tile = std::min(nq, kCoreTile);
        MVDB_TRY(ws->cand.reserve((size_t)tile * grid * k));
        a.k = k;
        a.cand = ws->cand.p;
        for (int q0 = 0; q0 < nq; q0 += tile) {
            const int take = std::min(tile, nq - q0);
            PostingsArgs b = a;
            b.q_off += q0;
            ++idx->pp_launches;
            if (a.mask)
                MVDB_TRY(profiled_launch("sparse_postings", s, [&](hipEvent_t done) {
                    launch_kernel(sparse_postings_kernel<1, 2>, dim3(grid, take), dim3(kPostThreads), 0, s, done, b);
                }, "sparse_postings_kernel<1, 2>"));
            else
                MVDB_TRY(profiled_launch("sparse_postings", s, [&](hipEvent_t done) {
                    launch_kernel(sparse_postings_kernel<1, 0>, dim3(grid, take), dim3(kPostThreads), 0, s, done, b);
                }, "sparse_postings_kernel<1, 0>"));
            MergeArgs mg;   // the scores are similarities whatever the index's metric
            mg.keys = ws->cand.p;
            mg.nlists = grid;
            mg.k = k;
            mg.metric = MVDB_METRIC_IP;
            mg.label_offset = label_offset;
            mg.D = D_dev + (int64_t)q0 * k;
            mg.I = I_dev + (int64_t)q0 * k;
            hipLaunchKernelGGL(merge_keys_kernel, dim3(take), dim3(kMergeThreads), 0, s, mg);
            MVDB_HIP(hipGetLastError());
        }
        return 0;
    }
    SparseScanArgs a = sparse_args(sp, ws, nq);
    MVDB_TRY(sparse_selector(idx, ws, rs, &a.mask, &a.mask_rows));
    const int grid = sparse_grid(idx, sp);
    const int tile = std::min(nq, kCoreTile);
    MVDB_TRY(ws->cand.reserve((size_t)tile * grid * k));
    a.k = k;
    a.cand = ws->cand.p;
    for (int q0 = 0; q0 < nq; q0 += tile) {
        const int take = std::min(tile, nq - q0);
        SparseScanArgs b = a;
        b.q_indptr += q0;
        ++idx->sp_launches;
        if (a.mask)
            MVDB_TRY(profiled_launch("sparse_scan", s, [&](hipEvent_t done) {
                launch_kernel(sparse_scan_kernel<1, 2>, dim3(grid, take), dim3(kSparseThreads), 0, s, done, b);
            }, "sparse_scan_kernel<1, 2>"));
        else
            MVDB_TRY(profiled_launch("sparse_scan", s, [&](hipEvent_t done) {
                launch_kernel(sparse_scan_kernel<1, 0>, dim3(grid, take), dim3(kSparseThreads), 0, s, done, b);
            }, "sparse_scan_kernel<1, 0>"));
        MergeArgs mg;   // the scores are similarities whatever the index's metric
        mg.keys = ws->cand.p;
        mg.nlists = grid;
        mg.k = k;
        mg.metric = MVDB_METRIC_IP;
        mg.label_offset = label_offset;
        mg.D = D_dev + (int64_t)q0 * k;
        mg.I = I_dev + (int64_t)q0 * k;
        hipLaunchKernelGGL(merge_keys_kernel, dim3(take), dim3(kMergeThreads), 0, s, mg);
        MVDB_HIP(hipGetLastError());
    }
    return 0;
}

// hybrid: per query the scoring launch writes T = sparse_weight * sparse into the boosted search's column, then its scan and merge
int hybrid_core(const mvdb_index* idx, const mvdb_sparse* sp, Workspace* ws, const float* q, int nq, int k, int normalize_q, float dense_weight,
                float sparse_weight, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    ++idx->sp_calls;
    if (nothing_selected(idx, rs)) return fill_padding(ws, D_dev, I_dev, (int64_t)nq * k);
    if (by_postings(idx, sp)) ++idx->pp_calls;
    MVDB_TRY(ws->bsT.reserve((size_t)idx->n));
    for (int i = 0; i < nq; ++i) {
        MVDB_TRY(sparse_column(idx, sp, ws, nq, i, sparse_weight, ws->bsT.p, nullptr));
        MVDB_TRY(boost_scan_core(idx, ws, q + (int64_t)i * idx->ld, 1, k, normalize_q, dense_weight, rs, label_offset, D_dev + (int64_t)i * k,
                                 I_dev + (int64_t)i * k));
    }
    return 0;
}

int check_sparse_k(int k) {
    if (k < 1 || k > kMaxFusedK) return fail(MVDB_ERR_ARG, "sparse search needs 1 <= k <= %d (got %d)", kMaxFusedK, k);
    return 0;
}

template <typename T>
hipError_t upload_new(T** dst, const T* src, size_t count) {
    hipError_t e = hipMalloc((void**)dst, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess && count) e = hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// a device entry point's workspace without dense queries (StreamCall pads queries)
struct SparseStreamCall {
    Workspace* const ws;
    std::unique_lock<std::mutex> use;
    RetireScope keep;
    SparseStreamCall(const mvdb_index* idx, void* stream)
        : ws(idx->for_stream((hipStream_t)stream)),
          use(ws ? std::unique_lock<std::mutex>(ws->use_mu) : std::unique_lock<std::mutex>()),
          keep(ws && note_capture(ws) ? &ws->retired : nullptr) {}
};

}  // namespace

extern "C" {

int mvdb_sparse_create(const mvdb_index* idx, const int64_t* indptr_host, const int32_t* indices_host, const float* values_host, int64_t n, int64_t dim,
                       mvdb_sparse** out) {
    if (!out) return fail(MVDB_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (n < 0) return fail(MVDB_ERR_ARG, "negative row count");
    if (dim < 1 || dim > 2147483647ll) return fail(MVDB_ERR_ARG, "sparse store: dim must be in [1, 2^31 - 1] (got %lld)", (long long)dim);
    if (!indptr_host) return fail(MVDB_ERR_ARG, "indptr is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (n != idx->n)
        return fail(MVDB_ERR_ARG, "a sparse store needs one sparse vector per stored row (%lld vectors, %lld rows)", (long long)n, (long long)idx->n);
    if (indptr_host[0] != 0) return fail(MVDB_ERR_ARG, "sparse store: indptr starts at %lld, not 0", (long long)indptr_host[0]);
    for (int64_t r = 0; r < n; ++r)
        if (indptr_host[r + 1] < indptr_host[r]) return fail(MVDB_ERR_ARG, "sparse store: indptr decreases at row %lld", (long long)r);
    const int64_t nnz = indptr_host[n];
    if (nnz > 0 && (!indices_host || !values_host)) return fail(MVDB_ERR_ARG, "indices or values is NULL");
    for (int64_t r = 0; r < n; ++r)
        for (int64_t i = indptr_host[r]; i < indptr_host[r + 1]; ++i) {
            if (indices_host[i] < 0 || indices_host[i] >= dim)
                return fail(MVDB_ERR_ARG, "sparse store: row %lld holds index %lld outside [0, %lld)", (long long)r, (long long)indices_host[i], (long long)dim);
            if (i > indptr_host[r] && indices_host[i] <= indices_host[i - 1])
                return fail(MVDB_ERR_ARG, "sparse store: the indices of row %lld are not strictly ascending", (long long)r);
        }
    // the tiles: consecutive rows, at most kSparseSpan entries and kSparseTileRows rows; a longer row alone
    std::vector<int64_t> tile_row, tile_ent;
    for (int64_t r = 0; r < n;) {
        tile_row.push_back(r);
        tile_ent.push_back(indptr_host[r]);
        const int64_t e0 = indptr_host[r];
        int64_t end = r + 1;
        while (end < n && end - r < kSparseTileRows && indptr_host[end + 1] - e0 <= kSparseSpan) ++end;
        r = end;
    }
    const int64_t ntiles = (int64_t)tile_row.size();
    tile_row.push_back(n);
    tile_ent.push_back(nnz);
    tile_row.insert(tile_row.end(), tile_ent.begin(), tile_ent.end());
    DeviceGuard dg(idx->device);
    mvdb_sparse* sp = new mvdb_sparse();
    sp->owner = idx->serial;
    sp->device = idx->device;
    sp->n = n;
    sp->renumbered = idx->renumbered;
    sp->dim = dim;
    sp->nnz = nnz;
    sp->ntiles = ntiles;
    hipError_t e = upload_new(&sp->indptr, indptr_host, (size_t)n + 1);
    if (e == hipSuccess) e = upload_new(&sp->tiles, tile_row.data(), tile_row.size());
    if (e == hipSuccess) e = hipMalloc((void**)&sp->entries, (size_t)(nnz + 2) * sizeof(SparseEntry));
    // the entries, interleaved, a chunk at a time; behind them the two padding entries
    const int64_t chunk = 1 << 22;
    std::vector<SparseEntry> buf((size_t)std::min<int64_t>(chunk, nnz + 2));
    for (int64_t c = 0; e == hipSuccess && c < nnz + 2; c += chunk) {
        const int64_t take = std::min(chunk, nnz + 2 - c);
        for (int64_t i = 0; i < take; ++i) {
            if (c + i < nnz) {
                buf[i].index = (uint32_t)indices_host[c + i];
                memcpy(&buf[i].value, values_host + c + i, sizeof(float));
            } else {
                buf[i] = SparseEntry{kSparsePadIndex, 0u};
            }
        }
        e = hipMemcpy(sp->entries + c, buf.data(), (size_t)take * sizeof(SparseEntry), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        (void)mvdb_sparse_free(sp);
        return fail(MVDB_ERR_HIP, "sparse store upload failed: %s", hipGetErrorString(e));
    }
    *out = sp;
    return 0;
}

int64_t mvdb_sparse_rows(const mvdb_sparse* sp) { return sp ? sp->n : -1; }
int64_t mvdb_sparse_nnz(const mvdb_sparse* sp) { return sp ? sp->nnz : -1; }
int64_t mvdb_sparse_dim(const mvdb_sparse* sp) { return sp ? sp->dim : -1; }

int mvdb_sparse_free(mvdb_sparse* sp) {
    if (!sp) return 0;
    {
        DeviceGuard dg(sp->device);
        if (sp->entries) (void)hipFree(sp->entries);
        if (sp->indptr) (void)hipFree(sp->indptr);
        if (sp->tiles) (void)hipFree(sp->tiles);
        if (sp->post) (void)hipFree(sp->post);
        if (sp->post_ptr) (void)hipFree(sp->post_ptr);
    }
    delete sp;
    return 0;
}

int mvdb_sparse_geometry(int* span_entries, int* tile_rows, int* table_slots) {
    if (span_entries) *span_entries = kSparseSpan;
    if (tile_rows) *tile_rows = kSparseTileRows;
    if (table_slots) *table_slots = kSparseSlots;
    return 0;
}

int mvdb_sparse_postings_geometry(int* block_rows, int* sort_lds_entries, long long* max_dim) {
    if (block_rows) *block_rows = kPostBlockRows;
    if (sort_lds_entries) *sort_lds_entries = kPostSortSeg;
    if (max_dim) *max_dim = (long long)kPostMaxDim;
    return 0;
}

int mvdb_sparse_drop_postings(mvdb_sparse* sp) {
    if (!sp) return fail(MVDB_ERR_ARG, "the sparse store is NULL");
    DeviceGuard dg(sp->device);
    sp->has_post = false;
    if (sp->post) (void)hipFree(sp->post);
    if (sp->post_ptr) (void)hipFree(sp->post_ptr);
    sp->post = nullptr;
    sp->post_ptr = nullptr;
    std::vector<int64_t>().swap(sp->post_ptr_host);
    return 0;
}

int mvdb_sparse_has_postings(const mvdb_sparse* sp) { return sp && sp->has_post ? 1 : 0; }

int mvdb_sparse_build_postings(const mvdb_index* idx, mvdb_sparse* sp) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(sparse_check(idx, sp));
    if (sp->n >= (1ll << 32)) return fail(MVDB_ERR_ARG, "sparse postings: %lld rows, a posting holds its row in 32 bits", (long long)sp->n);
    if (sp->dim > kPostMaxDim)
        return fail(MVDB_ERR_ARG, "sparse postings: dim %lld is above %lld (the directory takes 8 (dim + 1) bytes): create the store with a smaller dim",
                    (long long)sp->dim, (long long)kPostMaxDim);
    DeviceGuard dg(idx->device);
    MVDB_TRY(mvdb_sparse_drop_postings(sp));
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    hipStream_t s = call.ws->stream;
    const int64_t nnz = sp->nnz, dim = sp->dim;
    int bits = 0;
    while (bits < 32 && ((dim - 1) >> bits) != 0) ++bits;
    const int passes = std::max(1, (bits + kPostRadixBits - 1) / kPostRadixBits);
    const int64_t nseg = (nnz + kPostSortSeg - 1) / kPostSortSeg;
    const int64_t N = nseg * kPostRadixDigits;
    const int64_t nb = (N + kPostScanChunk - 1) / kPostScanChunk;
    // what the build needs and frees again: both key arrays, the second payload array, the digit table and its block sums
    DevBuf<uint32_t> keys[2];
    DevBuf<uint64_t> pay_tmp;
    DevBuf<int64_t> table, sums;
    const auto build = [&]() -> int {
        MVDB_HIP(hipMalloc((void**)&sp->post, (size_t)(nnz + 2) * sizeof(PostEntry)));
        MVDB_HIP(hipMalloc((void**)&sp->post_ptr, (size_t)(dim + 1) * sizeof(int64_t)));
        MVDB_HIP(hipMemsetAsync(sp->post + nnz, 0xFF, 2 * sizeof(PostEntry), s));   // the padding: row kPostPadRow
        if (nnz > 0) {
            MVDB_TRY(keys[0].reserve((size_t)nnz));
            MVDB_TRY(keys[1].reserve((size_t)nnz));
            MVDB_TRY(pay_tmp.reserve((size_t)nnz));
            MVDB_TRY(table.reserve((size_t)N));
            MVDB_TRY(sums.reserve((size_t)nb));
            // the last pass must land in sp->post: an odd number of passes starts from the other payload array
            PostEntry* pay[2] = {sp->post, reinterpret_cast<PostEntry*>(pay_tmp.p)};
            int src = passes & 1;
            hipLaunchKernelGGL(postings_expand_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, (const SparseEntry*)sp->entries,
                               (const int64_t*)sp->indptr, sp->n, nnz, keys[src].p, pay[src]);
            MVDB_HIP(hipGetLastError());
            const unsigned seg_blocks = (unsigned)((nseg + kPostWaves - 1) / kPostWaves);
            for (int p = 0; p < passes; ++p, src ^= 1) {
                const int shift = p * kPostRadixBits;
                hipLaunchKernelGGL(postings_hist_kernel, dim3(seg_blocks), dim3(kPostThreads), 0, s, (const uint32_t*)keys[src].p, nnz, shift, nseg, table.p);
                hipLaunchKernelGGL(postings_scan_sums_kernel, dim3((unsigned)nb), dim3(kPostThreads), 0, s, (const int64_t*)table.p, N, sums.p);
                hipLaunchKernelGGL(postings_scan_top_kernel, dim3(1), dim3(kPostThreads), 0, s, sums.p, nb);
                hipLaunchKernelGGL(postings_scan_apply_kernel, dim3((unsigned)nb), dim3(kPostThreads), 0, s, table.p, N, (const int64_t*)sums.p);
                hipLaunchKernelGGL(postings_scatter_kernel, dim3(seg_blocks), dim3(kPostThreads), 0, s, (const uint32_t*)keys[src].p,
                                   (const PostEntry*)pay[src], keys[src ^ 1].p, pay[src ^ 1], nnz, shift, nseg, (const int64_t*)table.p);
                MVDB_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(postings_directory_kernel, dim3((unsigned)((dim + 1 + 255) / 256)), dim3(256), 0, s, (const uint32_t*)keys[src].p, nnz, dim,
                               sp->post_ptr);
            MVDB_HIP(hipGetLastError());
        } else {
            MVDB_HIP(hipMemsetAsync(sp->post_ptr, 0, (size_t)(dim + 1) * sizeof(int64_t), s));
        }
        sp->post_ptr_host.resize((size_t)dim + 1);
        MVDB_HIP(hipMemcpyAsync(sp->post_ptr_host.data(), sp->post_ptr, (size_t)(dim + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        MVDB_HIP(hipStreamSynchronize(s));   // the one wait of the build: the host directory is read from here on, the temporaries go
        return 0;
    };
    const int rc = profiled_launch("sparse_postings_build", s, build);
    if (rc != 0) {
        (void)hipStreamSynchronize(s);
        (void)mvdb_sparse_drop_postings(sp);
        return rc;
    }
    sp->has_post = true;
    return 0;
}

int mvdb_sparse_postings_read(const mvdb_sparse* sp, int64_t* post_ptr_host, uint32_t* rows_host, float* values_host) {
    if (!sp) return fail(MVDB_ERR_ARG, "the sparse store is NULL");
    if (!sp->has_post) return fail(MVDB_ERR_ARG, "the sparse store has no postings (mvdb_sparse_build_postings)");
    if (post_ptr_host) memcpy(post_ptr_host, sp->post_ptr_host.data(), sp->post_ptr_host.size() * sizeof(int64_t));
    if ((rows_host || values_host) && sp->nnz > 0) {
        DeviceGuard dg(sp->device);
        std::vector<PostEntry> buf((size_t)sp->nnz);
        MVDB_HIP(hipMemcpy(buf.data(), sp->post, buf.size() * sizeof(PostEntry), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < buf.size(); ++i) {
            if (rows_host) rows_host[i] = buf[i].row;
            if (values_host) memcpy(values_host + i, &buf[i].value, sizeof(float));
        }
    }
    return 0;
}

int mvdb_index_sparse_postings_counters(const mvdb_index* idx, long long* calls, long long* launches, long long* entries) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->pp_calls.load();
    if (launches) *launches = (long long)idx->pp_launches.load();
    if (entries) *entries = (long long)idx->pp_entries.load();
    return 0;
}

int mvdb_index_sparse_scores(const mvdb_index* idx, const mvdb_sparse* sp, const int32_t* q_indices_host, const float* q_values_host, int m,
                             float* T_host, int32_t* matched_host) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(sparse_check(idx, sp));
    const int64_t q_indptr[2] = {0, m};
    MVDB_TRY(check_sparse_queries(sp, q_indptr, q_indices_host, q_values_host, 1));
    const int64_t n = idx->n;
    if (n == 0) return 0;
    if (!T_host) return fail(MVDB_ERR_ARG, "T is NULL");
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    MVDB_TRY(stage_routed_queries(idx, sp, ws, 0, q_indptr, q_indices_host, q_values_host, 1));
    MVDB_TRY(ws->bsT.reserve((size_t)n));
    if (matched_host) MVDB_TRY(ws->spmatched.reserve((size_t)n));
    MVDB_TRY(sparse_column(idx, sp, ws, 1, 0, 1.0f, ws->bsT.p, matched_host ? ws->spmatched.p : nullptr));
    MVDB_TRY(copy_back(ws, ws->bsT.p, (size_t)n * sizeof(float), "sparse scores"));
    memcpy(T_host, ws->pin_out.p, (size_t)n * sizeof(float));
    if (matched_host) {
        MVDB_TRY(copy_back(ws, ws->spmatched.p, (size_t)n * sizeof(int32_t), "sparse scores"));
        memcpy(matched_host, ws->pin_out.p, (size_t)n * sizeof(int32_t));
    }
    return 0;
}

int mvdb_index_search_sparse(const mvdb_index* idx, const mvdb_sparse* sp, const int64_t* q_indptr_host, const int32_t* q_indices_host,
                             const float* q_values_host, int nq, int k, const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    MVDB_TRY(check_sparse_k(k));
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (!D_host || !I_host) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(sparse_check(idx, sp));
    MVDB_TRY(check_sparse_queries(sp, q_indptr_host, q_indices_host, q_values_host, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(stage_routed_queries(idx, sp, call.ws, 0, q_indptr_host, q_indices_host, q_values_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(sparse_search_core(idx, sp, call.ws, nq, k, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_sparse_device(const mvdb_index* idx, const mvdb_sparse* sp, const int64_t* q_indptr_host, const int32_t* q_indices_host,
                                    const float* q_values_host, int nq, int k, const mvdb_rowset* rs, int64_t label_offset, float* D_dev,
                                    int64_t* I_dev, void* stream) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    MVDB_TRY(check_sparse_k(k));
    if (nq <= 0) return fail(MVDB_ERR_ARG, "nq must be positive (got %d)", nq);
    if (!D_dev || !I_dev) return fail(MVDB_ERR_ARG, "NULL buffer passed to search");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(sparse_check(idx, sp));
    MVDB_TRY(check_sparse_queries(sp, q_indptr_host, q_indices_host, q_values_host, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    if (stream_capturing((hipStream_t)stream)) return fail(MVDB_ERR_ARG, "sparse search cannot be captured into a hipGraph");
    SparseStreamCall call(idx, stream);
    if (!call.ws) return fail(MVDB_ERR_HIP, "workspace allocation failed");
    // the one host wait of this entry point: the staging copy of the queries belongs to the workspace (mvdb_index_search_boosted_device)
    MVDB_TRY(stage_routed_queries(idx, sp, call.ws, 0, q_indptr_host, q_indices_host, q_values_host, nq));
    MVDB_HIP(hipStreamSynchronize(call.ws->stream));
    return sparse_search_core(idx, sp, call.ws, nq, k, rs, label_offset, D_dev, I_dev);
}

int mvdb_index_search_hybrid(const mvdb_index* idx, const mvdb_sparse* sp, const float* q_host, int normalize_q, const int64_t* q_indptr_host,
                             const int32_t* q_indices_host, const float* q_values_host, int nq, int k, float dense_weight, float sparse_weight,
                             const mvdb_rowset* rs, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_sparse_k(k));
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "hybrid search needs an inner-product index");
    MVDB_TRY(sparse_check(idx, sp));
    MVDB_TRY(check_sparse_queries(sp, q_indptr_host, q_indices_host, q_values_host, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    Workspace* const ws = call.ws;
    // the dense queries and, behind them in the same pinned staging buffer, the sparse ones
    const size_t qbytes = (size_t)nq * idx->ld * sizeof(float);
    MVDB_TRY(ws->pin.reserve(qbytes + routed_query_bytes(idx, sp, q_indptr_host, nq)));
    MVDB_TRY(call.stage(q_host, nq));
    MVDB_TRY(stage_routed_queries(idx, sp, ws, qbytes, q_indptr_host, q_indices_host, q_values_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(hybrid_core(idx, sp, ws, ws->q.p, nq, k, normalize_q, dense_weight, sparse_weight, rs, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_hybrid_device(const mvdb_index* idx, const mvdb_sparse* sp, const float* q_dev, int normalize_q, const int64_t* q_indptr_host,
                                    const int32_t* q_indices_host, const float* q_values_host, int nq, int k, float dense_weight,
                                    float sparse_weight, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev, void* stream) {
    MVDB_TRY(check_sparse_k(k));
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (idx->metric != MVDB_METRIC_IP) return fail(MVDB_ERR_ARG, "hybrid search needs an inner-product index");
    MVDB_TRY(sparse_check(idx, sp));
    MVDB_TRY(check_sparse_queries(sp, q_indptr_host, q_indices_host, q_values_host, nq));
    if (rs) MVDB_TRY(rowset_check(idx, rs));
    DeviceGuard dg(idx->device);
    if (stream_capturing((hipStream_t)stream)) return fail(MVDB_ERR_ARG, "hybrid search cannot be captured into a hipGraph");
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    MVDB_TRY(stage_routed_queries(idx, sp, call.ws, 0, q_indptr_host, q_indices_host, q_values_host, nq));
    MVDB_HIP(hipStreamSynchronize(call.ws->stream));
    return hybrid_core(idx, sp, call.ws, call.q, nq, k, normalize_q, dense_weight, sparse_weight, rs, label_offset, D_dev, I_dev);
}

int mvdb_index_sparse_counters(const mvdb_index* idx, long long* calls, long long* score_launches) {
    if (!idx) return fail(MVDB_ERR_ARG, "index is NULL");
    if (calls) *calls = (long long)idx->sp_calls.load();
    if (score_launches) *score_launches = (long long)idx->sp_launches.load();
    return 0;
}

}  // extern "C"

// ---- grouped search: every query under its own row set (grouped_scan.hpp) ------------------------------------------------
namespace {

// rows in flight per wave: the gather policy, what the row-list forms of launch_scan use (U does not enter the arithmetic)
int launch_grouped(int metric, const GroupedScanArgs& a, int nitems, hipStream_t s) {
    return with_scan_shape(a.d4, [&](auto shape) {
        using S = decltype(shape);
        constexpr int U = gather_u(S::G, S::C);
        return with_scan_form<S::G, S::C>(a.d4, false, false, [&](auto form) {
            constexpr bool MASKED = decltype(form)::MASKED;
            void (*kern)(GroupedScanArgs) = metric == MVDB_METRIC_IP ? grouped_scan_kernel<S::G, S::C, U, 0, MASKED> : grouped_scan_kernel<S::G, S::C, U, 1, MASKED>;
            return profiled_launch("grouped_scan", s, [&](hipEvent_t done) { launch_kernel(kern, dim3(nitems), dim3(kScanThreads), 0, s, done, a); },
                                   "grouped_scan_kernel<%d, %d, %d, %d, %s>", S::G, S::C, U, metric == MVDB_METRIC_IP ? 0 : 1, MASKED ? "true" : "false");
        });
    });
}

// Cut the lists of the call's list-form queries into work items.  The rule:
//   S = max(S_min, ceil(sum m_i / T)) rows per item, rounded up to whole block steps (4 waves x RB rows);
//   T = CUs x items_per_cu — the launch fills the device when there is enough work;
//   S_min = min_batches block steps — a short list is ONE item, and an item is never so short that the query load, the
//           prologue and the block merge outweigh its rows;
//   query i gets ceil(m_i / S) items of equal length (to a block step).
// At most T + (number of list queries) items come out.
void plan_grouped(const mvdb_index* idx, int nq, const mvdb_rowset* const* sets, std::vector<GroupedQuery>& queries,
                  std::vector<GroupedItem>& items) {
    const Shape sh = choose_shape(idx->d4);
    const int64_t step = (int64_t)kScanWaves * (kWave / sh.G) * gather_u(sh.G, sh.C);  // rows one block takes per loop step
    const int per_cu = idx->kn.grouped_items_per_cu > 0 ? idx->kn.grouped_items_per_cu : 4;  // swept on the device: DESIGN.md section 6c
    const int64_t T = (int64_t)device_cus(idx->device) * per_cu;
    int64_t sum = 0;
    for (int i = 0; i < nq; ++i)
        if (sets[i] && sets[i]->rows) sum += sets[i]->count;
    int64_t S = std::max<int64_t>((int64_t)idx->kn.grouped_min_batches * step, (sum + T - 1) / T);
    S = (S + step - 1) / step * step;
    queries.resize((size_t)nq + 1);
    items.clear();
    for (int i = 0; i < nq; ++i) {
        GroupedQuery& gq = queries[i];
        gq.pad_ = 0;
        gq.first_item = (int)items.size();
        if (!(sets[i] && sets[i]->rows)) {  // bitmap or NULL: not part of the grouped launch
            gq.rows = nullptr;
            gq.m = -1;
            continue;
        }
        const int64_t m = sets[i]->count;
        gq.rows = m > 0 ? sets[i]->rows : nullptr;
        gq.m = m;
        if (m == 0) continue;
        const int64_t pieces = (m + S - 1) / S;
        const int64_t len = ((m + pieces - 1) / pieces + step - 1) / step * step;
        for (int64_t b = 0; b < m; b += len)
            items.push_back(GroupedItem{i, (uint32_t)b, (uint32_t)std::min(m, b + len), 0u});
    }
    queries[nq] = GroupedQuery{nullptr, -1, (int)items.size(), 0};
}

// The table reaches the device without a wait for the device: pinned staging + an asynchronous copy on the search's stream.
// A staging copy may be rewritten only once the upload that reads it has run, and the device entry must not wait for
// that: the workspace keeps a ring of copies, a call takes one whose upload has completed (hipEventQuery) or adds a new
// one (a few KB each).  Only with kMaxGroupedStages uploads all still pending — that many whole searches queued on one
// stream — does a call wait, for the oldest.
constexpr size_t kMaxGroupedStages = 64;
int stage_grouped_table(Workspace* ws, const std::vector<GroupedQuery>& queries, const std::vector<GroupedItem>& items,
                        const GroupedQuery** q_dev, const GroupedItem** it_dev) {
    const size_t qbytes = queries.size() * sizeof(GroupedQuery);
    const size_t ibytes = items.size() * sizeof(GroupedItem);
    const size_t bytes = qbytes + ibytes;
    MVDB_TRY(ws->gtab.reserve(bytes));
    const bool capturing = stream_capturing(ws->stream);
    void* pin = nullptr;
    Workspace::GroupedStage* slot = nullptr;
    if (capturing) {
        // the graph's upload node reads its staging copy at every replay: the call takes over the spare buffer an eager call
        // of the same shape has left behind (allocation is not capturable)
        if (ws->gpin_spare.cap < bytes)
            return fail(MVDB_ERR_ARG, "a grouped search is being captured before an eager call of the same shape has sized the workspace");
        pin = ws->gpin_spare.p;
        ws->gpin_captured.push_back(pin);
        ws->gpin_spare.p = nullptr;
        ws->gpin_spare.cap = 0;
    } else {
        if (!ws->own_stream) MVDB_TRY(ws->gpin_spare.reserve(bytes));  // (caller streams only: the host entry's workspaces are never captured)
        for (Workspace::GroupedStage* g : ws->gstage) {
            if (g->busy && hipEventQuery(g->ev) == hipSuccess) g->busy = false;
            if (!g->busy) {
                slot = g;
                break;
            }
        }
        (void)hipGetLastError();  // (hipErrorNotReady of a pending upload is not an error)
        if (!slot && ws->gstage.size() < kMaxGroupedStages) {
            slot = new Workspace::GroupedStage();
            ws->gstage.push_back(slot);
        }
        if (!slot) {
            slot = ws->gstage.front();
            MVDB_HIP(hipEventSynchronize(slot->ev));
            slot->busy = false;
            std::rotate(ws->gstage.begin(), ws->gstage.begin() + 1, ws->gstage.end());  // the oldest becomes the newest
        }
        MVDB_TRY(slot->buf.reserve(bytes));
        pin = slot->buf.p;
    }
    memcpy(pin, queries.data(), qbytes);
    if (ibytes) memcpy((char*)pin + qbytes, items.data(), ibytes);
    MVDB_HIP(hipMemcpyAsync(ws->gtab.p, pin, bytes, hipMemcpyHostToDevice, ws->stream));
    if (!capturing) {
        if (!slot->ev) MVDB_HIP(hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming));
        MVDB_HIP(hipEventRecord(slot->ev, ws->stream));
        slot->busy = true;
    }
    *q_dev = reinterpret_cast<const GroupedQuery*>(ws->gtab.p);
    *it_dev = reinterpret_cast<const GroupedItem*>(ws->gtab.p + qbytes);
    return 0;
}

int check_grouped_sets(const mvdb_index* idx, int nq, const mvdb_rowset* const* sets) {
    if (!sets) return fail(MVDB_ERR_ARG, "sets is NULL");
    for (int i = 0; i < nq; ++i)
        if (sets[i]) MVDB_TRY(rowset_check(idx, sets[i]));
    return 0;
}

// queries on the device (padded to ld), results to device buffers; every set has been checked
int grouped_search_core(const mvdb_index* idx, Workspace* ws, const float* q, int nq, int k, int normalize_q,
                        const mvdb_rowset* const* sets, int64_t label_offset, float* D_dev, int64_t* I_dev) {
    KnobScope knobs(&idx->kn);
    hipStream_t s = ws->stream;
    bool any_list = false;
    for (int i = 0; i < nq; ++i) any_list = any_list || (sets[i] && sets[i]->rows);
    const bool fused = k <= kMaxFusedK;
    if (fused && any_list) {
        thread_local std::vector<GroupedQuery> queries;
        thread_local std::vector<GroupedItem> items;
        plan_grouped(idx, nq, sets, queries, items);
        const GroupedQuery* q_tab = nullptr;
        const GroupedItem* it_tab = nullptr;
        MVDB_TRY(stage_grouped_table(ws, queries, items, &q_tab, &it_tab));
        const int nitems = (int)items.size();
        MVDB_TRY(ws->cand.reserve((size_t)std::max(nitems, 1) * k));
        if (nitems > 0) {
            GroupedScanArgs a;
            a.X = idx->X.p;
            a.ld = idx->ld;
            a.d4 = idx->d4;
            a.q = q;
            a.normalize_q = normalize_q;
            a.k = k;
            a.items = it_tab;
            a.queries = q_tab;
            a.cand = ws->cand.p;
            MVDB_TRY(launch_grouped(idx->metric, a, nitems, s));
        }
        MergeSegArgs mg;
        mg.keys = ws->cand.p;
        mg.queries = q_tab;
        mg.k = k;
        mg.metric = idx->metric;
        mg.label_offset = label_offset;
        mg.D = D_dev;
        mg.I = I_dev;
        MVDB_TRY(profiled_launch("grouped_merge", s, [&](hipEvent_t done) { launch_kernel(merge_keys_seg_kernel, dim3(nq), dim3(kMergeThreads), 0, s, done, mg); }));
    }
    // bitmap and NULL sets (and every query when k is beyond the fused select): the exact single-query routes, row by row
    for (int i = 0; i < nq; ++i) {
        const mvdb_rowset* rs = sets[i];
        if (fused && rs && rs->rows) continue;
        const float* qi = q + (int64_t)i * idx->ld;
        float* Di = D_dev + (int64_t)i * k;
        int64_t* Ii = I_dev + (int64_t)i * k;
        if (rs) MVDB_TRY(rowset_search_core(idx, ws, qi, 1, k, normalize_q, rs, label_offset, Di, Ii));
        else MVDB_TRY(search_core(idx, ws, qi, 1, k, normalize_q, nullptr, 0, label_offset, Di, Ii, /*allow_split=*/false));
    }
    return 0;
}

}  // namespace

extern "C" {

int mvdb_index_search_grouped(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                              const mvdb_rowset* const* sets, float* D_host, int64_t* I_host) {
    MVDB_TRY(check_search_args(idx, q_host, nq, k, D_host, I_host));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_grouped_sets(idx, nq, sets));
    DeviceGuard dg(idx->device);
    HostCall call(idx);
    if (!call.ws) return MVDB_ERR_HIP;
    MVDB_TRY(call.stage(q_host, nq));
    const size_t total = (size_t)nq * k;
    float* D_dev = nullptr;
    int64_t* I_dev = nullptr;
    MVDB_TRY(call.results(total, &D_dev, &I_dev));
    MVDB_TRY(grouped_search_core(idx, call.ws, call.ws->q.p, nq, k, normalize_q, sets, 0, D_dev, I_dev));
    return call.fetch(total, D_host, I_host);
}

int mvdb_index_search_grouped_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                     const mvdb_rowset* const* sets, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                     void* stream) {
    MVDB_TRY(check_search_args(idx, q_dev, nq, k, D_dev, I_dev));
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    MVDB_TRY(check_grouped_sets(idx, nq, sets));
    DeviceGuard dg(idx->device);
    StreamCall call(idx, stream, q_dev, nq);
    MVDB_TRY(call.rc);
    Workspace* ws = call.ws;
    return grouped_search_core(idx, ws, call.q, nq, k, normalize_q, sets, label_offset, D_dev, I_dev);
}

int mvdb_merge_topk_device(int metric, int nlists, int nq, int k, const float* D_dev,
                           int64_t list_stride_D, const int64_t* I_dev, int64_t list_stride_I,
                           float* D_out_dev, int64_t* I_out_dev, int device, void* stream) {
    if (!D_dev || !I_dev || !D_out_dev || !I_out_dev) return fail(MVDB_ERR_ARG, "NULL buffer");
    if (nlists <= 0 || nq <= 0 || k <= 0) return fail(MVDB_ERR_ARG, "non-positive size");
    MVDB_TRY(ensure_device(device));
    DeviceGuard dg(device);
    if (k > kMaxFusedK)  // more results than one wave holds: sort the gathered lists in LDS (collective.hip)
        return launch_merge_di_sort(metric, nlists, nq, k, D_dev, list_stride_D, I_dev, list_stride_I, D_out_dev,
                                    I_out_dev, device, (hipStream_t)stream);
    MergeDIArgs a{D_dev, I_dev, list_stride_D, list_stride_I, nlists, nq, k, metric, D_out_dev, I_out_dev};
    hipLaunchKernelGGL(merge_di_kernel, dim3(nq), dim3(kWave), 0, (hipStream_t)stream, a);
    MVDB_HIP(hipGetLastError());
    return 0;
}

int mvdb_normalize_l2(float* x_host, int64_t n, int d, int device) {
    if (n < 0 || d <= 0) return fail(MVDB_ERR_ARG, "bad shape");
    if (n == 0) return 0;
    if (!x_host) return fail(MVDB_ERR_ARG, "x is NULL");
    mvdb_index* tmp = nullptr;
    MVDB_TRY(mvdb_index_create(d, MVDB_METRIC_IP, device, &tmp));
    int rc = mvdb_index_add(tmp, x_host, n, 1);
    if (!rc) rc = mvdb_index_get_rows(tmp, 0, n, x_host);
    mvdb_index_free(tmp);
    return rc;
}

int mvdb_synth_fill_device(float* out_dev, int64_t n, int d, uint64_t seed, int64_t first_row,
                           int normalize, int device, void* stream) {
    if (!out_dev) return fail(MVDB_ERR_ARG, "out is NULL");
    if (n < 0 || d <= 0 || first_row < 0) return fail(MVDB_ERR_ARG, "bad shape");
    if (d % 4) return fail(MVDB_ERR_ARG, "mvdb_synth_fill_device needs d %% 4 == 0 (dense rows)");
    if (n == 0) return 0;
    MVDB_TRY(ensure_device(device));
    DeviceGuard dg(device);
    const int cus = device_cus(device);
    const int64_t total = n * (d / 4);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, (int64_t)cus * 16));
    hipLaunchKernelGGL(synth_fill_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out_dev, n,
                       (int64_t)d, d, seed, first_row);
    MVDB_HIP(hipGetLastError());
    if (normalize) {
        mvdb_index shape;  // only the geometry fields are read
        shape.d = d;
        shape.ld = d;
        shape.d4 = d / 4;
        shape.device = device;
        MVDB_TRY(normalize_range(&shape, out_dev, n, (hipStream_t)stream));
    }
    return 0;
}

double mvdb_half_eps(int d) { return d > 0 ? half_eps(d) : 0.0; }
int mvdb_half_max_queries(int d) { return d > 0 ? half_max_queries(d) : 0; }

int64_t mvdb_split_rerun_count(void) {
    // diagnostic: the counters live on the devices (the search path never reports to the host); finished work only —
    // synchronise the streams you searched on first (the host API does)
    std::lock_guard<std::mutex> lk(g_rerun_mu);
    int64_t total = 0;
    for (auto& kv : g_rerun_ctr) {
        DeviceGuard dg(kv.first);
        unsigned long long v = 0;
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(&v, kv.second, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess)
            total += (int64_t)v;
    }
    return total;
}

int mvdb_rescue_tile_stats(int64_t* listed, int64_t* total) {
    if (!listed || !total) return fail(MVDB_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(g_rerun_mu);
    *listed = *total = 0;
    for (auto& kv : g_rerun_ctr) {
        DeviceGuard dg(kv.first);
        unsigned long long v[2] = {0, 0};
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(v, kv.second + 1, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) {
            *listed += (int64_t)v[0];
            *total += (int64_t)v[1];
        }
    }
    return 0;
}

int mvdb_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (on && !g_prof_on) {
        g_prof_sym.clear();  // off -> on: a label that launches nothing from here on reads ""
        for (int slot = 0; slot < (int)g_prof.size(); ++slot)  // ... and the pairs nobody read go back to the pool
            if (g_prof[slot].state == ProfPair::kClosed) prof_release(slot);
    }
    g_prof_on = on != 0;
    return 0;
}

int64_t mvdb_prof_live_events(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return (int64_t)g_prof_ev.size();
}

int mvdb_prof_symbol(const char* name, char* out, int len) {
    if (!name || !out || len <= 0) return fail(MVDB_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof_sym.find(name);
    snprintf(out, (size_t)len, "%s", it == g_prof_sym.end() ? "" : it->second.c_str());
    return 0;
}

int mvdb_prof_read(const char* name, int64_t* launches, double* total_ms) {
    if (!name || !launches || !total_ms) return fail(MVDB_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int64_t cnt = 0;
    double ms = 0.0;
    int label = 0;
    while (label < (int)g_prof_labels.size() && g_prof_labels[label].name != name) ++label;
    for (int slot = 0; slot < (int)g_prof.size() && label < (int)g_prof_labels.size(); ++slot) {
        ProfPair& p = g_prof[slot];
        if (p.label != label || p.state != ProfPair::kClosed) continue;
        float t = 0.f;
        if (hipEventSynchronize(g_prof_ev[p.b].ev) == hipSuccess &&
            hipEventElapsedTime(&t, g_prof_ev[p.a].ev, g_prof_ev[p.b].ev) == hipSuccess) {
            ++cnt;
            ms += t;
        } else {
            (void)hipGetLastError();
        }
        prof_release(slot);
    }
    *launches = cnt;
    *total_ms = ms;
    return 0;
}

}  // extern "C"

// ================================================================================================
// large-k selection for the int8 cosine index (cos8.hip): the radix select above over one query's materialised
// scores, shared rather than compiled twice (the select kernels are defined in this translation unit only)
// ================================================================================================
namespace mvdb {

size_t select_state_bytes() { return sizeof(SelectState); }

// scores[n] (score = -distance; -inf = row not selected) -> the k best (D = distance, I = index into scores +
// label_offset), missing slots -1 / +FLT_MAX.  keys must hold pow2ceil(max(k, 2)) entries.
int select_scores_topk(const float* scores, int64_t n, int k, int64_t label_offset, float* D, int64_t* I, void* state,
                       uint64_t* keys, int device, hipStream_t s) {
    SelectState* st = (SelectState*)state;
    const int64_t k_eff = std::min<int64_t>(k, n);
    const int64_t P = pow2ceil(std::max<int64_t>(k, 2));
    const int sel_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, device_cus(device) * 8));
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, s, st, (uint64_t)k_eff);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3(sel_grid), dim3(256), 0, s, scores, n, shift, st);
        hipLaunchKernelGGL(radix_pick_kernel, dim3(1), dim3(256), 0, s, shift, st);
    }
    hipLaunchKernelGGL(radix_compact_kernel, dim3(sel_grid), dim3(256), 0, s, scores, n, st, keys);
    if (P > k_eff)
        hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)((P - k_eff + 255) / 256)), dim3(256), 0, s, keys, k_eff, P);
    if (P <= 4096) {
        hipLaunchKernelGGL(bitonic_sort_lds_kernel, dim3(1), dim3(1024), 0, s, keys, (int)P);
    } else {
        for (int64_t size = 2; size <= P; size <<= 1)
            for (int64_t stride = size >> 1; stride > 0; stride >>= 1)
                hipLaunchKernelGGL(bitonic_step_kernel, dim3((unsigned)((P / 2 + 255) / 256)), dim3(256), 0, s, keys, P,
                                   size, stride);
    }
    hipLaunchKernelGGL(emit_sorted_kernel, dim3((k + 255) / 256), dim3(256), 0, s, keys, k, MVDB_METRIC_L2, label_offset,
                       D, I, 1);
    MVDB_HIP(hipGetLastError());
    return 0;
}

}  // namespace mvdb
