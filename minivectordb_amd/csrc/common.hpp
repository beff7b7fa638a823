// common.hpp — host-side plumbing shared by the translation units of libmvdb.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mvdb.h"

namespace mvdb {

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define MVDB_HIP(expr)                                                                       \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ::mvdb::fail(e__ == hipErrorOutOfMemory ? MVDB_ERR_OOM : MVDB_ERR_HIP,    \
                                "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),      \
                                __FILE__, __LINE__);                                         \
    } while (0)

#define MVDB_TRY(expr)           \
    do {                         \
        int rc__ = (expr);       \
        if (rc__) return rc__;   \
    } while (0)

// RAII device switch: every entry point runs on its object's device and restores the caller's.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int ensure_device(int device);  // validates ordinal, MVDB_ERR_NODEVICE otherwise
int device_cus(int device);

// ---- profiling hooks ---------------------------------------------------------------------------
bool prof_enabled();
// The events of one bracket of `name` on `stream`, from the library's pool: its slot, *stop for the launch to carry
// (launch_kernel), and *start where the caller has to record one on `stream` before the launch — null where the bracket
// begins at the end of the bracket before it (ProfChain).  -1 and null events: profiling off, `stream` capturing (a timed
// event inside a graph measures nothing), or the label holds its cap of unread pairs (include/mvdb.h).
int prof_open(const char* name, hipStream_t stream, hipEvent_t* start, hipEvent_t* stop);
void prof_close(int slot, hipStream_t stream);  // the launch is enqueued: the pair is readable
// the recorded form, for brackets that hold several launches: prof_open + both events recorded on `stream` + prof_close
int prof_begin(const char* name, hipStream_t stream);
void prof_end(int slot, hipStream_t stream);
// While one is alive, the single-kernel brackets this thread launches on `stream` share their boundaries: a bracket begins
// where the one before it ended, at that kernel's stop event, and puts no marker of its own on the stream.  Its duration is
// then the time from the end of the kernel before it to the end of its own: the launch gap and the kernel.  For a run of
// brackets with NOTHING enqueued between them — a launch without a bracket would be counted into the next label.  The first
// bracket of the run records a start event.
struct ProfChain {
    hipStream_t stream;
    int last = -1;  // pool index of the stop event of the bracket before (the chain holds a reference), -1: none
    ProfChain* prev;
    explicit ProfChain(hipStream_t s);
    ProfChain(const ProfChain&) = delete;
    ProfChain& operator=(const ProfChain&) = delete;
    ~ProfChain();
};
// One kernel launch that carries a bracket's stop event: the runtime fills it from the kernel's own dispatch — its time is the
// kernel's end — and the stream gets no packet beside the kernel.  (A start event handed to the launch the same way is a marker
// on the stream again, and reads 5 us late: profiles/prof_bracket_overhead.jsonl.)  A null event: the plain launch.
template <typename... Params, typename... Args>
void launch_kernel(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t stop, Args... args) {
    if (stop) hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, stream, nullptr, stop, 0, args...);
    else hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
}
// while profiling is on: remember which kernel instantiation a label's launches run (mvdb_prof_symbol; bench.py checks
// the committed PMC profile against it)
void prof_symbol(const char* label, const char* fmt, ...);
// One launch inside its profiling bracket: the symbol of `label` (symbol...: the format and the arguments of prof_symbol; none:
// the label records no symbol), the event pair of the launch, and the launch's error.  A bracket of exactly one kernel takes
// launch(stop) and hands the event to launch_kernel (null: profiling is off, or the launch is not timed).  launch() is the
// recorded form, the pair around it on `stream`: it enqueues what it likes; one that brackets launches of its own returns their
// status, and a failure ends the call there.
template <typename Launch, typename... Sym>
int profiled_launch(const char* label, hipStream_t stream, Launch launch, Sym... symbol) {
    if constexpr (sizeof...(Sym) > 0) prof_symbol(label, symbol...);
    if constexpr (std::is_invocable_v<Launch, hipEvent_t>) {
        hipEvent_t start = nullptr, stop = nullptr;
        const int slot = prof_open(label, stream, &start, &stop);
        if (start) (void)hipEventRecord(start, stream);
        launch(stop);
        prof_close(slot, stream);
    } else {
        const int slot = prof_begin(label, stream);
        if constexpr (std::is_void_v<decltype(launch())>) launch();
        else MVDB_TRY(launch());
        prof_end(slot, stream);
    }
    MVDB_HIP(hipGetLastError());
    return 0;
}

// The one reader of the integer MVDB_* switches (read_knobs here, read_encoder_knobs in encoder.hip): unset or empty is `dflt`.
inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// Every MVDB_* tuning / A-B hook of the SEARCH path.  The environment is read ONCE per index — at mvdb_index_create, and
// again only when the caller asks (mvdb_index_reload_env: A/B runs and tests that flip a hook inside one process) — never on
// the search path.  Defaults are the measured best (docs/DESIGN_NOTES.md section 7).
struct Knobs {
    int scan_blocks_per_cu = 0;      // MVDB_SCAN_BLOCKS_PER_CU (0: the measured default per shape)
    int mfma_blocks_per_cu = 0;      // MVDB_MFMA_BLOCKS_PER_CU (0: 4 for the fragment-load kernel, 2 for the staged ones)
    int mfma_stage = 16;             // MVDB_MFMA_STAGE (8 | 16)
    int mfma_ng2 = -1;               // MVDB_MFMA_NG2 (-1: on for the staged kernel, off otherwise)
    int gemm_scan_min_nq = 104;      // MVDB_GEMM_SCAN_MIN_NQ
    int gemm_scan_blocks_per_cu = 2; // MVDB_GEMM_SCAN_BLOCKS_PER_CU
    int split_scan_min_nq = -1;      // MVDB_SPLIT_SCAN_MIN_NQ: fewest queries of a call for the certified pass (-1: by corpus size, mvdb.hip half_min_nq)
    bool disable_rescue = false;       // MVDB_DISABLE_RESCUE: refused queries go straight to the exact passes (A/B)
    bool disable_tile_skip = false;    // MVDB_DISABLE_TILE_SKIP: the rescue launches scan every tile of the shadow (A/B)
    int tile_flags_mode = -1;          // MVDB_TILE_FLAGS: -1 kept while the index refuses certificates (mvdb.hip: tile_flags_wanted), 1 always, 0 never
    int tile_flag_min_tiles = 12288;   // MVDB_TILE_FLAG_MIN_TILES: rows / 32 from which the certified pass keeps tile flags for the rescue pass
                                       // (393k rows.  Clustered corpus, with / without flags: 1M rows 0.43 / 0.51 ms at 32 per call, 0.91 / 0.96 at
                                       // 256; 500k rows 0.31 / 0.34, 0.645 / 0.639; 200k rows 0.166 / 0.166, 0.336 / 0.321)
    bool disable_rerun_floor = false;  // MVDB_DISABLE_RERUN_FLOOR: the exact re-run of refused queries starts every list from -inf (A/B)
    int half_phase_growth = 0;       // MVDB_HALF_PHASE_GROWTH (0: by the pass width — 16 / 6 up to 128 queries per pass, 6 / 4 at 256)
    int half_last_growth = 0;        // MVDB_HALF_LAST_GROWTH
    bool split_stats = false;        // MVDB_SPLIT_STATS
    bool disable_mfma_scan = false, disable_l2_mfma = false, disable_gemm_scan = false, disable_split_scan = false,
         disable_half_scan = false, disable_masked_batch = false,
         disable_l2_cert = false,    // MVDB_DISABLE_* (L2_CERT: L2 batches back on the exact fp32 kernels)
         disable_half_shadow = false;  // MVDB_DISABLE_HALF_SHADOW (index option half_shadow = 0): no fp16 shadow, batches on the exact fp32 passes
    bool shadow_single_query = false;  // MVDB_SHADOW_SINGLE_QUERY (1: single queries through the certified fp16-shadow pass too)
    bool code8_single_query = true;    // index option code8_single_query: single queries over large inner-product indexes through the int8 prefilter
    long long code8_capacity = 32768;  // index option code8_capacity: candidates the prefilter may hand to the exact re-score
    int code8_front_plane = 1;         // index option code8_front_plane: 1 the code keeps a plane of the top 5 bits and the prefilter streams it
                                       // (+5 d / 8 bytes per row), 0 no such plane; diagnostic: 2 as 1 and the front form is never suspended, 3 as 1 and it always is
    int code8_bit_plane = 1;           // index option code8_bit_plane: 1 an index that keeps the front plane also keeps the plane of bit 2 (+d / 8 bytes per
                                       // row) and the front form lifts its survivors from it (code8_scan.hpp: LIFT), 0 no such plane: they are gathered
    int code8_front_u = 0;             // MVDB_CODE8_FRONT_U: tuning hook, tiles per batch of the front form (4 | 8; the quad layout: 1 | 2 | 4; 0: the measured default)
    int code8_handoff = 0;             // MVDB_CODE8_HANDOFF: A/B hook, the survivor wave of the front form's lift (code8_scan.hpp: HANDOFF): 0 the measured default (on), 1 never, 2 always
    int code8_ring = 0;                // MVDB_CODE8_RING: tuning hook, entries of its rings in LDS, all four together (a power of two, 64 .. 4096; 0: 1024)
    int range_shared = 0;              // index option range_shared: batches of a range search on the shared fp16 pass (0 never — the default until the
                                       // route has been timed, DESIGN.md section 6e —, 1 by size, 2 wherever eligible)
    int join_shared = 1;               // index option join_shared: the range join on the shared fp16 pass (0 never, 1 by size — the default: a join has
                                       // as many queries as rows, DESIGN.md section 6j —, 2 wherever eligible)
    long long range_candidates = 0;    // index option range_candidates: candidates per query that pass holds (0: max(2 cap rounded up to a power of two, 4096))
    long long distinct_table_bytes = 256ll << 20;  // index option distinct_table_bytes: budget of the distinct search's tier-2 table (mvdb.hip: distinct_core)
    long long groups_partials_bytes = 64ll << 20;  // index option groups_partials_bytes: budget of the group hits search's block lists (mvdb.hip: groups_core)
    long long maxsim_table_bytes = 2ll << 30;  // index option maxsim_table_bytes: most bytes of a MaxSim search's table, T x n_groups x 8 (mvdb.hip: check_maxsim_state)
    int maxsim_tokens_per_pass = 0;    // index option maxsim_tokens_per_pass: query vectors per corpus pass of a MaxSim search (0: maxsim_scan.hpp maxsim_tokens_per_pass)
    int assign_vectors_per_pass = 0;   // index option assign_vectors_per_pass: vectors per corpus pass of an assignment (0: assign_scan.hpp assign_vectors_per_pass)
    int examples_vectors_per_pass = 0; // index option examples_vectors_per_pass: vectors per corpus pass of a search by examples (0: examples_scan.hpp examples_vectors_per_pass)
    long long probe_table_bytes = 256ll << 20;  // index option probe_table_bytes: most bytes of a probed search's item and candidate tables; beyond it the queries go in chunks (mvdb.hip: probe_core)
    int sparse_postings = 1;           // index option sparse_postings: 1 a sparse store that has postings answers through them (sparse_postings.hpp), 0 always the CSR pass
    int grouped_items_per_cu = 0;      // MVDB_GROUPED_ITEMS_PER_CU: work items per CU the grouped launch aims at (0: the default of mvdb.hip plan_grouped; sweep in DESIGN.md section 6c)
    int grouped_min_batches = 4;       // MVDB_GROUPED_MIN_BATCHES: fewest row batches per wave of a work item
    long long compact_bytes = 512ll << 20;  // MVDB_COMPACT_BYTES: staging buffer of a row compaction (mvdb_index_remove_rows)
    bool compact_inplace = true;            // MVDB_COMPACT_INPLACE (0: a few deleted rows take the staging path too)
    int code8_seed_blocks = 0;         // MVDB_CODE8_SEED_BLOCKS: tuning hook, grid of code8_seed_kernel (0: one block per CU)
    int code8_seed_threads = 0;        // MVDB_CODE8_SEED_THREADS: tuning hook, 256 | 512 | 1024 threads per block of it (0: 512)
    int code8_rescore_rows = 0;        // MVDB_CODE8_RESCORE_ROWS: tuning hook, candidates per active block of code8_rescore_kernel (0: 32)
};
Knobs read_knobs();

// hipOccupancyMaxActiveBlocksPerMultiprocessor, asked once per (kernel, dynamic LDS) and remembered
int cached_occupancy(const void* kern, int threads, size_t lds, int dflt);
// hipFuncAttributeMaxDynamicSharedMemorySize >= lds for `kern`, set once per (kernel, device); `device` is the current device
int ensure_dynamic_lds(const void* kern, size_t lds, int device);

// A search captured into a hipGraph bakes its workspace pointers into the graph.  While a retire list is installed
// (RetireScope: searches on a workspace that has been captured once), a buffer that must grow is NOT freed — it goes on
// the list and lives as long as the workspace, so replaying the earlier graph still reads and writes valid memory.
extern thread_local std::vector<void*>* tls_retire;
struct RetireScope {
    std::vector<void*>* prev;
    explicit RetireScope(std::vector<void*>* list) : prev(tls_retire) { tls_retire = list; }
    ~RetireScope() { tls_retire = prev; }
};

// The two buffer types own their memory: whatever holds one frees it by going away (with the owner's device current).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        if (p) {
            if (tls_retire) tls_retire->push_back((void*)p);
            else (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        size_t want = n + n / 4 + 64;
        MVDB_HIP(hipMalloc((void**)&p, want * sizeof(T)));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 4 + 256;
        MVDB_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The stream a workspace created for itself (none for a caller's stream or the legacy default stream).  Declared as the FIRST
// member of its workspace, so destroyed last: the workspace's buffers are freed before the stream they were used on goes.
struct OwnedStream {
    hipStream_t h = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() {
        if (h) (void)hipStreamDestroy(h);
    }
};

}  // namespace mvdb
