/*
 * mvdb.h — C-ABI of libmvdb.so, the MI355X (gfx950) replacement for the native calls on
 * MiniVectorDB's embed+search hot path.
 *
 * The reference (cnmoro/MiniVectorDB @ 2024-10-08) has no FFI of its own: the hot path is
 * executed inside third-party wheels (faiss-cpu, transformers/torch).  Each entry point below
 * names the reference call site it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; mvdb_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure on the calling thread;
 *   - plain pointers and sizes only; "host" pointers are ordinary CPU memory owned by the caller
 *     for the duration of the call, "dev" pointers are device memory on the index' GPU;
 *   - the library copies on add (as faiss IndexFlatIP.add does) and owns all device memory;
 *   - result conventions match faiss: rows sorted by score descending, labels int64,
 *     missing slots label -1 / score -FLT_MAX (IP) or +FLT_MAX (L2);
 *   - ties are broken by ascending row number (deterministic);
 *   - mvdb_index_search* are re-entrant on one index from many host threads; add / reset /
 *     free take the index exclusively.
 *   - There is NO CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef MVDB_H
#define MVDB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVDB_METRIC_IP 0 /* inner product, larger is better (faiss.IndexFlatIP)            */
#define MVDB_METRIC_L2 1 /* squared L2, smaller is better (extension; not in the reference) */

#define MVDB_OK 0
#define MVDB_ERR_ARG 1     /* bad argument                       */
#define MVDB_ERR_HIP 2     /* HIP runtime / device failure       */
#define MVDB_ERR_NODEVICE 3 /* no usable gfx950 device            */
#define MVDB_ERR_OOM 4     /* device allocation failed           */

typedef struct mvdb_index mvdb_index;
typedef struct mvdb_encoder mvdb_encoder;

/* ---- library / device ------------------------------------------------------------------- */

/* Thread-local description of the last error on this thread ("" if none). */
const char* mvdb_last_error(void);

/* ABI version of this header (bumped on incompatible change). */
int mvdb_abi_version(void);

/* Number of visible HIP devices; fails with MVDB_ERR_NODEVICE when there is none. */
int mvdb_device_count(int* count);

/* ---- flat index --------------------------------------------------------------------------
 * Replaces faiss.IndexFlatIP(d)                  minivectordb/vector_database.py:43, :511
 *                                                minivectordb/sharded_vector_database.py:80, :639
 * The corpus lives in HBM as one row-major fp32 matrix, row stride = d rounded up to a
 * multiple of 4 floats (16-byte rows), zero padded. */
int mvdb_index_create(int d, int metric, int device, mvdb_index** out);
int mvdb_index_free(mvdb_index* idx);

/* The MVDB_* tuning / A-B hooks of the search path (docs/DESIGN_NOTES.md section 7) are read from the environment ONCE, by
 * mvdb_index_create; the search path itself never calls getenv.  This re-reads them for an existing index (A/B runs and tests
 * that flip a hook inside one process).  No reference counterpart. */
int mvdb_index_reload_env(mvdb_index* idx);

/* Per-index switches a caller sets in code rather than through the environment (the value survives until the next
 * mvdb_index_reload_env).  No reference counterpart.
 *   "shadow_single_query" (0 | 1, default 0): ONE query per call also goes through the certified nomination pass over the fp16
 *       shadow of the rows (>= 500,000 rows at d = 256 / 384 / 512): the same ids and fp32 scores as the exact scan — nominees
 *       re-scored in fp32, every result certified, uncertified queries re-run exactly — at about half the bytes per query
 *       (10M x 512: 2.84 -> 1.58 ms), for 2 more bytes per stored element.  Off by default: the single-query scan is the exact
 *       fp32 kernel the headline roofline is defined on.
 *   "code8_single_query" (0 | 1, default 1): ONE unfiltered inner-product query over >= 500,000 unpadded rows of width
 *       384 / 512 / 1024 is answered in two steps: a pass over an int8 code of the rows (1 byte per element, kept beside the
 *       matrix: mvdb_index_code8_rows) keeps every row whose proven upper bound reaches a proven floor of the k-th best score,
 *       then the exact fp32 kernel scores the kept rows.  D and I are bit for bit those of the exact scan (option 0).
 *       "shadow_single_query" = 1 takes precedence.
 *   "code8_capacity" (1 .. 65536, default 32768): most candidate rows a call of that route may keep; a call that keeps more (or fewer
 *       than k) is answered by the full exact scan, enabled on the device.  Diagnostic: a small value forces that fallback.
 *   "code8_front_plane" (0 .. 3, default 1): 1 = the int8 code keeps a third plane, the top 5 bits of every code (+5 d / 8
 *       bytes per row: 3.2 GB at 10M x 512), and the prefilter streams that plane, fetching the 6-bit plane only for the rows
 *       it cannot reject; an index whose queries leave too many such rows goes back to streaming the 6-bit plane by itself
 *       (mvdb_index_code8_front_counters).  0 frees the plane.  Diagnostic: 2 = 1, never going back; 3 = 1, the plane kept
 *       and never streamed.  D, I and the candidate
 *       rows of a call do not depend on this option.  An allocation that fails leaves the index without the plane, no more.
 *   "code8_bit_plane" (0 | 1, default 1): 1 = an index that keeps the front plane also keeps the plane of bit 2 of every code
 *       (+d / 8 bytes per row: 640 MB at 10M x 512), and the rows the front plane cannot reject fetch their d / 8 bytes of it
 *       where they would fetch 3 d / 4 + 8 of the 6-bit plane.  0 frees this plane alone ("code8_front_plane" = 0 does not
 *       free it); 1 again rebuilds the code with it at the next eligible query.  D, I, the candidate rows and the counters
 *       of a call do not depend on this option.  An allocation that fails leaves the index without the plane, no more.
 *   "half_shadow" (0 | 1, default 1): 0 = batches nominate from the fp32 rows (no second copy of the corpus).
 *   "compact_bytes" (> 0, default 512 MiB): staging buffer of mvdb_index_remove_rows. */
int mvdb_index_set_option(mvdb_index* idx, const char* name, long long value);

/* The opt-in single-query route over the shadow ("shadow_single_query") costs more than the exact scan whenever its certificate
 * is refused (clustered / duplicate-heavy corpora: the nomination pass AND the exact scan).  The library watches the refusals
 * (a device counter mirrored into host-mapped memory: no synchronisation) in windows of 32 such calls; when half of a window
 * was refused the next 512 single queries take the exact scan directly, then the route probes again.  Returns how many times
 * that has happened on this index (diagnostics; -1 for NULL).  Results are identical either way. */
long long mvdb_index_single_route_suspensions(const mvdb_index* idx);

/* Drop all rows (capacity is kept). */
int mvdb_index_reset(mvdb_index* idx);

/* Rows currently stored / dimension / device ordinal. */
int64_t mvdb_index_ntotal(const mvdb_index* idx);
int mvdb_index_dim(const mvdb_index* idx);
int mvdb_index_device(const mvdb_index* idx);

/* Rows held in the index' fp16 SHADOW (0: none).  An index of width d = 128 / 256 / 384 / 512 / 640 / 768 / 896 / 1024 (unpadded
 * rows) that answers a batch the certified pass takes — 2+ queries from 500k rows, 8+ from 100k, 33+ below (thresholds measured
 * at d = 512 and applied to every shadow width: the pass is bound by the shadow's bytes at all of them) — keeps, lazily, from
 * the first such search on (that search builds it: one blocking conversion pass and a hipMalloc inside an otherwise asynchronous
 * call), an fp16 copy of its rows next to the fp32 matrix (2 more bytes per element = +50 % of the index's device memory): the
 * nomination pass of those batches streams it (the fp32 matrix stays the home of the exact scans and of every returned score).
 * add extends it, remove_rows / reset / a re-allocation drop it (the next batch search rebuilds it: ~5 ms per 10M x 512 rows).
 * Without a shadow — option "half_shadow" = 0, MVDB_DISABLE_HALF_SHADOW=1, or its allocation failed — batches are answered by
 * the exact fp32 passes (32 queries per corpus pass; until round 6 a second nomination generation read the fp32 rows).
 * No reference counterpart. */
int64_t mvdb_index_shadow_rows(const mvdb_index* idx);

/* Rows held in the index' int8 CODE (0: none): d int8 values per row, stored as two planes in the same d bytes — the top 6
 * bits of every code (3 d / 4 bytes per row, the plane the prefilter streams) and the low 2 bits (d / 4 bytes per row, fetched
 * only for the rows the first plane cannot reject: mvdb_code8_pack) — an fp32 scale and an fp32 bound of the coding residual
 * (+25 % of the index's device memory at d = 512, and a fixed 131,072 x (d + 8) bytes for a second, contiguous copy of the
 * sampled rows the route takes its floor from), the operand of the single-query prefilter (option "code8_single_query").
 * Built by the first eligible single query (one blocking conversion pass and the allocations inside that call; never while the
 * stream is being captured: such a call takes the exact scan), extended by add, dropped by remove_rows / reset / a
 * re-allocation — the exact scan answers the next two eligible queries after the LATEST such change before the code is
 * rebuilt (every delete restarts the count), so a workload that alternates deletes and queries never pays for builds.  An
 * allocation failure leaves the exact scan in charge for the life of the index.  The build also fills the last row of the
 * readable slack behind the matrix with NaN (the padding entry of the candidate list); no stored row is touched.
 * No reference counterpart. */
int64_t mvdb_index_code8_rows(const mvdb_index* idx);

/* Diagnostics of the prefilter route, read from host-mapped words without synchronising (they lag by the calls in flight):
 * calls that fell back to the full exact scan, the candidate rows of the latest call, calls served.  Any pointer may be NULL. */
int mvdb_index_code8_counters(const mvdb_index* idx, long long* fallbacks, long long* last_candidates, long long* calls);

/* The prefilter's margin: for a stored row x with |x| <= row_norm_bound whose code has residual bound r,
 * and a query image of norm <= qnorm rounded with step qstep, the fp32 score the exact kernel computes lies within
 * alpha * r + beta of the coded score.  Pure host arithmetic (no device needed). */
int mvdb_code8_margin(int d, float qnorm, float qstep, float row_norm_bound, float* alpha, float* beta);

/* The two planes of the code: the d int8 codes of one row (d a multiple of 16) <-> the 3 d / 4 bytes
 * of its high plane (the top 6 bits of every code) and the d / 4 bytes of its low plane (the low 2 bits).  The very functions
 * the device code packs and unpacks 16-code chunks with.  Pure host arithmetic (no device needed). */
int mvdb_code8_pack(int d, const int8_t* codes, uint8_t* high, uint8_t* low);
int mvdb_code8_unpack(int d, const uint8_t* high, const uint8_t* low, int8_t* codes);

/* The FRONT plane of the code: the top 5 bits of every code, c & ~7, at 5 d / 8 bytes per row — what
 * the prefilter streams first where the index holds it (option "code8_front_plane").  The d int8 codes of one row (d a
 * multiple of 32, at most 2048; other widths are refused) <-> the row's image in the plane: the 16-byte parts of its d / 32
 * chunks, then their 4-byte parts.  unpack returns c & ~7.  The very functions the device code uses.  Pure host arithmetic. */
int mvdb_code8_front_pack(int d, const int8_t* codes, uint8_t* image);
int mvdb_code8_front_unpack(int d, const uint8_t* image, int8_t* codes);

/* Diagnostic: mvdb_code8_scan_geometry for the form of the prefilter's launch that streams the front plane. */
int mvdb_code8_front_geometry(int d, int64_t n, int device, int* rows_per_batch, int* waves);

/* Diagnostics of the front form: the rows its first look (the front plane) could not reject, summed over its calls; those
 * calls; how often its window has suspended it (the mean share of such rows over 32 calls was above the share at which
 * the other form is faster: the next 512 calls stream the 6-bit plane); whether the code holds the plane.  Any pointer may
 * be NULL.  Reads device words: synchronises with the device. */
int mvdb_index_code8_front_counters(const mvdb_index* idx, long long* survivors, long long* calls, long long* suspensions, int* held);

/* Diagnostic: one stored row of the code as the device holds it — its 3 d / 4 bytes of the high plane, d / 4 of the low
 * plane and its 5 d / 8-byte image in the front plane (mvdb_code8_front_unpack).  Any pointer may be NULL. */
int mvdb_index_code8_read_row(const mvdb_index* idx, int64_t row, uint8_t* high, uint8_t* low, uint8_t* front);

/* Diagnostic: where the device keeps the two parts of a row's 32-code chunk in the front plane of an index of width d — the
 * byte offsets of its 16-byte part and of its 4-byte part from the start of the plane.  The plane is stored in tiles of the
 * rows one wave-instruction of the prefilter covers; at d = 512 a tile is 16 rows in five 1-KiB slabs (a lane quad per row,
 * four chunks per lane), at the other widths the 16-byte parts of the tile's rows and behind them the 4-byte parts.  Pure host
 * arithmetic: the very functions every reader and writer of the plane uses. */
int mvdb_code8_front_offset(int d, int64_t row, int chunk, int64_t* wide, int64_t* narrow);

/* The bit plane of the code (option "code8_bit_plane"): bit 2 of every code, d / 8 bytes per row — bit i of dword s of a row
 * is bit 2 of code 32 s + i.  With H5 = c & ~7 (the front plane) and b2 = (c >> 2) & 1: c & ~3 = H5 + 4 b2, so the sum over
 * the 6-bit plane is Q . H5 + 4 Q . b2.  pack: d codes (d a multiple of 32, at most 2048) -> d / 8 bytes; unpack: -> b2 of every
 * code, 0 or 1.  Host only. */
int mvdb_code8_bit2_pack(int d, const int8_t* codes, uint8_t* bits);
int mvdb_code8_bit2_unpack(int d, const uint8_t* bits, int8_t* codes);

/* Diagnostic: the d / 8 bytes of one stored row in the bit plane as the device holds them (bits may be NULL), and whether
 * the code holds the plane (held may be NULL). */
int mvdb_index_code8_read_bit2(const mvdb_index* idx, int64_t row, uint8_t* bits, int* held);

/* Diagnostic: how the prefilter's launch shares n rows of width d (384 / 512 / 1024) out on `device`: wave w of `waves`
 * takes the batches w, w + waves, ... of rows_per_batch consecutive rows.  Tests plant rows by it. */
int mvdb_code8_scan_geometry(int d, int64_t n, int device, int* rows_per_batch, int* waves);

/* Diagnostic: the rows whose low plane the prefilter has fetched (the rows its first stage could not reject), summed over
 * all calls on this index since the code's counters were allocated.  Reads a device word: synchronises with the device. */
int mvdb_index_code8_refined(const mvdb_index* idx, long long* rows);

/* Reserve device capacity for at least n rows in total (amortises repeated add). */
int mvdb_index_reserve(mvdb_index* idx, int64_t n);

/* Append n rows from host memory x[n,d] (C-contiguous fp32).  normalize != 0 L2-normalises each
 * appended row on the device first (zero-norm rows are left untouched).
 * Replaces faiss.normalize_L2(self.embeddings) + index.add(self.embeddings)
 *                                                minivectordb/vector_database.py:45-46, :512
 *                                                minivectordb/sharded_vector_database.py:82-83, :640 */
int mvdb_index_add(mvdb_index* idx, const float* x_host, int64_t n, int normalize);

/* Same, rows already in device memory (x_dev[n,d], dense, same GPU). */
int mvdb_index_add_device(mvdb_index* idx, const float* x_dev, int64_t n, int normalize);

/* Append n synthetic rows generated on the device by the counter-based generator documented in
 * DESIGN.md (element (i,j) of the stream `seed` with i = first_row + local row); bit-identical
 * to oracle/synth.py on the host before normalisation.  Used by bench.py and the full-size
 * tests so that 10M x 512 corpora never cross PCIe.  No reference counterpart. */
int mvdb_index_add_synthetic(mvdb_index* idx, int64_t n, uint64_t seed, int64_t first_row,
                             int normalize);

/* Copy rows [row0,row0+n) back to host memory out[n,d] (what faiss calls reconstruct_n);
 * used for get_vector after the in-place normalisation side effect
 *                                                minivectordb/vector_database.py:45, :49-55 */
int mvdb_index_get_rows(const mvdb_index* idx, int64_t row0, int64_t n, float* out_host);

/* Remove the given rows (ascending or not, duplicates rejected) and compact the matrix so the
 * remaining rows keep their relative order — the numbering np.delete leaves behind.  Rows before
 * the first deleted one do not move.  One row (the reference's own delete), a run of rows or up to 8
 * scattered rows: the tail is shifted in place in ONE pass, every byte read once and written once
 * (row 5 of 10M x 512: 8.2 ms).  More: the tail is compacted in place through a bounded staging buffer
 * (512 MiB, kept by the index; 14.5 - 18 ms there).  Neither needs memory proportional to the index.
 *                                                minivectordb/vector_database.py:126, :139-152 */
int mvdb_index_remove_rows(mvdb_index* idx, const int64_t* rows_host, int64_t m);

/* Overwrite the m listed stored rows with x[m,d]; row numbers, ntotal, capacity and every device pointer stay as they are.
 * rows_host: each in [0, ntotal), any order; a duplicate, an out-of-range row or a NULL pointer with m > 0 is MVDB_ERR_ARG and
 * leaves the index untouched (the list is a host array: it is checked before anything is enqueued).  m == 0: no-op, returns 0.
 * Takes the index exclusively and waits for its enqueued searches, as add does; works on the mutators' stream; returns when
 * the rows are in place (the caller's buffers are free again).
 * Afterwards no search can tell the index from one built by add of the final rows in the same order:
 *   - the fp32 row is, bit for bit, what add(..., normalize) writes for that input (the same normalisation arithmetic, a
 *     zero-norm row left alone, the padding up to the row stride zeroed);
 *   - the fp16 shadow, the |x|^2/2 offsets and the int8 code, where present and covering the row, get what their converters
 *     write for the stored row (the same device code as add's, driven by the list).  Nothing is dropped or rebuilt:
 *     mvdb_index_shadow_rows, mvdb_index_code8_rows and the counters read the same before and after, the wait before a dropped
 *     code is rebuilt is not restarted, nothing is reallocated.  A derived store that is absent or was emptied by a delete is
 *     left as it is;
 *   - rows are not renumbered: resident row sets (list and bitmap form) stay valid and mean the same row numbers; a graph
 *     captured on a caller's stream stays replayable and sees the new rows.
 * The norm bounds only ever widen, as with add: they are updated from the new rows and never narrowed for the rows that went
 * away (a non-finite new row leaves the bound non-finite, as a raw add does).  One consequence: if the widened bound moves the
 * shadow's scale, the shadow is emptied exactly as add does it and the next batch search converts in place.
 * Cost: proportional to m * d, never to ntotal; host rows go through a bounded staging buffer (32 MiB, kept by the index) in
 * chunks, a fixed number of launches per chunk.  No reference counterpart (it raises on a duplicate id). */
int mvdb_index_set_rows(mvdb_index* idx, const int64_t* rows_host, const float* x_host, int64_t m, int normalize);

/* Same, the new rows already in device memory (x_dev[m,d], dense, same GPU; complete, or ordered before the legacy stream, as
 * for mvdb_index_add_device).  The row numbers are still a host array. */
int mvdb_index_set_rows_device(mvdb_index* idx, const int64_t* rows_host, const float* x_dev /*[m,d] dense, same GPU*/, int64_t m,
                               int normalize);

/* k nearest rows for nq queries.  q_host[nq,d], D_host[nq,k], I_host[nq,k].
 * normalize_q != 0 L2-normalises each query on the device first.
 * Every path returns exact-fp32 scores of the exact top-k.  Which pass answers a call (csrc/mvdb.hip: search_core):
 *   1 query                      the exact fp32 scan (the reference's call shape; option "shadow_single_query" sends it through
 *                                the certified pass too, which suspends itself while its certificates are being refused);
 *   2+ queries, k <= 32, a width with a shadow (previous comment), enough rows to bury the pass's fixed cost (2 queries from
 *   500k rows, 8 from 100k, 33 below)
 *                                the CERTIFIED pass, 128 / 256 queries per pass over the fp16 shadow: ONE fp16 product nominates
 *                                64 rows per query, fp32 re-scores decide, a worst-case bound (mvdb_half_eps) certifies each
 *                                query.  A query whose certificate is refused (near-duplicate neighbourhoods) goes to the RESCUE
 *                                pass — once more over the shadow (inner product, k <= 16, ~400k rows and more, from the second
 *                                refused call of an index on: over the 32-row tiles the certified pass flagged for it, a few
 *                                percent of them — the flags are kept only while the index refuses certificates), every row above its floor kept
 *                                and re-scored in fp32: exact — and, where that cannot hold its neighbourhood, to a device-gated
 *                                exact fp32-MFMA pass
 *                                (mvdb_split_rerun_count counts the chunks that held a refused query);
 *   other batches                exact fp32 passes on the matrix cores: 32 (d <= 512) / 16 (d <= 1024) queries per corpus pass
 *                                at d = 64 and the multiples of 128; elsewhere the GEMM-tiled exact scan from 6 queries
 *                                (128 per launch, k <= 16), else one query at a time;  k > 64: scores + radix select.
 * A batch returns what nq separate calls return — ids identical AWAY FROM fp32 NEAR-TIES: rows whose scores lie within
 * ~2e-6 of each other (exact duplicates aside: those tie exactly and come back lowest row first on every path) may be ranked
 * either way by two fp32 summation orders, so on near-duplicate corpora a batch and a single call can swap such rows
 * (tests/bigcheck.py adjudicates every difference in float64).
 * MVDB_METRIC_L2 (an extension: the reference builds IndexFlatIP only): one query sums (q - x)^2 directly; several queries
 * share corpus passes — on the certified pass where the rows have one norm (nomination by inner product, distance re-score,
 * norm-range certificate) or, for ANY norms, by q.x - |x|^2 / 2 with per-row offsets beside the shadow, also under a bitmap;
 * else on the fp32 matrix cores as |q|^2 + |x|^2 - 2 q.x (d % 128 == 0, d <= 768; differences of the two forms are at the
 * rounding level of the norms).
 * NON-FINITE ROWS AND QUERIES (NaN, +/-inf, -0.0) — one contract for every route of this call and of its subset, masked and
 * row-set forms:
 *   - The key score of a row is q.x for IP and -sum (q_j - x_j)^2 for L2.  NaN arises only where IEEE arithmetic on the
 *     DIRECT form gives it: a NaN element, inf * 0, inf - inf.
 *   - A row whose key score is NaN is never a result, on any route and at any k.
 *   - Rows scoring +inf come first and rows scoring -inf come after every finite row.  Within equal scores, +/-inf included,
 *     the lower row (or lower position in a row list) comes first.
 *   - Slots beyond the non-NaN rows are I = -1, D = -FLT_MAX (IP) / +FLT_MAX (L2).  This holds whether the shortfall comes from
 *     k > n, from the selection or from NaN rows.
 *   - normalize_q follows fvec_renorm_L2 literally: nr > 0 false leaves the query as it is, and nr = inf multiplies by 0.
 *   - A score that overflows to +/-inf from FINITE elements is outside the contract.  It depends on summation order and on
 *     fused multiply-add.
 * Replaces faiss.normalize_L2(embedding) + index.search(embedding, search_k)
 *                                                minivectordb/vector_database.py:475, :497
 *                                                minivectordb/sharded_vector_database.py:604, :626 */
int mvdb_index_search(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                      float* D_host, int64_t* I_host);

/* Same with every buffer in device memory and the work enqueued on `stream` (a hipStream_t, or
 * NULL for the legacy default stream).  label_offset is added to every label (global row number of
 * this shard's first row).  This is the entry point the one-process-per-GPU sharded search uses
 * ahead of its RCCL all-gather.
 * Synchronisation: NONE, whatever the batch size.  The host never reads a certification flag: the queries a
 * certified batch pass could not certify are compacted, re-run on the exact kernels and scattered back by launches
 * that are enabled ON THE DEVICE (they return at once when every query certified).  The call can therefore be captured
 * into a hipGraph — after one eager call of the same shape on that stream has sized its workspace (allocation is not
 * capturable) — e.g. encoder forward -> search as ONE graph.  A captured graph names the stream's workspace buffers: from
 * the first capture on, that workspace never frees a buffer it outgrows (a later, LARGER eager call on the same stream
 * allocates new ones and parks the old until the index goes), so replaying the earlier graph stays valid.
 * One search at a time per (index, stream): concurrent calls naming the same stream are serialised.
 * Mutators (add / remove_rows / reset / reserve) wait for the searches enqueued on THIS index — its streams only, no
 * device-wide synchronise — and do their own work on a private non-blocking stream. */
int mvdb_index_search_device(const mvdb_index* idx, const float* q_dev, int nq, int k,
                             int normalize_q, int64_t label_offset, float* D_dev, int64_t* I_dev,
                             void* stream);

/* Search restricted to the m listed rows of the resident corpus (labels returned are positions
 * in rows_host[], exactly what the reference's throw-away sub-index returns).
 * Replaces self.embeddings[list(filtered)] -> IndexFlatIP.add -> search
 *                                                minivectordb/vector_database.py:510-514
 *                                                minivectordb/sharded_vector_database.py:636-642 */
int mvdb_index_search_subset(const mvdb_index* idx, const float* q_host, int nq, int k,
                             int normalize_q, const int64_t* rows_host, int64_t m, float* D_host,
                             int64_t* I_host);

/* Device-resident variant of mvdb_index_search_subset for the one-process-per-GPU sharded search: queries, the row
 * list (rows_dev[m], int64, every entry in [0, ntotal) — validated by the caller, this entry point does not
 * synchronise) and outputs live in device memory, work is enqueued on `stream`.  map_labels == 0: labels are
 * positions in rows_dev[] (+ label_offset), as above; map_labels != 0: labels are rows_dev[position] + label_offset,
 * i.e. global row numbers of a shard whose first row is label_offset.
 * Replaces the per-shard half of             minivectordb/sharded_vector_database.py:634-649 */
int mvdb_index_search_subset_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const int64_t* rows_dev, int64_t m, int map_labels, int64_t label_offset,
                                    float* D_dev, int64_t* I_dev, void* stream);

/* Search restricted to the rows whose bit is set in a BITMAP over the resident corpus: mask[(ntotal + 63) / 64] 64-bit
 * words, bit (r & 63) of word r >> 6 = row r; bits at or beyond ntotal are ignored.  Every row is scored in ONE pass at
 * the full scan's rate and rows with a clear bit are never offered to the top-k — the form for filters that keep MOST
 * rows (the reference's exclude-filters: a row list of ~ntotal entries gathered row by row is slower than the scan it
 * avoids, and its 8 bytes per row are the upload).  labels == 0: positions in the ascending list of the set rows — exactly
 * what mvdb_index_search_subset returns for that list; labels == 1: row numbers.  Exact score ties resolve to the lower
 * row number in both.  Fewer than k rows selected: the tail is -1 / -FLT_MAX (IP) as everywhere.
 * nq > 1 (inner product, d % 128 == 0, k <= 64): the batch shares corpus passes like an unfiltered one — 33+ queries on the
 * certified fp16 pass (the bit is consulted where a row is about to be nominated), fewer on the fp32-MFMA pass, which also
 * re-runs uncertified queries under the bitmap; other shapes answer the bitmap one query at a time.
 * Replaces the same per-query sub-index as mvdb_index_search_subset
 *                                                minivectordb/vector_database.py:508-523 (exclude filters :354-386)
 *                                                minivectordb/sharded_vector_database.py:634-649 */
int mvdb_index_search_masked(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                             const uint64_t* mask_host, int labels, float* D_host, int64_t* I_host);

/* Device-resident variant (mask_dev, queries and outputs in device memory, enqueued on `stream`, no synchronisation);
 * labels == 1: row number + label_offset. */
int mvdb_index_search_masked_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const uint64_t* mask_dev, int labels, int64_t label_offset, float* D_dev,
                                    int64_t* I_dev, void* stream);

/* A filter's rows kept RESIDENT on the device, so that consecutive searches under the same filter (the reference
 * re-evaluates its filter and re-gathers the rows for every query, vector_database.py:477-523) pay neither the host pass
 * over the list nor its upload again.  excluded == 0: the m listed rows (labels order ties by list position, as
 * mvdb_index_search_subset); excluded != 0: every row BUT the listed ones (an exclude-filter: m is small, the set is
 * ~ntotal rows).  The library picks the representation: a bitmap (n / 8 bytes; one full-rate pass per search) for excluded
 * sets and for sorted lists that keep >= 90 % of the rows, a device row list otherwise — a SORTED list (>= 1 row in 64) also
 * carries its bitmap, under which a BATCH of queries shares corpus passes where that beats one gathered scan per query (10M x
 * 512, 30 % of the rows: 64 queries 1.7 ms instead of 58 ms).  A set belongs to the index state it
 * was built against: rows appended later are not part of it; after a removal (rows renumbered) searching it fails with
 * MVDB_ERR_ARG.  A set also belongs to its INDEX: every search entry point that takes a row set refuses, with MVDB_ERR_ARG
 * and without writing anything, a set that was created on another index object, even one of the same device, row count and
 * removal history (its row numbers mean other rows there). */
typedef struct mvdb_rowset mvdb_rowset;
int mvdb_rowset_create(const mvdb_index* idx, const int64_t* rows_host, int64_t m, int excluded, mvdb_rowset** out);
int64_t mvdb_rowset_size(const mvdb_rowset* rs);      /* rows selected */
int mvdb_rowset_is_bitmap(const mvdb_rowset* rs);
int mvdb_rowset_free(mvdb_rowset* rs);
/* labels are ROW NUMBERS of the index (not positions).  Replaces the same call sites as mvdb_index_search_subset. */
int mvdb_index_search_rowset(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                             const mvdb_rowset* rs, float* D_host, int64_t* I_host);
/* Device-resident variant (queries and outputs in device memory, enqueued on `stream`, no synchronisation; labels are row
 * numbers + label_offset): what a rank of the row-partitioned search runs for a filter whose LOCAL rows it keeps resident.
 * Replaces the per-shard half of             minivectordb/sharded_vector_database.py:634-649 */
int mvdb_index_search_rowset_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                    const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                    void* stream);

/* A batch in which EVERY QUERY HAS ITS OWN ROW SET (a serving layer that collects the queries of many callers, each with
 * its own filter): query i is searched under sets[i]; a NULL entry means every row.  Several queries may name the same set.
 * Contract: row i of (D, I) is BIT FOR BIT what mvdb_index_search_rowset (mvdb_index_search for a NULL entry) returns for
 * query i alone with nq = 1 on the default routing — not "identical away from fp32 near-ties" as the shared-pass batch
 * contract above.  Labels are row numbers.  The shadow_single_query option does not apply to this entry point.
 * Routing: all queries whose set is in LIST form share ONE gathered launch over work items (query, slice of its list) and
 * one segmented merge that also maps positions to row numbers; a long list is cut into many items, so one large filter
 * beside many small ones does not serialise the launch.  A query whose set is a BITMAP (mvdb_rowset_is_bitmap) or NULL is
 * answered by the exact single-query scan straight into row i: callers with many such queries under one set should use
 * mvdb_index_search_rowset / mvdb_index_search, which share corpus passes.  k > 64: every query takes the scores +
 * radix-select route on its own list — correct, not fast.
 * Every set is checked before anything is enqueued: one stale or foreign set fails the whole call with MVDB_ERR_ARG and
 * nothing is written.  No reference counterpart (the reference answers one query per call). */
int mvdb_index_search_grouped(const mvdb_index* idx, const float* q_host, int nq, int k, int normalize_q,
                              const mvdb_rowset* const* sets, float* D_host, int64_t* I_host);
/* Device-resident variant, under the contract of mvdb_index_search_device: enqueued on `stream`, one search at a time per
 * (index, stream), capturable into a hipGraph after one eager call of the same shape (same sets) has sized the workspace;
 * labels are row numbers + label_offset.  The item table travels through a pinned staging copy and an asynchronous copy on
 * `stream`.  The call does not wait for the device: a stream's workspace keeps a ring of staging copies and takes one whose
 * upload has already run, or adds one (a few KB); only with 64 grouped calls all still queued on one stream does a call wait
 * for the oldest upload.  A CAPTURED call takes over a pinned staging copy of its own (left behind by the eager call of the
 * same shape), which the graph re-reads at every replay: it is kept until the index is freed, one per capture. */
int mvdb_index_search_grouped_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int normalize_q,
                                     const mvdb_rowset* const* sets, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                     void* stream);

/* RANGE SEARCH: every selected row whose score reaches a threshold, instead of the k best (faiss.IndexFlat.range_search
 * beside search).  rs == NULL: every row; else the resident row set (list or bitmap).  cap: the most results per query the
 * caller has room for, >= 0.
 *   counts[i]  = number of selected rows whose score reaches the threshold (inner product: score >= threshold; L2: squared
 *                distance <= threshold), WHATEVER cap is.  cap == 0 is a pure count; D / I may then be NULL.
 *   counts[i] <= cap: row i of (D [nq,cap], I [nq,cap]) holds those rows best first, exact ties to the lower row (for an
 *                unsorted row list: to the lower list position, as mvdb_index_search_rowset); labels are row numbers; the
 *                tail is -1 / -FLT_MAX (inner product) or +FLT_MAX (L2) as everywhere.
 *   counts[i] >  cap: row i holds only missing markers — the order in which the device appends results is not defined, so a
 *                partial answer would not be reproducible; call again with cap >= counts[i].
 * Bit identity: every returned score is bit for bit the score mvdb_index_search / mvdb_index_search_rowset returns for that
 * (query, row) with nq = 1 on the default routing; row i equals the leading counts[i] entries of that call with
 * k = counts[i], and entry counts[i] + 1 of a longer one, if there is one, is below the threshold.
 * Corpus passes.  A single query, an L2 index and a list-form row set take one pass over the fp32 rows per query.
 * A batch may share passes instead.  It is eligible if the index is inner product, the call names every row or a
 * bitmap-form set, and the index's shape keeps an fp16 shadow (mvdb_index_shadow_rows).  Option "range_shared" decides:
 * 0 never (the default: the route has not been timed yet), 1 from 33 queries on, 2 wherever the call
 * is eligible.
 * On the shared route one pass over the shadow per 128 / 256 queries names every row whose fp16 score is not provably below
 * the query's threshold (band: mvdb_range_band).  The exact kernel re-scores those rows in the single-query scan's
 * arithmetic and decides.  A query with more candidates than the route holds per query (option "range_candidates":
 * 64 .. 2^20, 0 = default = max(2 cap rounded up to a power of two, 4096), at most 256 MiB of candidates per launch) is
 * answered by its own fp32 pass, enabled on the device.  The results are the same bits on every route.  The route builds the
 * shadow as a batch search does (first eligible call, never while the stream is capturing: such a call takes the per-query
 * passes).
 * A NaN threshold is MVDB_ERR_ARG; -inf (inner product) selects every row whose score is not NaN; rows with NaN scores never
 * match.  A stale or foreign row set: MVDB_ERR_ARG before anything is enqueued, nothing written.  Empty index: counts 0.
 * The host entry point reads the counts back before it sorts, so its sort and its copy are sized by the results, not by cap.
 * Workspace: nq x (cap rounded up to a power of two) 8-byte keys — not nq x n scores.  No reference counterpart (the
 * reference's autocut heuristic serves the same wish on a fixed k). */
int mvdb_index_range_search(const mvdb_index* idx, const float* q_host, int nq, float threshold, int normalize_q,
                            const mvdb_rowset* rs, int64_t cap, int64_t* counts_host, float* D_host, int64_t* I_host);
/* Device-resident variant under the contract of mvdb_index_search_device: queries, counts and outputs in device memory,
 * enqueued on `stream`, no synchronisation, one search at a time per (index, stream); labels are row numbers +
 * label_offset.  Its sort is sized by cap (each block looks its query's count up on the device and sorts no more than that).
 * Capturable into a hipGraph after one eager call of the same shape (same nq, cap, set) has sized the workspace. */
int mvdb_index_range_search_device(const mvdb_index* idx, const float* q_dev, int nq, float threshold, int normalize_q,
                                   const mvdb_rowset* rs, int64_t cap, int64_t label_offset, int64_t* counts_dev,
                                   float* D_dev, int64_t* I_dev, void* stream);
/* PER-QUERY THRESHOLDS: the contract of mvdb_index_range_search / _device word for word, with `threshold` read as
 * thresholds[i] for query i (counts, cap, overflow markers, ties, labels, NaN rows, stale or foreign sets, the empty index,
 * both metrics, capturability, routing).  A NaN entry of the HOST array is MVDB_ERR_ARG before anything is enqueued; the
 * device variant cannot look: a NaN threshold there matches nothing (count 0). */
int mvdb_index_range_search_each(const mvdb_index* idx, const float* q_host, int nq, const float* thresholds_host /*[nq]*/,
                                 int normalize_q, const mvdb_rowset* rs, int64_t cap, int64_t* counts_host, float* D_host,
                                 int64_t* I_host);
int mvdb_index_range_search_each_device(const mvdb_index* idx, const float* q_dev, int nq, const float* thresholds_dev /*[nq]*/,
                                        int normalize_q, const mvdb_rowset* rs, int64_t cap, int64_t label_offset,
                                        int64_t* counts_dev, float* D_dev, int64_t* I_dev, void* stream);
/* The band of the shared pass: for a query of norm qnorm and any stored row x, |x| <= row_norm_bound,
 * the fp16 nomination score lies within the returned value of the fp32 score the exact scans compute (in the scans' own
 * summation order, for the widths that keep a shadow).  Below 1e-3 * qnorm * row_norm_bound at d = 1024.  Pure host arithmetic
 * (no device needed); linear in qnorm and in row_norm_bound. */
double mvdb_range_band(int d, float qnorm, float row_norm_bound);
/* Diagnostics of the shared pass, read without synchronising (the device-side words lag by the calls in flight): calls that
 * took it, queries its fallback answered (running total), candidates held by the latest launch group of up to 1024 queries.
 * Any pointer may be NULL. */
int mvdb_index_range_counters(const mvdb_index* idx, long long* shared_calls, long long* fallback_queries,
                              long long* last_candidates);

/* RANGE JOIN: which stored rows are near each other — a range search whose queries are stored rows, each matched against
 * the rows stored BEFORE it, so that every pair is found once, from its later member (duplicate checks over a corpus, or
 * over the rows a bulk add appended).  The contract is mvdb_index_range_search's, word for word (counts, cap, overflow
 * markers, cap == 0, ties, labels, NaN rows, stale or foreign sets), with two differences:
 *   - query i is stored row qrows[i], with its fp32 bits as they sit in the matrix and normalize_q = 0.  It is never
 *     uploaded; only the row numbers travel.
 *   - only rows whose row number is below qrows[i] can match.
 * So counts[i] is the true number of rows j < qrows[i] that are in rs (if given) and whose score reaches the threshold
 * (inner product: score >= threshold; L2: squared distance <= threshold), and row i of (D, I) lists them best first.  Every
 * returned score is bit for bit what mvdb_index_range_search returns for the query get_rows(qrows[i]) with normalize_q = 0;
 * order and labels match too.  qrows may be in any order and may repeat; a query row need not be in rs; rows appended after
 * rs was created are not in the set, as for every row-set call.
 * Argument errors are MVDB_ERR_ARG before anything is enqueued, nothing written: NULL buffers (D / I may be NULL with
 * cap == 0), nq <= 0, a NaN threshold, cap < 0, a row number outside [0, ntotal), a row set of another index.
 * Corpus passes.  Option "join_shared": 0 never shares — one fp32 pass per query row, ended at the row's own bound (the
 * correctness baseline); 1 (default) shares where mvdb_index_range_search's batches may (inner product, every row or a
 * bitmap-form set, an index that keeps an fp16 shadow) from 33 query rows on; 2 wherever the call is eligible.  The default
 * is 1, not 0 as "range_shared": a join has as many queries as rows, and the per-query route costs rows x rows x d x 4 / 2
 * bytes.  On the shared route one pass over the shadow per 128 / 256 query rows covers rows [0, largest bound of those
 * query rows) and admits a row for a query only below the query's bound; the band is mvdb_range_band unchanged (the queries
 * are not re-normalised), the exact re-score and the per-query fallback (option "range_candidates" sizes the candidate
 * segments) are the range search's.  Both metrics, every width, padded rows and indexes that hold non-finite rows work,
 * through the per-query route.  The results are the same bits on every route.
 * A device-resident, capturable _device variant is out of scope: this entry point reads the counts back before it sorts. */
int mvdb_index_range_join(const mvdb_index* idx, const int64_t* qrows_host /*[nq] row numbers, each in [0, ntotal)*/, int nq,
                          float threshold, const mvdb_rowset* rs /*NULL: every row*/, int64_t cap,
                          int64_t* counts_host /*[nq]*/, float* D_host /*[nq, cap]*/, int64_t* I_host /*[nq, cap]*/);
/* Diagnostics of the join's shared pass, counters of its own (mvdb_index_range_counters keeps reporting range calls only):
 * calls that took it, query rows its fallback answered (running total, read without synchronising).  Any pointer may be NULL. */
int mvdb_index_join_counters(const mvdb_index* idx, long long* shared_calls, long long* fallback_queries);

/* MMR SEARCH (maximal marginal relevance): k rows that are relevant AND unlike each other, picked greedily on the device from
 * the fetch_k best — the answer to a top-k that is k near-copies of one passage.  Inner-product indexes only.
 * Candidates.  The candidates of query i are, bit for bit, row i of what mvdb_index_search (rs == NULL) or
 * mvdb_index_search_rowset returns for the same (q, nq, fetch_k, normalize_q): the same routing, tie order and -1 padding.
 * rel[j] is the fp32 score of candidate position j.
 * Selection, per query.  Step 0 picks position 0.  Step t >= 1 picks the not yet picked valid position j that maximises
 *     obj[j] = lambda * rel[j] - (1 - lambda) * max over the picked p of s(p, j)
 * in fp32 (1 - lambda rounded once, each product rounded, then the difference), where s(p, j) is the fp32 inner product of
 * the two STORED rows as they sit in the matrix — the quantity the relevance is.  Ties go to the lower candidate position
 * (the lower row number, or the lower list position for an unsorted list: the search's own tie order).  A NaN objective
 * compares as -inf.  The summation order of s depends on d alone, not on the position, the step, the query's place in the
 * batch or the form below: exact duplicate rows score bit-identically and a call is reproducible run to run.
 * lambda = 1 returns the first k candidates (while every s is finite); lambda = 0 ignores relevance after the first pick.
 * Output.  Row i of I [nq,k]: the picked rows in selection order (row numbers; + label_offset in the device variant); row i
 * of D [nq,k]: their rel values, the very bits the search returned.  A query with fewer than k valid candidates is padded
 * with -1 / -FLT_MAX.
 * Arguments.  1 <= k <= fetch_k <= 1024; lambda in [0, 1] (NaN or outside: MVDB_ERR_ARG); an L2 index: MVDB_ERR_ARG; a stale
 * or foreign row set: MVDB_ERR_ARG before anything is enqueued, nothing written; an empty index or set: all missing markers.
 * Cost.  The candidate search, then ONE launch, a workgroup per query, k - 1 passes over the candidates' rows:
 * mvdb_mmr_form says from where — 0: the fetch_k rows are gathered into LDS once (fetch_k * ld * 4 bytes; the everyday shapes,
 * fetch_k 20 - 64 at d <= 512), 1: every pass reads them from the matrix through L2 ((k - 1) * fetch_k * ld * 4 bytes per
 * query, at most fetch_k * ld * 4 distinct).  The rule looks at d, fetch_k and the device's LDS only; < 0: error.
 * Workspace: nq (at most 1024 at a time) x fetch_k candidates, never anything sized by the index.
 * The device variant follows the contract of mvdb_index_search_device: no synchronisation, no host read, one call at a time
 * per (index, stream), capturable into a hipGraph after one eager call of the same shape has sized the workspace.
 * No reference counterpart (its autocut and hybrid_rerank_results work on a fixed top-k after the fact). */
int mvdb_index_search_mmr(const mvdb_index* idx, const float* q_host, int nq, int k, int fetch_k, float lambda,
                          int normalize_q, const mvdb_rowset* rs, float* D_host, int64_t* I_host);
int mvdb_index_search_mmr_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int fetch_k, float lambda,
                                 int normalize_q, const mvdb_rowset* rs, int64_t label_offset,
                                 float* D_dev, int64_t* I_dev, void* stream);
int mvdb_mmr_form(int d, int fetch_k, int device);   /* 0 = candidates held in LDS, 1 = streamed; < 0 = error */

/* DISTINCT SEARCH: the best row of each GROUP of stored rows, the k best groups — "the k best documents" of a store whose
 * documents are chunked into several rows.  Inner-product indexes only.
 * Grouping.  One int32 group code per stored row, resident on the index's device (4 bytes per row).  n must equal
 * mvdb_index_ntotal, every code must lie in [0, n_groups), 1 <= n_groups <= n: anything else is MVDB_ERR_ARG before any
 * allocation (the host array is checked on the host).  n == 0 gives an empty grouping without device memory, for an empty
 * index.  A grouping belongs to the index state it was built against: a search refuses it with MVDB_ERR_ARG, before anything
 * is enqueued and with nothing written, when it belongs to another index, when rows were added since (the row count
 * differs) or when rows were removed since.  mvdb_index_set_rows renumbers nothing: the grouping stays valid.  There is no
 * extend call: re-creating a grouping after a write is one upload (4 MB per million rows).
 * Contract, per query i.  m: the rows selected (ntotal, or mvdb_rowset_size(rs)).  R_i: row i of what mvdb_index_search
 * (rs == NULL) or mvdb_index_search_rowset returns for the same (q, nq, fetch_k, normalize_q) — its routing, bits, tie order
 * and -1 padding; v: its valid entries, g: the distinct codes among them.  The COLLAPSE of a ranking keeps, in order, the
 * first entry of every group.
 *   Tier 1 (g >= k, or v < fetch_k, or fetch_k >= m): the first k entries of the collapse of R_i, bit for bit.  Exact: a
 *   group absent from R_i has no row above R_i's last score, so the k best groups are the first k it holds, each by its best
 *   row; and an R_i that is not full, or covers the selection, is the whole ranking.
 *   Tier 2 (otherwise: R_i is full, does not cover the selection and holds fewer than k groups — one document fills the
 *   fetch): the first k entries of the collapse of the FULL ranking of the selected rows, i.e. of what mvdb_index_search /
 *   mvdb_index_search_rowset returns for query i alone with nq = 1 and k = m on the default routing: the scores are bit for
 *   bit the single-query scan's, ties go to the lower row number (an unsorted row list: the lower list position), rows whose
 *   score is NaN are never results.
 *   In a batch, a tier-2 query therefore carries the single-query scan's bits while its tier-1 neighbours carry the bits of
 *   the route the batch took.
 * Output.  I [nq,k]: row numbers (+ label_offset in the device variant), best group first; D [nq,k]: their scores; G [nq,k]
 * (may be NULL): their group codes.  Fewer than k groups: padded with -1 / -FLT_MAX / -1.  Reproducible run to run.
 * Arguments.  1 <= k <= 64 (tier 2 keeps one result per lane of a wave), k <= fetch_k <= 1024; an L2 index: MVDB_ERR_ARG;
 * rs == NULL: every row, else a resident row set of any form, checked as every row-set search checks it; an empty index or
 * set: all missing markers.
 * Cost.  The candidate search, then ONE launch, a workgroup per query, that reads no row of the matrix.  Behind it, unless
 * fetch_k >= m, three launches per T queries that cost a query answered by tier 1 nothing: they clear, fill and read a
 * table of T x n_groups x 8 bytes, T = max(1, min(queries, budget / (8 n_groups))), budget = index option
 * "distinct_table_bytes" (default 256 MiB).  A tier-2 query costs one exact scan of the selected rows + 4 bytes per row.
 * The device variant follows the contract of mvdb_index_search_device: no synchronisation, no host read, one call at a time
 * per (index, stream), capturable into a hipGraph after one eager call of the same shape (same grouping, same set).
 * mvdb_index_distinct_counters: calls served (counted on the host) and queries tier 2 answered (a running total, read
 * without synchronising: the device-side word lags by the calls in flight).  Either pointer may be NULL.
 * No reference counterpart. */
typedef struct mvdb_grouping mvdb_grouping;
int mvdb_grouping_create(const mvdb_index* idx, const int32_t* codes_host /*[n]*/, int64_t n, int64_t n_groups, mvdb_grouping** out);
int64_t mvdb_grouping_rows(const mvdb_grouping* g);
int64_t mvdb_grouping_groups(const mvdb_grouping* g);
int mvdb_grouping_free(mvdb_grouping* g);
int mvdb_index_search_distinct(const mvdb_index* idx, const float* q_host, int nq, int k, int fetch_k, int normalize_q,
                               const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_host, int64_t* I_host,
                               int32_t* G_host /* [nq,k] or NULL */);
int mvdb_index_search_distinct_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int fetch_k, int normalize_q,
                                      const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_dev, int64_t* I_dev,
                                      int32_t* G_dev /* [nq,k] or NULL */, int64_t label_offset, void* stream);
int mvdb_index_distinct_counters(const mvdb_index* idx, long long* calls, long long* fallback_queries);

/* GROUP HITS SEARCH: the k best groups of stored rows, each with its group_size best rows — "the 5 best documents, and the 3
 * best chunks of each" of a chunked store, in one call.  Inner-product indexes only.  The grouping is distinct search's.
 * Contract, per query i.  m: the rows selected (ntotal, or mvdb_rowset_size(rs)).
 *   Groups.  G[i] is exactly what mvdb_index_search_distinct returns for the same (q, nq, k, fetch_k, normalize_q, grp, rs):
 *   the same k groups in the same order, -1 padded.  The call runs distinct search unchanged, both tiers.
 *   Members.  F_i: the FULL ranking of the selected rows for query i alone, i.e. what mvdb_index_search /
 *   mvdb_index_search_rowset returns with nq = 1 and k = m on the default routing.  For each j with G[i][j] >= 0, D[i][j][:]
 *   and I[i][j][:] are the first group_size entries of F_i whose code is G[i][j], best first: the scores are bit for bit
 *   the single-query scan's, equal scores go to the lower position (the row number; of a row list: the list position), rows
 *   whose score is NaN are never offered, -0.0 sorts below +0.0.  A group with fewer members is padded with -FLT_MAX / -1;
 *   a padding group (G[i][j] == -1) is all padding.  I holds physical rows (+ label_offset for valid entries in the device
 *   variant).
 *   Relation to distinct search.  With nq = 1, D[0][j][0] and I[0][j][0] equal distinct search's (D, I) bit for bit.  With
 *   nq > 1 the heads come from the member pass like every other member, so they carry the single-query scan's bits, while
 *   distinct search's candidate search may have ranked near-ties with the bits of the route the batch took: G is its
 *   answer, and a head may then differ from distinct search's row where two rows of a group tie to within those bits.
 * Arguments.  1 <= k <= 64, 1 <= group_size <= 16, fetch_k as for distinct search (k <= fetch_k <= 1024); an L2 index:
 * MVDB_ERR_ARG.  A stale or foreign grouping or row set is refused as distinct search refuses it: before anything is enqueued,
 * with nothing written.  An empty index or an empty set: all padding.
 * Cost.  Distinct search, then per T queries two launches.  The first streams the selected rows' CODES — 4 bytes per row
 * (+ 8 of a row list, + 1 bit of a bitmap) — and reads from the matrix only the rows whose code is one of the query's k
 * groups; it writes one list of k x group_size keys per workgroup.  The second merges them, one workgroup per query.
 * T = max(1, min(queries, budget / (grid x k x group_size x 8))), budget = index option "groups_partials_bytes" (default
 * 64 MiB): the answer does not depend on T.  Every list is a maximum over integer keys: reproducible run to run, no
 * floating-point atomics.
 * The device variant follows the contract of mvdb_index_search_distinct_device: no synchronisation, no host read, one call at
 * a time per (index, stream), capturable into a hipGraph after one eager call of the same shape (same grouping, same set).
 * mvdb_index_groups_counters: calls served (counted on the host) and member_rows, the running total of selected rows whose
 * code was one of their query's k groups — rows scoring NaN included —, read without synchronising: the device-side word
 * lags by the calls in flight.  Either pointer may be NULL.
 * No reference counterpart. */
int mvdb_index_search_groups(const mvdb_index* idx, const float* q_host, int nq, int k, int group_size, int fetch_k, int normalize_q,
                             const mvdb_grouping* grp, const mvdb_rowset* rs /* or NULL */, float* D_host /* [nq,k,group_size] */,
                             int64_t* I_host /* [nq,k,group_size] */, int32_t* G_host /* [nq,k] or NULL */);
int mvdb_index_search_groups_device(const mvdb_index* idx, const float* q_dev, int nq, int k, int group_size, int fetch_k,
                                    int normalize_q, const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_dev, int64_t* I_dev,
                                    int32_t* G_dev /* [nq,k] or NULL */, int64_t label_offset, void* stream);
int mvdb_index_groups_counters(const mvdb_index* idx, long long* calls, long long* member_rows);

/* MAXSIM SEARCH: ONE question that is T query vectors (sub-questions, paraphrases, the token states of a late-interaction
 * encoder); a GROUP of stored rows — a document — scores the sum, over the vectors, of its best row for each vector.
 * Inner-product indexes only.  One call is one question; a batch is a loop of calls (a call is a corpus pass of milliseconds).
 * Contract.  Groups come from an mvdb_grouping (above), the selected rows are all rows (rs == NULL) or those of a resident
 * row set of any form.
 *   Per-vector maximum m[t][g], for every group g with at least one selected row and every vector t: the maximum over the
 *   selected rows of g of the inner product of the row and q_t, each score BIT FOR BIT the single-query scan's — what
 *   mvdb_index_search / mvdb_index_search_rowset returns for q_t alone with nq = 1 and k = the rows selected (tier 2 of
 *   distinct search defines its scores the same way).  normalize_q normalises every vector on its own, with the scan's own
 *   prologue.  A row whose score is NaN is never offered.  Equal scores inside a group go to the lower position (row number;
 *   of a row list: the list position).  Scores are ordered as the scan's keys order them: -0.0 below +0.0.
 *   Group score S[g] = m[0][g], then S = S + m[t][g] for t = 1 .. T-1: plain fp32 adds in this order.  A group that has no
 *   offer for some t (every selected row of it scored NaN there) is never a result; nor is a group whose S is NaN (+inf and
 *   -inf met).  +inf ranks first, -inf last.
 * Output.  The k groups with the largest S, best first, equal S to the LOWER group code: D [k] = S, G [k] = the code;
 * I_tok [k,T] (may be NULL): the row that gave m[t][G[j]], a physical row number (+ label_offset in the device variant);
 * D_tok [k,T] (may be NULL): m[t][G[j]].  Fewer than k groups: padded with -FLT_MAX / -1 / -1 / -FLT_MAX.  Reproducible run
 * to run: integer maxima and a fixed order of the adds.
 * Arguments.  1 <= T <= 256, 1 <= k <= 64; an L2 index: MVDB_ERR_ARG.  The grouping and the row set are checked as
 * mvdb_index_search_distinct checks them: refused before anything is enqueued, with nothing written.  An empty index or an
 * empty set: all padding.
 * Cost.  A table of T x n_groups x 8 bytes, group-major, held whole for the call: above the index option
 * "maxsim_table_bytes" (default 2 GiB) the call is MVDB_ERR_ARG and the message states the bytes needed.  One launch clears
 * it; ceil(T / Tp) passes over the selected rows fill it, each scoring every row against Tp of the vectors held in LDS,
 * Tp = min(T, 32, 128 KiB / (4 ld)) with ld the row stride in floats (d rounded up to 4); the index option
 * "maxsim_tokens_per_pass" (1 .. 32; 0, the default: that rule) lowers it — for tests and for measuring what a pass per
 * vector costs.  Results do not depend on Tp.  Two launches pick the k groups and write the outputs.
 * The device variant follows the contract of mvdb_index_search_distinct_device: no synchronisation, no host read, one call at
 * a time per (index, stream), capturable into a hipGraph after one eager call of the same shape (same grouping, same set).
 * mvdb_index_maxsim_counters: calls served and corpus passes enqueued, both counted on the host.  Either pointer may be NULL.
 * No reference counterpart. */
int mvdb_index_search_maxsim(const mvdb_index* idx, const float* q_host /*[T,d]*/, int T, int k, int normalize_q,
                             const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_host /*[k]*/, int32_t* G_host /*[k]*/,
                             int64_t* I_tok_host /*[k,T] or NULL*/, float* D_tok_host /*[k,T] or NULL*/);
int mvdb_index_search_maxsim_device(const mvdb_index* idx, const float* q_dev /*[T,d]*/, int T, int k, int normalize_q,
                                    const mvdb_grouping* grp, const mvdb_rowset* rs, float* D_dev, int32_t* G_dev,
                                    int64_t* I_tok_dev /*[k,T] or NULL*/, float* D_tok_dev /*[k,T] or NULL*/,
                                    int64_t label_offset, void* stream);
int mvdb_index_maxsim_counters(const mvdb_index* idx, long long* calls, long long* passes);

/* ASSIGN AND K-MEANS: questions about the WHOLE corpus in terms of C vectors.  mvdb_index_assign labels every stored row with
 * the nearest (largest inner product) of C vectors; mvdb_index_kmeans clusters the rows into C clusters with spherical k-means
 * (Lloyd's algorithm under the inner product, centres of unit length).  Inner-product indexes only: nearest by L2 is out of
 * scope, an L2 index is MVDB_ERR_ARG.
 * ASSIGN.  The selected rows are all rows (rs == NULL) or those of a resident row set of any form.
 *   Outputs are indexed by PHYSICAL row number, [ntotal], whatever form the set has — list, bitmap or excluded.  A row that
 *   is not selected gets label -1 and score -FLT_MAX; an empty index or an empty set gives all padding.
 *   Scores.  For a selected row r and vector j the score is BIT FOR BIT what mvdb_index_search / mvdb_index_search_rowset
 *   returns for c_j alone with nq = 1: the scan's chunk order and butterfly, as MaxSim search defines its scores.  normalize_c
 *   normalises every vector on its own, with the scan's own prologue.
 *   Labels.  labels[r] is the j with the largest score, scores ordered as the scan's keys order them (-0.0 below +0.0); equal
 *   scores go to the LOWER j; a NaN score is never a candidate; a row whose every score is NaN gets -1 / -FLT_MAX.  scores[r]
 *   (may be NULL) is the winning score.  Reproducible run to run.
 *   Arguments.  1 <= C <= 4096 — a guard, not a measured limit: every Vp vectors are one corpus pass.  A stale or foreign row
 *   set is refused before anything is enqueued, with nothing written, as mvdb_index_search_maxsim refuses one.
 *   Cost.  ceil(C / Vp) passes over the selected rows, each scoring every row against Vp of the vectors held in LDS,
 *   Vp = min(C, 32, 128 KiB / (4 ld)) — MaxSim's rule; the index option "assign_vectors_per_pass" (1 .. 32; 0, the default:
 *   that rule) lowers it.  Results do not depend on Vp: a row's running best is carried across the passes as one 64-bit
 *   (score, inverted j) word, merged by the lanes that own the row with a plain read-compare-write — no floating-point
 *   atomics, no dependence on the order of arrival, no workgroup waits for another.  Workspace: 8 bytes per stored row plus
 *   the staged vectors (the host variant packs label and score into the row's word for its one copy back).
 *   The device variant does no synchronisation and no host read; one call at a time per (index, stream).  Capture into a
 *   hipGraph is not supported.
 *   mvdb_index_assign_counters: assignments served (those k-means runs included) and corpus passes enqueued, both counted on
 *   the host.  Either pointer may be NULL.
 * K-MEANS.  The loop, exactly (a numpy restatement reproduces every bit: tests/kmeans_oracle.py):
 *     centres = the initial centres, each normalised by the scan's prologue
 *     for it = 1 .. max_iter:
 *         labels = assign(centres)
 *         if it > 1 and no label changed: stop          (one 8-byte read per iteration: a bulk call)
 *         centres = update(labels, centres)
 *     if the loop ran out: labels = assign(centres)
 *   so the returned labels / scores ALWAYS equal assign(returned centres).  update, for cluster c: its member rows in ascending
 *   physical row number, cut into chunks of 256 members; each chunk summed element-wise, sequentially in member order, in
 *   fp64; the chunk partials summed sequentially in chunk order, in fp64 (both sums START at their first term); divided by the
 *   count in fp64; norm = the square root of the sequential fp64 sum of the squares (product rounded, then added), in element
 *   order; centre = (float)(mean / norm).  IEEE fp64 throughout.  A cluster with no members keeps its centre; so does one whose
 *   norm is not a positive finite number (a zero or non-finite mean).  Rows labelled -1 belong to no cluster.
 *   Outputs.  centres [C,d]: in, the initial centres; out, the final ones.  labels / scores [ntotal] (either may be NULL) as
 *   assign writes them; counts [C]: members under the returned labels; *iterations (may be NULL): updates performed.
 *   Bit-identical run to run: the member lists are a stable counting sort (per-slice histograms, a column scan, an ordered
 *   scatter inside each slice) and no sum depends on scheduling.  No floating-point atomics.
 *   Arguments.  Those of assign, and max_iter >= 1.
 *   Workspace.  assign's 8 bytes per stored row; the centres; two label arrays and the member lists, 4 bytes per stored row
 *   each; the list build's counts, 4 C x min(ceil(n / 2048), 2048) bytes; and (n / 256 + C) x d fp64 chunk partials.
 * No reference counterpart (the reference delegates its arithmetic to faiss, whose Kmeans is the sibling of IndexFlatIP). */
int mvdb_index_assign(const mvdb_index* idx, const float* c_host /*[C,d]*/, int C, int normalize_c, const mvdb_rowset* rs /*NULL: every row*/,
                      int32_t* labels_host /*[ntotal]*/, float* scores_host /*[ntotal] or NULL*/);
int mvdb_index_assign_device(const mvdb_index* idx, const float* c_dev /*[C,d]*/, int C, int normalize_c, const mvdb_rowset* rs,
                             int32_t* labels_dev /*[ntotal]*/, float* scores_dev /*[ntotal] or NULL*/, void* stream);
int mvdb_index_assign_counters(const mvdb_index* idx, long long* calls, long long* passes);
int mvdb_index_kmeans(const mvdb_index* idx, float* centres_host /*[C,d] in: initial centres, out: final*/, int C, int max_iter,
                      const mvdb_rowset* rs, int32_t* labels_host /*[ntotal] or NULL*/, float* scores_host /*[ntotal] or NULL*/,
                      int64_t* counts_host /*[C]*/, int* iterations /*or NULL*/);

/* PROBED SEARCH: the stored rows partitioned into C member lists by their nearest centre; a query is scored against the C
 * centres and only the lists of its nprobe best centres are scanned.  The library's one APPROXIMATE route: it is taken only
 * by these entry points, never by another call.  Only the choice of lists is approximate — given the lists, the answer is
 * exact and bit for bit the single-query scan's.  Inner-product indexes only: an L2 index is MVDB_ERR_ARG, as for assign.
 * Partition.  A resident object, a sibling of mvdb_grouping, on the index's device: the centres [C, ld] in fp32 after their
 * own normalisation, one int32 label per stored row, the member lists as uint32 row numbers — ascending inside each list —
 * and C + 1 offsets: 8 bytes per stored row plus the centres.  1 <= C <= 4096 (assign's guard).
 *   create.  normalize_c normalises each centre with the scan's prologue, exactly as assign does.  labels_host == NULL: the
 *   library labels every row itself with assign's pass; the labels are integer for integer what mvdb_index_assign(centres,
 *   normalize_c) returns.  labels_host given: used as is, each checked on the host to lie in [-1, C); they need not be the
 *   nearest centres.  A row labelled -1 is in no list and is never a result (so a row that scores NaN against every centre).
 *   The lists come from the stable counting sort of k-means: they do not depend on scheduling.
 *   Validity.  The partition belongs to its index, identified by the index's serial number, not its address.  A search refuses
 *   with MVDB_ERR_ARG, before anything is enqueued and with nothing written, when the partition belongs to another index,
 *   when the row count differs (rows were added since) or when rows were removed since.  mvdb_index_set_rows renumbers
 *   nothing: the partition stays valid, a changed row stays in its old list and is scored with its new vector until update
 *   names it.
 *   update.  Brings the partition to the index's current state after adds and set_rows: the rows [mvdb_partition_rows(p),
 *   ntotal) and the m listed rows are assigned to their nearest centres — one assign under a list-form selection of just
 *   those rows, their new labels again what mvdb_index_assign gives for them —, written into the label array, and the lists
 *   are rebuilt.  Cost: the rows touched plus one counting sort over the labels.  After a removal it is refused: read the
 *   labels back (mvdb_partition_labels), drop the removed rows' and re-create from them.  update excludes the searches and
 *   readers of the same partition (host calls; searches enqueued by the device variant must have finished).
 *   labels / centres / sizes read the label array, the stored centres [C,d] and the list sizes [C] back; rows is the row
 *   count the partition covers, lists is C.
 * Search contract, per query i.
 *   Probes.  P_i is the set of valid entries of what mvdb_index_search returns for (q_i, nq = 1, k = nprobe, normalize_q) on an
 *   inner-product index whose rows are exactly the partition's stored centres, as mvdb_partition_centres returns them, added
 *   without normalisation: that call's scores, its order, ties to the lower centre, NaN never a candidate.  An empty list
 *   still takes a probe slot.
 *   Result.  Row i of (D, I) is bit for bit what mvdb_index_search_rowset returns with nq = 1 and the same k for the ascending
 *   list of the rows whose label lies in P_i, restricted to the rows of rs when rs is given: scores are the single-query
 *   scan's bits for the index's (G, C, MASKED) shape, ties go to the lower row number, padding is -1 / -FLT_MAX, labels are
 *   row numbers (+ label_offset in the device variant); a query whose every score is NaN gets all missing markers.
 *   nprobe = C: the exact search over every row whose label is >= 0.
 * Arguments.  nq >= 1, 1 <= k <= 64, 1 <= nprobe <= C.  rs: NULL or a BITMAP-form set (mvdb_rowset_is_bitmap), excluded form
 *   included, checked like every row-set search checks it (a stale or foreign set is refused); a LIST-form set is
 *   MVDB_ERR_ARG — a filter that small is already cheap on the exact gathered scan (mvdb_index_search_rowset).
 * Cost.  Per chunk of queries four launches: the coarse scores (the single-query scan over the centre matrix, a grid row per
 *   query), the plan (a workgroup per query orders its C keys in LDS, keeps nprobe and cuts their lists into work items of
 *   128 list positions), the gathered scan of the items (the grid is sized on the host from the nprobe LARGEST lists;
 *   blocks beyond a query's real item count return at once) and a segmented merge.  Bytes: the centres, then (4 ld + 4) per
 *   row of the probed lists.  The item and candidate tables of a chunk stay within the index option "probe_table_bytes"
 *   (default 256 MiB; at least one query per chunk); results do not depend on the chunking.
 * The device variant does no synchronisation and no host read; one call at a time per (index, stream).  Capture into a
 * hipGraph is not supported: a capturing stream is MVDB_ERR_ARG.
 * mvdb_index_probe_counters: probed searches served and launches they enqueued, both counted on the host.  Either pointer may
 * be NULL.
 * No reference counterpart. */
typedef struct mvdb_partition mvdb_partition;
int mvdb_partition_create(const mvdb_index* idx, const float* centres_host /*[C,d]*/, int C, int normalize_c,
                          const int32_t* labels_host /*[ntotal], each in [-1, C); or NULL*/, mvdb_partition** out);
int mvdb_partition_update(mvdb_partition* p, const mvdb_index* idx, const int64_t* changed_rows_host /*[m] or NULL*/, int64_t m);
int mvdb_partition_labels(const mvdb_partition* p, int64_t row0, int64_t n, int32_t* labels_host /*[n]*/);
int mvdb_partition_centres(const mvdb_partition* p, float* centres_host /*[C,d]*/);
int mvdb_partition_sizes(const mvdb_partition* p, int64_t* counts_host /*[C]*/);
int64_t mvdb_partition_rows(const mvdb_partition* p);
int mvdb_partition_lists(const mvdb_partition* p);
int mvdb_partition_free(mvdb_partition* p);
int mvdb_index_search_probe(const mvdb_index* idx, const mvdb_partition* p, const float* q_host, int nq, int k, int nprobe,
                            int normalize_q, const mvdb_rowset* rs /*NULL or a bitmap-form set*/, float* D_host, int64_t* I_host);
int mvdb_index_search_probe_device(const mvdb_index* idx, const mvdb_partition* p, const float* q_dev, int nq, int k, int nprobe,
                                   int normalize_q, const mvdb_rowset* rs, int64_t label_offset, float* D_dev, int64_t* I_dev,
                                   void* stream);
int mvdb_index_probe_counters(const mvdb_index* idx, long long* calls, long long* probe_launches);

/* SEARCH BY EXAMPLES: the question is stored-style vectors, not a query — "more like these P, unlike those N" (what other
 * stores call recommend).  v is [P + N, d]: the P positives, then the N negatives.  Inner-product indexes only: an L2 index
 * is MVDB_ERR_ARG, as for assign.  The selected rows are all rows (rs == NULL) or those of a resident row set of any form —
 * list, bitmap or excluded.
 * Score ("best score" rule), for a selected row r:
 *   s(v, r) is BIT FOR BIT what mvdb_index_search / mvdb_index_search_rowset returns for v alone with nq = 1: the scan's chunk
 *   order and butterfly, as MaxSim search and assign define their scores.  normalize normalises every vector on its own, with
 *   the scan's own prologue.
 *   bp(r) is the largest s(p_j, r) over the positives whose score is not NaN, scores ordered as the scan's keys order them
 *   (-0.0 below +0.0).  A row with no such positive is never a result.
 *   bn(r) is the same maximum over the negatives; -inf when N = 0 or when every negative scores NaN.
 *   S(r) = bp if bp > bn (the IEEE fp32 comparison), else -(bn * bn) (one fp32 multiply, then a negation): a row that is no
 *   closer to a positive than to a negative is ranked by how far it is from the negatives.
 * Result.  The k rows with the largest S, best first: S ordered as the scan's keys order scores, +inf first, and -inf is still
 *   a result; equal S goes to the LOWER physical row number, for list-form sets too.  Fewer than k rows end in -FLT_MAX / -1.
 *   I holds physical row numbers (+ label_offset in the device variant).  An empty index or an empty set gives all padding.
 *   N = 0: the per-row maximum over the positives.  P = 1, N = 0: mvdb_index_search, bit for bit, minus the skipped rows.
 * Skip rows.  The n_skip listed rows are never results, whatever they score (the examples themselves, when they are stored
 *   rows).  Duplicates are allowed.  They do not touch the row set.  The host variant refuses a row outside [0, ntotal) with
 *   MVDB_ERR_ARG; the device variant, which reads nothing back, ignores such a row.
 * Arguments.  1 <= P, 0 <= N, P + N <= 256, 1 <= k <= 64, 0 <= n_skip <= 1024.  A stale or foreign row set is refused before
 *   anything is enqueued, with nothing written, as mvdb_index_assign refuses one.
 * Cost.  ceil((P + N) / Vp) passes over the selected rows, each scoring every row against Vp consecutive vectors of v held in
 *   LDS (a pass may hold positives and negatives), Vp = min(P + N, 32, 128 KiB / (4 ld)) — MaxSim's rule; the index option
 *   "examples_vectors_per_pass" (1 .. 32; 0, the default: that rule) lowers it.  Results do not depend on Vp: a row's two
 *   running maxima are carried across the passes in one 64-bit word (image of bp | image of bn), merged by the lanes that own
 *   the row with a plain read / max / write — no atomics, no dependence on the order of arrival, no workgroup waits for
 *   another.  Then the skip rows' words are zeroed, and a selection over the ntotal words keeps the k best keys (S, row).
 *   Bytes: passes x (n ld 4 + 8 n) + 16 n.  Workspace: 8 bytes per stored row plus the staged vectors.
 * The device variant does no synchronisation and no host read; one call at a time per (index, stream).  Capture into a
 * hipGraph is not supported: a capturing stream is MVDB_ERR_ARG.
 * mvdb_index_examples_counters: searches by examples served and corpus passes they enqueued, both counted on the host.  Either
 * pointer may be NULL.
 * No reference counterpart. */
int mvdb_index_search_examples(const mvdb_index* idx, const float* v_host /*[P+N,d]: the positives, then the negatives*/, int P, int N,
                               int k, int normalize, const mvdb_rowset* rs /*NULL: every row*/,
                               const int64_t* skip_rows_host /*[n_skip] or NULL*/, int n_skip, float* D_host /*[k]*/, int64_t* I_host /*[k]*/);
int mvdb_index_search_examples_device(const mvdb_index* idx, const float* v_dev /*[P+N,d]*/, int P, int N, int k, int normalize,
                                      const mvdb_rowset* rs, const int64_t* skip_rows_dev /*[n_skip] or NULL*/, int n_skip,
                                      int64_t label_offset, float* D_dev /*[k]*/, int64_t* I_dev /*[k]*/, void* stream);
int mvdb_index_examples_counters(const mvdb_index* idx, long long* calls, long long* passes);

/* BOOSTED SEARCH: something besides the embedding takes part in the SCORE — recency, popularity, authority ("cosine +
 * w * metadata[key]", what other stores call score boosting or a function score), or the per-query scores of a lexical engine
 * (the convex combination of hybrid search: a value on the engine's hits, 0 elsewhere).  A selected row r scores
 *   S(r) = w_s * s(r) + T[r]
 * and the k rows with the largest S are the result: ONE pass over the selected rows, exact over every one of them — a row
 * that wins on S from rank k + 1 of the plain search is found, which no re-ranking of a fetched top-k can promise.
 * mvdb_rowterm: one fp32 value per stored row, resident on the index's device.  mvdb_rowterm_create needs n == ntotal
 *   (MVDB_ERR_ARG otherwise).  A search refuses a term whose row count differs from ntotal — rows were added since — with an
 *   MVDB_ERR_ARG that names both counts, and a term created before a remove_rows / reset (the rule of mvdb_rowset: the rows
 *   were renumbered); mvdb_index_set_rows, which keeps the row numbers, does not outdate it.  mvdb_rowterm_rows: its row
 *   count (-1 for NULL); mvdb_rowterm_free(NULL) is a no-op.
 * Arithmetic — all fp32, every operation rounded on its own (no contraction: numpy float32 arithmetic reproduces every bit):
 *   T[r] = w_1 * t_1[r]; then for j = 2 .. nterms, in call order, T[r] = T[r] + (w_j * t_j[r]).
 *   For each sparse entry (r, v): T[r] = T[r] + v.  With nterms = 0 (sparse entries only) T starts as +0.0.
 *   S = (w_s * s) + T[r]: one multiply, then one add.
 *   s is BIT FOR BIT what mvdb_index_search / mvdb_index_search_rowset returns for the query alone with nq = 1: the scan's
 *   chunk order of fmaf, its xor butterfly, and (normalize_q) its query normalisation prologue.
 * Result.  A row is a candidate iff it is selected and S == S (not NaN: a NaN score, a NaN term, +inf and -inf meeting);
 *   -inf and +inf are ordinary scores.  Best first, S ordered as the scan's keys order scores; equal S goes to the LOWER
 *   physical row number in every row-set form, under an unsorted row list too (the convention of search by examples, not of
 *   mvdb_index_search_rowset).  I holds physical row numbers (+ label_offset in the device variant); fewer than k candidates
 *   end in -FLT_MAX / -1.  One term of -0.0 at weight 1 with w_s = 1 is mvdb_index_search, bit for bit.
 * Arguments.  Inner-product indexes only: an L2 index is MVDB_ERR_ARG.  1 <= k <= 64, 1 <= nq, 0 <= nterms <= 4; nterms = 0
 *   with nsparse = 0 is MVDB_ERR_ARG (nothing to boost by).  Sparse entries need nq = 1; their rows are distinct and inside
 *   [0, ntotal) — both checked on the host, MVDB_ERR_ARG otherwise.  A stale or foreign term or row set is refused before
 *   anything is enqueued.  terms / weights may be NULL when nterms = 0, the sparse arrays when nsparse = 0.
 * Launches.  boost_combine_kernel writes T (4 n (nterms + 1) bytes), boost_scatter_kernel adds the sparse entries, ONE
 *   boost_scan_kernel per 1,024 queries scans the selected rows with the queries as the grid's y dimension — n (4 ld + 4) bytes
 *   per query: the queries of a batch share T, not the corpus pass — and the merge of the block lists writes the results.
 *   Nothing is selected (an empty index, an empty set): no combine, no scan, every output is padding.
 *   Workspace: 4 bytes per stored row.
 * The device variant takes the sparse rows and values as HOST arrays, as mvdb_index_set_rows_device takes its rows.  With
 *   nsparse == 0 it enqueues and returns without a host synchronisation or a read from the device, like its siblings; with
 *   nsparse > 0 it waits once, for the upload of the entries, before it enqueues the rest.  One call at a time per (index,
 *   stream).  Capture into a hipGraph is not supported: a capturing stream is MVDB_ERR_ARG.
 * mvdb_index_boost_combine runs the combine and scatter launches alone and copies T [ntotal] back: the column can be held to
 *   the arithmetic above by itself.  It takes the term, weight and sparse arguments of a search with nq = 1.
 * mvdb_index_boost_counters: boosted searches served (mvdb_index_boost_combine is not one) and boost_scan_kernel launches
 *   enqueued — one per search and 1,024 queries, none where nothing is selected —, both counted on the host.  Either pointer
 *   may be NULL.
 * No reference counterpart. */
typedef struct mvdb_rowterm mvdb_rowterm;
int mvdb_rowterm_create(const mvdb_index* idx, const float* values_host /*[n]*/, int64_t n, mvdb_rowterm** out);
int64_t mvdb_rowterm_rows(const mvdb_rowterm* t);
int mvdb_rowterm_free(mvdb_rowterm* t);
int mvdb_index_search_boosted(const mvdb_index* idx, const float* q_host /*[nq,d]*/, int nq, int k, int normalize_q, float score_weight,
                              const mvdb_rowterm* const* terms /*[nterms]*/, const float* weights /*[nterms]*/, int nterms,
                              const int64_t* sparse_rows_host /*[nsparse] or NULL*/, const float* sparse_values_host /*[nsparse] or NULL*/,
                              int64_t nsparse, const mvdb_rowset* rs /*NULL: every row*/, float* D_host /*[nq,k]*/, int64_t* I_host /*[nq,k]*/);
int mvdb_index_search_boosted_device(const mvdb_index* idx, const float* q_dev /*[nq,d]*/, int nq, int k, int normalize_q, float score_weight,
                                     const mvdb_rowterm* const* terms, const float* weights, int nterms, const int64_t* sparse_rows_host,
                                     const float* sparse_values_host, int64_t nsparse, const mvdb_rowset* rs, int64_t label_offset,
                                     float* D_dev /*[nq,k]*/, int64_t* I_dev /*[nq,k]*/, void* stream);
int mvdb_index_boost_combine(const mvdb_index* idx, const mvdb_rowterm* const* terms, const float* weights, int nterms,
                             const int64_t* sparse_rows_host, const float* sparse_values_host, int64_t nsparse, float* T_host /*[ntotal]*/);
int mvdb_index_boost_counters(const mvdb_index* idx, long long* calls, long long* scan_launches);

/* SPARSE VECTORS AND HYBRID SEARCH: beside its embedding a stored row may hold a SPARSE vector — BM25 or SPLADE weights, the
 * lexical weights a model emits as {token id: weight} — and a sparse query is scored against every one of them: exact sparse
 * top-k, and hybrid search as dense_weight * s(r) + sparse_weight * sparse(r) ranked exactly over every selected row in one
 * pass (not a re-ranking of the dense top-k: a row that wins on the combined score from further down is found).
 * mvdb_sparse: one sparse vector per stored row in CSR form, resident on the index's device.  mvdb_sparse_create needs
 *   n == ntotal, indptr[0] == 0, indptr non-decreasing (indptr[n] = nnz), every index inside [0, dim), the indices of a row
 *   strictly ascending and 1 <= dim <= 2^31 - 1 — all checked on the host, MVDB_ERR_ARG otherwise.  Values may be anything,
 *   non-finite included; empty rows are ordinary.  The store follows mvdb_rowterm's rules: a search refuses it with an
 *   MVDB_ERR_ARG that names both counts when rows were added since, and when it was created before a remove_rows / reset;
 *   mvdb_index_set_rows does not outdate it.  At creation the host also cuts the rows into TILES — consecutive rows with at
 *   most span_entries non-zeros and tile_rows rows, a row longer than the span alone — and uploads the tile table (first
 *   row, first entry): the launches balance by non-zeros and need no device-side scan.  Device memory: 8 bytes per
 *   non-zero + 8 per row.  mvdb_sparse_rows / _nnz / _dim: -1 for NULL; mvdb_sparse_free(NULL) is a no-op.
 *   mvdb_sparse_geometry: span_entries, tile_rows and table_slots of this build (any pointer may be NULL).
 * Query: m distinct indices in any order, 1 <= m <= 1024, each inside [0, dim); a duplicate, m = 0, m > 1024 and an index
 *   out of range are MVDB_ERR_ARG, checked on the host.  A batch is given in CSR form too (q_indptr[0] == 0).
 * Arithmetic — all fp32, every operation rounded on its own (numpy float32 reproduces every bit):
 *   sparse(r): acc = +0.0; for the row's entries IN STORED ORDER whose index is in the query: acc = acc + (q[index] * value).
 *   matched(r) counts the entries used.  (acc is never -0.0, so a skipped entry may add +0.0: the same bits.)
 * mvdb_index_sparse_scores runs the scoring launch alone over every row and copies sparse(r) back, and matched(r) where
 *   matched_host is not NULL: the kernel can be held to the arithmetic above by itself.
 * mvdb_index_search_sparse: a row is a candidate iff it is selected by rs, matched >= 1 and its score is not NaN (a matched
 *   row whose products cancel to 0 is one; -inf and +inf are ordinary scores).  Best first, equal scores to the LOWER
 *   physical row in every row-set form; fewer than k candidates end in -FLT_MAX / -1.  1 <= k <= 64, nq >= 1.  It works on
 *   an index of either metric and never reads the dense matrix.
 * mvdb_index_search_hybrid: S(r) = (dense_weight * s(r)) + (sparse_weight * sparse(r)) — one rounded multiply for the sparse
 *   term, then exactly the boosted search's S = (w_s * s) + T[r].  Every selected row is a candidate (an unmatched row's
 *   sparse term is sparse_weight * +0.0); candidacy, order, ties, padding and limits are the boosted search's, inner-product
 *   indexes only.  The call returns, bit for bit, what mvdb_index_search_boosted returns for the same dense query with one
 *   term — the column of mvdb_index_sparse_scores — at weight sparse_weight and score_weight = dense_weight.
 * Launches.  sparse_scan_kernel: the query sits in LDS as an open-addressed table of table_slots slots; a block streams a
 *   tile's entries with 16-byte loads into an LDS staging buffer of products, then one lane per row adds the row's products
 *   in order.  mvdb_index_sparse_scores: one launch.  mvdb_index_search_sparse: one launch per 1,024 queries — the queries
 *   are the grid's y dimension — and the merge of its block lists; a row LIST is first turned into a bitmap (n / 8 bytes of
 *   workspace).  mvdb_index_search_hybrid: per query the scoring launch writes T into the boosted search's workspace column
 *   (4 bytes per stored row), then boost_scan_kernel and its merge run; the queries of a call follow each other on one
 *   stream over one column.  Nothing is selected (an empty index, an empty set): no launches, every output is padding.
 * The device variants take the sparse queries as HOST arrays (as mvdb_index_search_boosted_device takes its sparse entries)
 *   and wait once, for their upload, before they enqueue the rest; I holds row numbers + label_offset.  One call at a time
 *   per (index, stream).  Capture into a hipGraph is not supported: a capturing stream is MVDB_ERR_ARG.
 * mvdb_index_sparse_counters: sparse and hybrid searches served (mvdb_index_sparse_scores is not one) and sparse_scan_kernel
 *   launches enqueued — one per mvdb_index_sparse_scores, one per sparse search and 1,024 queries, one per query of a hybrid
 *   search, none where nothing is selected —, both counted on the host; a refused call counts nothing.  Either pointer may
 *   be NULL.  (The boost_scan_kernel launches of a hybrid search are counted by mvdb_index_boost_counters' scan_launches.)
 * No reference counterpart. */
typedef struct mvdb_sparse mvdb_sparse;
int mvdb_sparse_create(const mvdb_index* idx, const int64_t* indptr_host /*[n+1]*/, const int32_t* indices_host /*[nnz]*/,
                       const float* values_host /*[nnz]*/, int64_t n, int64_t dim, mvdb_sparse** out);
int64_t mvdb_sparse_rows(const mvdb_sparse* sp);
int64_t mvdb_sparse_nnz(const mvdb_sparse* sp);
int64_t mvdb_sparse_dim(const mvdb_sparse* sp);
int mvdb_sparse_free(mvdb_sparse* sp);
int mvdb_sparse_geometry(int* span_entries, int* tile_rows, int* table_slots);
int mvdb_index_sparse_scores(const mvdb_index* idx, const mvdb_sparse* sp, const int32_t* q_indices_host /*[m]*/, const float* q_values_host /*[m]*/,
                             int m, float* T_host /*[ntotal]*/, int32_t* matched_host /*[ntotal] or NULL*/);
int mvdb_index_search_sparse(const mvdb_index* idx, const mvdb_sparse* sp, const int64_t* q_indptr_host /*[nq+1]*/, const int32_t* q_indices_host,
                             const float* q_values_host, int nq, int k, const mvdb_rowset* rs /*NULL: every row*/, float* D_host /*[nq,k]*/,
                             int64_t* I_host /*[nq,k]*/);
int mvdb_index_search_sparse_device(const mvdb_index* idx, const mvdb_sparse* sp, const int64_t* q_indptr_host, const int32_t* q_indices_host,
                                    const float* q_values_host, int nq, int k, const mvdb_rowset* rs, int64_t label_offset, float* D_dev /*[nq,k]*/,
                                    int64_t* I_dev /*[nq,k]*/, void* stream);
int mvdb_index_search_hybrid(const mvdb_index* idx, const mvdb_sparse* sp, const float* q_host /*[nq,d]*/, int normalize_q, const int64_t* q_indptr_host,
                             const int32_t* q_indices_host, const float* q_values_host, int nq, int k, float dense_weight, float sparse_weight,
                             const mvdb_rowset* rs /*NULL: every row*/, float* D_host /*[nq,k]*/, int64_t* I_host /*[nq,k]*/);
int mvdb_index_search_hybrid_device(const mvdb_index* idx, const mvdb_sparse* sp, const float* q_dev /*[nq,d]*/, int normalize_q,
                                    const int64_t* q_indptr_host, const int32_t* q_indices_host, const float* q_values_host, int nq, int k,
                                    float dense_weight, float sparse_weight, const mvdb_rowset* rs, int64_t label_offset, float* D_dev /*[nq,k]*/,
                                    int64_t* I_dev /*[nq,k]*/, void* stream);
int mvdb_index_sparse_counters(const mvdb_index* idx, long long* calls, long long* score_launches);

/* SPARSE POSTINGS: the opt-in INVERTED form of a sparse store — posting lists by index, resident beside the CSR form — and a
 * scoring launch that reads only the lists of the query's terms instead of every stored non-zero.  The results are the CSR
 * pass's, bit for bit: the indices of a stored row are strictly ascending, so "the row's entries in stored order" is
 * "ascending index", and the posting launch takes the query's terms in ascending index order — for every row the same chain
 * acc = +0.0; acc = acc + (q[index] * value) in the same order.  Every line of SPARSE VECTORS AND HYBRID SEARCH above holds
 * unchanged for a store that has postings.
 * mvdb_sparse_build_postings(idx, sp) builds, on the device, from the resident CSR entries:
 *   post_ptr [dim + 1] (int64): list t is [post_ptr[t], post_ptr[t + 1]);
 *   post [nnz + 2]: 8-byte (row: uint32, value: fp32 bits) entries, every list in ascending row order, two padding entries
 *     behind them;
 *   and a host copy of post_ptr, taken at the end of the build — the call waits for its stream once, there.
 *   The layout is the stable transposition of the CSR arrays (np.argsort(indices, kind="stable") applied to the entries): a
 *   pure function of them, the same bytes from run to run.  The build is an LSD radix sort of (index; row, value), 8 bits a
 *   pass, every pass stable (one wave ranks sort_lds_entries entries at a time in LDS; the digit table is scanned by a
 *   multi-block exclusive scan), and post_ptr is a binary search per index over the sorted keys: integer LDS atomics count
 *   digits, nothing else is atomic.  Limits, checked on the host, MVDB_ERR_ARG: ntotal < 2^32 (the row is 32 bits), dim <=
 *   max_dim = 2^26 (the directory costs 8 (dim + 1) bytes, 512 MiB at the cap: beyond it create the store with a smaller dim
 *   or stay on CSR), and the store must be current for idx (the rules of a search).  Device memory: + 8 bytes per non-zero
 *   + 8 (dim + 1), and 16 bytes per non-zero more while the build runs.  nnz == 0 builds an empty directory and no lists.  A
 *   second build replaces the first.  No search may run on the store while it is built or dropped.
 * mvdb_sparse_drop_postings frees them; mvdb_sparse_has_postings: 1 or 0 (0 for NULL).  They go with the store, which is
 *   outdated by a write under the rules above.
 * mvdb_sparse_postings_geometry: block_rows (rows a workgroup of the scoring launch owns at a time), sort_lds_entries and
 *   max_dim of this build (any pointer may be NULL).
 * mvdb_sparse_postings_read copies the layout back: post_ptr [dim + 1], rows [nnz], values [nnz] (any may be NULL); a store
 *   without postings is MVDB_ERR_ARG.
 * Routing: index option "sparse_postings" (mvdb_index_set_option).  1, the default: a store that HAS postings answers
 *   mvdb_index_sparse_scores, mvdb_index_search_sparse(_device) and the scoring step of mvdb_index_search_hybrid(_device)
 *   through sparse_postings_kernel; 0: always the CSR pass.  A store without postings behaves as before.  There is no
 *   fallback by query size.
 * Launch, sparse_postings_kernel: the host sorts the query's terms by index, drops those whose list is empty (host
 *   directory) and uploads (list begin, list end, index, value) per term.  A workgroup owns block_rows rows at a time and
 *   holds their fp32 sums and 16-bit matched counts in LDS; one lane per term finds the part of the term's list inside the
 *   block by binary search (bounded by the list length) and cuts it at the waves' row quarters; every wave then walks the
 *   terms in order over its own rows.  No atomics on scores.  Launch counts are the CSR route's.
 * mvdb_index_sparse_counters keeps its meaning: calls counts searches served by either route, score_launches counts
 *   sparse_scan_kernel launches only.  mvdb_index_sparse_postings_counters: searches served through the postings,
 *   sparse_postings_kernel launches enqueued (mvdb_index_sparse_scores' included), and entries — the sum of the list lengths
 *   of the terms of the queries staged for the posting launch, from the host directory; all counted on the host, any pointer
 *   may be NULL.
 * No reference counterpart. */
int mvdb_sparse_build_postings(const mvdb_index* idx, mvdb_sparse* sp);
int mvdb_sparse_drop_postings(mvdb_sparse* sp);
int mvdb_sparse_has_postings(const mvdb_sparse* sp);
int mvdb_sparse_postings_geometry(int* block_rows, int* sort_lds_entries, long long* max_dim);
int mvdb_sparse_postings_read(const mvdb_sparse* sp, int64_t* post_ptr_host /*[dim+1]*/, uint32_t* rows_host /*[nnz]*/, float* values_host /*[nnz]*/);
int mvdb_index_sparse_postings_counters(const mvdb_index* idx, long long* calls, long long* launches, long long* entries);

/* Merge `nlists` sorted top-k lists per query into one [nq,k] result on the device.  List l lives
 * at D_dev + l*list_stride_D (floats, [nq,k]) and I_dev + l*list_stride_I (int64, [nq,k]) — the
 * layout one RCCL all-gather of each rank's packed {I,D} block produces.  Labels must already be
 * global; lists must be ordered by ascending shard base (ties resolve to the lower label).
 * k <= 64: one wave per query; larger k: nlists * k <= 16384 keys sorted in LDS by one block per query.
 * No reference counterpart (the reference never partitions a search). */
int mvdb_merge_topk_device(int metric, int nlists, int nq, int k, const float* D_dev,
                           int64_t list_stride_D, const int64_t* I_dev, int64_t list_stride_I,
                           float* D_out_dev, int64_t* I_out_dev, int device, void* stream);

/* ---- exchange step of the row-partitioned multi-GPU search -------------------------
 * One process per GPU; rank r holds rows [base_r, base_r + n_r) resident and answers from them
 * (mvdb_index_search_device with label_offset = base_r); ONE all-gather of every rank's packed result block
 * ([I: nq*k int64 | D: nq*k fp32], 12*k bytes per query) over xGMI; mvdb_merge_topk_device on every rank.
 * The communicator is RCCL's: rank 0 draws a unique id (mvdb_comm_unique_id), the launcher hands the 128 bytes
 * to every rank (torch.distributed / a file / MPI — any side channel), every rank calls mvdb_comm_create.
 * RCCL is bound at run time (dlopen); a single-GPU process never loads it.  No reference counterpart: the
 * reference searches one stacked matrix (minivectordb/sharded_vector_database.py:598-662); the contract kept is
 * that function's result — top-k of the union, ties to the lower global row. */
typedef struct mvdb_comm mvdb_comm;
int mvdb_comm_available(void); /* 0 when librccl could be bound in this process (every rank checks BEFORE the collective init) */
int mvdb_comm_unique_id(unsigned char* out128);
int mvdb_comm_create(const unsigned char* id128, int rank, int world, int device, mvdb_comm** out);
int mvdb_comm_free(mvdb_comm* comm);
int mvdb_comm_rank(const mvdb_comm* comm);
int mvdb_comm_world(const mvdb_comm* comm);

/* ncclAllGather of nbytes_per_rank bytes from local_dev into gathered_dev[world * nbytes_per_rank] (rank order),
 * enqueued on `stream`; returns without synchronising. */
int mvdb_allgather_topk(mvdb_comm* comm, const void* local_dev, void* gathered_dev, int64_t nbytes_per_rank,
                        void* stream);

/* In-place row-wise L2 normalisation of host matrix x[n,d] on the device.
 * Replaces faiss.normalize_L2                     minivectordb/vector_database.py:45, :475 */
int mvdb_normalize_l2(float* x_host, int64_t n, int d, int device);

/* Device generator of the synthetic stream into dense device memory out_dev[n,d] (queries). */
int mvdb_synth_fill_device(float* out_dev, int64_t n, int d, uint64_t seed, int64_t first_row,
                           int normalize, int device, void* stream);

/* ---- profiling hooks (bench.py's roofline leg) ---------------------------------------------
 * When enabled, every launch of the dominant kernels is timed by a pair of hipEvents.  A bracket of one kernel hands its
 * stop event to the launch itself (hipExtLaunchKernel): the runtime fills it from the kernel's own dispatch — its time is the
 * kernel's end — and the stream carries nothing behind the kernel.  Its start event is recorded on the launch stream in front
 * of the kernel, one marker, so the duration is the kernel's plus that marker's hand-over.  The four launches of the
 * single-query int8 route ("ip_scan_code8_seed", "ip_scan", "ip_scan_code8_rescore", "ip_scan_code8_fallback") follow one
 * another with nothing in between and share their boundaries: only the first records a start, each of the others begins at
 * the stop event of the one before it, and its duration is the time from the end of that kernel to the end of its own — the
 * launch gap and the kernel (measured against a kernel trace: profiles/prof_bracket_overhead.jsonl).  A call of that route puts
 * one marker on the stream.  A bracket of several launches or of a graph launch ("encoder", "ip_scan_mfma_masked") records
 * both events on the launch stream around them, and its duration includes those two markers.
 * mvdb_prof_read drains the finished pairs of kernel `name` ("ip_scan", "ip_scan_mfma",
 * "ip_scan_gemm", "ip_scan_half", "ip_scan_half_seed", "ip_scan_rescue", "ip_scan_rerun", "ip_scan_scores",
 * "distinct_collapse", "distinct_scan", "distinct_select", "groups_scan", "groups_select", "maxsim_scan", "maxsim_select", "assign_scan", "examples_scan", "examples_select", "boost_combine", "boost_scan", "encoder") and returns the number of launches and their summed duration;
 * pairs recorded while profiling was on stay readable after it is turned off.
 * Launches on a stream that is being captured are not counted: a timed event inside a graph measures nothing, so a captured
 * search holds its kernels and no event, whether profiling is on or not, and neither the capture nor a replay adds a launch.
 * The events come from a pool that is created on first use and only recycled afterwards: mvdb_prof_read returns the pairs it
 * drains to it.  Pairs that nobody reads are bounded by two rules.  Turning profiling on while it was off returns every unread
 * pair to the pool (and forgets the symbols recorded so far, mvdb_prof_symbol: after it, a label under which nothing has been
 * launched since reads "", not the symbol of an earlier bracket).  And a label holds at most MVDB_PROF_LABEL_CAP unread pairs:
 * past that its launches run untimed and uncounted until a read or an off -> on makes room.  So the pool never holds more than
 * 2 * (the most pairs left unread at one time since the library was loaded) events, and no label contributes more than
 * 2 * MVDB_PROF_LABEL_CAP of them.  mvdb_prof_live_events: the events the pool holds, in use or free.  Diagnostic only. */
#define MVDB_PROF_LABEL_CAP 8192
int mvdb_prof_enable(int on);
int mvdb_prof_read(const char* name, int64_t* launches, double* total_ms);
int64_t mvdb_prof_live_events(void);
/* The kernel instantiation last launched under label `name` while profiling was on, as rocprofv3 prints it
 * ("flat_scan_kernel<64, 2, 2, 0, 0, true, 0, false>"; "" if none): bench.py refuses a committed PMC profile whose kernel
 * differs from what the timed run launched.  The ops of an encoder forward record theirs with the grid, the block and the LDS
 * bytes — "gemm_x3_dma_kernel<EPI_BIAS_QKV, 64, 3, 4, 64, 1, 0> grid=(18,2,1) block=256 lds=49152 sel=0" — under enc_pack,
 * enc_embed, enc_qkv, enc_qkv_epi, enc_attn, enc_ctx_split, enc_wo, enc_ln1, enc_ffn1, enc_ffn1_epi, enc_ffn2, enc_ln2, enc_pool,
 * and the second GEMM of a (256-row form, fallback) pair under <label>_fallback (tests/test_encoder_launch_table_gpu.py). */
int mvdb_prof_symbol(const char* name, char* out, int len);

/* Number of chunks (up to 256 queries) of the certified batch passes that held a query which failed certification — those
 * queries were answered by the rescue pass or re-run on the exact fp32 kernels — since the library was loaded.
 * Diagnostic only. */
int64_t mvdb_split_rerun_count(void);

/* Tiles (32 rows) the rescue launches were handed since the library was loaded, and the tiles they would have scanned without
 * the tile flags the certified pass keeps (inner product, k <= 16, ~400k rows and more, while the index has been refusing
 * certificates; MVDB_TILE_FLAGS=1 / 0: always / never).  Diagnostic only; synchronises the devices. */
int mvdb_rescue_tile_stats(int64_t* listed, int64_t* total);

/* The certificate's error bound per unit |q| * max|x| at dimension d for the fp16 single-product nomination pass
 * (half_scan.hip: both operands rounded to fp16, d products accumulated in fp32, 64 nominees per query re-scored
 * in fp32): rounding of both operands, elements below fp16's normal range, worst-case fp32 accumulation, the fp32
 * re-score, |q| and the comparison (docs/DESIGN_NOTES.md section 4.3d; tests/test_split_bound.py).  Diagnostic.
 * mvdb_half_max_queries: queries per corpus pass of that pass at dimension d, 0 where it has no kernel. */
double mvdb_half_eps(int d);
int mvdb_half_max_queries(int d);

/* ---- int8 cosine index (csrc/cos8.hip) ---------------------------------------------------
 * Replaces usearch.index.Index(ndim=d, metric='cos', dtype='int8') built per query over the filtered rows
 *                                                minivectordb/sharded_vector_database_usearch.py:617-629
 * with an EXACT scan under the same quantisation and distance (INTEGRATION.md "int8 cosine contract").
 *
 * Quantisation of a row or query x (fp32, length d), one device function (csrc/cos8_kernels.hpp: cos8_quantize_row):
 *   mag    = sqrt(sum_i (double)x_i^2), summed sequentially in index order in fp64;
 *   code_i = (int8) trunc((double)(float)(x_i * 127.0f) / mag), clamped to [-127, 127];
 *   mag == 0 or not finite: all codes 0.   a2 = sum_i code_i^2 (int32).
 * Distance for the int32 sums ab = a.b, a2, b2:
 *   a2 == 0 and b2 == 0: 0;  exactly one of them 0, or ab == 0: 1;
 *   else (float)(1.0 - (double)ab / sqrt((double)a2 * (double)b2))  (IEEE fp64 division and square root).
 * Results: ascending distance, ties to the lower row; missing slots label -1 / distance +FLT_MAX.  A batch returns,
 * bit for bit, what nq single calls return (integer dot products do not depend on summation order).
 * Device store: codes [n, stride] (stride = d rounded up to 16 bytes, zero padded) and a2 [n]; no fp32 rows.
 * d <= 4096.  k > 64: every distance is materialised and radix-selected.  Searches are re-entrant from many host
 * threads; add / remove_rows / reset / reserve take the index exclusively and wait for its searches. */
typedef struct mvdb_cos8 mvdb_cos8;
int mvdb_cos8_create(int d, int device, mvdb_cos8** out);
int mvdb_cos8_free(mvdb_cos8* ix);
int mvdb_cos8_reset(mvdb_cos8* ix);
int mvdb_cos8_reserve(mvdb_cos8* ix, int64_t n);
int64_t mvdb_cos8_ntotal(const mvdb_cos8* ix);
int mvdb_cos8_dim(const mvdb_cos8* ix);

/* Quantise and append n fp32 rows: x_host[n,d] (C-contiguous; uploaded in chunks) or x_dev[n,d] (dense, same GPU). */
int mvdb_cos8_add(mvdb_cos8* ix, const float* x_host, int64_t n);
int mvdb_cos8_add_device(mvdb_cos8* ix, const float* x_dev, int64_t n);

/* Rows [row0, row0 + n) back to the host: codes_host[n,d] (unpadded) and a2_host[n]; either may be NULL.  For tests. */
int mvdb_cos8_get_codes(const mvdb_cos8* ix, int64_t row0, int64_t n, int8_t* codes_host, int32_t* a2_host);

/* Remove the given rows (duplicates rejected); the remaining rows keep their relative order (np.delete numbering). */
int mvdb_cos8_remove_rows(mvdb_cos8* ix, const int64_t* rows_host, int64_t m);

/* Overwrite the m listed stored rows with the quantised x[m,d] (x_host: uploaded in chunks; x_dev: dense, same GPU).  Codes
 * and a2 are what add gives for the same input (one quantisation rule).  rows_host is a host array, each row in [0, ntotal),
 * any order; a duplicate, an out-of-range row or a NULL pointer with m > 0 is MVDB_ERR_ARG and leaves the index untouched;
 * m == 0 returns 0.  Exclusive like add; rows are not renumbered, so resident row sets stay valid; nothing is reallocated. */
int mvdb_cos8_set_rows(mvdb_cos8* ix, const int64_t* rows_host, const float* x_host, int64_t m);
int mvdb_cos8_set_rows_device(mvdb_cos8* ix, const int64_t* rows_host, const float* x_dev, int64_t m);

/* k nearest rows for nq fp32 queries (quantised on the device by the same rule): q_host[nq,d], D_host[nq,k] distances,
 * I_host[nq,k] row numbers. */
int mvdb_cos8_search(const mvdb_cos8* ix, const float* q_host, int nq, int k, float* D_host, int64_t* I_host);

/* Same with every buffer in device memory, enqueued on `stream` (hipStream_t, NULL = legacy default stream); labels are
 * row + label_offset.  No host synchronisation; capturable into a hipGraph after one eager call of the same shape on that
 * stream (the eager call sizes the stream's workspace; a capture that would need a larger one fails with MVDB_ERR_ARG). */
int mvdb_cos8_search_device(const mvdb_cos8* ix, const float* q_dev, int nq, int k, int64_t label_offset,
                            float* D_dev, int64_t* I_dev, void* stream);

/* A filter's rows resident on the device: excluded == 0 the m listed rows, excluded != 0 every row but them.  Kept as an
 * exclusion bitmap (excluded sets, and lists that keep >= 1/8 of the rows) or a sorted row list.  Labels are row
 * numbers either way, ties to the lower row.  A set belongs to the index state it was built against: after a removal
 * searching it fails with MVDB_ERR_ARG; rows appended later are not part of it. */
typedef struct mvdb_cos8_rowset mvdb_cos8_rowset;
int mvdb_cos8_rowset_create(const mvdb_cos8* ix, const int64_t* rows_host, int64_t m, int excluded,
                            mvdb_cos8_rowset** out);
int64_t mvdb_cos8_rowset_size(const mvdb_cos8_rowset* rs);
int mvdb_cos8_rowset_is_bitmap(const mvdb_cos8_rowset* rs);
int mvdb_cos8_rowset_free(mvdb_cos8_rowset* rs);
int mvdb_cos8_search_rowset(const mvdb_cos8* ix, const float* q_host, int nq, int k, const mvdb_cos8_rowset* rs,
                            float* D_host, int64_t* I_host);
int mvdb_cos8_search_rowset_device(const mvdb_cos8* ix, const float* q_dev, int nq, int k, const mvdb_cos8_rowset* rs,
                                   int64_t label_offset, float* D_dev, int64_t* I_dev, void* stream);

/* ---- encoder (BERT-architecture sentence encoder: e5-small / e5-large) ---------------------
 * Replaces self.model(**batch_dict) + average_pool + F.normalize
 *                                                minivectordb/embedding_model.py:66-70, :50-53 */
typedef struct mvdb_encoder_cfg {
    int vocab_size;
    int hidden;        /* H  */
    int layers;        /* L  */
    int heads;         /* nh (head_dim = H / nh) */
    int intermediate;  /* FFN width */
    int max_positions;
    int type_vocab;
    int position_offset; /* 0 for BERT; padding_idx+1 for XLM-R style position ids */
    float ln_eps;
    int pooling;         /* 0 = attention-masked mean (e5, embedding_model.py:50-53);
                            1 = first valid token / CLS (BGE-M3 dense_vecs, embedding_model.py:74-78) */
} mvdb_encoder_cfg;

/* Weight table: device pointers (fp32, PyTorch nn.Linear layout [out,in]) in the order given by
 * mvdb_encoder_weight_name(i) for i in [0, mvdb_encoder_weight_count(cfg)). The encoder keeps
 * the pointers (the caller — a torch state_dict — owns the memory).
 * mvdb_encoder_create reads every MVDB_* switch of the encoder (docs/DESIGN_NOTES.md, the switch list) into the encoder: a
 * switch set afterwards does not reach it, one process can hold encoders created under different switches, and no forward
 * reads the environment.  (Earlier builds read most of them once per PROCESS, at the first launch that consulted them.)
 * Per process still: MVDB_WALK_LOCK and MVDB_WALK_LOCK_DIR, the per-device gate all encoders share. */
int mvdb_encoder_weight_count(const mvdb_encoder_cfg* cfg);
const char* mvdb_encoder_weight_name(const mvdb_encoder_cfg* cfg, int i);
int mvdb_encoder_create(const mvdb_encoder_cfg* cfg, const void* const* weight_ptrs_dev, int device,
                        mvdb_encoder** out);
int mvdb_encoder_free(mvdb_encoder* enc);

/* ids[B,S], mask[B,S] (int32, host) -> out[B,H] pooled (cfg.pooling) + L2-normalised (host).
 * compute: 0 = exact-fp32 MFMA; 2 = split-precision GEMMs on the fp16 matrix cores (a.w ~ al.wh + ah.wl + ah.wh with
 * (h, l) the fp16 RNE split of an fp32 value — 22 significant bits —, weights scaled per tensor by a power of two,
 * fp32 accumulate; needs |activation| <= 65504; embeddings within 6e-7 of transformers' fp32 output like the exact
 * mode's; the two attention products run the same split, softmax / LayerNorm / pooling stay fp32) — what the Python
 * drop-in uses by default.  (1, the single-bf16-product mode of earlier builds, was removed: MVDB_ERR_ARG.)
 * Up to 64 token slots the forward is ONE layer-walking launch in exact fp32 whatever `compute` says
 * (mvdb_encoder_walks below). */
int mvdb_encoder_forward(mvdb_encoder* enc, const int32_t* ids_host, const int32_t* mask_host,
                         int B, int S, int compute, float* out_host);
int mvdb_encoder_forward_device(mvdb_encoder* enc, const int32_t* ids_dev, const int32_t* mask_dev,
                                int B, int S, int compute, float* out_dev, float* hidden_dev,
                                void* stream);

/* Device address of ONE uint32 that every forward clears when it starts and ORs 1 into when a pooled row of a non-empty sentence
 * is not finite — the split-precision mode (compute = 2) takes activations as fp16 pieces, so an activation beyond 65504
 * overflows.  mvdb_encoder_forward_device never synchronises: its callers (and a graph that chains the forward into a search)
 * test this word on the device, or read it back behind their own synchronisation, and re-run in the exact mode (compute = 0) —
 * which is what mvdb_encoder_forward's Python wrapper does on the host path.  Valid until mvdb_encoder_free. */
const unsigned int* mvdb_encoder_overflow_flag(const mvdb_encoder* enc);

/* ---- BGE-M3's heads: lexical weights and ColBERT vectors from the same forward (csrc/m3_heads.hpp) ----
 * With x[b,t,:] the last hidden state of token slot t of sentence b and len_b its valid tokens (masks are prefixes):
 *   token weight   tw[b,t] = relu(sparse_w . x[b,t] + sparse_b) for t < len_b, 0 for masked slots (fp32; NaN stays NaN);
 *   lexical weights of b: over t < len_b with ids[b,t] >= 0, not among unused_ids, and tw[b,t] > 0 — for every distinct token
 *                  id its largest weight, emitted by ascending id (a NaN weight fails > 0 and is dropped, +inf is kept);
 *   ColBERT vector v[b,t-1,:] = u / max(|u|_2, 1e-12), u = colbert_w x[b,t] + colbert_b, for 1 <= t < len_b (the CLS slot is
 *                  dropped, the EOS slot kept): max(len_b - 1, 0) rows; the rows behind them read 0.
 * colbert_dim C: a multiple of 32 with C <= hidden (the GEMM launchers' column granularity; BGE-M3: 1024).  Every reduction
 * has a fixed order: the same bits run to run.  A token weight of a valid token, or a ColBERT row's squared norm, that is not
 * finite ORs 1 into the overflow word above — the pooled row's protocol: re-run with compute = 0 when compute was 2.
 *
 * mvdb_encoder_set_heads keeps the pointers (device, fp32, 16-byte aligned; the caller owns the memory), like the weight table;
 * NULL removes the heads.  unused_ids: at most 8 token ids that never get a lexical weight (BGE-M3: cls, pad, eos, unk =
 * 0, 1, 2, 3). */
typedef struct mvdb_m3_heads {
    const float* sparse_w;   /* [H]   device, fp32 */
    const float* sparse_b;   /* [1] */
    const float* colbert_w;  /* [C,H] nn.Linear layout; NULL: no ColBERT head */
    const float* colbert_b;  /* [C] */
    int colbert_dim;         /* C */
    int n_unused;
    int unused_ids[8];
} mvdb_m3_heads;
int mvdb_encoder_set_heads(mvdb_encoder* enc, const mvdb_m3_heads* heads);

/* The outputs wanted beside the pooled row; any pointer NULL = output not wanted; all device memory.  The padding is written
 * by the forward's own kernels (no memset): token_weights of masked slots, ColBERT rows from colbert_count[b] on and
 * lex_indices / lex_values from lex_count[b] on read 0.  lex_count, lex_indices and lex_values go together. */
typedef struct mvdb_m3_out {
    float* token_weights;    /* [B,S] */
    int32_t* lex_count;      /* [B] */
    int32_t* lex_indices;    /* [B,S] ascending token ids */
    float* lex_values;       /* [B,S] */
    float* colbert;          /* [B,S-1,C], 16-byte aligned */
    int32_t* colbert_count;  /* [B] */
} mvdb_m3_out;
/* mvdb_encoder_forward_device's dense output plus the heads' outputs, from ONE forward; never synchronises, allocates nothing
 * once the workspace has the batch's size.  It always runs the per-op kernels (never the layer-walking launch), on one lane,
 * as plain launches on `stream` (not through the encoder's graph cache: the outputs are the caller's own buffers).  The heads
 * run behind the last layer on the PACKED token states, in the call's compute mode.
 * MVDB_ERR_ARG, before anything is enqueued: no heads set; a ColBERT output without a ColBERT head; the lexical outputs asked
 * for in part; S > 1024 (the per-sentence sort of the lexical weights lives in 8 KiB of LDS); a misaligned `colbert`. */
int mvdb_encoder_forward_multi_device(mvdb_encoder* enc, const int32_t* ids_dev, const int32_t* mask_dev, int B, int S,
                                      int compute, float* dense_out_dev, const mvdb_m3_out* out, void* stream);

/* 1 when a forward of B x S token slots is of the shape the ONE layer-walking launch serves (csrc/encoder_walk.hpp: at most 64
 * token slots — one sentence per call is the reference's only shape, embedding_model.py:62-71; beyond 64 slots the per-op kernels
 * are faster since round 6 —, exact fp32 matrix cores whatever `compute` says), 0 when it runs the per-op kernels.
 * MVDB_ENCODER_WALK=0 (read at mvdb_encoder_create) switches the launch off.  A forward of that shape still takes the per-op
 * kernels when the caller is CAPTURING the stream, while another process holds the GPU's walking gate, and for a while after a
 * launch was abandoned (next paragraph). */
int mvdb_encoder_walks(const mvdb_encoder* enc, int B, int S);

/* The walking launch is a persistent grid whose workgroups wait for each other, so it completes only when all of them are
 * resident.  It is guarded three ways (csrc/encoder.hip "Walking launches ..."): one such launch at a time per device inside
 * a process (whatever encoder, stream or host thread); an advisory flock on /dev/shm/mvdb_walk_<GPU UUID>.lock across
 * processes (MVDB_WALK_LOCK=0 switches it off, MVDB_WALK_LOCK_DIR moves it); and BOUNDED waits inside the kernel: no wait
 * outlasts MVDB_WALK_DEADLINE_US (default 20000, read when the encoder is created) — the launch then abandons itself, fills
 * `out` with NaN, raises the overflow word above and counts itself.  mvdb_encoder_forward notices that behind its own stream
 * wait and re-runs the forward on the per-op kernels within the same call; a caller of mvdb_encoder_forward_device sees the
 * overflow word (or `aborts` here) behind ITS stream wait and calls again.  After an abandoned launch the next 256 forwards of
 * the encoder take the per-op kernels.  aborts = launches abandoned so far (completed ones), fallbacks = forwards
 * mvdb_encoder_forward re-ran, suspended_calls = forwards left before the next walking attempt; any pointer may be NULL. */
int mvdb_encoder_walk_stats(const mvdb_encoder* enc, unsigned long long* aborts, unsigned long long* fallbacks,
                            int* suspended_calls);

/* Which tile form of the split-precision GEMM a batch of `tokens` packed tokens selects for an N-wide product on a
 * device with `compute_units` CUs: 256 or 192 = the 256-row form on 256 x 256 / 256 x 192 tiles (one eight-wave workgroup
 * per CU; N % 256 == 0 resp. N % 192 == 0 and the tiles make whole rounds of the CUs: >= 1 round, and >= 4 rounds or a
 * last round >= 85 % full), 0 = the 64- / 128-row forms.  The same predicate runs on the device, on the packed token
 * count, inside the paired launches of a forward; exported so that the rule is testable without a GPU. */
int mvdb_encoder_gemm_tile_form(int64_t tokens, int n, int compute_units);

/* Planes a SMALL batch's N = H GEMM (attention output projection, FFN2; on the wide shapes also QKV and FFN1) is split into over
 * K (0: not split): a K-step of the GEMM is a latency step — one barrier and one DMA round trip — so while the 64 x 128 tiles of
 * a batch leave CUs idle, K is cut into min(8, (k / 32) / 4, compute_units / tiles) planes (snapped to 2 / 3 / 4 / 6 / 8), summed in
 * plane order by the LayerNorm / image kernel behind the GEMM.  The same rule on the host, from the padded token count; exported
 * so that it is testable without a GPU (tests/test_encoder_tiles.py).  MVDB_GEMM_X3_SPLITK* environment switches: csrc/encoder.hip; this function, which has no encoder, reads them at the call. */
int mvdb_encoder_splitk_planes(int64_t tokens, int n, int k, int compute_units);

#ifdef __cplusplus
}
#endif
#endif /* MVDB_H */
