// SPLADE's head on the encoder's last hidden states (included by encoder.hip, inside its kernel namespace): the masked-language-
// model head of BERT / XLM-R, reduced per sentence to one weight per vocabulary entry,
//   t       = LayerNorm(gelu(x W_t^T + b_t))                     the MLM transform, on the packed token states [T, H]
//   z[p, v] = t[p] . E[v] + b_v                                  the decoder: E [V, H] (tied to the word embeddings, or its own)
//   w[b, v] = max over the tokens p of sentence b of log(1 + relu(z[p, v]))
// then pruned to the max_terms largest weights of every sentence.
//
// The transform is one more GEMM of the forward's own launchers (EPI_BIAS_GELU) and a LayerNorm, in the call's compute mode
// (enqueue_splade_head, encoder.hip).  In the split-precision mode that GEMM's epilogue writes the (hi | lo) fp16 image, not
// fp32, so the LayerNorm's rows are loaded from the image there (splade_ln_image_kernel: the loader is new, the LayerNorm is
// wave_layernorm).
//
// THE VOCABULARY PRODUCT IS ALWAYS THE SPLIT-PRECISION FORM (fp16 x 3 on v_mfma_f32_32x32x16_f16, fp32 accumulate: 2^-22 per
// operand), whatever `compute` says: `compute` governs the layers and the transform only.  An exact-fp32 product over
// V = 30,522 ... 250,002 columns would cost 16 / 3 of the matrix-core time for nothing the bound of the weights needs.
//
// [T, V] logits never exist: splade_vocab_max_kernel takes the per-sentence maximum in its epilogue and merges it into a
// [sentences, V] buffer of float BITS with an unsigned-integer atomicMax.  w >= 0, so the order of the bits is the order of the
// values; maximum is exactly associative and commutative, so the buffer holds the same bits run to run.  No floating-point
// atomic anywhere.  A NaN logit becomes the canonical quiet NaN 0x7fc00000, which is above +inf in that order: it wins the
// maximum, as torch's max does, and is dropped by the pruning (NaN > 0 is false).
#pragma once

constexpr int kSpladeMaxTerms = 1024;  // the limit of a sparse query and of kM3MaxS
constexpr int kSpladeMaxUnused = 8;
constexpr int SV_BM = 128, SV_BN = 128;  // token rows x vocabulary columns of a workgroup's tile
constexpr int SV_STAGE = (SV_BM + SV_BN) * 128;       // one K-step (32 k) of both operands as (hi | lo) lines
constexpr int SV_LDS = 2 * SV_STAGE + 3 * SV_BM * 4 + 16;  // two stages (reused as the [segments][128] maxima), the segment tables
constexpr int SV_GROUP = 32;  // row bands per raster group: 16 column tiles x 32 bands are resident at once on 256 CUs

// The kernels of this header are compiled without the packed fp32 operations (v_pk_add_f32 and kin), as maxsim_mfma.hip is: a
// target attribute of the device pass (the host pass does not know the feature).  Lambdas inside them are forced inline — the
// inliner keeps functions of different target features apart otherwise.
#ifdef __HIP_DEVICE_COMPILE__
#define SPLADE_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__
#else
#define SPLADE_KERNEL __global__
#endif
#define SPLADE_INLINE __attribute__((always_inline))

// A float as an unsigned word whose integer order is the float order (-inf lowest, +inf highest of the numbers; 0 is below all of
// them: "no value yet").  The maximum of logits z is taken on these words: log(1 + relu(z)) does not decrease with z, so the
// maximum of the weights is the weight of the maximum, and log1pf runs once per (segment, column), not once per logit.
__device__ __forceinline__ unsigned int splade_ordered(float z) {
    const unsigned int b = __float_as_uint(z);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
constexpr unsigned int kSpladeNaN = 0xffffffffu;  // above every number: a NaN logit wins the maximum, as torch's max

struct SpladeUnused {
    int n;
    int id[kSpladeMaxUnused];
};

// out[i] = 0: the node that clears the [sentences, V] buffer (a kernel, not a memset node)
SPLADE_KERNEL __launch_bounds__(256) void splade_zero_kernel(unsigned int* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = 0u;
}

// t[p, :] = LayerNorm(g[p, :]) with g read from the (hi | lo) image the GELU epilogue of the split-precision GEMM wrote
// ([row][H / 32][hi 32 | lo 32] fp16: value = hi + lo).  One wave per row, as ln_kernel.
template <int VPT>
SPLADE_KERNEL __launch_bounds__(256) void splade_ln_image_kernel(const _Float16* __restrict__ img, const int* __restrict__ seq_start, int B,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              int H, float* __restrict__ t) {
    const int T = seq_start[B];
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= T) return;
    const _Float16* row = img + (int64_t)p * H * 2;
    float v[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int c = lane + i * 64;
        const int o = (c >> 5) * 64 + (c & 31);
        v[i] = c < H ? (float)row[o] + (float)row[o + 32] : 0.f;
    }
    wave_layernorm<VPT, false>(v, H, lane, eps, gamma, beta, t + (int64_t)p * H, nullptr);
}

// ---- the fused vocabulary product and per-sentence maximum --------------------------------------------------------------------
// A workgroup (four waves, 2 x 2) owns a band of 128 packed token rows of the sentences [b0, b1) and a tile of 128 vocabulary
// columns, and walks K = H in steps of 32 through two LDS stages:
//   * t rows arrive as fp32 and are split into (hi, lo) fp16 WHILE they are staged (x3_split2, as attention_x3_kernel splits K
//     and V); E rows are 128-byte lines of the resident (hi | lo) image (make_interleaved; scaled by the power of two 1 / inv_scale);
//     both sit in LDS as [row][hi 32 | lo 32] with the GEMMs' bank swizzle (16-byte slot p of row r at p ^ ((r >> 1) & 7));
//   * the next K-step's global loads are in flight under the current step's MFMAs (registers -> LDS behind them), one barrier a step;
//   * a wave's tile is 64 rows x 64 columns; the TOKEN fragment is the first MFMA operand, so a lane's 16 accumulator values are 16
//     ROWS of ONE vocabulary column (lane & 31): row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the 32-row tile, ascending in r.
// Epilogue: the decoder bias per value; then the segmented maximum over the rows of each sentence inside the band, relu and log1pf
// on the maximum (splade_ordered: the same value as the maximum of log1pf(relu(z)), 1 / 32 of the log1pf calls at the least).  A
// band may hold several sentences and a sentence may span several bands: every row's segment (its sentence's index among the
// sentences that have rows in this band, from seq_start) is tabled before the K loop.  A lane walks its 32 rows of a column in
// ascending order keeping the running maximum IN REGISTERS and hands it over when the segment changes; the hand-over goes across
// the lane halves and the waves through LDS (an unsigned ds_max on [segment][column], in the staging memory, free by then).
// Last, every (segment, column) cell whose weight is > 0 is merged into out[sentence - b0][column] by ONE unsigned atomicMax: at
// most one atomic per (sentence, column, workgroup), none for a zero (the buffer was cleared by a node of the same enqueue).
// Rows past the chunk's last token and columns past V take part in no maximum, no atomic and no flag: zero rows / lines are
// staged for them.  flag: ORed with 1 when a logit of a valid token is not finite (the pooled row's protocol).
// Grid: 1-D, rastered in groups of SV_GROUP bands x all column tiles, bands fastest: what is resident together shares few E
// tiles and few bands.  H % 32 == 0 (HBK).
SPLADE_KERNEL __launch_bounds__(256) void splade_vocab_max_kernel(const float* __restrict__ t, const _Float16* __restrict__ Ep, float inv_scale,
                                                               const float* __restrict__ dec_b, const int* __restrict__ seq_start,
                                                               int b0, int b1, int H, int V, int nbands, int ncols,
                                                               unsigned int* __restrict__ out, unsigned int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sv_lds[];
    int* s_sent = reinterpret_cast<int*>(sv_lds + 2 * SV_STAGE);  // [128] sentence of the row, -1 past the end
    int* s_seg = s_sent + SV_BM;                                  // [128] segment of the row, -1 past the end
    int* s_segb = s_seg + SV_BM;                                  // [128] sentence - b0 of the segment
    int* s_misc = s_segb + SV_BM;                                 // [0] heads in wave 0, [1] segments
    unsigned int* red = reinterpret_cast<unsigned int*>(sv_lds);  // [segments][128] maxima, behind the K loop

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    // raster: group g = SV_GROUP bands (the last group: what is left), all columns; inside, the band runs fastest
    const int per_group = SV_GROUP * ncols;
    const int g = blockIdx.x / per_group, in_g = blockIdx.x - g * per_group;
    const int gb = min(SV_GROUP, nbands - g * SV_GROUP);
    const int band = g * SV_GROUP + in_g % gb, ctile = in_g / gb;
    const int row_lo = seq_start[b0], row_hi = seq_start[b1];
    const int r0 = row_lo + band * SV_BM;
    if (r0 >= row_hi) return;  // (the grid is sized by the padded batch)
    const int v0 = ctile * SV_BN;

    // ---- the band's segments
    if (tid < SV_BM) {
        const int row = r0 + tid;
        int sent = -1;
        if (row < row_hi) {  // the last sentence of [b0, b1) that starts at or before the row: the one that holds it
            int lo = b0, hi = b1 - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (seq_start[mid] <= row) lo = mid;
                else hi = mid - 1;
            }
            sent = lo;
        }
        s_sent[tid] = sent;
    }
    __syncthreads();
    int head = 0, before = 0;
    if (tid < SV_BM) {  // (waves 0 and 1, whole)
        const int sent = s_sent[tid];
        head = sent >= 0 && (tid == 0 || s_sent[tid - 1] != sent);
        const unsigned long long m = __ballot(head);
        before = __popcll(m & ((1ull << lane) - 1ull));
        if (tid == 0) s_misc[0] = __popcll(m);
        if (tid == 64) s_misc[1] = __popcll(m);
    }
    __syncthreads();
    if (tid < SV_BM) {
        const int seg = before + head - 1 + (wave == 1 ? s_misc[0] : 0);
        s_seg[tid] = s_sent[tid] >= 0 ? seg : -1;
        if (head) s_segb[seg] = s_sent[tid] - b0;
    }
    const int nseg_w0 = s_misc[0];
    __syncthreads();
    if (tid == 0) s_misc[1] += nseg_w0;  // segments of the band (read behind the K loop's barriers)

    // ---- staging: thread -> (row, 16-byte slot) of four pieces per operand and K-step
    f32x4 ta[4];
    uint4 eb[4];
    auto load = [&](int kt) SPLADE_INLINE {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, row = idx >> 3, c = idx & 7;
            ta[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r0 + row < row_hi) ta[q] = *reinterpret_cast<const f32x4*>(t + (int64_t)(r0 + row) * H + kt * 32 + c * 4);
            eb[q] = uint4{0u, 0u, 0u, 0u};
            if (v0 + row < V) eb[q] = *reinterpret_cast<const uint4*>(Ep + ((int64_t)(v0 + row) * (H >> 5) + kt) * 64 + c * 8);
        }
    };
    auto store = [&](int stage) SPLADE_INLINE {
        unsigned char* sb = sv_lds + stage * SV_STAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, row = idx >> 3, c = idx & 7;
            const int sw = (row >> 1) & 7;
            uint32_t h0, l0, h1, l1;
            x3_split2(ta[q][0], ta[q][1], h0, l0);
            x3_split2(ta[q][2], ta[q][3], h1, l1);
            // k = 4 c .. 4 c + 3: slot c >> 1 of the hi plane (slots 0 - 3), 4 + (c >> 1) of the lo plane, 8 bytes each
            *reinterpret_cast<uint2*>(sb + row * 128 + (((c >> 1) ^ sw) << 4) + (c & 1) * 8) = uint2{h0, h1};
            *reinterpret_cast<uint2*>(sb + row * 128 + (((4 + (c >> 1)) ^ sw) << 4) + (c & 1) * 8) = uint2{l0, l1};
            *reinterpret_cast<uint4*>(sb + SV_BM * 128 + row * 128 + ((c ^ sw) << 4)) = eb[q];
        }
    };
    // fragment byte offsets inside a stage: [k-block][plane] of the wave's first token / vocabulary tile (the second: + 4096)
    int t_off[2][2], e_off[2][2];
    const int ga = (fr >> 1) & 7;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            t_off[ks][pl] = (wm * 64 + fr) * 128 + (((4 * pl + 2 * ks + fh) ^ ga) << 4);
            e_off[ks][pl] = SV_BM * 128 + (wn * 64 + fr) * 128 + (((4 * pl + 2 * ks + fh) ^ ga) << 4);
        }
    f32x16 acc[2][2];  // [token tile][vocabulary tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = H >> 5;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load(kt + 1);
        const unsigned char* sb = sv_lds + (kt & 1) * SV_STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            x3_h8 th[2], tl[2], eh[2], el[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                th[i] = *reinterpret_cast<const x3_h8*>(sb + t_off[ks][0] + i * 4096);
                tl[i] = *reinterpret_cast<const x3_h8*>(sb + t_off[ks][1] + i * 4096);
                eh[i] = *reinterpret_cast<const x3_h8*>(sb + e_off[ks][0] + i * 4096);
                el[i] = *reinterpret_cast<const x3_h8*>(sb + e_off[ks][1] + i * 4096);
            }
            // the small cross terms first, the leading product last
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl[i], eh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[i], el[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[i], eh[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) store((kt + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: the staging memory becomes the [segments][128] maxima
    const int nseg = s_misc[1];
    for (int i = tid; i < nseg * SV_BN; i += 256) red[i] = 0u;
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cl = wn * 64 + j * 32 + fr, col = v0 + cl;
        const bool cok = col < V;
        const float bias = cok ? dec_b[col] : 0.f;
        int cur = -1;
        float run = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int seg = s_seg[wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh];
                if (seg != cur) {  // (rows ascend: a segment is one run)
                    if (cur >= 0 && cok) atomicMax(&red[cur * SV_BN + cl], nan ? kSpladeNaN : splade_ordered(run));
                    cur = seg;
                    run = -INFINITY;
                    nan = false;
                }
                const float z = acc[i][j][r] * inv_scale + bias;  // (the scale is a power of two)
                bad = bad || (cok && seg >= 0 && !(fabsf(z) < INFINITY));
                nan = nan || z != z;
                run = fmaxf(run, z);
            }
        if (cur >= 0 && cok) atomicMax(&red[cur * SV_BN + cl], nan ? kSpladeNaN : splade_ordered(run));
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(flag, 1u);
    __syncthreads();
    for (int i = tid; i < nseg * SV_BN; i += 256) {
        const unsigned int o = red[i];
        const int col = v0 + (i & (SV_BN - 1));
        if (!(o & 0x80000000u) || col >= V) continue;  // nothing handed over, or a maximum below zero: relu gives 0, what the buffer holds
        const float z = __uint_as_float(o & 0x7fffffffu);
        const unsigned int bits = o == kSpladeNaN ? 0x7fc00000u : z > 0.f ? __float_as_uint(log1pf(z)) : 0u;
        if (bits) atomicMax(out + (int64_t)s_segb[i >> 7] * V + col, bits);
    }
}

// ---- pruning: one workgroup per sentence ----------------------------------------------------------------------------------------
// Keeps the max_terms largest weights of w[b, 0..V) that are > 0 (NaN fails it, +inf passes) and whose id is not an unused id;
// equal weights go to the lower id; emitted by ascending id into idx / val [b, 0..max_terms) with cnt[b], zeros behind the count.
// Exact selection: the threshold = the max_terms-th largest value, found by a radix select over the float bits (four passes of
// eight bits, a 256-bin histogram in LDS each: integer atomics only); then one ordered pass: every id above the threshold, and
// the first `ties` ids AT the threshold, compacted by a block scan per 2048 ids (the counts of both kinds packed in one word).
// dense: NULL, or [b, 0..V) to receive a copy of the row (the caller's weights_dev).
constexpr int SP_ITEMS = 8;
SPLADE_KERNEL __launch_bounds__(256) void splade_prune_kernel(const unsigned int* __restrict__ w, int V, int max_terms, SpladeUnused unused,
                                                           int32_t* __restrict__ cnt, int32_t* __restrict__ idx, float* __restrict__ val,
                                                           float* __restrict__ dense) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned int s_prefix, s_need, s_total;
    __shared__ unsigned int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int* row = w + (int64_t)b * V;
    auto key_of = [&](int id) SPLADE_INLINE -> unsigned int {  // the bits of an eligible weight, 0 otherwise
        const unsigned int bits = row[id];
        bool keep = __uint_as_float(bits) > 0.f;
        for (int u = 0; u < kSpladeMaxUnused; ++u) keep = keep && !(u < unused.n && unused.id[u] == id);
        return keep ? bits : 0u;
    };
    if (tid == 0) {
        s_prefix = 0u;
        s_need = (unsigned int)max_terms;
        s_total = 0u;
    }
    // the threshold: byte by byte from the top, among the keys that agree with the prefix found so far
    for (int pass = 3; pass >= 0; --pass) {
        hist[tid] = 0u;
        __syncthreads();
        const unsigned int prefix = s_prefix, hi_mask = pass == 3 ? 0u : 0xffffffffu << (8 * (pass + 1));
        unsigned int mine = 0u;
        for (int id = tid; id < V; id += 256) {
            const unsigned int key = key_of(id);
            if (pass == 3 && dense) dense[(int64_t)b * V + id] = __uint_as_float(row[id]);
            if (key && (key & hi_mask) == prefix) {
                atomicAdd(&hist[(key >> (8 * pass)) & 255u], 1u);
                ++mine;
            }
        }
        if (pass == 3 && mine) atomicAdd(&s_total, mine);
        __syncthreads();
        if (s_total <= (unsigned int)max_terms) break;  // everything eligible is kept (uniform: s_total is final after pass 3)
        if (tid == 0) {
            unsigned int need = s_need, bin = 255u;
            for (;; --bin) {  // bins from the top: the one that holds the need-th largest (it exists: s_total > max_terms >= need)
                if (hist[bin] >= need || bin == 0u) break;
                need -= hist[bin];
            }
            s_need = need;
            s_prefix = prefix | (bin << (8 * pass));
        }
        __syncthreads();
    }
    __syncthreads();
    const bool all = s_total <= (unsigned int)max_terms;
    const unsigned int thr = all ? 0u : s_prefix;        // keep keys > thr ...
    const unsigned int ties = all ? 0u : s_need;         // ... and the first `ties` keys == thr by ascending id
    // ordered compaction: thread -> SP_ITEMS consecutive ids of a 2048-id chunk; word = (count above) | (count at) << 16
    unsigned int above_run = 0u, at_run = 0u;
    for (int base = 0; base < V; base += 256 * SP_ITEMS) {
        unsigned int key[SP_ITEMS];
        unsigned int word = 0u;
        const int id0 = base + tid * SP_ITEMS;
#pragma unroll
        for (int u = 0; u < SP_ITEMS; ++u) {
            key[u] = id0 + u < V ? key_of(id0 + u) : 0u;
            word += key[u] > thr ? 1u : (key[u] && key[u] == thr ? 0x10000u : 0u);
        }
        unsigned int incl = word;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        __syncthreads();  // (wsum of the chunk before)
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned int excl = incl - word;
        for (int q = 0; q < wave; ++q) excl += wsum[q];
        const unsigned int chunk = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        unsigned int above = above_run + (excl & 0xffffu), at = at_run + (excl >> 16);
#pragma unroll
        for (int u = 0; u < SP_ITEMS; ++u) {
            const bool is_above = key[u] > thr, is_at = !is_above && key[u] && key[u] == thr;
            if (is_above || (is_at && at < ties)) {
                const unsigned int pos = above + min(at, ties);
                idx[(int64_t)b * max_terms + pos] = id0 + u;
                val[(int64_t)b * max_terms + pos] = __uint_as_float(key[u]);
            }
            above += is_above;
            at += is_at;
        }
        above_run += chunk & 0xffffu;
        at_run += chunk >> 16;
    }
    const int total = (int)(above_run + min(at_run, ties));
    for (int i = total + tid; i < max_terms; i += 256) {
        idx[(int64_t)b * max_terms + i] = 0;
        val[(int64_t)b * max_terms + i] = 0.f;
    }
    if (tid == 0) cnt[b] = total;
}
