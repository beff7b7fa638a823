// BGE-M3's two extra heads on the encoder's last hidden states (included by encoder.hip, inside its kernel namespace):
//   token weight   tw[b,t] = relu(sparse_w . x[b,t] + sparse_b)                      (sparse_linear: Linear(H, 1) + ReLU)
//   lexical weights of a sentence = for every distinct token id that is not an unused id, the LARGEST tw among its tokens
//   ColBERT vector v[b,t-1] = normalize(colbert_w x[b,t] + colbert_b), t >= 1        (colbert_linear: Linear(H, C); CLS dropped)
// The ColBERT projection is one more GEMM of the encoder's own launchers (enqueue_m3_heads, encoder.hip); the two kernels here do
// the rest.  Neither uses an atomic in a sum: every reduction is lane-strided partial sums in column order, then the xor butterfly
// 32, 16, ... 1 — the same bits run to run, whatever the batch around a sentence.
//
// C = colbert_dim: a multiple of 32 with C <= H (the GEMM launchers tile N in 32-column pieces — every width of this encoder is a
// multiple of 32 in the split-precision mode, H = 96 included — and the rows here are read in 16-byte pieces).
#pragma once

constexpr int kM3MaxS = 1024;    // m3_lex_kernel sorts a sentence in LDS: 8 KiB of keys at S = 1024
constexpr int kM3MaxUnused = 8;  // unused_ids (BGE-M3: cls, pad, eos, unk)

struct M3Unused {
    int n;
    int id[kM3MaxUnused];
};

// sum over the wave, fixed order
__device__ __forceinline__ float m3_wave_sum(float s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    return s;
}

// One wave per token SLOT (b, t) of the padded batch, V4 = ceil(H / 256) 16-byte pieces per lane (the last one bounds-tested:
// H = 96 fills 24 of the 64 lanes).  A valid slot (rank >= 0; its packed row p = seq_start[b] + rank):
//   tw[b,t] = relu(sparse_w . x[p] + sparse_b) (NaN stays NaN, as torch.relu), and, t >= 1, colbert[b,t-1,:] = y[p] / max(|y[p]|, 1e-12)
//   (y = the projected rows, [T][C]).  A masked slot writes tw = 0 and a zero ColBERT row: the KERNEL covers the padding, no memset
//   node — every output element is written exactly once per forward.  The wave of slot t = 0 also writes colbert_count[b].
// flag: ORed with 1 when a valid token's weight, or the squared norm of a ColBERT row, is not finite (the pooled row's protocol).
// tw / colbert may be NULL (output not wanted).
template <int V4>
__global__ __launch_bounds__(256) void m3_rows_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      const int* __restrict__ rank, const int* __restrict__ seq_start,
                                                      const int* __restrict__ count, int B, int S, int H, int C,
                                                      const float* __restrict__ sparse_w, const float* __restrict__ sparse_b,
                                                      float* __restrict__ tw, float* __restrict__ colbert,
                                                      int32_t* __restrict__ colbert_count, unsigned int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t bt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= (int64_t)B * S) return;
    const int b = (int)(bt / S), t = (int)(bt - (int64_t)b * S);
    const int r = rank[bt];
    const int h4 = H >> 2, c4 = C >> 2;
    float4* crow = colbert && t >= 1 ? reinterpret_cast<float4*>(colbert + ((int64_t)b * (S - 1) + (t - 1)) * C) : nullptr;
    if (colbert_count && t == 0 && lane == 0) colbert_count[b] = max(count[b] - 1, 0);
    if (r < 0) {
        if (tw && lane == 0) tw[bt] = 0.f;
        if (crow) {
#pragma unroll
            for (int i = 0; i < V4; ++i)
                if (lane + 64 * i < c4) crow[lane + 64 * i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const int64_t p = (int64_t)seq_start[b] + r;
    if (tw) {
        const float4* xr = reinterpret_cast<const float4*>(x + p * H);
        const float4* wr = reinterpret_cast<const float4*>(sparse_w);
        float4 xv[V4], wv[V4];
#pragma unroll
        for (int i = 0; i < V4; ++i) {
            const int q = lane + 64 * i < h4 ? lane + 64 * i : 0;
            xv[i] = xr[q];
            wv[i] = wr[q];
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V4; ++i)
            if (lane + 64 * i < h4) s += xv[i].x * wv[i].x + xv[i].y * wv[i].y + xv[i].z * wv[i].z + xv[i].w * wv[i].w;
        s = m3_wave_sum(s) + sparse_b[0];
        const float v = (s > 0.f || s != s) ? s : 0.f;
        if (lane == 0) {
            tw[bt] = v;
            if (!(v < INFINITY)) atomicOr(flag, 1u);
        }
    }
    if (crow) {
        const float4* yr = reinterpret_cast<const float4*>(y + p * C);
        float4 u[V4];
#pragma unroll
        for (int i = 0; i < V4; ++i) u[i] = yr[lane + 64 * i < c4 ? lane + 64 * i : 0];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < V4; ++i)
            if (lane + 64 * i < c4) ss += u[i].x * u[i].x + u[i].y * u[i].y + u[i].z * u[i].z + u[i].w * u[i].w;
        ss = m3_wave_sum(ss);
        const float denom = fmaxf(sqrtf(ss), 1e-12f);
        if (lane == 0 && !(ss < INFINITY)) atomicOr(flag, 1u);
#pragma unroll
        for (int i = 0; i < V4; ++i)
            if (lane + 64 * i < c4) crow[lane + 64 * i] = make_float4(u[i].x / denom, u[i].y / denom, u[i].z / denom, u[i].w / denom);
    }
}

// One workgroup per sentence: the (id, tw) pairs of its S slots as 64-bit keys id << 32 | bits(tw) in LDS — kept weights are
// > 0 (or +inf), so the order of the bits is the order of the values —, a bitonic sort over n = the next power of two >= S, then
// the LAST key of every run of equal ids (= that id's maximum) is kept and the kept keys are compacted by a block scan.
// Masked slots, unused ids, ids < 0 and weights that are not > 0 (zero, NaN) become the all-ones key, which sorts last.
// Writes idx[b, 0..m) (ascending), val[b, 0..m), cnt[b] = m, and zeros behind m up to S (the outputs hold no stale word).
__global__ __launch_bounds__(256) void m3_lex_kernel(const int32_t* __restrict__ ids, const int* __restrict__ rank,
                                                     const float* __restrict__ tw, int S, M3Unused unused,
                                                     int32_t* __restrict__ cnt, int32_t* __restrict__ idx, float* __restrict__ val) {
    __shared__ unsigned long long keys[kM3MaxS];
    __shared__ int part[256];
    constexpr unsigned long long kLast = ~0ull;
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = 2;
    while (n < S) n <<= 1;
    for (int t = tid; t < n; t += 256) {
        unsigned long long key = kLast;
        if (t < S && rank[(int64_t)b * S + t] >= 0) {
            const int id = ids[(int64_t)b * S + t];
            const float w = tw[(int64_t)b * S + t];
            bool keep = id >= 0 && w > 0.f;
#pragma unroll
            for (int u = 0; u < kM3MaxUnused; ++u) keep = keep && !(u < unused.n && unused.id[u] == id);
            if (keep) key = ((unsigned long long)(unsigned int)id << 32) | __float_as_uint(w);
        }
        keys[t] = key;
    }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (n >> 1); i += 256) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], c = keys[hi];
                const bool up = (lo & k) == 0;
                if ((a > c) == up) {
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    // thread `tid` owns the keys [tid * per, tid * per + per): per = n / 256 (1 below 256 keys: the threads past n own none)
    const int per = n >= 256 ? n >> 8 : 1;
    const int k0 = tid * per;
    unsigned int kept = 0;  // bit u: key k0 + u is the last of its id's run
    if (k0 < n) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u >= per) break;
            const unsigned long long key = keys[k0 + u];
            const unsigned long long next = k0 + u + 1 < n ? keys[k0 + u + 1] : kLast;
            if (key != kLast && (key >> 32) != (next >> 32)) kept |= 1u << u;
        }
    }
    const int mine = __popc(kept);
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan
        const int add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const int total = part[255];
    int pos = part[tid] - mine;
    if (k0 < n) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u >= per) break;
            if (kept >> u & 1u) {
                const unsigned long long key = keys[k0 + u];
                idx[(int64_t)b * S + pos] = (int32_t)(key >> 32);
                val[(int64_t)b * S + pos] = __uint_as_float((unsigned int)key);
                ++pos;
            }
        }
    }
    for (int t = total + tid; t < S; t += 256) {
        idx[(int64_t)b * S + t] = 0;
        val[(int64_t)b * S + t] = 0.f;
    }
    if (tid == 0) cnt[b] = total;
}
