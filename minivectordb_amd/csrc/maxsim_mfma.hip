// maxsim_mfma.hip — the one translation unit that instantiates maxsim_mfma_kernel (maxsim_mfma.hpp) and launches it.
// The Makefile builds it without the packed fp32 operations.
#include "maxsim_mfma.hpp"

namespace mvdb {
namespace {

template <int PS, int SEL>
int launch_maxsim_mfma_inst(const MaxsimMfmaArgs& a, int device, size_t lds_limit, hipStream_t stream) {
    void (*kern)(MaxsimMfmaArgs) = maxsim_mfma_kernel<PS, SEL>;
    const size_t lds = maxsim_mfma_lds_bytes(a.ld);
    if (lds > lds_limit)
        return fail(MVDB_ERR_ARG, "MaxSim search on the matrix cores: a pass needs %zu bytes of LDS, the device gives a workgroup %zu", lds, lds_limit);
    MVDB_TRY(ensure_dynamic_lds((const void*)kern, lds, device));
    // two resident workgroups per CU — two waves per SIMD, one's epilogue under the other's matrix instructions — where the
    // vectors leave LDS for them (d <= 512)
    const int per_cu = std::max(1, std::min(cached_occupancy((const void*)kern, kMaxsimMfmaThreads, lds, 1), 2));
    const int64_t ntiles = (a.n + kMaxsimMfmaRows - 1) / kMaxsimMfmaRows;
    const int64_t want = (ntiles + kMaxsimMfmaWaves - 1) / kMaxsimMfmaWaves;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cus(device) * per_cu));
    return profiled_launch("maxsim_scan", stream, [&](hipEvent_t done) { launch_kernel(kern, dim3(nblocks), dim3(kMaxsimMfmaThreads), lds, stream, done, a); },
                           "maxsim_mfma_kernel<%d, %d>", PS, SEL);
}

template <int PS>
int launch_maxsim_mfma_sel(const MaxsimMfmaArgs& a, int device, size_t lds_limit, hipStream_t stream) {
    if (a.rows) return launch_maxsim_mfma_inst<PS, 1>(a, device, lds_limit, stream);
    if (a.mask) return launch_maxsim_mfma_inst<PS, 2>(a, device, lds_limit, stream);
    return launch_maxsim_mfma_inst<PS, 0>(a, device, lds_limit, stream);
}

}  // namespace

int launch_maxsim_mfma(const MaxsimMfmaArgs& a, int device, size_t lds_limit, hipStream_t stream) {
    if (!maxsim_mfma_width_ok((int64_t)a.d4 * 4, a.ld) || a.Tp < 1 || a.Tp > kMaxsimMfmaTokens || a.n < 1)
        return fail(MVDB_ERR_ARG, "MaxSim search on the matrix cores: unsupported shape (d %d, ld %lld, %d vectors)", a.d4 * 4, (long long)a.ld, a.Tp);
    switch (maxsim_mfma_ps(a.ld)) {
        case 4: return launch_maxsim_mfma_sel<4>(a, device, lds_limit, stream);
        case 2: return launch_maxsim_mfma_sel<2>(a, device, lds_limit, stream);
        default: return launch_maxsim_mfma_sel<1>(a, device, lds_limit, stream);
    }
}

}  // namespace mvdb
