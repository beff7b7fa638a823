// join_scan.hpp — the range join (mvdb_index_range_join): a range search whose queries are STORED rows, each matched against
// the rows stored before it.  Query i is row qrows[i] with its fp32 bits as they sit in the matrix, and only rows whose row
// number is below qrows[i] can match: every pair of near rows is reported once, from its later member.
//
// The arithmetic is range_scan.hpp's, unchanged — join_scan_kernel is range_scan_body.hpp with the bound switched on — so a returned
// score is bit for bit what mvdb_index_range_search returns for the same row uploaded as a query (tests/test_join_gpu.py).
//
// Roofline: HBM.  Algorithmic bytes per launch of join_scan_kernel = sum over the queries of min(before_i, n) * ld * 4 for the
// streamed forms (the batch loop ends at the bound), m * (ld * 4 + 8) per query for a row list (every listed row is read, the
// bound gates what is kept), + 8 per passing row.  The shared pass (half_scan.hip: join_nominate_h16_kernel) streams
// max(before) * d * 2 bytes of the fp16 shadow once per 128 / 256 query rows.
#pragma once
#include "range_scan.hpp"

namespace mvdb {

struct JoinScanArgs : RangeScanArgs {
    const int64_t* before = nullptr;  // [nq]: query i matches rows whose row number is below before[i]
};

template <int G, int C, int U, int METRIC, int SEL, bool MASKED>
__global__ __launch_bounds__(kScanThreads) void join_scan_kernel(JoinScanArgs a) {
    constexpr bool BOUND = true;
    const int64_t* const bounds = a.before;
#include "range_scan_body.hpp"
}

// The query rows of one launch group that are not consecutive: dst[i, :] = X[qrows[i], :] at the matrix' stride (the padding
// floats travel with the row), 16 bytes per thread.
__global__ __launch_bounds__(256) void join_gather_kernel(float* __restrict__ dst, const float* __restrict__ X,
                                                          const int64_t* __restrict__ qrows, int64_t nq, int64_t ld) {
    const int64_t d4 = ld / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * d4) return;
    const int64_t r = i / d4, c = i - r * d4;
    *reinterpret_cast<f32x4*>(dst + r * ld + c * 4) = *reinterpret_cast<const f32x4*>(X + qrows[r] * ld + c * 4);
}

}  // namespace mvdb
