// The second launch of a two-stage reduction: the fixed-order sum of the partials that a first kernel left in a workspace.
#pragma once
#include "dr_common.h"

// part holds `parts` partials of total = n0 + n1 + n2 floats.  Element t of the result is 0.f + part[0][t] + part[1][t] + ... in that
// order (so the bits, a -0.f included, depend on the partials alone) and goes to dst0 | dst1 | dst2 by segment; a null destination
// skips its segment's store.  Grid-strided: the values do not depend on the grid.  Internal linkage, as the kernels of
// gemm_f32_core.h: several translation units of the one library include this header.
namespace {
__global__ __launch_bounds__(256) void dr_sum_partials_kernel(const float* __restrict__ part, int64_t parts, int64_t n0, int64_t n1,
                                                              int64_t n2, float* __restrict__ dst0, float* __restrict__ dst1,
                                                              float* __restrict__ dst2) {
    const int64_t total = n0 + n1 + n2, stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        float acc = 0.f;
        for (int64_t k = 0; k < parts; ++k) acc += part[k * total + t];
        if (t < n0) { if (dst0 != nullptr) dst0[t] = acc; }
        else if (t < n0 + n1) { if (dst1 != nullptr) dst1[t - n0] = acc; }
        else if (dst2 != nullptr) dst2[t - n0 - n1] = acc;
    }
}
}  // namespace

static inline int dr_sum_partials(const float* part, int64_t parts, float* dst0, int64_t n0, float* dst1, int64_t n1, float* dst2,
                                  int64_t n2, unsigned grid, hipStream_t stream) {
    return dr_launch(dr_sum_partials_kernel, dim3(grid), dim3(256), 0, stream, part, parts, n0, n1, n2, dst0, dst1, dst2);
}
