// The integer kernels around the skip-gram step (csrc/sgns.hip, csrc/eges.hip): negatives drawn from a Vose alias table, and uniform or
// weighted random walks over a CSR graph (DeepWalk, Perozzi et al., KDD 2014).  All are counter-based: element i of a call is a function of (seed, position)
// alone through dr_mix32, so a draw does not depend on the launch geometry and a run is reproducible from its seed.
//
//   alias   e = offset + i;  h1 = dr_mix32(seed, 2 e);  h2 = dr_mix32(seed, 2 e + 1);  slot = (h1 * V) >> 32;  r = (h2 >> 8) * 2^-24
//           out[i] = r < prob[slot] ? slot : alias[slot]                         (r is exact in fp32: one compare, no rounding anywhere)
//   walk    walks[w, 0] = starts[w];  from v = walks[w, t - 1]:  deg = row_ptr[v + 1] - row_ptr[v],
//           walks[w, t] = col[row_ptr[v] + ((dr_mix32(seed, w L + t) * deg) >> 32)];  v outside [0, n_rows) or deg == 0 ends the walk: that
//           step and all later ones are -1.
//   weighted  the same walk with integer edge weights, given as cum [nnz], their inclusive prefix sums over the whole col array: with
//           lo = row_ptr[v], hi = row_ptr[v + 1], base = lo > 0 ? cum[lo - 1] : 0, total = cum[hi - 1] - base (< 2^32, the caller's promise),
//           t = (dr_mix32(seed, w L + t_step) * total) >> 32, the next node is col[e] for the smallest e in [lo, hi) with
//           cum[e] - base > t (binary search): edge e is taken for exactly weight(e) of the total values of t, a zero-weight edge never;
//           total == 0 ends the walk like deg == 0.  With all weights 1, cum[e] - base = e - lo + 1 and e = lo + t: dr_random_walk's walk.
// One lane per element / per walk.  A walk's loads depend on each other (row_ptr[v] -> col[...] -> the next v) and L is small: there is
// nothing to overlap inside a walk, occupancy across walks is the only lever, and the graph (Cora: 13 K edges) sits in L2.
#include "dr_common.h"

namespace {

__global__ __launch_bounds__(256) void alias_sample_kernel(const float* __restrict__ prob, const int32_t* __restrict__ alias, uint64_t V,
                                                           int64_t n, uint64_t seed, uint64_t offset, int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t e = offset + (uint64_t)i;
        const uint32_t h1 = dr_mix32(seed, 2 * e), h2 = dr_mix32(seed, 2 * e + 1);
        const uint64_t slot = ((uint64_t)h1 * V) >> 32;        // < V
        const float r = (float)(h2 >> 8) * 5.9604644775390625e-8f;   // 2^-24: a 24-bit integer, exact
        out[i] = r < prob[slot] ? (int64_t)slot : (int64_t)alias[slot];
    }
}

__global__ __launch_bounds__(256) void random_walk_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          int64_t n_rows, const int64_t* __restrict__ starts, int64_t W, int32_t L,
                                                          uint64_t seed, int64_t* __restrict__ walks) {
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < W; w += (int64_t)gridDim.x * 256) {
        int64_t v = starts[w];
        walks[w * L] = v;
        for (int t = 1; t < L; ++t) {
            int64_t next = -1;
            if (v >= 0 && v < n_rows) {
                const int64_t lo = row_ptr[v], deg = row_ptr[v + 1] - lo;
                if (deg > 0) {
                    const uint32_t h = dr_mix32(seed, (uint64_t)w * (uint64_t)L + (uint64_t)t);
                    next = col[lo + (int64_t)(((uint64_t)h * (uint64_t)deg) >> 32)];
                }
            }
            v = next;
            walks[w * L + t] = v;
        }
    }
}

__global__ __launch_bounds__(256) void random_walk_weighted_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                   const int64_t* __restrict__ cum, int64_t n_rows,
                                                                   const int64_t* __restrict__ starts, int64_t W, int32_t L, uint64_t seed,
                                                                   int64_t* __restrict__ walks) {
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < W; w += (int64_t)gridDim.x * 256) {
        int64_t v = starts[w];
        walks[w * L] = v;
        for (int t = 1; t < L; ++t) {
            int64_t next = -1;
            if (v >= 0 && v < n_rows) {
                const int64_t lo = row_ptr[v], hi = row_ptr[v + 1];
                if (hi > lo) {
                    const int64_t base = lo > 0 ? cum[lo - 1] : 0;
                    const int64_t total = cum[hi - 1] - base;
                    if (total > 0) {
                        const uint32_t h = dr_mix32(seed, (uint64_t)w * (uint64_t)L + (uint64_t)t);
                        const int64_t pick = (int64_t)(((uint64_t)h * (uint64_t)total) >> 32);       // < total
                        int64_t a = lo, b = hi - 1;                // cum[b] - base = total > pick: the answer lies in [a, b]
                        while (a < b) {
                            const int64_t mid = a + ((b - a) >> 1);
                            if (cum[mid] - base > pick) b = mid; else a = mid + 1;
                        }
                        next = col[a];
                    }
                }
            }
            v = next;
            walks[w * L + t] = v;
        }
    }
}

}  // namespace

extern "C" int dr_alias_sample(const float* prob, const int32_t* alias, int64_t V, int64_t n, uint64_t seed, uint64_t offset,
                               int64_t* out, dr_stream_t stream) {
    if (V < 1 || V >= (1ll << 31) || n < 0) return DR_EINVAL;
    if (n == 0) return DR_OK;
    if (!prob || !alias || !out) return DR_EINVAL;
    return dr_launch(alias_sample_kernel, dim3(dr_grid_for(n, 256)), dim3(256), 0, dr_s(stream), prob, alias, (uint64_t)V, n, seed,
                     offset, out);
}

extern "C" int dr_random_walk(const int64_t* row_ptr, const int32_t* col, int64_t n_rows, const int64_t* starts, int64_t W, int32_t L,
                              uint64_t seed, int64_t* walks, dr_stream_t stream) {
    if (n_rows < 0 || W < 0 || L < 1) return DR_EINVAL;
    if (W == 0) return DR_OK;
    if (!row_ptr || !starts || !walks) return DR_EINVAL;      // col may be NULL for a graph without edges: no degree is > 0
    return dr_launch(random_walk_kernel, dim3(dr_grid_for(W, 256)), dim3(256), 0, dr_s(stream), row_ptr, col, n_rows, starts, W, L,
                     seed, walks);
}

extern "C" int dr_random_walk_weighted(const int64_t* row_ptr, const int32_t* col, const int64_t* cum, int64_t n_rows,
                                       const int64_t* starts, int64_t W, int32_t L, uint64_t seed, int64_t* walks, dr_stream_t stream) {
    if (n_rows < 0 || W < 0 || L < 1) return DR_EINVAL;
    if (W == 0) return DR_OK;
    if (!row_ptr || !starts || !walks || (col == nullptr) != (cum == nullptr)) return DR_EINVAL;     // both NULL: a graph without edges
    return dr_launch(random_walk_weighted_kernel, dim3(dr_grid_for(W, 256)), dim3(256), 0, dr_s(stream), row_ptr, col, cum, n_rows, starts,
                     W, L, seed, walks);
}
