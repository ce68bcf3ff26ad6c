// Exclusive scan of int64 counts on the device, shared by the graph kernels (csrc/graph.hip: the long-row plan and the transpose's
// radix sort; csrc/neighbor_sample.hip: the frontier's radix sort and the block CSR's row_ptr).
#pragma once
#include "dr_common.h"

namespace {

// ---- exclusive scan of int64 counts (fixed tiles: the result is exact, no atomics) ---------------------------------------------
constexpr int SCAN_TILE = 256 * 8;

__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t* red, int64_t& total) {
    // red: 4 entries of LDS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int64_t off = 0;
    for (int i = 0; i < w; ++i) off += red[i];
    total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return off + inc - v;
}

__global__ __launch_bounds__(256) void scan_reduce_kernel(const int64_t* __restrict__ x, int64_t n, int64_t* __restrict__ sums) {
    __shared__ int64_t red[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
    int64_t acc = 0;
    for (int i = threadIdx.x; i < SCAN_TILE; i += 256)
        if (base + i < n) acc += x[base + i];
    int64_t total;
    block_excl_scan(acc, red, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: exclusive scan of the nb tile sums in place, in tiles of 256
__global__ __launch_bounds__(256) void scan_top_kernel(int64_t* __restrict__ sums, int64_t nb) {
    __shared__ int64_t red[4];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t v = i < nb ? sums[i] : 0;
        int64_t total;
        const int64_t e = block_excl_scan(v, red, total);
        if (i < nb) sums[i] = carry + e;
        carry += total;
    }
}

// each thread takes 8 consecutive elements of the tile
__global__ __launch_bounds__(256) void scan_down_kernel(const int64_t* __restrict__ x, int64_t n, const int64_t* __restrict__ sums,
                                                        int64_t* __restrict__ y) {
    __shared__ int64_t red[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 8;
    int64_t v[8], acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = base + i < n ? x[base + i] : 0;
        acc += v[i];
    }
    int64_t total;
    int64_t e = block_excl_scan(acc, red, total) + sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (base + i < n) y[base + i] = e;
        e += v[i];
    }
}

inline int64_t scan_blocks(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

// y = exclusive_scan(x) (y may alias x); tmp holds scan_blocks(n) int64
void excl_scan(const int64_t* x, int64_t n, int64_t* y, int64_t* tmp, hipStream_t st) {
    const int64_t nb = scan_blocks(n);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, x, n, tmp);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, st, tmp, nb);
    hipLaunchKernelGGL(scan_down_kernel, dim3((unsigned)nb), dim3(256), 0, st, x, n, tmp, y);
}

}  // namespace
