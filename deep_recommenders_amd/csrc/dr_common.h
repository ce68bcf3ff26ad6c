// Shared helpers for the gfx950 kernels behind include/dr_hotpath.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dr_hotpath.h"

#define DR_WAVE 64

#define DR_CHECK_LAUNCH()                                   \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return DR_ELAUNCH;           \
    } while (0)

static inline hipStream_t dr_s(dr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// memory-bound kernels: cap the grid at 256 CUs x 8 blocks and grid-stride the rest
static inline int dr_grid_for(int64_t work_items, int items_per_block, int max_blocks = 2048) {
    int64_t g = (work_items + items_per_block - 1) / items_per_block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

// ---- argument checks shared by the entry points ----
// float4 access needs a 16-byte address; a null pointer is aligned (whether it may be null is the caller's test)
static inline bool dr_aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }
// a row pitch in floats that float4 rows of `width` floats cannot use
static inline bool dr_bad_ld(int64_t ld, int64_t width) { return (ld & 3) != 0 || ld < width; }
// the smallest power of two >= n (1 for n <= 1)
static inline int dr_pow2_ceil(int n) { int v = 1; while (v < n) v <<= 1; return v; }

// Launches `kernel` with `lds` bytes of dynamic LDS and returns DR_OK or DR_ELAUNCH.  A request above OPTIN_KB KiB first raises the
// kernel's hipFuncAttributeMaxDynamicSharedMemorySize to it (64 KiB is the runtime's limit without it; din.hip and metrics.hip
// opt in from 48 KiB).
template <int OPTIN_KB = 64, typename K, typename... Args>
static inline int dr_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
    if (lds > (size_t)OPTIN_KB * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DR_ELAUNCH;
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// ---- device vocabulary ----
typedef float dr_f32x4 __attribute__((ext_vector_type(4)));
typedef float dr_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float4 dr_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float dr_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float dr_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int dr_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// lane `src`'s value on every lane; src is wave-uniform (a scalar read)
__device__ __forceinline__ float dr_readlane(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// lowbias32-style integer hash of (seed, index): well mixed, one multiply chain per element.  The dropout kernels (dr_dropout_fwd,
// dr_attn_*, dr_token_embedding_*) keep an element iff dr_mix32(seed, index) >= dr_drop_thresh(rate).
__host__ __device__ __forceinline__ uint32_t dr_mix32(uint64_t seed, uint64_t idx) {
    uint64_t z = idx * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
__host__ __device__ __forceinline__ uint32_t dr_drop_thresh(float rate) {
    return (uint32_t)fminf(4294967040.f, rate * 4294967296.f);
}

// The sigmoid of dr_sigmoid_fwd; dr_confusion_hist_update(from_logits = 1) must bin exactly the probability that kernel stores.
__device__ __forceinline__ float dr_sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// Binary cross-entropy terms of one example, logit x, label z (shared by the stand-alone loss kernel and the fused tower
// head).  mode 0: [TF] sigmoid_cross_entropy_with_logits  max(x,0) - x z + log1p(exp(-|x|)) ; mode 1: tf.losses.log_loss
// on p = sigmoid(x) (eps 1e-7) ; mode 2: keras binary_crossentropy (p clipped to [eps, 1-eps] first).  Outputs the
// probability, the loss term and d(loss term)/dx.
__device__ __forceinline__ void dr_bce_terms(float x, float z, int mode, float& p, float& l, float& g) {
    p = 1.f / (1.f + expf(-x));
    if (mode == 0) {
        l = fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
        g = p - z;
    } else {
        const float eps = 1e-7f;
        float pc = p;
        float dclip = 1.f;
        if (mode == 2) {
            if (p < eps) { pc = eps; dclip = 0.f; }
            else if (p > 1.f - eps) { pc = 1.f - eps; dclip = 0.f; }
        }
        l = -z * logf(pc + eps) - (1.f - z) * logf(1.f - pc + eps);
        const float dl_dp = -z / (pc + eps) + (1.f - z) / (1.f - pc + eps);
        g = dl_dp * dclip * p * (1.f - p);
    }
}

// dst[0] += alpha * sum_{i<n} x[i], computed by ONE 256-thread block in a fixed order (deterministic) and written
// with a plain read-modify-write: the caller guarantees this block is the only writer of dst during the kernel.
// Replaces "one same-address atomic per wave": tens of thousands of those serialise on a single L2 channel
// (~88 per microsecond on MI355X) and were costing more than the scatter kernel they decorated.
__device__ __forceinline__ void dr_block_sum_axpy(const float* __restrict__ x, int64_t n, float alpha,
                                                  float* __restrict__ dst) {
    __shared__ float dr_wsum_[4];
    float acc = 0.f;
    const int64_t nv = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? (n >> 2) : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int64_t i = threadIdx.x; i < nv; i += 256 * 4) {
        float4 a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t q = i + j * 256;
            a[j] = x4[q < nv ? q : i];
            if (q >= nv) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (a[j].x + a[j].y) + (a[j].z + a[j].w);
    }
    for (int64_t i = (nv << 2) + threadIdx.x; i < n; i += 256) acc += x[i];
    acc = dr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) dr_wsum_[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dst[0] = fmaf(alpha, (dr_wsum_[0] + dr_wsum_[1]) + (dr_wsum_[2] + dr_wsum_[3]), dst[0]);
}
