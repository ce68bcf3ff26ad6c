// The row gather of the CSR kernels: float4 column slots of a row, and sum_k val[k] X[col[k]] over a segment of a CSR by a group of lanes.
// Shared by graph.hip (dr_csr_spmm) and intent_conv.hip (dr_intent_conv_fwd), which therefore sum a row in the same order and give the
// same bits.  Internal linkage, as dr_sum_partials.h: several translation units of the one library include this header.
#pragma once
#include "dr_common.h"

namespace {

constexpr int CSR_GATHER_BATCH = 8;           // row gathers in flight per lane

// columns 4s .. 4s+3 of a row (fewer at the tail: scalar loads, never past column D)
__device__ __forceinline__ float4 load_cols(const float* __restrict__ row, int s, int D) {
    const int c = 4 * s;
    if (c + 4 <= D) return *reinterpret_cast<const float4*>(row + c);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    r.x = row[c];
    if (c + 1 < D) r.y = row[c + 1];
    if (c + 2 < D) r.z = row[c + 2];
    return r;
}
__device__ __forceinline__ void store_cols(float* __restrict__ row, int s, int D, float4 v) {
    const int c = 4 * s;
    if (c + 4 <= D) { *reinterpret_cast<float4*>(row + c) = v; return; }
    row[c] = v.x;
    if (c + 1 < D) row[c + 1] = v.y;
    if (c + 2 < D) row[c + 2] = v.z;
}
__device__ __forceinline__ void fma4(float a, float4 x, float4& acc) {
    acc.x = fmaf(a, x.x, acc.x);
    acc.y = fmaf(a, x.y, acc.y);
    acc.z = fmaf(a, x.z, acc.z);
    acc.w = fmaf(a, x.w, acc.w);
}

// lane `src`'s value on the calling lane; G == 64 (one group per wave): src is wave-uniform, a scalar read
template <int G>
__device__ __forceinline__ int bcast_i(int v, int src) {
    if constexpr (G == 1) return v;
    else if constexpr (G == 64) return __builtin_amdgcn_readlane(v, src);
    else return __shfl(v, src, 64);
}
template <int G>
__device__ __forceinline__ float bcast_f(float v, int src) {
    return __int_as_float(bcast_i<G>(__float_as_int(v), src));
}

// sum_k val[k] X[col[k], 4s .. 4s+3] over [kb, ke) for the group of G lanes this lane belongs to (gl = lane in group).  The group
// reads PAIRS (col, val) pairs per step, coalesced (lane gl holds pairs gl, gl + G, ...), and broadcasts them in ascending k; each
// lane then has CSR_GATHER_BATCH gathers in flight.  Every lane of the wave must call this (the loop runs to the wave's longest segment).
template <int G>
__device__ __forceinline__ float4 gather_seg(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t kb, int64_t ke,
                                             const float* __restrict__ X, int64_t ld_x, int s, int D) {
    constexpr int BATCH = CSR_GATHER_BATCH;
    constexpr int PAIRS = G < BATCH ? BATCH : G;
    constexpr int P = PAIRS / G;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const int gbase = lane - gl;
    const int64_t len = ke > kb ? ke - kb : 0;
    const int n_it = dr_wave_max((int)((len + PAIRS - 1) / PAIRS));
    const bool col_ok = 4 * s < D;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int it = 0; it < n_it; ++it) {
        int cj[P];
        float vj[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int64_t k = kb + (int64_t)it * PAIRS + p * G + gl;
            cj[p] = -1;
            vj[p] = 0.f;
            if (k < ke) {
                cj[p] = col[k];
                vj[p] = val[k];
            }
        }
#pragma unroll 1
        for (int j0 = 0; j0 < PAIRS; j0 += BATCH) {     // one batch at a time: unrolled, the loads of all batches hoist (VGPRs)
            float4 x[BATCH];
            float a[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int j = j0 + u;
                const int c = bcast_i<G>(cj[P == 1 ? 0 : j / G], gbase + (j % G));
                a[u] = bcast_f<G>(vj[P == 1 ? 0 : j / G], gbase + (j % G));
                x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c >= 0 && col_ok) x[u] = load_cols(X + (int64_t)c * ld_x, s, D);
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) fma4(a[u], x[u], acc);
        }
    }
    return acc;
}

}  // namespace
