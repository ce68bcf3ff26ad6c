// The tower tail's arithmetic, shared by its two homes: tower_tail_fused_kernel (tower_tail.hip: a pass of its own over h0) and the
// tail epilogue of the fused first-layer forward (bf3_emb_linear.hip: the same steps on the accumulators, h0 is not read back from HBM).
// Both kernels keep x in the 32x32 MFMA's C/D layout -- lane (c, h) holds x[tt_row(s, h)][column c of its tile], s < 16 -- and run
// the three bodies below, so a row's prob / d_logit / d_h / dx are the same bits whichever kernel produced them.
#pragma once
#include "dr_common.h"

namespace drtail {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TT_ROWS = 32;     // rows per chunk (one MFMA tile)
constexpr int TT_P = 33;        // LDS pitch of the dy chunk
constexpr int TAIL_HEAD_PART = 34;          // == HEAD_PART of gemm_f32_core.h: dw2[32], db2, loss

// s_barrier behind the wave's own LDS traffic only.  __syncthreads() also waits vmcnt(0): with it every barrier of the tail's loop would
// sit out the NEXT chunk's prefetch (and this chunk's dx stores) -- three times per chunk.  The hazards the barriers order are all
// LDS ones; registers loaded from HBM are waited for by the compiler where they are used.
__device__ __forceinline__ void tail_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ int tt_row(int j, int h) { return (j & 3) + 8 * (j >> 2) + 4 * h; }

// The three stage bodies are macros, not functions: as inlined functions they compile tower_tail_fused_kernel to the same operations
// in another order and with swapped operands, and tools/asm_compare.py holds that kernel to its text.
//
// Head product, one 32-column slice of x: ACC1[m][n] += sum_j x[m][cb + j] W1[cb + j][n] over the 16 columns XR points at (row m = the
// lane's c, cb = slice base + 16 h; row-major in the LDS, 16-byte aligned), W1F[j] = W1[cb + j][n = c].  NQ < 4 is a timing experiment
// of tower_tail.hip (wrong results).
#define DR_TAIL_HEAD_MFMA(NQ, ACC1, XR, W1F)                                                          \
    _Pragma("unroll") for (int q = 0; q < (NQ); ++q) {                                               \
        const float4 v = *reinterpret_cast<const float4*>((XR) + 4 * q);                             \
        ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, W1F[4 * q + 0], ACC1, 0, 0, 0);             \
        ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, W1F[4 * q + 1], ACC1, 0, 0, 0);             \
        ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, W1F[4 * q + 2], ACC1, 0, 0, 0);             \
        ACC1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, W1F[4 * q + 3], ACC1, 0, 0, 0);             \
    }

// Head epilogue of ONE row (gemm_f32_core.h EPI_HEAD), lane c = hidden unit: V comes in as the row's pre-activation sum (the slices' partial
// products added in slice order) and leaves as the activation; Dense(1) as a 32-lane butterfly, + the extra logit EXT, the BCE terms
// against the label LAB (BCE = false: a timing experiment of tower_tail.hip), GS = d logit / n, DH = d h1.  A row that is not LIVE
// contributes no loss and no gradient.  Declares P, L, GS, DH (and dot, lg, gr) in the caller's scope.
#define DR_TAIL_HEAD_ROW(BCE, V, B1J, CV, W2J, B2V, EXT, LAB, LOSS_MODE, INV_N, LIVE, P, L, GS, DH) \
    V = fmaxf(V + (B1J), 0.f);                                                                      \
    if (!(CV)) V = 0.f;                                                                             \
    float dot = V * (W2J);                                                                          \
    _Pragma("unroll") for (int o = 1; o < 32; o <<= 1) dot += __shfl_xor(dot, o, 64);               \
    const float lg = (dot + (B2V)) + (EXT);                                                         \
    float P, L, gr;                                                                                 \
    if constexpr (!(BCE)) { P = lg; L = lg; gr = lg - (LAB); }                                      \
    else dr_bce_terms(lg, (LAB), (LOSS_MODE), P, L, gr);                                            \
    float GS = gr * (INV_N);                                                                        \
    if (!(LIVE)) { L = 0.f; GS = 0.f; }                                                             \
    const float DH = !(V > 0.f) ? 0.f : GS * (W2J);

// Narrow backward of one 32 x 32 tile of x (rows = the chunk, columns = the lane's tile): ACCW[k][n] += sum_m x[m][k] dh[m][n], then
// dx = (dh W1^T) masked by x > 0, which OVERWRITES XV.  DXA[s] = dh[m = c][n = 2 s + h], DWB[s] = dh[m = tt_row(s, h)][n = c],
// WF[s] = W1[column c of the tile][2 s + h] (zero past H).  NS < 16 is a timing experiment of tower_tail.hip (wrong results).
#define DR_TAIL_BWD_TILE(NS, XV, DXA, DWB, WF, ACCW, DX_MAX)                                                                      \
    _Pragma("unroll") for (int s = 0; s < (NS); ++s) ACCW = __builtin_amdgcn_mfma_f32_32x32x2f32(XV[s], DWB[s], ACCW, 0, 0, 0);   \
    {                                                                                                                             \
        drtail::f32x16 acc_;                                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) acc_[j] = 0.f;                                                             \
        _Pragma("unroll") for (int s = 0; s < (NS); ++s) acc_ = __builtin_amdgcn_mfma_f32_32x32x2f32(DXA[s], WF[s], acc_, 0, 0, 0); \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                                                          \
            float v_ = acc_[j];                                                                                                   \
            if (!(XV[j] > 0.f)) v_ = 0.f;                                                                                         \
            DX_MAX = fmaxf(DX_MAX, fabsf(v_));                                                                                    \
            XV[j] = v_;                                                                                                           \
        }                                                                                                                         \
    }

// The fixed-order reduce of the tail's per-block partials (tower_tail_reduce_kernel, tower_tail.hip): partial [nparts][(K + 1) * 32],
// head_partial [nparts][34], amax_part [nparts] (may be null).  Applies the four steps, writes the loss and STORES the dx record.
int launch_reduce(const float* partial, const float* head_partial, int32_t nparts, int32_t K, int32_t H, float scale, float inv_n,
                  float* dst_w1, int64_t ld_dst_w1, float* dst_b1, float* dst_w2, int64_t ld_dst_w2, float* dst_b2, float* loss_out,
                  const uint32_t* amax_part, uint32_t* dx_amax, dr_stream_t stream);

}  // namespace drtail
