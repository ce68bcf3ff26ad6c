// Tile helpers of the score-sweep kernels: sampled_softmax.hip (YoutubeNet's loss) and margin_rank.hip (EBR's).  A block of 4 waves
// owns 64 rows, each wave 16 of them in registers as the B operand of the TRANSPOSED score tile S^T = T U^T on
// v_mfma_f32_16x16x4_f32, whose accumulator layout is the B operand of the product that follows; the other side's rows come through a
// 64-row LDS tile.  Internal linkage: each translation unit instantiates its own copies.
#pragma once
#include "dr_common.h"

namespace {

constexpr int SS_TILE = 64;                         // rows of a tile in LDS; 4 waves x 16 owned rows per block
static_assert(SS_TILE == DR_SAMPLED_SOFTMAX_TILE && SS_TILE == DR_MARGIN_RANK_TILE, "one tile geometry for both families");

// rows base[rowid[r] * ld .. + D) for r < 64 -> lds[64][DP + 4]; a row with rowid[r] < 0 and the columns beyond D are zeros
template <int DP>
__device__ __forceinline__ void ss_load_tile(float* lds, const float* base, int64_t ld, const int* rowid, int D) {
    constexpr int LS = DP + 4, C4 = DP / 4;
    for (int i = threadIdx.x; i < SS_TILE * C4; i += 256) {
        const int r = i / C4, c = (i - r * C4) * 4;
        const int rid = rowid[r];
        dr_f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (rid >= 0 && c < D) val = *reinterpret_cast<const dr_f32x4*>(base + (int64_t)rid * ld + c);
        *reinterpret_cast<dr_f32x4*>(lds + r * LS + c) = val;
    }
}

// the wave's own 16 rows as an MFMA operand: reg[4c + e] = row[16c + 4g + e] (row == nullptr: zeros)
template <int DP>
__device__ __forceinline__ void ss_load_frag(float (&reg)[DP / 4], const float* row, int D, int g) {
#pragma unroll
    for (int c = 0; c < DP / 16; ++c) {
        const int d0 = 16 * c + 4 * g;
        dr_f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (row && d0 < D) val = *reinterpret_cast<const dr_f32x4*>(row + d0);
#pragma unroll
        for (int e = 0; e < 4; ++e) reg[4 * c + e] = val[e];
    }
}

// S^T tile: acc[t][r] = sum_d tile[16t + 4g + r][d] * own[i16][d]
template <int DP>
__device__ __forceinline__ void ss_tile_dot(const float* tile, const float (&own)[DP / 4], int i16, int g, dr_f32x4 (&acc)[4]) {
    constexpr int LS = DP + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dr_f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DP / 16; ++c) {
            const dr_f32x4 a = *reinterpret_cast<const dr_f32x4*>(tile + (16 * t + i16) * LS + 16 * c + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], own[4 * c + e], a4, 0, 0, 0);
        }
        acc[t] = a4;
    }
}

// out^T += tile^T w: out[dt][r'] (column 16dt + 4g + r' of row i16) += sum_{t, r} tile[16t + 4g + r][.] * w[t][r]
template <int DP>
__device__ __forceinline__ void ss_tile_acc(const float* tile, const dr_f32x4 (&w)[4], int i16, int g, dr_f32x4 (&out)[DP / 16]) {
    constexpr int LS = DP + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* src = tile + (16 * t + 4 * g + r) * LS + i16;
#pragma unroll
            for (int dt = 0; dt < DP / 16; ++dt) out[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(src[16 * dt], w[t][r], out[dt], 0, 0, 0);
        }
}

// u_i . trow_i with the arithmetic of a score: the 16 x 16 product of the wave's 16 partner rows with its 16 own rows, of which
// lane (i16, g = i16 / 4) holds the diagonal entry in register i16 % 4.  A tile column holding the same row scores the same bits.
template <int DP>
__device__ __forceinline__ float ss_true_dot(const float* trow, const float (&own)[DP / 4], int D, int i16, int g) {
    dr_f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DP / 16; ++c) {
        const int d0 = 16 * c + 4 * g;
        dr_f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (trow && d0 < D) a = *reinterpret_cast<const dr_f32x4*>(trow + d0);
#pragma unroll
        for (int e = 0; e < 4; ++e) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], own[4 * c + e], a4, 0, 0, 0);
    }
    const int r = i16 & 3;
    const float cand = r == 0 ? a4[0] : r == 1 ? a4[1] : r == 2 ? a4[2] : a4[3];
    return __shfl(cand, i16 + 16 * (i16 >> 2), 64);
}

}  // namespace
