// The Transformer package (keras/models/nlp/ of the reference) on gfx950:
//   * dr_attn_fwd / dr_attn_bwd     ScaledDotProductAttention inside MultiHeadAttention (multi_head_attention.py:60-86, 122-149):
//     softmax(Q K^T / sqrt(dh) [+ mask * M] [future: where]) -> dropout -> . V for every (batch, head), the heads addressed by stride
//     inside the projected [B, L, H * dh] tensors (no split / concat copies), the [Lq, Lk] score matrix never written: online softmax
//     over 64-key tiles in the forward, recomputation from the saved (max, sum) row statistic in the backward;
//   * dr_add_layernorm_fwd / _bwd   the residual add + LayerNormalization of transformer.py:109-113, 212-219;
//   * dr_token_embedding_fwd / _bwd gather * sqrt(D) + position table + dropout (transformer.py:195-204) and its scatter back.
//
// Arithmetic of the attention: every product is the fp32-input MFMA v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation:
// the reference's tf.matmul on fp32, no operand split); head widths are zero-padded in LDS / registers to a multiple of 16.
// One wave owns 16 rows (queries in the forward and the dQ sweep, keys in the dK/dV sweep) and computes the TRANSPOSED score tile
// S^T = K Q^T, whose accumulator layout (lane = (row i16, group g): 4 consecutive tile rows 4g..4g+3 of column i16) is already the
// B-operand layout of the next product (O^T = V^T P^T) once the k slots of that MFMA are read as "tile row 16t + 4g + r": no
// transposition through LDS, and the softmax's row reductions are 16 values inside a lane plus two cross-lane steps.
//
// Masking is the reference's arithmetic in fp32, not -inf: s + mask * M with M = -2^32 + 1 (== -2^32 in fp32), then the future
// mask REPLACES entries above the diagonal by M.  A row whose scores are all M attends uniformly, so no key tile is ever skipped.
// The backward passes the gradient through the additive mask (identity) and stops it at replaced entries.
// Determinism: the dK/dV sweep owns a key block and runs over all queries, the dQ sweep owns a query block and runs over all keys
// (with the delta pass nine products instead of five); no float atomics, no waiting between workgroups; the dropout mask is regenerated from the hash.
#include "dr_common.h"
#include "dr_owner_rows.h"
#include "dr_sum_partials.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr float ATTN_MASK = -4294967296.f;      // float32(-2^32 + 1)
constexpr int ATTN_TILE = 64;                   // rows of a tile in LDS; 4 waves x 16 owned rows per block

struct AttnP {
    const float *q, *k, *v, *d_o, *stats;
    float* delta;
    const uint8_t* mask;
    float *out, *stats_out, *dq, *dk, *dv;
    int64_t ld_q, ld_k, ld_v, ld_o, ld_do, ld_dq, ld_dk, ld_dv;
    int32_t B, H, Lq, Lk, dh, future, tiles;
    uint32_t thresh;
    uint64_t seed;
    float inv_keep, sdiv, smul, gmul, gdiv;
    int32_t vec_q, vec_k, vec_v, vec_o, vec_do, vec_dq, vec_dk, vec_dv;
};

// rows [r0, r0 + 64) of a [L, dh] slice (row pitch ld) -> lds[64][DHP + 4], zero beyond L and dh
template <int DHP>
__device__ __forceinline__ void attn_load_tile(float* lds, const float* base, int64_t ld, int r0, int L, int dh, bool vec) {
    constexpr int LS = DHP + 4;
    if (vec) {
        constexpr int C4 = DHP / 4;
        for (int i = threadIdx.x; i < ATTN_TILE * C4; i += 256) {
            const int r = i / C4, c = (i - r * C4) * 4;
            dr_f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < L && c < dh) val = *reinterpret_cast<const dr_f32x4*>(base + (int64_t)(r0 + r) * ld + c);
            *reinterpret_cast<dr_f32x4*>(lds + r * LS + c) = val;
        }
    } else {
        for (int i = threadIdx.x; i < ATTN_TILE * DHP; i += 256) {
            const int r = i / DHP, c = i - r * DHP;
            lds[r * LS + c] = (r0 + r < L && c < dh) ? base[(int64_t)(r0 + r) * ld + c] : 0.f;
        }
    }
}

// the wave's own 16 rows as an MFMA operand: reg[4c + e] = row[16c + 4g + e] (row == nullptr: zeros)
template <int DHP>
__device__ __forceinline__ void attn_load_frag(float (&reg)[DHP / 4], const float* row, int dh, int g) {
#pragma unroll
    for (int c = 0; c < DHP / 16; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 16 * c + 4 * g + e;
            reg[4 * c + e] = (row && d < dh) ? row[d] : 0.f;
        }
}

// transposed accumulators (acc[dt][r] = column 16dt + 4g + r of the lane's row) -> row[d] = acc * mul / div
template <int DHP>
__device__ __forceinline__ void attn_store_frag(float* row, const dr_f32x4 (&acc)[DHP / 16], float mul, float div, int dh, int g, bool vec) {
    if (!row) return;
#pragma unroll
    for (int dt = 0; dt < DHP / 16; ++dt) {
        const int d0 = 16 * dt + 4 * g;
        dr_f32x4 val;
#pragma unroll
        for (int r = 0; r < 4; ++r) val[r] = acc[dt][r] * mul / div;
        if (vec) {
            if (d0 < dh) *reinterpret_cast<dr_f32x4*>(row + d0) = val;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (d0 + r < dh) row[d0 + r] = val[r];
        }
    }
}

// the reference's logit: scale after the product, additive padding mask, replacing future mask; -inf only for tile padding
__device__ __forceinline__ float attn_logit(float qk, const AttnP& p, float mask_add, bool hidden, bool outside) {
    float s = p.smul != 0.f ? qk * p.smul : qk / p.sdiv;
    s = s + mask_add;
    if (hidden) s = ATTN_MASK;
    if (outside) s = -INFINITY;
    return s;
}

__device__ __forceinline__ bool attn_keep(const AttnP& p, uint64_t row_base, int j) {
    return p.thresh == 0u || dr_mix32(p.seed, row_base + (uint64_t)j) >= p.thresh;
}

// S^T tile: acc[t][r] = sum_d tile[16t + 4g + r][d] * own[i16][d]
template <int DHP>
__device__ __forceinline__ void attn_tile_dot(const float* tile, const float (&own)[DHP / 4], int i16, int g, dr_f32x4 (&acc)[4]) {
    constexpr int LS = DHP + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dr_f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DHP / 16; ++c) {
            const dr_f32x4 a = *reinterpret_cast<const dr_f32x4*>(tile + (16 * t + i16) * LS + 16 * c + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], own[4 * c + e], a4, 0, 0, 0);
        }
        acc[t] = a4;
    }
}

// out^T += tile^T w: out[dt][r'] (column 16dt + 4g + r' of row i16) += sum_{t, r} tile[16t + 4g + r][.] * w[t][r]
template <int DHP>
__device__ __forceinline__ void attn_tile_acc(const float* tile, const dr_f32x4 (&w)[4], int i16, int g, dr_f32x4 (&out)[DHP / 16]) {
    constexpr int LS = DHP + 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* src = tile + (16 * t + 4 * g + r) * LS + i16;
#pragma unroll
            for (int dt = 0; dt < DHP / 16; ++dt) out[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(src[16 * dt], w[t][r], out[dt], 0, 0, 0);
        }
}

template <int DHP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnP p) {
    constexpr int LS = DHP + 4, NC = DHP / 16;
    __shared__ __attribute__((aligned(16))) float Ks[ATTN_TILE * LS];
    __shared__ __attribute__((aligned(16))) float Vs[ATTN_TILE * LS];
    __shared__ float mvs[ATTN_TILE];
    const int bh = blockIdx.x / p.tiles, tile = blockIdx.x - bh * p.tiles;
    const int b = bh / p.H, h = bh - b * p.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int qi = tile * ATTN_TILE + wave * 16 + i16;
    const bool qok = qi < p.Lq;
    const float* Kb = p.k + (int64_t)b * p.Lk * p.ld_k + h * p.dh;
    const float* Vb = p.v + (int64_t)b * p.Lk * p.ld_v + h * p.dh;
    float qreg[DHP / 4];
    attn_load_frag<DHP>(qreg, qok ? p.q + ((int64_t)b * p.Lq + qi) * p.ld_q + h * p.dh : nullptr, p.dh, g);
    dr_f32x4 oacc[NC];
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) oacc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const uint64_t row_base = ((uint64_t)bh * p.Lq + (uint64_t)qi) * (uint64_t)p.Lk;
    for (int kt = 0; kt < p.Lk; kt += ATTN_TILE) {
        __syncthreads();
        attn_load_tile<DHP>(Ks, Kb, p.ld_k, kt, p.Lk, p.dh, p.vec_k);
        attn_load_tile<DHP>(Vs, Vb, p.ld_v, kt, p.Lk, p.dh, p.vec_v);
        if (threadIdx.x < ATTN_TILE) {
            const int j = kt + threadIdx.x;
            mvs[threadIdx.x] = (p.mask && j < p.Lk && p.mask[(int64_t)b * p.Lk + j]) ? ATTN_MASK : 0.f;
        }
        __syncthreads();
        dr_f32x4 s[4];
        attn_tile_dot<DHP>(Ks, qreg, i16, g, s);
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * t + 4 * g + r, j = kt + jl;
                s[t][r] = attn_logit(s[t][r], p, mvs[jl], p.future && j > qi, j >= p.Lk);
                mx = fmaxf(mx, s[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        float ls = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = expf(s[t][r] - mn);
                ls += e;
                s[t][r] = attn_keep(p, row_base, kt + 16 * t + 4 * g + r) ? e : 0.f;
            }
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        l = l * alpha + ls;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < NC; ++dt) oacc[dt] *= alpha;
        attn_tile_acc<DHP>(Vs, s, i16, g, oacc);
    }
    if (qok) {
        attn_store_frag<DHP>(p.out + ((int64_t)b * p.Lq + qi) * p.ld_o + h * p.dh, oacc, p.inv_keep / l, 1.f, p.dh, g, p.vec_o);
        if (g == 0) {
            float* st = p.stats_out + 2 * ((int64_t)bh * p.Lq + qi);
            st[0] = m;
            st[1] = l;
        }
    }
}

// The query-owning sweep: the wave owns 16 queries and runs over all key tiles.  DELTA_ONLY: delta_i = sum_j P_ij dP_ij (dP with
// the dropout factor), written for the two sweeps that follow; otherwise dQ.  delta is summed from the recomputed P and dP themselves
// and not taken as rowsum(dO * O): sum_j dS_ij must vanish to the accuracy of THESE P and dP, or the part of K's and Q's inputs that
// every key shares -- which cancels in the weight gradients of the projections -- comes back multiplied by the error of delta
// (measured: 3-4 x the error on the decoder's key / query projections).  Two more products per backward.
template <int DHP, bool DELTA_ONLY>
__device__ __forceinline__ void attn_bwd_q_sweep(const AttnP& p) {
    constexpr int LS = DHP + 4, NC = DHP / 16;
    __shared__ __attribute__((aligned(16))) float Ks[ATTN_TILE * LS];
    __shared__ __attribute__((aligned(16))) float Vs[ATTN_TILE * LS];
    __shared__ float mvs[ATTN_TILE];
    const int bh = blockIdx.x / p.tiles, tile = blockIdx.x - bh * p.tiles;
    const int b = bh / p.H, h = bh - b * p.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int qi = tile * ATTN_TILE + wave * 16 + i16;
    const bool qok = qi < p.Lq;
    const float* Kb = p.k + (int64_t)b * p.Lk * p.ld_k + h * p.dh;
    const float* Vb = p.v + (int64_t)b * p.Lk * p.ld_v + h * p.dh;
    float qreg[DHP / 4], doreg[DHP / 4];
    attn_load_frag<DHP>(qreg, qok ? p.q + ((int64_t)b * p.Lq + qi) * p.ld_q + h * p.dh : nullptr, p.dh, g);
    attn_load_frag<DHP>(doreg, qok ? p.d_o + ((int64_t)b * p.Lq + qi) * p.ld_do + h * p.dh : nullptr, p.dh, g);
    float m = 0.f, linv = 0.f, delta = 0.f;
    if (qok) {
        const float* st = p.stats + 2 * ((int64_t)bh * p.Lq + qi);
        m = st[0];
        linv = 1.f / st[1];
        if (!DELTA_ONLY) delta = p.delta[(int64_t)bh * p.Lq + qi];
    }
    dr_f32x4 acc[NC];
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) acc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    const uint64_t row_base = ((uint64_t)bh * p.Lq + (uint64_t)qi) * (uint64_t)p.Lk;
    for (int kt = 0; kt < p.Lk; kt += ATTN_TILE) {
        __syncthreads();
        attn_load_tile<DHP>(Ks, Kb, p.ld_k, kt, p.Lk, p.dh, p.vec_k);
        attn_load_tile<DHP>(Vs, Vb, p.ld_v, kt, p.Lk, p.dh, p.vec_v);
        if (threadIdx.x < ATTN_TILE) {
            const int j = kt + threadIdx.x;
            mvs[threadIdx.x] = (p.mask && j < p.Lk && p.mask[(int64_t)b * p.Lk + j]) ? ATTN_MASK : 0.f;
        }
        __syncthreads();
        dr_f32x4 s[4], dp[4];
        attn_tile_dot<DHP>(Ks, qreg, i16, g, s);
        attn_tile_dot<DHP>(Vs, doreg, i16, g, dp);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * t + 4 * g + r, j = kt + jl;
                const bool hidden = p.future && j > qi;
                const float sv = attn_logit(s[t][r], p, mvs[jl], hidden, j >= p.Lk);
                const float pr = expf(sv - m) * linv;
                const float dpd = attn_keep(p, row_base, j) ? dp[t][r] * p.inv_keep : 0.f;
                if (DELTA_ONLY) delta = fmaf(pr, dpd, delta);
                else s[t][r] = hidden ? 0.f : pr * (dpd - delta);
            }
        if (!DELTA_ONLY) attn_tile_acc<DHP>(Ks, s, i16, g, acc);
    }
    if (DELTA_ONLY) {
        delta += __shfl_xor(delta, 16, 64);
        delta += __shfl_xor(delta, 32, 64);
        if (qok && g == 0) p.delta[(int64_t)bh * p.Lq + qi] = delta;
    } else if (qok) {
        attn_store_frag<DHP>(p.dq + ((int64_t)b * p.Lq + qi) * p.ld_dq + h * p.dh, acc, p.gmul, p.gdiv, p.dh, g, p.vec_dq);
    }
}
template <int DHP>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(const AttnP p) { attn_bwd_q_sweep<DHP, true>(p); }
template <int DHP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const AttnP p) { attn_bwd_q_sweep<DHP, false>(p); }

// dK / dV sweep: the wave owns 16 keys and runs over all query tiles
template <int DHP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const AttnP p) {
    constexpr int LS = DHP + 4, NC = DHP / 16;
    __shared__ __attribute__((aligned(16))) float Qs[ATTN_TILE * LS];
    __shared__ __attribute__((aligned(16))) float Gs[ATTN_TILE * LS];
    __shared__ float ms[ATTN_TILE], lis[ATTN_TILE], des[ATTN_TILE];
    const int bh = blockIdx.x / p.tiles, tile = blockIdx.x - bh * p.tiles;
    const int b = bh / p.H, h = bh - b * p.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int kj = tile * ATTN_TILE + wave * 16 + i16;
    const bool kok = kj < p.Lk;
    const float* Qb = p.q + (int64_t)b * p.Lq * p.ld_q + h * p.dh;
    const float* Gb = p.d_o + (int64_t)b * p.Lq * p.ld_do + h * p.dh;
    float kreg[DHP / 4], vreg[DHP / 4];
    attn_load_frag<DHP>(kreg, kok ? p.k + ((int64_t)b * p.Lk + kj) * p.ld_k + h * p.dh : nullptr, p.dh, g);
    attn_load_frag<DHP>(vreg, kok ? p.v + ((int64_t)b * p.Lk + kj) * p.ld_v + h * p.dh : nullptr, p.dh, g);
    const float mask_add = (p.mask && kok && p.mask[(int64_t)b * p.Lk + kj]) ? ATTN_MASK : 0.f;
    dr_f32x4 dkacc[NC], dvacc[NC];
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) dkacc[dt] = dvacc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = 0; qt < p.Lq; qt += ATTN_TILE) {
        __syncthreads();
        attn_load_tile<DHP>(Qs, Qb, p.ld_q, qt, p.Lq, p.dh, p.vec_q);
        attn_load_tile<DHP>(Gs, Gb, p.ld_do, qt, p.Lq, p.dh, p.vec_do);
        if (threadIdx.x < ATTN_TILE) {
            const int i = qt + threadIdx.x;
            float mm = 0.f, li = 0.f, de = 0.f;
            if (i < p.Lq) {
                const float* st = p.stats + 2 * ((int64_t)bh * p.Lq + i);
                mm = st[0];
                li = 1.f / st[1];
                de = p.delta[(int64_t)bh * p.Lq + i];
            }
            ms[threadIdx.x] = mm;
            lis[threadIdx.x] = li;
            des[threadIdx.x] = de;
        }
        __syncthreads();
        dr_f32x4 s[4], dp[4];
        attn_tile_dot<DHP>(Qs, kreg, i16, g, s);
        attn_tile_dot<DHP>(Gs, vreg, i16, g, dp);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * t + 4 * g + r, i = qt + il;
                const bool hidden = p.future && kj > i;
                const float sv = attn_logit(s[t][r], p, mask_add, hidden, !kok);
                const float pr = expf(sv - ms[il]) * lis[il];
                const float keep = attn_keep(p, ((uint64_t)bh * p.Lq + (uint64_t)i) * (uint64_t)p.Lk, kj) ? p.inv_keep : 0.f;
                s[t][r] = hidden ? 0.f : pr * (dp[t][r] * keep - des[il]);
                dp[t][r] = pr * keep;
            }
        attn_tile_acc<DHP>(Gs, dp, i16, g, dvacc);
        attn_tile_acc<DHP>(Qs, s, i16, g, dkacc);
    }
    if (kok) {
        attn_store_frag<DHP>(p.dk + ((int64_t)b * p.Lk + kj) * p.ld_dk + h * p.dh, dkacc, p.gmul, p.gdiv, p.dh, g, p.vec_dk);
        attn_store_frag<DHP>(p.dv + ((int64_t)b * p.Lk + kj) * p.ld_dv + h * p.dh, dvacc, 1.f, 1.f, p.dh, g, p.vec_dv);
    }
}

inline int attn_vec(const void* ptr, int64_t ld, int dh) {
    return (dh % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0) ? 1 : 0;
}

// shared argument checks; fills the scale / dropout constants
inline int attn_common(AttnP& p, int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t future, float rate, uint64_t seed) {
    if (B < 0 || H <= 0 || Lq <= 0 || Lk <= 0 || dh <= 0 || !(rate >= 0.f) || !(rate < 1.f)) return DR_EINVAL;
    if (dh > 128 || (future && Lq != Lk)) return DR_ESHAPE;
    if ((int64_t)B * H * ((std::max(Lq, Lk) + ATTN_TILE - 1) / ATTN_TILE) >= (int64_t)1 << 31) return DR_ESHAPE;
    p.B = B; p.H = H; p.Lq = Lq; p.Lk = Lk; p.dh = dh; p.future = future ? 1 : 0;
    p.thresh = rate > 0.f ? dr_drop_thresh(rate) : 0u;
    p.seed = seed;
    p.inv_keep = 1.f / (1.f - rate);
    p.sdiv = (float)sqrt((double)dh);
    int ex = 0;
    const bool pow2 = frexpf(p.sdiv, &ex) == 0.5f && p.sdiv * p.sdiv == (float)dh;
    p.smul = pow2 ? 1.f / p.sdiv : 0.f;           // an exact reciprocal: the division by sqrt(dh) as a multiplication
    p.gmul = pow2 ? p.smul : 1.f;
    p.gdiv = pow2 ? 1.f : p.sdiv;
    return DR_OK;
}

#define ATTN_DISPATCH(KERNEL, grid, stream, p)                                                                     \
    do {                                                                                                           \
        if (p.dh <= 16) hipLaunchKernelGGL(KERNEL<16>, dim3(grid), dim3(256), 0, dr_s(stream), p);                 \
        else if (p.dh <= 32) hipLaunchKernelGGL(KERNEL<32>, dim3(grid), dim3(256), 0, dr_s(stream), p);            \
        else if (p.dh <= 64) hipLaunchKernelGGL(KERNEL<64>, dim3(grid), dim3(256), 0, dr_s(stream), p);            \
        else hipLaunchKernelGGL(KERNEL<128>, dim3(grid), dim3(256), 0, dr_s(stream), p);                           \
    } while (0)

// ---- residual add + LayerNormalization --------------------------------------------------------------------------------------------
// a lane group of G lanes (a power of two <= 64, sized from D) per row; stats[row] = (mean, 1 / sqrt(var + eps))
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const float* __restrict__ a, int64_t ld_a, const float* __restrict__ b, int64_t ld_b,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int64_t M, int32_t D,
                                                         float eps, int32_t G, float* __restrict__ y, int64_t ld_y, float* __restrict__ stats) {
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < M;
    const float* ar = a + (ok ? row : 0) * ld_a;
    const float* br = b ? b + (ok ? row : 0) * ld_b : nullptr;
    float sum = 0.f;
    if (ok)
        for (int c = sub; c < D; c += G) sum += br ? ar[c] + br[c] : ar[c];
    for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const float mean = sum / (float)D;
    float sq = 0.f;
    if (ok)
        for (int c = sub; c < D; c += G) {
            const float d = (br ? ar[c] + br[c] : ar[c]) - mean;
            sq = fmaf(d, d, sq);
        }
    for (int off = G >> 1; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    const float rstd = 1.f / sqrtf(sq / (float)D + eps);
    if (!ok) return;
    for (int c = sub; c < D; c += G) {
        const float xh = ((br ? ar[c] + br[c] : ar[c]) - mean) * rstd;
        y[row * ld_y + c] = fmaf(gamma[c], xh, beta[c]);
    }
    if (sub == 0) {
        stats[2 * row] = mean;
        stats[2 * row + 1] = rstd;
    }
}

// d_s = rstd * (g gamma - mean_c(g gamma) - xhat * mean_c(g gamma xhat))
__global__ __launch_bounds__(256) void add_ln_bwd_dx_kernel(const float* __restrict__ a, int64_t ld_a, const float* __restrict__ b, int64_t ld_b,
                                                            const float* __restrict__ gamma, const float* __restrict__ stats,
                                                            const float* __restrict__ dy, int64_t ld_dy, int64_t M, int32_t D, int32_t G,
                                                            float* __restrict__ ds, int64_t ld_ds) {
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < M;
    const float* ar = a + (ok ? row : 0) * ld_a;
    const float* br = b ? b + (ok ? row : 0) * ld_b : nullptr;
    const float* gr = dy + (ok ? row : 0) * ld_dy;
    const float mean = ok ? stats[2 * row] : 0.f, rstd = ok ? stats[2 * row + 1] : 0.f;
    float c1 = 0.f, c2 = 0.f;
    if (ok)
        for (int c = sub; c < D; c += G) {
            const float xh = ((br ? ar[c] + br[c] : ar[c]) - mean) * rstd;
            const float gg = gr[c] * gamma[c];
            c1 += gg;
            c2 = fmaf(gg, xh, c2);
        }
    for (int off = G >> 1; off > 0; off >>= 1) {
        c1 += __shfl_xor(c1, off, 64);
        c2 += __shfl_xor(c2, off, 64);
    }
    if (!ok) return;
    c1 /= (float)D;
    c2 /= (float)D;
    for (int c = sub; c < D; c += G) {
        const float xh = ((br ? ar[c] + br[c] : ar[c]) - mean) * rstd;
        ds[row * ld_ds + c] = rstd * (gr[c] * gamma[c] - c1 - xh * c2);
    }
}

constexpr int LN_CHUNK = 128;   // rows per partial of the column reduction

// stage 1: partial[chunk][0][c] = sum over the chunk's rows (ascending) of g * xhat, partial[chunk][1][c] = sum of g
__global__ __launch_bounds__(256) void add_ln_bwd_partial_kernel(const float* __restrict__ a, int64_t ld_a, const float* __restrict__ b,
                                                                 int64_t ld_b, const float* __restrict__ stats, const float* __restrict__ dy,
                                                                 int64_t ld_dy, int64_t M, int32_t D, float* __restrict__ partial) {
    const int64_t r0 = (int64_t)blockIdx.x * LN_CHUNK;
    const int64_t r1 = r0 + LN_CHUNK < M ? r0 + LN_CHUNK : M;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < D; c += gridDim.y * 256) {
        float dg = 0.f, db = 0.f;
        for (int64_t r = r0; r < r1; ++r) {
            const float s = b ? a[r * ld_a + c] + b[r * ld_b + c] : a[r * ld_a + c];
            const float xh = (s - stats[2 * r]) * stats[2 * r + 1];
            const float gv = dy[r * ld_dy + c];
            dg = fmaf(gv, xh, dg);
            db += gv;
        }
        partial[((int64_t)blockIdx.x * 2) * D + c] = dg;
        partial[((int64_t)blockIdx.x * 2 + 1) * D + c] = db;
    }
}

inline int ln_group(int32_t D) {
    int G = 8;
    while (G < 64 && G * 4 < D) G <<= 1;
    return G;
}

// ---- token embedding ----------------------------------------------------------------------------------------------------------------
// out[n, c] = dropout(table[ids[n], c] * sqrt(D) + pos[n % L, c]); element index of the hash: n * D + c.  Two roundings (product,
// then sum) as the reference's two ops.  An id outside [0, V) reads as a zero row.
__global__ __launch_bounds__(256) void token_emb_fwd_kernel(const int64_t* __restrict__ ids, int64_t N, int32_t L, const float* __restrict__ table,
                                                            int64_t V, int32_t D, const float* __restrict__ pos, float scale, uint32_t thresh,
                                                            uint64_t seed, float inv_keep, float* __restrict__ out, int64_t ld_out) {
    const int64_t n_el = N * D, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_el; i += stride) {
        const int64_t n = i / D;
        const int c = (int)(i - n * D);
        const int64_t id = ids[n];
        float val = (id >= 0 && id < V) ? __fmul_rn(table[id * D + c], scale) : 0.f;
        if (pos) val = __fadd_rn(val, pos[(n % L) * D + c]);
        const bool keep = thresh == 0u || dr_mix32(seed, (uint64_t)i) >= thresh;
        out[n * ld_out + c] = keep ? val * inv_keep : 0.f;
    }
}

// One owner block per table row (dr_owner_rows.h): d_table[id] += sqrt(D) * the kept d_out rows of the id's positions / (1 - rate),
// summed in a fixed order, no atomics.
__global__ __launch_bounds__(256) void token_emb_bwd_kernel(const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ order, int64_t N,
                                                            int64_t V, int32_t D, int32_t CW, const float* __restrict__ d_out, int64_t ld_do,
                                                            float scale, uint32_t thresh, uint64_t seed, float inv_keep,
                                                            float* __restrict__ d_table) {
    dr_owner_row_scatter(sorted_ids, order, N, V, D, CW, scale, d_table, [&](int64_t n, int c, float& acc) {
        const bool keep = thresh == 0u || dr_mix32(seed, (uint64_t)(n * D + c)) >= thresh;
        if (keep) acc += d_out[n * ld_do + c] * inv_keep;
    });
}

}  // namespace

extern "C" int dr_attn_fwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v, const uint8_t* key_mask,
                           int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t future, float rate, uint64_t seed, float* out,
                           int64_t ld_o, float* stats, dr_stream_t stream) {
    AttnP p = {};
    const int st = attn_common(p, B, H, Lq, Lk, dh, future, rate, seed);
    if (st != DR_OK) return st;
    const int64_t w = (int64_t)H * dh;
    if (ld_q < w || ld_k < w || ld_v < w || ld_o < w) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!q || !k || !v || !out || !stats) return DR_EINVAL;
    p.q = q; p.k = k; p.v = v; p.mask = key_mask; p.out = out; p.stats_out = stats;
    p.ld_q = ld_q; p.ld_k = ld_k; p.ld_v = ld_v; p.ld_o = ld_o;
    p.vec_k = attn_vec(k, ld_k, dh); p.vec_v = attn_vec(v, ld_v, dh); p.vec_o = attn_vec(out, ld_o, dh);
    p.tiles = (Lq + ATTN_TILE - 1) / ATTN_TILE;
    const unsigned grid = (unsigned)((int64_t)B * H * p.tiles);
    ATTN_DISPATCH(attn_fwd_kernel, grid, stream, p);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_attn_bwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v, const uint8_t* key_mask,
                           const float* d_out, int64_t ld_do, const float* stats, int32_t B, int32_t H,
                           int32_t Lq, int32_t Lk, int32_t dh, int32_t future, float rate, uint64_t seed, float* dq, int64_t ld_dq,
                           float* dk, int64_t ld_dk, float* dv, int64_t ld_dv, float* delta, dr_stream_t stream) {
    AttnP p = {};
    const int st = attn_common(p, B, H, Lq, Lk, dh, future, rate, seed);
    if (st != DR_OK) return st;
    const int64_t w = (int64_t)H * dh;
    if (ld_q < w || ld_k < w || ld_v < w || ld_do < w || ld_dq < w || ld_dk < w || ld_dv < w) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!q || !k || !v || !d_out || !stats || !dq || !dk || !dv || !delta) return DR_EINVAL;
    p.q = q; p.k = k; p.v = v; p.mask = key_mask; p.d_o = d_out; p.stats = stats; p.delta = delta;
    p.dq = dq; p.dk = dk; p.dv = dv;
    p.ld_q = ld_q; p.ld_k = ld_k; p.ld_v = ld_v; p.ld_do = ld_do; p.ld_dq = ld_dq; p.ld_dk = ld_dk; p.ld_dv = ld_dv;
    p.vec_q = attn_vec(q, ld_q, dh); p.vec_k = attn_vec(k, ld_k, dh); p.vec_v = attn_vec(v, ld_v, dh);
    p.vec_do = attn_vec(d_out, ld_do, dh); p.vec_dq = attn_vec(dq, ld_dq, dh); p.vec_dk = attn_vec(dk, ld_dk, dh);
    p.vec_dv = attn_vec(dv, ld_dv, dh);
    p.tiles = (Lq + ATTN_TILE - 1) / ATTN_TILE;
    ATTN_DISPATCH(attn_bwd_delta_kernel, (unsigned)((int64_t)B * H * p.tiles), stream, p);
    p.tiles = (Lk + ATTN_TILE - 1) / ATTN_TILE;
    ATTN_DISPATCH(attn_bwd_dkv_kernel, (unsigned)((int64_t)B * H * p.tiles), stream, p);
    p.tiles = (Lq + ATTN_TILE - 1) / ATTN_TILE;
    ATTN_DISPATCH(attn_bwd_dq_kernel, (unsigned)((int64_t)B * H * p.tiles), stream, p);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_add_layernorm_fwd(const float* a, int64_t ld_a, const float* b, int64_t ld_b, const float* gamma, const float* beta,
                                    int64_t M, int32_t D, float eps, float* y, int64_t ld_y, float* stats, dr_stream_t stream) {
    if (M < 0 || D <= 0 || ld_a < D || (b && ld_b < D) || ld_y < D || !(eps >= 0.f)) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!a || !gamma || !beta || !y || !stats) return DR_EINVAL;
    const int G = ln_group(D), rows = 256 / G;
    if ((M + rows - 1) / rows >= (int64_t)1 << 31) return DR_ESHAPE;
    hipLaunchKernelGGL(add_ln_fwd_kernel, dim3((unsigned)((M + rows - 1) / rows)), dim3(256), 0, dr_s(stream), a, ld_a, b, ld_b, gamma, beta,
                       M, D, eps, G, y, ld_y, stats);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_add_layernorm_bwd_workspace_bytes(int64_t M, int32_t D) {
    if (M <= 0 || D <= 0) return 0;
    return ((M + LN_CHUNK - 1) / LN_CHUNK) * 2 * (int64_t)D * (int64_t)sizeof(float);
}

extern "C" int dr_add_layernorm_bwd(const float* a, int64_t ld_a, const float* b, int64_t ld_b, const float* gamma, const float* stats,
                                    const float* dy, int64_t ld_dy, int64_t M, int32_t D, float* d_s, int64_t ld_ds, float* d_gamma,
                                    float* d_beta, float* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    if (M < 0 || D <= 0 || ld_a < D || (b && ld_b < D) || ld_dy < D || ld_ds < D) return DR_EINVAL;
    if (!d_gamma || !d_beta) return DR_EINVAL;
    if (M == 0) {
        (void)hipMemsetAsync(d_gamma, 0, sizeof(float) * D, dr_s(stream));
        (void)hipMemsetAsync(d_beta, 0, sizeof(float) * D, dr_s(stream));
        return DR_OK;
    }
    if (!a || !gamma || !stats || !dy || !d_s || !workspace) return DR_EINVAL;
    if (workspace_bytes < dr_add_layernorm_bwd_workspace_bytes(M, D)) return DR_EINVAL;
    const int G = ln_group(D), rows = 256 / G;
    const int64_t chunks = (M + LN_CHUNK - 1) / LN_CHUNK;
    if ((M + rows - 1) / rows >= (int64_t)1 << 31) return DR_ESHAPE;
    hipLaunchKernelGGL(add_ln_bwd_dx_kernel, dim3((unsigned)((M + rows - 1) / rows)), dim3(256), 0, dr_s(stream), a, ld_a, b, ld_b, gamma,
                       stats, dy, ld_dy, M, D, G, d_s, ld_ds);
    const unsigned cy = (unsigned)std::min<int64_t>((D + 255) / 256, 64);
    hipLaunchKernelGGL(add_ln_bwd_partial_kernel, dim3((unsigned)chunks, cy), dim3(256), 0, dr_s(stream), a, ld_a, b, ld_b, stats, dy, ld_dy,
                       M, D, workspace);
    // stage 2: d_gamma | d_beta = the partials summed in chunk order
    return dr_sum_partials(workspace, chunks, d_gamma, D, d_beta, D, nullptr, 0, (unsigned)((D + 255) / 256), dr_s(stream));
}

extern "C" int dr_token_embedding_fwd(const int64_t* ids, int64_t N, int32_t L, const float* table, int64_t V, int32_t D, const float* pos,
                                      float rate, uint64_t seed, float* out, int64_t ld_out, dr_stream_t stream) {
    if (N < 0 || L <= 0 || V <= 0 || D <= 0 || ld_out < D || !(rate >= 0.f) || !(rate < 1.f)) return DR_EINVAL;
    if (N % L != 0) return DR_ESHAPE;
    if (N == 0) return DR_OK;
    if (!ids || !table || !out) return DR_EINVAL;
    hipLaunchKernelGGL(token_emb_fwd_kernel, dim3(dr_grid_for(N * D, 256)), dim3(256), 0, dr_s(stream), ids, N, L, table, V, D, pos,
                       (float)sqrt((double)D), rate > 0.f ? dr_drop_thresh(rate) : 0u, seed, 1.f / (1.f - rate), out, ld_out);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_token_embedding_bwd(const int64_t* sorted_ids, const int64_t* order, int64_t N, int64_t V, int32_t D, const float* d_out,
                                      int64_t ld_do, float rate, uint64_t seed, float* d_table, dr_stream_t stream) {
    if (N < 0 || V <= 0 || D <= 0 || ld_do < D || !(rate >= 0.f) || !(rate < 1.f)) return DR_EINVAL;
    if (N >= (int64_t)1 << 31) return DR_ESHAPE;
    if (N == 0) return DR_OK;
    if (!sorted_ids || !order || !d_out || !d_table) return DR_EINVAL;
    const int CW = dr_owner_row_cw(D);
    hipLaunchKernelGGL(token_emb_bwd_kernel, dim3((unsigned)N), dim3(256), 0, dr_s(stream), sorted_ids, order, N, V, D, CW, d_out, ld_do,
                       (float)sqrt((double)D), rate > 0.f ? dr_drop_thresh(rate) : 0u, seed, 1.f / (1.f - rate), d_table);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
