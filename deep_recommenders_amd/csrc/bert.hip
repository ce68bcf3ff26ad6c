// BERT (Devlin et al., NAACL 2019) on gfx950: the four kernel families its encoder and pre-training step need beyond the Transformer
// package (csrc/attention.hip) and the GEMM path; the arithmetic is spelled out in include/dr_hotpath.h, "BERT".
//   * dr_gelu_fwd / _bwd          the exact (erf) GELU of the feed-forward block and the MLM transform, its derivative through the saved
//     PRE-activation (GELU is not monotonic: the output does not determine it).  Streaming, 8 B / 12 B per element.
//   * dr_bert_embed_fwd / _bwd    dropout(LayerNorm(tok[ids] + pos[l] + seg[segment])) in one pass over the row -- a lane group per row,
//     the row summed in registers, (mean, rstd) saved -- and its backward: d_s per row, d_gamma / d_beta / d_seg by a fixed-order
//     column reduction over 128-row chunks, d_pos by one over 16-sequence chunks, d_tok by one owner block per table row
//     (dr_owner_rows.h, shared with dr_token_embedding_bwd).
//   * dr_softmax_ce_ids           softmax cross-entropy over integer labels, in place: one 1024-thread block owns a row, stages it once
//     in dynamic LDS (up to DR_SOFTMAX_CE_IDS_LDS_COLS columns, 128 KiB of the CU's 160) and writes the gradient over it -- the
//     [M, C] logits move once in and once out.  A wider row is re-read from memory by the same code, to the same bits.
//     dr_colsum_add is the bias gradient: a fixed-order two-stage column sum.
//   * dr_mlm_mask                 BERT's dynamic masking, one wave per sequence: candidates are compacted into LDS with their hashes and
//     the n smallest keys selected by the rank count of dr_rank_select.h (shared with dr_neighbor_sample).
// No float atomics; every reduction has a fixed order, so results are bit-identical from run to run, and a row's outputs do not
// depend on the batch around it (the column reductions, whose chunks are cut by the row index, excepted).
#include "dr_common.h"
#include "dr_owner_rows.h"
#include "dr_rank_select.h"
#include "dr_sum_partials.h"
#include <math.h>
#include <algorithm>

#ifndef DR_SOFTMAX_CE_IDS_LDS_COLS
#define DR_SOFTMAX_CE_IDS_LDS_COLS 32768    // columns of a row staged in LDS (mirrored as ops.SOFTMAX_CE_IDS_LDS_COLS)
#endif

namespace {

// ---- GELU ---------------------------------------------------------------------------------------------------------------------------
// Phi(z) = erfc(-z / sqrt 2) / 2: 0.5 (1 + erf(z / sqrt 2)) without the cancellation of 1 + erf at negative z
__device__ __forceinline__ float gelu_cdf(float z) { return 0.5f * erfcf(-0.70710678118654752440f * z); }
// Phi(z) + z phi(z), phi(z) = exp(-z^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float gelu_dgrad(float v) { return gelu_cdf(v) + v * (0.39894228040143267794f * expf(-0.5f * v * v)); }

__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ z, int64_t ld_z, int64_t M, int32_t N, float* __restrict__ h,
                                                       int64_t ld_h) {
    const int64_t n = M * N, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / N, c = i - r * N;
        const float v = z[r * ld_z + c];
        h[r * ld_h + c] = v * gelu_cdf(v);
    }
}

// dz = dy (Phi(z) + z phi(z)), phi(z) = exp(-z^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ z, int64_t ld_z, float* __restrict__ dy, int64_t ld_dy,
                                                       int64_t M, int32_t N) {
    const int64_t n = M * N, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / N, c = i - r * N;
        const float v = z[r * ld_z + c];
        dy[r * ld_dy + c] *= gelu_dgrad(v);
    }
}

// The same arithmetic on float4: rows whose width and pitches are multiples of 4 floats at 16-byte aligned bases (what the GEMM path
// hands over).  dense: both pitches equal the width, the matrix is one flat array and no index is divided.
template <bool BWD>
__global__ __launch_bounds__(256) void gelu_vec_kernel(const float4* __restrict__ z, int64_t ldz4, float4* __restrict__ y, int64_t ldy4,
                                                       int64_t M, int32_t N4, int32_t dense) {
    const int64_t n4 = M * N4, stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += stride) {
        int64_t iz = q, iy = q;
        if (!dense) {
            const int64_t r = q / N4, c = q - r * N4;
            iz = r * ldz4 + c;
            iy = r * ldy4 + c;
        }
        const float4 v = z[iz];
        float4 o;
        if (BWD) {
            const float4 d = y[iy];
            o = make_float4(d.x * gelu_dgrad(v.x), d.y * gelu_dgrad(v.y), d.z * gelu_dgrad(v.z), d.w * gelu_dgrad(v.w));
        } else {
            o = make_float4(v.x * gelu_cdf(v.x), v.y * gelu_cdf(v.y), v.z * gelu_cdf(v.z), v.w * gelu_cdf(v.w));
        }
        y[iy] = o;
    }
}

inline bool gelu_vec_ok(const void* a, int64_t ld_a, const void* b, int64_t ld_b, int32_t N) {
    return (N & 3) == 0 && (ld_a & 3) == 0 && (ld_b & 3) == 0 && dr_aligned16(a) && dr_aligned16(b);
}

// ---- embedding + LayerNorm + dropout ----------------------------------------------------------------------------------------------------
constexpr int BE_CHUNK = 128;      // rows per partial of the d_gamma / d_beta / d_seg column reduction
constexpr int BE_SEQS = 16;        // sequences per partial of the d_pos reduction

// lanes per row: a power of two, 8 .. 64, so that a lane holds at most 4 float4 of a row of D <= 1024
inline int be_group(int32_t D) {
    int G = 8;
    while (G < 64 && G * 4 < D) G <<= 1;
    return G;
}

struct BertEmbP {
    const int64_t *ids, *segment;
    const float *tok, *pos, *seg, *gamma, *beta, *stats, *d_out;
    float *out, *stats_out, *d_s;
    int64_t N, V, ld_out, ld_do;
    int32_t L, T, D, G;
    float eps, inv_keep;
    uint32_t thresh;
    uint64_t seed;
};

// the table rows of position n: a null pointer stands for the zero row of an id or segment out of range (never an address)
__device__ __forceinline__ void be_rows(const BertEmbP& p, int64_t n, const float*& tr, const float*& pr, const float*& sr) {
    const int64_t id = p.ids[n], sg = p.segment[n];
    tr = (id >= 0 && id < p.V) ? p.tok + id * p.D : nullptr;
    pr = p.pos + (n % p.L) * p.D;
    sr = (sg >= 0 && sg < p.T) ? p.seg + sg * p.D : nullptr;
}
__device__ __forceinline__ float be_s(const float* tr, const float* pr, const float* sr, int c) {
    return __fadd_rn(__fadd_rn(tr ? tr[c] : 0.f, pr[c]), sr ? sr[c] : 0.f);
}
__device__ __forceinline__ float4 be_s4(const float* tr, const float* pr, const float* sr, int q) {
    const float4 t = tr ? reinterpret_cast<const float4*>(tr)[q] : dr_zero4();
    const float4 o = reinterpret_cast<const float4*>(pr)[q];
    const float4 s = sr ? reinterpret_cast<const float4*>(sr)[q] : dr_zero4();
    return make_float4(__fadd_rn(__fadd_rn(t.x, o.x), s.x), __fadd_rn(__fadd_rn(t.y, o.y), s.y), __fadd_rn(__fadd_rn(t.z, o.z), s.z),
                       __fadd_rn(__fadd_rn(t.w, o.w), s.w));
}
__device__ __forceinline__ float be_group_sum(float v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ bool be_keep(const BertEmbP& p, int64_t idx) {
    return p.thresh == 0u || dr_mix32(p.seed, (uint64_t)idx) >= p.thresh;
}

// a lane group of G lanes per row, the row's float4 q = sub, sub + G, ... in registers
__global__ __launch_bounds__(256) void bert_embed_fwd_kernel(BertEmbP p) {
    const int G = p.G, D4 = p.D >> 2;
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < p.N;
    const float *tr = nullptr, *pr = nullptr, *sr = nullptr;
    if (ok) be_rows(p, row, tr, pr, sr);
    float4 s[4];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = sub + k * G;
        s[k] = (ok && q < D4) ? be_s4(tr, pr, sr, q) : dr_zero4();
        sum += (s[k].x + s[k].y) + (s[k].z + s[k].w);
    }
    const float mean = be_group_sum(sum, G) / (float)p.D;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (sub + k * G < D4) {
            const float dx = s[k].x - mean, dy = s[k].y - mean, dz = s[k].z - mean, dw = s[k].w - mean;
            sq = fmaf(dx, dx, sq); sq = fmaf(dy, dy, sq); sq = fmaf(dz, dz, sq); sq = fmaf(dw, dw, sq);
        }
    const float rstd = 1.f / sqrtf(be_group_sum(sq, G) / (float)p.D + p.eps);
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = sub + k * G;
        if (q < D4) {
            const float4 g = reinterpret_cast<const float4*>(p.gamma)[q], b = reinterpret_cast<const float4*>(p.beta)[q];
            const int64_t e = row * p.D + 4 * q;
            float4 y;
            y.x = fmaf(g.x, (s[k].x - mean) * rstd, b.x);
            y.y = fmaf(g.y, (s[k].y - mean) * rstd, b.y);
            y.z = fmaf(g.z, (s[k].z - mean) * rstd, b.z);
            y.w = fmaf(g.w, (s[k].w - mean) * rstd, b.w);
            y.x = be_keep(p, e) ? y.x * p.inv_keep : 0.f;
            y.y = be_keep(p, e + 1) ? y.y * p.inv_keep : 0.f;
            y.z = be_keep(p, e + 2) ? y.z * p.inv_keep : 0.f;
            y.w = be_keep(p, e + 3) ? y.w * p.inv_keep : 0.f;
            reinterpret_cast<float4*>(p.out + row * p.ld_out)[q] = y;
        }
    }
    if (sub == 0) {
        p.stats_out[2 * row] = mean;
        p.stats_out[2 * row + 1] = rstd;
    }
}

// the gradient that reaches the LayerNorm's output at element (n, c): d_out through the regenerated dropout mask
__device__ __forceinline__ float be_g(const BertEmbP& p, int64_t n, int c) {
    return be_keep(p, n * p.D + c) ? p.d_out[n * p.ld_do + c] * p.inv_keep : 0.f;
}

// d_s = rstd * (g gamma - mean_c(g gamma) - xhat * mean_c(g gamma xhat)), s recomputed from the tables
__global__ __launch_bounds__(256) void bert_embed_bwd_dx_kernel(BertEmbP p) {
    const int G = p.G, D4 = p.D >> 2;
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < p.N;
    const float *tr = nullptr, *pr = nullptr, *sr = nullptr;
    if (ok) be_rows(p, row, tr, pr, sr);
    const float mean = ok ? p.stats[2 * row] : 0.f, rstd = ok ? p.stats[2 * row + 1] : 0.f;
    float xh[4][4], gg[4][4];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = sub + k * G;
        const bool in = ok && q < D4;
        const float4 s = in ? be_s4(tr, pr, sr, q) : dr_zero4();
        const float4 gm = in ? reinterpret_cast<const float4*>(p.gamma)[q] : dr_zero4();
        const float sv[4] = {s.x, s.y, s.z, s.w}, gv[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[k][e] = in ? (sv[e] - mean) * rstd : 0.f;
            gg[k][e] = in ? be_g(p, row, 4 * q + e) * gv[e] : 0.f;
            c1 += gg[k][e];
            c2 = fmaf(gg[k][e], xh[k][e], c2);
        }
    }
    c1 = be_group_sum(c1, G) / (float)p.D;
    c2 = be_group_sum(c2, G) / (float)p.D;
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = sub + k * G;
        if (q < D4) {
            float4 d;
            d.x = rstd * (gg[k][0] - c1 - xh[k][0] * c2);
            d.y = rstd * (gg[k][1] - c1 - xh[k][1] * c2);
            d.z = rstd * (gg[k][2] - c1 - xh[k][2] * c2);
            d.w = rstd * (gg[k][3] - c1 - xh[k][3] * c2);
            reinterpret_cast<float4*>(p.d_s + row * p.D)[q] = d;
        }
    }
}

// stage 1 of the column reductions over rows: partial[chunk] = [ sum g xhat (D) | sum g (D) | per segment t: sum of the d_s rows
// with segment == t (T * D) ], the chunk's rows in ascending order
__global__ __launch_bounds__(256) void bert_embed_bwd_partial_kernel(BertEmbP p, float* __restrict__ partial) {
    const int64_t r0 = (int64_t)blockIdx.x * BE_CHUNK;
    const int64_t r1 = r0 + BE_CHUNK < p.N ? r0 + BE_CHUNK : p.N;
    float* part = partial + (int64_t)blockIdx.x * (2 + p.T) * p.D;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < p.D; c += gridDim.y * 256) {
        float dg = 0.f, db = 0.f;
        for (int64_t r = r0; r < r1; ++r) {
            const float *tr, *pr, *sr;
            be_rows(p, r, tr, pr, sr);
            const float xh = (be_s(tr, pr, sr, c) - p.stats[2 * r]) * p.stats[2 * r + 1];
            const float gv = be_g(p, r, c);
            dg = fmaf(gv, xh, dg);
            db += gv;
        }
        part[c] = dg;
        part[p.D + c] = db;
        for (int t = 0; t < p.T; ++t) {
            float acc = 0.f;
            for (int64_t r = r0; r < r1; ++r)
                if (p.segment[r] == t) acc += p.d_s[r * p.D + c];
            part[(int64_t)(2 + t) * p.D + c] = acc;
        }
    }
}

// stage 1 of d_pos: partial[chunk][l, c] = sum over the chunk's sequences b (ascending) of d_s[b L + l, c]
__global__ __launch_bounds__(256) void bert_embed_bwd_pos_kernel(const float* __restrict__ d_s, int64_t B, int32_t L, int32_t D,
                                                                 float* __restrict__ partial) {
    const int64_t LD = (int64_t)L * D;
    const int64_t b0 = (int64_t)blockIdx.y * BE_SEQS;
    const int64_t b1 = b0 + BE_SEQS < B ? b0 + BE_SEQS : B;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < LD; e += (int64_t)gridDim.x * 256) {
        float acc = 0.f;
        for (int64_t b = b0; b < b1; ++b) acc += d_s[b * LD + e];
        partial[(int64_t)blockIdx.y * LD + e] = acc;
    }
}

__global__ __launch_bounds__(256) void bert_embed_bwd_tok_kernel(const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ order,
                                                                 int64_t N, int64_t V, int32_t D, int32_t CW, const float* __restrict__ d_s,
                                                                 float* __restrict__ d_tok) {
    dr_owner_row_scatter(sorted_ids, order, N, V, D, CW, 1.f, d_tok, [&](int64_t n, int c, float& acc) { acc += d_s[n * D + c]; });
}

inline int bert_embed_check(int64_t N, int32_t L, int64_t V, int32_t T, int32_t D, float rate) {
    if (N < 0 || L <= 0 || V <= 0 || T <= 0 || D <= 0 || !(rate >= 0.f) || !(rate < 1.f)) return DR_EINVAL;
    if (D % 4 != 0 || D > 1024 || N % L != 0 || N >= (int64_t)1 << 31) return DR_ESHAPE;
    return DR_OK;
}

// ---- softmax cross-entropy over integer labels -----------------------------------------------------------------------------------------
constexpr int CE_THREADS = 1024, CE_WAVES = CE_THREADS / 64;
constexpr int CE_LDS_COLS = DR_SOFTMAX_CE_IDS_LDS_COLS;
static_assert(CE_LDS_COLS % 4 == 0 && CE_LDS_COLS * 4 + 1024 <= 160 * 1024, "the staged row and the reduction slots must fit the CU's LDS");

// fixed order: the wave's butterfly, then the waves' results in wave order
__device__ __forceinline__ float ce_block_max(float v, float* red) {
    v = dr_wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < CE_WAVES; ++i) r = fmaxf(r, red[i]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float ce_block_sum(float v, float* red) {
    v = dr_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < CE_WAVES; ++i) r += red[i];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float4 ce_add_bias(float4 v, const float* __restrict__ bias, int q) {
    if (bias) {
        v.x += bias[4 * q]; v.y += bias[4 * q + 1]; v.z += bias[4 * q + 2]; v.w += bias[4 * q + 3];
    }
    return v;
}

// One block per row.  STAGE: z = logits + bias goes to LDS in pass 1, exp(z - max) over it in pass 2, and pass 3 reads that; otherwise
// every pass reads the row from memory and recomputes the same values.  vec: the row is read as float4 up to C & ~3.
template <bool STAGE>
__global__ __launch_bounds__(CE_THREADS) void softmax_ce_ids_kernel(float* __restrict__ logits, int64_t ld, const float* __restrict__ bias,
                                                                    const int64_t* __restrict__ labels, const float* __restrict__ weight,
                                                                    int64_t M, int32_t C, int32_t vec, float smoothing, float row_scale,
                                                                    const float* __restrict__ denom, float denom_eps,
                                                                    float* __restrict__ row_loss) {
    extern __shared__ float ce_row[];
    __shared__ float red[CE_WAVES];
    const int tid = threadIdx.x;
    const int nv = vec ? C >> 2 : 0;
    float4* row4 = reinterpret_cast<float4*>(ce_row);
    const float eps_c = smoothing / (float)C;
    for (int64_t row = blockIdx.x; row < M; row += gridDim.x) {
        float* x = logits + row * ld;
        float4* x4 = reinterpret_cast<float4*>(x);
        const int64_t label = labels[row];
        if (label < 0) {                                       // padding: the row is written, never read
            for (int q = tid; q < nv; q += CE_THREADS) x4[q] = dr_zero4();
            for (int j = (nv << 2) + tid; j < C; j += CE_THREADS) x[j] = 0.f;
            if (tid == 0) row_loss[row] = 0.f;
            continue;
        }
        // pass 1: z and its maximum
        float m = -INFINITY;
        for (int q = tid; q < nv; q += CE_THREADS) {
            const float4 z = ce_add_bias(x4[q], bias, q);
            if (STAGE) row4[q] = z;
            m = fmaxf(m, fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w)));
        }
        for (int j = (nv << 2) + tid; j < C; j += CE_THREADS) {
            const float z = bias ? x[j] + bias[j] : x[j];
            if (STAGE) ce_row[j] = z;
            m = fmaxf(m, z);
        }
        m = ce_block_max(m, red);
        float zl = 0.f;                                        // label >= C breaks the contract; no address is formed from it
        if (label < C) zl = STAGE ? ce_row[label] : (bias ? x[label] + bias[label] : x[label]);
        __syncthreads();                                       // pass 2 writes over the staged z
        // pass 2: sum of exp(z - max) and of z
        float se = 0.f, sz = 0.f;
        for (int q = tid; q < nv; q += CE_THREADS) {
            const float4 z = STAGE ? row4[q] : ce_add_bias(x4[q], bias, q);
            const float4 e = make_float4(expf(z.x - m), expf(z.y - m), expf(z.z - m), expf(z.w - m));
            if (STAGE) row4[q] = e;
            se += (e.x + e.y) + (e.z + e.w);
            sz += (z.x + z.y) + (z.z + z.w);
        }
        for (int j = (nv << 2) + tid; j < C; j += CE_THREADS) {
            const float z = STAGE ? ce_row[j] : (bias ? x[j] + bias[j] : x[j]);
            const float e = expf(z - m);
            if (STAGE) ce_row[j] = e;
            se += e;
            sz += z;
        }
        se = ce_block_sum(se, red);
        sz = ce_block_sum(sz, red);
        const float lse = m + logf(se), inv = 1.f / se;
        const float w = weight ? weight[row] : 1.f;
        if (tid == 0) row_loss[row] = w * ((1.f - smoothing) * (lse - zl) + smoothing * (lse - sz / (float)C));
        const float coef = row_scale * w / (denom ? denom[0] + denom_eps : 1.f);
        const float hit = 1.f - smoothing;
        // pass 3: the gradient over the logits
        for (int q = tid; q < nv; q += CE_THREADS) {
            float4 e;
            if (STAGE) e = row4[q];
            else {
                const float4 z = ce_add_bias(x4[q], bias, q);
                e = make_float4(expf(z.x - m), expf(z.y - m), expf(z.z - m), expf(z.w - m));
            }
            const int j = 4 * q;
            float4 g;
            g.x = coef * (e.x * inv - eps_c - (j == label ? hit : 0.f));
            g.y = coef * (e.y * inv - eps_c - (j + 1 == label ? hit : 0.f));
            g.z = coef * (e.z * inv - eps_c - (j + 2 == label ? hit : 0.f));
            g.w = coef * (e.w * inv - eps_c - (j + 3 == label ? hit : 0.f));
            x4[q] = g;
        }
        for (int j = (nv << 2) + tid; j < C; j += CE_THREADS) {
            const float e = STAGE ? ce_row[j] : expf((bias ? x[j] + bias[j] : x[j]) - m);
            x[j] = coef * (e * inv - eps_c - (j == label ? hit : 0.f));
        }
        __syncthreads();                                       // the next row's pass 1 writes over ce_row
    }
}

constexpr int CS_CHUNK = 32;       // rows per partial of dr_colsum_add

__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ g, int64_t ld, int64_t M, int32_t C,
                                                             float* __restrict__ partial) {
    const int64_t r0 = (int64_t)blockIdx.y * CS_CHUNK;
    const int64_t r1 = r0 + CS_CHUNK < M ? r0 + CS_CHUNK : M;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < C; j += gridDim.x * 256) {
        float acc = 0.f;
        for (int64_t r = r0; r < r1; ++r) acc += g[r * ld + j];
        partial[(int64_t)blockIdx.y * C + j] = acc;
    }
}
__global__ __launch_bounds__(256) void colsum_apply_kernel(const float* __restrict__ partial, int64_t parts, int32_t C, float* __restrict__ dst) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < C; j += gridDim.x * 256) {
        float acc = 0.f;
        for (int64_t k = 0; k < parts; ++k) acc += partial[k * C + j];
        dst[j] += acc;
    }
}

// ---- masked-LM masking -----------------------------------------------------------------------------------------------------------------
constexpr int MLM_MAX_L = 512, MLM_MAX_P = 128;

// One wave per sequence, four per block and pass.  Candidates go to LDS in ascending l (hash and position), every lane ranks its own
// candidates against all of them, and the takers write themselves out in ascending l.  Every element of out_ids has one writer.
__global__ __launch_bounds__(256) void mlm_mask_kernel(const int64_t* __restrict__ ids, int64_t B, int32_t L, int64_t V, int64_t num_special,
                                                       int64_t mask_id, uint32_t prob_q16, int32_t P, uint64_t seed,
                                                       int64_t* __restrict__ out_ids, int32_t* __restrict__ positions,
                                                       int64_t* __restrict__ labels) {
    __shared__ uint32_t hs[4][MLM_MAX_L];
    __shared__ int32_t ps[4][MLM_MAX_L];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t* h = hs[w];
    int32_t* pl = ps[w];
    const uint64_t lt_mask = dr_lanes_below(lane);
    for (int64_t base = (int64_t)blockIdx.x * 4; base < B; base += (int64_t)gridDim.x * 4) {
        const int64_t b = base + w;
        const bool ok = b < B;
        int n_cand = 0;
        if (ok)
            for (int l0 = 0; l0 < L; l0 += 64) {
                const int l = l0 + lane;
                const int64_t id = l < L ? ids[b * L + l] : 0;
                const bool cand = l < L && id >= num_special;
                const uint64_t bal = __ballot(cand);
                if (cand) {
                    const int ci = n_cand + __popcll(bal & lt_mask);
                    h[ci] = dr_mix32(seed, (uint64_t)(b * L + l));
                    pl[ci] = l;
                } else if (l < L) {
                    out_ids[b * L + l] = id;
                }
                n_cand += __popcll(bal);
            }
        __syncthreads();
        if (ok) {
            int n = 0;
            if (n_cand > 0) {
                n = (int)(((uint32_t)n_cand * prob_q16 + 32768u) >> 16);
                n = n < 1 ? 1 : n;
                n = n > P ? P : n;
            }
            int written = 0;
            for (int j0 = 0; j0 < n_cand; j0 += 64) {
                const int j = j0 + lane;
                bool take = false;
                int l = 0;
                int64_t id = 0;
                if (j < n_cand) {
                    l = pl[j];
                    id = ids[b * L + l];
                    take = dr_key_rank(h, n_cand, h[j], j) < n;
                }
                const uint64_t bal = __ballot(take);
                if (j < n_cand) {
                    const uint64_t e = (uint64_t)(b * L + l);
                    int64_t put = id;
                    if (take) {
                        const int slot = written + __popcll(bal & lt_mask);       // exactly n keys rank below n
                        positions[b * P + slot] = l;
                        labels[b * P + slot] = id;
                        const uint32_t r = dr_mix32(seed + 1, e) % 10u;
                        if (r < 8u) put = mask_id;
                        else if (r == 8u) put = num_special + (int64_t)((uint64_t)dr_mix32(seed + 2, e) % (uint64_t)(V - num_special));
                    }
                    out_ids[b * L + l] = put;
                }
                written += __popcll(bal);
            }
            for (int j = n + lane; j < P; j += 64) {
                positions[b * P + j] = -1;
                labels[b * P + j] = -1;
            }
        }
        __syncthreads();                                       // h / pl are rewritten by the next pass
    }
}

}  // namespace

extern "C" int dr_gelu_fwd(const float* z, int64_t ld_z, int64_t M, int32_t N, float* h, int64_t ld_h, dr_stream_t stream) {
    if (M < 0 || N <= 0 || ld_z < N || ld_h < N) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!z || !h) return DR_EINVAL;
    if (gelu_vec_ok(z, ld_z, h, ld_h, N))
        hipLaunchKernelGGL(gelu_vec_kernel<false>, dim3(dr_grid_for(M * (N / 4), 256, 4096)), dim3(256), 0, dr_s(stream),
                           reinterpret_cast<const float4*>(z), ld_z / 4, reinterpret_cast<float4*>(h), ld_h / 4, M, N / 4,
                           (ld_z == N && ld_h == N) ? 1 : 0);
    else
        hipLaunchKernelGGL(gelu_fwd_kernel, dim3(dr_grid_for(M * N, 256)), dim3(256), 0, dr_s(stream), z, ld_z, M, N, h, ld_h);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_gelu_bwd(const float* z, int64_t ld_z, float* dy, int64_t ld_dy, int64_t M, int32_t N, dr_stream_t stream) {
    if (M < 0 || N <= 0 || ld_z < N || ld_dy < N) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!z || !dy) return DR_EINVAL;
    if (gelu_vec_ok(z, ld_z, dy, ld_dy, N))
        hipLaunchKernelGGL(gelu_vec_kernel<true>, dim3(dr_grid_for(M * (N / 4), 256, 4096)), dim3(256), 0, dr_s(stream),
                           reinterpret_cast<const float4*>(z), ld_z / 4, reinterpret_cast<float4*>(dy), ld_dy / 4, M, N / 4,
                           (ld_z == N && ld_dy == N) ? 1 : 0);
    else
        hipLaunchKernelGGL(gelu_bwd_kernel, dim3(dr_grid_for(M * N, 256)), dim3(256), 0, dr_s(stream), z, ld_z, dy, ld_dy, M, N);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_bert_embed_fwd(const int64_t* ids, const int64_t* segment, int64_t N, int32_t L, const float* tok, int64_t V,
                                 const float* pos, int32_t max_position, const float* seg, int32_t T, const float* gamma, const float* beta,
                                 int32_t D, float eps, float rate, uint64_t seed, float* out, int64_t ld_out, float* stats,
                                 dr_stream_t stream) {
    const int st = bert_embed_check(N, L, V, T, D, rate);
    if (st != DR_OK) return st;
    if (L > max_position) return DR_ESHAPE;
    if (!(eps >= 0.f) || dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (N == 0) return DR_OK;
    if (!ids || !segment || !tok || !pos || !seg || !gamma || !beta || !out || !stats) return DR_EINVAL;
    if (!dr_aligned16(tok) || !dr_aligned16(pos) || !dr_aligned16(seg) || !dr_aligned16(gamma) || !dr_aligned16(beta) || !dr_aligned16(out))
        return DR_EINVAL;
    BertEmbP p = {};
    p.ids = ids; p.segment = segment; p.tok = tok; p.pos = pos; p.seg = seg; p.gamma = gamma; p.beta = beta;
    p.out = out; p.stats_out = stats; p.N = N; p.V = V; p.ld_out = ld_out; p.L = L; p.T = T; p.D = D; p.G = be_group(D);
    p.eps = eps; p.inv_keep = 1.f / (1.f - rate); p.thresh = rate > 0.f ? dr_drop_thresh(rate) : 0u; p.seed = seed;
    const int rows = 256 / p.G;
    hipLaunchKernelGGL(bert_embed_fwd_kernel, dim3((unsigned)((N + rows - 1) / rows)), dim3(256), 0, dr_s(stream), p);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_bert_embed_bwd_workspace_bytes(int64_t N, int32_t L, int32_t D, int32_t T) {
    if (N <= 0 || L <= 0 || D <= 0 || T <= 0 || N % L != 0) return 0;
    const int64_t chunks = (N + BE_CHUNK - 1) / BE_CHUNK, seq_chunks = (N / L + BE_SEQS - 1) / BE_SEQS;
    return (chunks * (2 + (int64_t)T) * D + seq_chunks * L * D) * (int64_t)sizeof(float);
}

extern "C" int dr_bert_embed_bwd(const int64_t* ids, const int64_t* segment, const int64_t* sorted_ids, const int64_t* order, int64_t N,
                                 int32_t L, const float* tok, int64_t V, const float* pos, const float* seg, int32_t T, const float* gamma,
                                 const float* stats, int32_t D, const float* d_out, int64_t ld_do, float rate, uint64_t seed, float* d_s,
                                 float* d_gamma, float* d_beta, float* d_tok, float* d_pos, float* d_seg, float* workspace,
                                 int64_t workspace_bytes, dr_stream_t stream) {
    const int st = bert_embed_check(N, L, V, T, D, rate);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_do, D)) return DR_EINVAL;
    if (N == 0) return DR_OK;
    if (!ids || !segment || !sorted_ids || !order || !tok || !pos || !seg || !gamma || !stats || !d_out || !d_s || !d_gamma || !d_beta ||
        !d_tok || !d_pos || !d_seg || !workspace)
        return DR_EINVAL;
    if (!dr_aligned16(tok) || !dr_aligned16(pos) || !dr_aligned16(seg) || !dr_aligned16(gamma) || !dr_aligned16(d_s)) return DR_EINVAL;
    if (workspace_bytes < dr_bert_embed_bwd_workspace_bytes(N, L, D, T)) return DR_EINVAL;
    const int64_t B = N / L, chunks = (N + BE_CHUNK - 1) / BE_CHUNK, seq_chunks = (B + BE_SEQS - 1) / BE_SEQS;
    if (seq_chunks > 65535) return DR_ESHAPE;
    hipStream_t s = dr_s(stream);
    BertEmbP p = {};
    p.ids = ids; p.segment = segment; p.tok = tok; p.pos = pos; p.seg = seg; p.gamma = gamma; p.stats = stats; p.d_out = d_out;
    p.d_s = d_s; p.N = N; p.V = V; p.ld_do = ld_do; p.L = L; p.T = T; p.D = D; p.G = be_group(D);
    p.inv_keep = 1.f / (1.f - rate); p.thresh = rate > 0.f ? dr_drop_thresh(rate) : 0u; p.seed = seed;
    const int rows = 256 / p.G;
    hipLaunchKernelGGL(bert_embed_bwd_dx_kernel, dim3((unsigned)((N + rows - 1) / rows)), dim3(256), 0, s, p);
    float* part_rows = workspace;
    float* part_pos = workspace + chunks * (2 + (int64_t)T) * D;
    hipLaunchKernelGGL(bert_embed_bwd_partial_kernel, dim3((unsigned)chunks, (unsigned)((D + 255) / 256)), dim3(256), 0, s, p, part_rows);
    const int64_t LD = (int64_t)L * D;
    hipLaunchKernelGGL(bert_embed_bwd_pos_kernel, dim3((unsigned)dr_grid_for(LD, 256), (unsigned)seq_chunks), dim3(256), 0, s, d_s, B, L, D,
                       part_pos);
    hipLaunchKernelGGL(bert_embed_bwd_tok_kernel, dim3((unsigned)N), dim3(256), 0, s, sorted_ids, order, N, V, D, dr_owner_row_cw(D), d_s,
                       d_tok);
    DR_CHECK_LAUNCH();
    // stage 2: the partials summed in chunk order
    int rc = dr_sum_partials(part_rows, chunks, d_gamma, D, d_beta, D, d_seg, (int64_t)T * D, (unsigned)dr_grid_for((2 + (int64_t)T) * D, 256), s);
    if (rc != DR_OK) return rc;
    return dr_sum_partials(part_pos, seq_chunks, d_pos, LD, nullptr, 0, nullptr, 0, (unsigned)dr_grid_for(LD, 256), s);
}

extern "C" int dr_softmax_ce_ids(float* logits, int64_t ld, const float* bias, const int64_t* labels, const float* weight, int64_t M,
                                 int32_t C, float smoothing, float row_scale, const float* denom, float denom_eps, float* row_loss,
                                 int32_t path, dr_stream_t stream) {
    if (M < 0 || C <= 0 || ld < C || !(smoothing >= 0.f) || !(smoothing < 1.f) || path < 0 || path > 2) return DR_EINVAL;
    if (path == 1 && C > CE_LDS_COLS) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    if (!logits || !labels || !row_loss) return DR_EINVAL;
    const bool stage = path == 1 || (path == 0 && C <= CE_LDS_COLS);
    const int32_t vec = (dr_aligned16(logits) && (ld & 3) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)std::min<int64_t>(M, 1024);
    if (stage)
        return dr_launch(softmax_ce_ids_kernel<true>, dim3(grid), dim3(CE_THREADS), (size_t)((C + 3) / 4 * 4) * sizeof(float), dr_s(stream),
                         logits, ld, bias, labels, weight, M, C, vec, smoothing, row_scale, denom, denom_eps, row_loss);
    return dr_launch(softmax_ce_ids_kernel<false>, dim3(grid), dim3(CE_THREADS), 0, dr_s(stream), logits, ld, bias, labels, weight, M, C, vec,
                     smoothing, row_scale, denom, denom_eps, row_loss);
}

extern "C" int32_t dr_softmax_ce_ids_lds_cols(void) { return CE_LDS_COLS; }

extern "C" int64_t dr_colsum_add_workspace_bytes(int64_t M, int32_t C) {
    if (M <= 0 || C <= 0) return 0;
    return ((M + CS_CHUNK - 1) / CS_CHUNK) * (int64_t)C * (int64_t)sizeof(float);
}

extern "C" int dr_colsum_add(const float* g, int64_t ld, int64_t M, int32_t C, float* dst, float* workspace, int64_t workspace_bytes,
                             dr_stream_t stream) {
    if (M < 0 || C <= 0 || ld < C) return DR_EINVAL;
    if (M == 0) return DR_OK;
    const int64_t chunks = (M + CS_CHUNK - 1) / CS_CHUNK;
    if (chunks > 65535) return DR_ESHAPE;
    if (!g || !dst || !workspace || workspace_bytes < dr_colsum_add_workspace_bytes(M, C)) return DR_EINVAL;
    const unsigned gx = (unsigned)dr_grid_for(C, 256);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(gx, (unsigned)chunks), dim3(256), 0, dr_s(stream), g, ld, M, C, workspace);
    hipLaunchKernelGGL(colsum_apply_kernel, dim3(gx), dim3(256), 0, dr_s(stream), workspace, chunks, C, dst);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_mlm_mask(const int64_t* ids, int64_t B, int32_t L, int64_t V, int64_t num_special, int64_t mask_id, uint32_t prob_q16,
                           int32_t P, uint64_t seed, int64_t* out_ids, int32_t* positions, int64_t* labels, dr_stream_t stream) {
    if (B < 0 || L < 1 || P < 1 || P > MLM_MAX_P || num_special < 0 || V <= num_special || prob_q16 > 65536u) return DR_EINVAL;
    if (L > MLM_MAX_L || B * (int64_t)std::max(L, P) >= (int64_t)1 << 40) return DR_ESHAPE;
    if (B == 0) return DR_OK;
    if (!ids || !out_ids || !positions || !labels) return DR_EINVAL;
    hipLaunchKernelGGL(mlm_mask_kernel, dim3(dr_grid_for(B, 4)), dim3(256), 0, dr_s(stream), ids, B, L, V, num_special, mask_id, prob_q16, P,
                       seed, out_ids, positions, labels);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
