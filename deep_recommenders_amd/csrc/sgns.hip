// Skip-gram with negative sampling (Mikolov et al., NIPS 2013): the training step of Word2Vec, Item2Vec and DeepWalk, forward and gradient
// rows, straight from the two tables.
//
//   example b:  c = centers[b],  o_0 = contexts[b],  o_1 .. o_K = negatives[b, :],  u = in_table[c],  v_j = out_table[o_j],  z_j = (j == 0)
//   s_j    = <u, v_j>
//   loss_b = w_b * sum_j softplus((1 - 2 z_j) s_j)          softplus(x) = max(x, 0) + log1p(exp(-|x|))      (dr_bce_terms, mode 0)
//   g_j    = w_b * (sigmoid(s_j) - z_j)
//   c_j    = row_scale * g_j (one pass) | d_loss[b] * g_j (backward);   d_ctx[b, j, :] = c_j u;   d_center[b, :] = sum_j c_j v_j, j ascending
//
// 2 + K random rows in, 1 + K dot products: there is nothing to reuse and nothing to stage, the kernels are gather bandwidth.  A GROUP OF
// G LANES OWNS ONE EXAMPLE, G = D / 4 rounded up to a power of two (1 .. 64), lane l holds the float4 at column 4 l of every row: u stays in
// registers, SGNS_U rows v_j are loaded before the first is consumed, the dot meets in an xor butterfly inside the group.  No sum crosses
// groups: no atomic, no LDS, no barrier, no workspace; an example's bits depend neither on the batch around it nor on its place in it.
// A SKIPPED SLOT (the example's c or o_0 < 0; o_j < 0; o_j == o_0 under DR_SGNS_SKIP_EQUAL) loads nothing -- whatever its id would address
// is never formed into a pointer that is dereferenced -- and has s_j = g_j = 0, a d_ctx row of +0.0 and no term in loss_b or d_center.
// The one-pass forward and the backward share sgns_grad_slot(): given d_loss[b] == row_scale they write the same bits.
#include "sgns_common.h"

namespace {

constexpr int SGNS_MAX_K = 63;        // ids [B, 1 + K] go through the sorted K4, which takes F <= 64

struct SgnsP {
    const float* in_table; const float* out_table;
    const int64_t* centers; const int64_t* contexts; const int64_t* negatives;
    const float* sample_weight;                  // forward, may be NULL
    const float* coeff_in; const float* d_loss;  // backward
    float* loss_rows; float* coeff; float* scores;          // forward; scores may be NULL
    float* d_center; int64_t ld_dc;              // [B, D]; forward: may be NULL together with d_ctx
    float* d_ctx; int64_t ld_dx;                 // [B, (1 + K) D]
    float row_scale;
    int64_t B;
    int32_t D, K, skip_equal;
};

// BWD false: scores, loss, coeff and (d_center != NULL) the gradient rows of row_scale * loss_b.  BWD true: the gradient rows from coeff
// and d_loss.
template <int G, bool BWD>
__global__ __launch_bounds__(256) void sgns_kernel(const SgnsP p) {
    constexpr int EPB = 256 / G;                               // examples per block
    const int gl = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * EPB + threadIdx.x / G;
    const bool bv = b0 < p.B;
    const int64_t b = bv ? b0 : p.B - 1;                       // a group past the end repeats the last example and stores nothing
    const int D = p.D, K = p.K, S = K + 1;
    const bool active = 4 * gl < D;                            // D / 4 lanes of the group carry the row
    const int col = 4 * gl;
    const int64_t c = p.centers[b], o0 = p.contexts[b];
    const bool ex_ok = c >= 0 && o0 >= 0;
    const bool grads = BWD || p.d_center != nullptr;
    float4 u = dr_zero4();
    if (ex_ok && active) u = *reinterpret_cast<const float4*>(p.in_table + c * D + col);
    float w = 1.f, scale;
    if constexpr (BWD) {
        scale = p.d_loss[b];
    } else {
        if (p.sample_weight != nullptr) w = p.sample_weight[b];
        scale = p.row_scale;
    }
    float loss = 0.f;
    float4 acc = dr_zero4();
    for (int j0 = 0; j0 < S; j0 += SGNS_U) {                    // uniform over the block: S depends on K only
        float4 v[SGNS_U];
        bool skip[SGNS_U];
        float gin[SGNS_U];
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int j = j0 + t;
            const bool jv = j < S;
            int64_t id = -1;
            if (jv && ex_ok) id = j == 0 ? o0 : p.negatives[b * K + (j - 1)];
            skip[t] = id < 0 || (j > 0 && p.skip_equal && id == o0);
            v[t] = dr_zero4();
            if (!skip[t] && active) v[t] = *reinterpret_cast<const float4*>(p.out_table + id * D + col);
            if constexpr (BWD) gin[t] = jv ? p.coeff_in[b * S + j] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int j = j0 + t;
            const bool jv = j < S;
            float g;
            if constexpr (BWD) {
                g = gin[t];
            } else {
                const float s = sgns_group_sum<G>(sgns_dot4(u, v[t]));
                g = sgns_loss_term(s, j == 0, skip[t], w, loss);
                if (bv && jv && gl == 0) {
                    p.coeff[b * S + j] = g;
                    if (p.scores != nullptr) p.scores[b * S + j] = skip[t] ? 0.f : s;
                }
            }
            if (grads) {
                float4 dx;
                sgns_grad_slot(scale * g, skip[t], u, v[t], acc, dx);
                if (bv && jv && active) *reinterpret_cast<float4*>(p.d_ctx + b * p.ld_dx + (int64_t)j * D + col) = dx;
            }
        }
    }
    if constexpr (!BWD) {
        if (bv && gl == 0) p.loss_rows[b] = w * loss;
    }
    if (grads && bv && active) *reinterpret_cast<float4*>(p.d_center + b * p.ld_dc + col) = acc;
}

int sgns_sizes(SgnsP& p, int64_t B, int32_t D, int32_t K, int32_t flags) {
    if (B < 0 || D < 4 || D > SGNS_MAX_D || (D & 3) || K < 0 || K > SGNS_MAX_K || (flags & ~DR_SGNS_SKIP_EQUAL)) return DR_EINVAL;
    p.B = B; p.D = D; p.K = K; p.skip_equal = (flags & DR_SGNS_SKIP_EQUAL) ? 1 : 0;
    return DR_OK;
}

template <bool BWD>
int sgns_launch(const SgnsP& p, dr_stream_t stream) {
    const int g = dr_pow2_ceil(p.D >> 2);
    const int64_t grid = (p.B + 256 / g - 1) / (256 / g);
    if (grid > 0x7fffffff) return DR_EINVAL;
    const dim3 gr((unsigned)grid), bl(256);
    switch (g) {
        case 1: return dr_launch(sgns_kernel<1, BWD>, gr, bl, 0, dr_s(stream), p);
        case 2: return dr_launch(sgns_kernel<2, BWD>, gr, bl, 0, dr_s(stream), p);
        case 4: return dr_launch(sgns_kernel<4, BWD>, gr, bl, 0, dr_s(stream), p);
        case 8: return dr_launch(sgns_kernel<8, BWD>, gr, bl, 0, dr_s(stream), p);
        case 16: return dr_launch(sgns_kernel<16, BWD>, gr, bl, 0, dr_s(stream), p);
        case 32: return dr_launch(sgns_kernel<32, BWD>, gr, bl, 0, dr_s(stream), p);
        default: return dr_launch(sgns_kernel<64, BWD>, gr, bl, 0, dr_s(stream), p);
    }
}

// the two gradient buffers: both given, aligned and pitched for float4 rows
bool sgns_bad_grads(const float* d_center, int64_t ld_dc, const float* d_ctx, int64_t ld_dx, int32_t D, int32_t K) {
    return !d_center || !d_ctx || !dr_aligned16(d_center) || !dr_aligned16(d_ctx) || dr_bad_ld(ld_dc, D) ||
           dr_bad_ld(ld_dx, (int64_t)(K + 1) * D);
}

}  // namespace

extern "C" int dr_sgns_fwd(const float* in_table, const float* out_table, int32_t D, const int64_t* centers, const int64_t* contexts,
                           const int64_t* negatives, int64_t B, int32_t K, const float* sample_weight, int32_t flags, float row_scale,
                           float* loss_rows, float* coeff, float* scores, float* d_center, int64_t ld_dc, float* d_ctx, int64_t ld_dx,
                           dr_stream_t stream) {
    SgnsP p = {};
    const int st = sgns_sizes(p, B, D, K, flags);
    if (st != DR_OK) return st;
    const bool grads = d_center != nullptr || d_ctx != nullptr;
    if (grads && (dr_bad_ld(ld_dc, D) || dr_bad_ld(ld_dx, (int64_t)(K + 1) * D))) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!in_table || !out_table || !centers || !contexts || (K > 0 && !negatives) || !loss_rows || !coeff) return DR_EINVAL;
    if (!dr_aligned16(in_table) || !dr_aligned16(out_table)) return DR_EINVAL;
    if (grads && sgns_bad_grads(d_center, ld_dc, d_ctx, ld_dx, D, K)) return DR_EINVAL;
    p.in_table = in_table; p.out_table = out_table; p.centers = centers; p.contexts = contexts; p.negatives = negatives;
    p.sample_weight = sample_weight; p.row_scale = row_scale; p.loss_rows = loss_rows; p.coeff = coeff; p.scores = scores;
    p.d_center = d_center; p.ld_dc = ld_dc; p.d_ctx = d_ctx; p.ld_dx = ld_dx;
    return sgns_launch<false>(p, stream);
}

extern "C" int dr_sgns_bwd(const float* in_table, const float* out_table, int32_t D, const int64_t* centers, const int64_t* contexts,
                           const int64_t* negatives, int64_t B, int32_t K, int32_t flags, const float* coeff, const float* d_loss,
                           float* d_center, int64_t ld_dc, float* d_ctx, int64_t ld_dx, dr_stream_t stream) {
    SgnsP p = {};
    const int st = sgns_sizes(p, B, D, K, flags);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_dc, D) || dr_bad_ld(ld_dx, (int64_t)(K + 1) * D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!in_table || !out_table || !centers || !contexts || (K > 0 && !negatives) || !coeff || !d_loss) return DR_EINVAL;
    if (!dr_aligned16(in_table) || !dr_aligned16(out_table) || sgns_bad_grads(d_center, ld_dc, d_ctx, ld_dx, D, K)) return DR_EINVAL;
    p.in_table = in_table; p.out_table = out_table; p.centers = centers; p.contexts = contexts; p.negatives = negatives;
    p.coeff_in = coeff; p.d_loss = d_loss; p.d_center = d_center; p.ld_dc = ld_dc; p.d_ctx = d_ctx; p.ld_dx = ld_dx;
    return sgns_launch<true>(p, stream);
}
