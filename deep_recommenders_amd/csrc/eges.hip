// Skip-gram with side information: EGES (Wang et al., KDD 2018) and, with one field and two positives, Airbnb's listing embeddings
// (Grbovic & Cheng, KDD 2018).  The centre's vector is a softmax-weighted sum of table rows, the slots are csrc/sgns.hip's.
//
//   example b:  field s is PRESENT when side_ids[b, s] >= 0, its row w_s = side_table[row_base[s] + side_ids[b, s]]
//   a_s = att[att_ids[b], s]  (0 when att == NULL or att_ids[b] < 0);  m = max_present a_s;  e_s = expf(a_s - m);  Z = sum_present e_s
//   alpha_s = e_s / Z  (0 for a missing field);   u = sum_present alpha_s w_s
//   slots j = 0 .. P + K - 1: o_j from contexts [B, P] then negatives [B, K], z_j = (j < P); s_j, loss_b, g_j as in csrc/sgns.hip
//   c_j = row_scale g_j (one pass) | d_loss[b] g_j (backward);  d_u = sum_j c_j v_j;  d_ctx[b, j, :] = c_j u
//   d_side[b, s, :] = alpha_s d_u;  q_s = <d_u, w_s>;  r = sum_present alpha_s q_s;  d_att[b, s] = alpha_s (q_s - r)
// every sum in ascending index order, one fmaf per term added (the first term of u is the rounded product itself).
//
// The shape is sgns.hip's: A GROUP OF G LANES OWNS ONE EXAMPLE, G = D / 4 rounded up to a power of two, lane l holds the float4 at column
// 4 l of every row; u and d_u stay in registers, SGNS_U rows are in flight per lane, the dots meet in an xor butterfly inside the group.
// No atomic, no LDS, no barrier, no workspace.  d_side and d_att need d_u, which is complete only after the last slot: THE S ROWS w_s
// ARE READ A SECOND TIME then (they were touched P + K row loads ago and sit in L2), not kept -- 4 S registers per lane would be 64 at
// S = 16 on top of what the slot loop holds (DESIGN.md section 21 has the counts).  Nothing is kept per field either: alpha_s is
// evaluated again where it is needed, and q_s waits in its own output element d_att[b, s] until r is whole.
// With ONE FIELD the forward and the embed take an exact shortcut (alpha = 1: no logit, no passes, no second read), see `single` below.
// A MISSING FIELD, A SKIPPED SLOT and A SKIPPED EXAMPLE (no field present, or contexts[b, 0] < 0) load no table row: their ids are read
// (an id is data) and compared, never formed into an address that is dereferenced.
#include "sgns_common.h"

namespace {

constexpr int EGES_MAX_S = 16;
constexpr int EGES_MAX_P = 4;
constexpr int EGES_MAX_SLOTS = 64;    // ids [B, P + K] go through the sorted K4, which takes F <= 64

enum EgesMode { EGES_FWD = 0, EGES_BWD = 1, EGES_EMBED = 2 };

struct EgesP {
    const float* side_table; const int64_t* row_base; const int64_t* side_ids;
    const float* att; int64_t ld_att; const int64_t* att_ids;
    const float* out_table; const int64_t* contexts; const int64_t* negatives;
    const float* sample_weight;                                // forward, may be NULL
    const float* coeff_in; const float* alpha_in; const float* d_loss;      // backward
    float* loss_rows; float* coeff; float* alpha; float* scores;            // forward; scores may be NULL
    float* d_side; int64_t ld_ds;                // [B, S D]; forward: NULL together with d_att and d_ctx
    float* d_att; int64_t ld_da;                 // [B, ld_da]
    float* d_ctx; int64_t ld_dx;                 // [B, (P + K) D]
    float* out; int64_t ld_out;                  // embed: [B, D]
    float row_scale;
    int64_t B;
    int32_t D, S, P, K, skip_equal;
};

__device__ __forceinline__ float4 eges_load(const float* table, int64_t row, int D, int col) {
    return *reinterpret_cast<const float4*>(table + row * D + col);
}

template <int G, int MODE>
__global__ __launch_bounds__(256) void eges_kernel(const EgesP p) {
    constexpr int EPB = 256 / G;                               // examples per block
    constexpr bool BWD = MODE == EGES_BWD;
    const int gl = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * EPB + threadIdx.x / G;
    const bool bv = b0 < p.B;
    const int64_t b = bv ? b0 : p.B - 1;                       // a group past the end repeats the last example and stores nothing
    const int D = p.D, S = p.S, P = p.P, K = p.K, J = P + K;
    const bool active = 4 * gl < D;                            // D / 4 lanes of the group carry the row
    const int col = 4 * gl;
    const int64_t* sid = p.side_ids + b * S;

    const int64_t* ctx = MODE == EGES_EMBED ? nullptr : p.contexts + b * P;
    const bool ctx_ok = MODE == EGES_EMBED || ctx[0] >= 0;

    // the weights: presence, then the softmax over the present fields (backward: the forward's alpha).  alpha_s is not kept per field:
    // alpha_of(s) evaluates it again from m and Z -- the same instructions on the same values, hence the same bits every time.
    // ONE FIELD (forward and embed; uniform over the launch): the softmax of one finite logit is expf(0) / 1 = 1 whatever the logit, so
    // u = 1 w, d_side = 1 d_u and d_att = 1 (q - fma(1, q, 0)) = +0.0 are exact and need neither the logit, the two passes, nor -- after
    // the slots -- the row a second time.  The same bits as the general path, without its prologue and tail: what an Airbnb step runs.
    const bool single = !BWD && S == 1;
    const int64_t aid0 = (p.att != nullptr && !single) ? p.att_ids[b] : -1;
    const int64_t aid = ctx_ok ? aid0 : -1;
    const bool use_att = aid >= 0;
    const float* arow = use_att ? p.att + aid * p.ld_att : nullptr;
    uint32_t pres = 0;
    float m = -INFINITY, Z = 0.f;
    if (single) {
        pres = (ctx_ok && sid[0] >= 0) ? 1u : 0u;
    } else {
        for (int s = 0; s < S; ++s) {
            const int64_t id = sid[s];                         // loaded whether or not the example is live: an id is data, only the
            if (ctx_ok && id >= 0) {                           // row address formed from it is guarded
                pres |= 1u << s;
                if (!BWD && use_att) m = fmaxf(m, arow[s]);
            }
        }
        if (!use_att) m = 0.f;
        if constexpr (!BWD) {
            for (int s = 0; s < S; ++s) {
                if ((pres >> s) & 1u) Z += expf((use_att ? arow[s] : 0.f) - m);
            }
        }
    }
    auto alpha_of = [&](int s) -> float {
        if (!((pres >> s) & 1u)) return 0.f;
        if constexpr (BWD) return p.alpha_in[b * S + s];
        else return single ? 1.f : expf((use_att ? arow[s] : 0.f) - m) / Z;
    };
    if constexpr (MODE == EGES_FWD) {
        if (bv && gl == 0) {
            for (int s = 0; s < S; ++s) p.alpha[b * S + s] = alpha_of(s);
        }
    }
    const bool ex_ok = pres != 0;                              // at least one field, and (not embed) a first positive

    // u = sum_present alpha_s w_s
    float4 u = dr_zero4();
    bool first = true;
    for (int s0 = 0; s0 < S; s0 += SGNS_U) {                    // uniform over the block
        float4 w[SGNS_U];
        float al[SGNS_U];
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int s = s0 + t;
            const bool here = s < S && ((pres >> s) & 1u);
            w[t] = dr_zero4();
            if (here && active) w[t] = eges_load(p.side_table, p.row_base[s] + sid[s], D, col);
            al[t] = here ? alpha_of(s) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int s = s0 + t;
            if (s < S && ((pres >> s) & 1u)) {
                const float a = al[t];
                u = first ? make_float4(a * w[t].x, a * w[t].y, a * w[t].z, a * w[t].w)
                          : make_float4(fmaf(a, w[t].x, u.x), fmaf(a, w[t].y, u.y), fmaf(a, w[t].z, u.z), fmaf(a, w[t].w, u.w));
                first = false;
            }
        }
    }
    if constexpr (MODE == EGES_EMBED) {
        if (bv && active) *reinterpret_cast<float4*>(p.out + b * p.ld_out + col) = u;
        return;
    }

    // the slots, as in sgns_kernel
    const bool grads = BWD || p.d_ctx != nullptr;
    float wgt = 1.f, scale;
    if constexpr (BWD) {
        scale = p.d_loss[b];
    } else {
        if (p.sample_weight != nullptr) wgt = p.sample_weight[b];
        scale = p.row_scale;
    }
    float loss = 0.f;
    float4 acc = dr_zero4();
    for (int j0 = 0; j0 < J; j0 += SGNS_U) {                    // uniform over the block: J depends on P and K only
        float4 v[SGNS_U];
        bool skip[SGNS_U];
        float gin[SGNS_U];
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int j = j0 + t;
            const bool jv = j < J;
            int64_t id = -1;
            if (jv) id = j < P ? ctx[j] : p.negatives[b * K + (j - P)];
            if (!ex_ok) id = -1;
            bool eq = false;
            if (j >= P && p.skip_equal) {                       // the positives are read again here (P cached loads) rather than held in
                for (int q = 0; q < P; ++q) eq = eq || id == ctx[q];                //   8 registers through the loop; id < 0 is skipped anyway
            }
            skip[t] = id < 0 || eq;
            v[t] = dr_zero4();
            if (!skip[t] && active) v[t] = eges_load(p.out_table, id, D, col);
            if constexpr (BWD) gin[t] = jv ? p.coeff_in[b * J + j] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int j = j0 + t;
            const bool jv = j < J;
            float g;
            if constexpr (BWD) {
                g = gin[t];
            } else {
                const float s = sgns_group_sum<G>(sgns_dot4(u, v[t]));
                g = sgns_loss_term(s, j < P, skip[t], wgt, loss);
                if (bv && jv && gl == 0) {
                    p.coeff[b * J + j] = g;
                    if (p.scores != nullptr) p.scores[b * J + j] = skip[t] ? 0.f : s;
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
        if (bv && gl == 0) p.loss_rows[b] = wgt * loss;
    }
    if (!grads) return;

    // d_u = acc is complete: the fields once more.  q_s waits in d_att[b, s] (lane 0 of the group writes it and is the one to read it
    // back) until r is whole.
    float r = 0.f;
    float* da = p.d_att + b * p.ld_da;
    if (single) {
        if (bv && active) *reinterpret_cast<float4*>(p.d_side + b * p.ld_ds + col) = pres ? acc : dr_zero4();
        if (bv && gl == 0) {
            for (int s = 0; s < (int)p.ld_da; ++s) da[s] = 0.f;
        }
        return;
    }
    for (int s0 = 0; s0 < S; s0 += SGNS_U) {
        float4 w[SGNS_U];
        float al[SGNS_U];
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int s = s0 + t;
            const bool here = s < S && ((pres >> s) & 1u);
            w[t] = dr_zero4();
            if (here && active) w[t] = eges_load(p.side_table, p.row_base[s] + sid[s], D, col);
            al[t] = here ? alpha_of(s) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < SGNS_U; ++t) {
            const int s = s0 + t;
            const bool here = s < S && ((pres >> s) & 1u);
            const float qs = sgns_group_sum<G>(sgns_dot4(acc, w[t]));                // every lane of the group takes part
            const float a = al[t];
            if (here) r = fmaf(a, qs, r);
            const float4 ds = here ? make_float4(a * acc.x, a * acc.y, a * acc.z, a * acc.w) : dr_zero4();
            if (s < S && bv) {
                if (active) *reinterpret_cast<float4*>(p.d_side + b * p.ld_ds + (int64_t)s * D + col) = ds;
                if (gl == 0) da[s] = qs;
            }
        }
    }
    if (bv && gl == 0) {
        for (int s = 0; s < (int)p.ld_da; ++s) {
            const bool here = s < S && use_att && ((pres >> s) & 1u);
            da[s] = here ? alpha_of(s) * (da[s] - r) : 0.f;
        }
    }
}

int eges_sizes(EgesP& p, int64_t B, int32_t D, int32_t S) {
    if (B < 0 || D < 4 || D > SGNS_MAX_D || (D & 3) || S < 1 || S > EGES_MAX_S) return DR_EINVAL;
    p.B = B; p.D = D; p.S = S;
    return DR_OK;
}

int eges_slots(EgesP& p, int32_t P, int32_t K, int32_t flags) {
    if (P < 1 || P > EGES_MAX_P || K < 0 || K > EGES_MAX_SLOTS - P || (flags & ~DR_SGNS_SKIP_EQUAL)) return DR_EINVAL;
    p.P = P; p.K = K; p.skip_equal = (flags & DR_SGNS_SKIP_EQUAL) ? 1 : 0;
    return DR_OK;
}

bool eges_bad_pitches(const EgesP& p, int64_t ld_ds, int64_t ld_da, int64_t ld_dx) {
    return dr_bad_ld(ld_ds, (int64_t)p.S * p.D) || dr_bad_ld(ld_da, p.S) || ld_da > EGES_MAX_S ||
           dr_bad_ld(ld_dx, (int64_t)(p.P + p.K) * p.D);
}

// the gather side: required pointers, alignment, the attention table's pitch
bool eges_bad_inputs(const float* side_table, const int64_t* row_base, const int64_t* side_ids, const float* att, int64_t ld_att,
                     const int64_t* att_ids, int32_t S) {
    if (!side_table || !row_base || !side_ids || !dr_aligned16(side_table)) return true;
    return att != nullptr && (!att_ids || ld_att < S);
}

bool eges_bad_grads(const float* d_side, const float* d_att, const float* d_ctx) {
    return !d_side || !d_att || !d_ctx || !dr_aligned16(d_side) || !dr_aligned16(d_att) || !dr_aligned16(d_ctx);
}

template <int MODE>
int eges_launch(const EgesP& p, dr_stream_t stream) {
    const int g = dr_pow2_ceil(p.D >> 2);
    const int64_t grid = (p.B + 256 / g - 1) / (256 / g);
    if (grid > 0x7fffffff) return DR_EINVAL;
    const dim3 gr((unsigned)grid), bl(256);
    switch (g) {
        case 1: return dr_launch(eges_kernel<1, MODE>, gr, bl, 0, dr_s(stream), p);
        case 2: return dr_launch(eges_kernel<2, MODE>, gr, bl, 0, dr_s(stream), p);
        case 4: return dr_launch(eges_kernel<4, MODE>, gr, bl, 0, dr_s(stream), p);
        case 8: return dr_launch(eges_kernel<8, MODE>, gr, bl, 0, dr_s(stream), p);
        case 16: return dr_launch(eges_kernel<16, MODE>, gr, bl, 0, dr_s(stream), p);
        case 32: return dr_launch(eges_kernel<32, MODE>, gr, bl, 0, dr_s(stream), p);
        default: return dr_launch(eges_kernel<64, MODE>, gr, bl, 0, dr_s(stream), p);
    }
}

}  // namespace

extern "C" int dr_eges_fwd(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S,
                           const float* att, int64_t ld_att, const int64_t* att_ids, const float* out_table, const int64_t* contexts,
                           int32_t P, const int64_t* negatives, int32_t K, int64_t B, const float* sample_weight, int32_t flags,
                           float row_scale, float* loss_rows, float* coeff, float* alpha, float* scores, float* d_side, int64_t ld_ds,
                           float* d_att, int64_t ld_da, float* d_ctx, int64_t ld_dx, dr_stream_t stream) {
    EgesP p = {};
    int st = eges_sizes(p, B, D, S);
    if (st == DR_OK) st = eges_slots(p, P, K, flags);
    if (st != DR_OK) return st;
    const bool grads = d_side != nullptr || d_att != nullptr || d_ctx != nullptr;
    if (grads && eges_bad_pitches(p, ld_ds, ld_da, ld_dx)) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (eges_bad_inputs(side_table, row_base, side_ids, att, ld_att, att_ids, S)) return DR_EINVAL;
    if (!out_table || !dr_aligned16(out_table) || !contexts || (K > 0 && !negatives) || !loss_rows || !coeff || !alpha) return DR_EINVAL;
    if (grads && eges_bad_grads(d_side, d_att, d_ctx)) return DR_EINVAL;
    p.side_table = side_table; p.row_base = row_base; p.side_ids = side_ids; p.att = att; p.ld_att = ld_att; p.att_ids = att_ids;
    p.out_table = out_table; p.contexts = contexts; p.negatives = negatives; p.sample_weight = sample_weight; p.row_scale = row_scale;
    p.loss_rows = loss_rows; p.coeff = coeff; p.alpha = alpha; p.scores = scores;
    p.d_side = d_side; p.ld_ds = ld_ds; p.d_att = d_att; p.ld_da = ld_da; p.d_ctx = d_ctx; p.ld_dx = ld_dx;
    return eges_launch<EGES_FWD>(p, stream);
}

extern "C" int dr_eges_bwd(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S,
                           const float* att, const int64_t* att_ids, const float* out_table, const int64_t* contexts, int32_t P,
                           const int64_t* negatives, int32_t K, int64_t B, int32_t flags, const float* coeff, const float* alpha,
                           const float* d_loss, float* d_side, int64_t ld_ds, float* d_att, int64_t ld_da, float* d_ctx, int64_t ld_dx,
                           dr_stream_t stream) {
    EgesP p = {};
    int st = eges_sizes(p, B, D, S);
    if (st == DR_OK) st = eges_slots(p, P, K, flags);
    if (st != DR_OK) return st;
    if (eges_bad_pitches(p, ld_ds, ld_da, ld_dx)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (eges_bad_inputs(side_table, row_base, side_ids, att, S, att_ids, S)) return DR_EINVAL;
    if (!out_table || !dr_aligned16(out_table) || !contexts || (K > 0 && !negatives) || !coeff || !alpha || !d_loss) return DR_EINVAL;
    if (eges_bad_grads(d_side, d_att, d_ctx)) return DR_EINVAL;
    p.side_table = side_table; p.row_base = row_base; p.side_ids = side_ids; p.att = att; p.att_ids = att_ids;
    p.out_table = out_table; p.contexts = contexts; p.negatives = negatives; p.coeff_in = coeff; p.alpha_in = alpha; p.d_loss = d_loss;
    p.d_side = d_side; p.ld_ds = ld_ds; p.d_att = d_att; p.ld_da = ld_da; p.d_ctx = d_ctx; p.ld_dx = ld_dx;
    return eges_launch<EGES_BWD>(p, stream);
}

extern "C" int dr_eges_embed(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S,
                             const float* att, int64_t ld_att, const int64_t* att_ids, int64_t n, float* out, int64_t ld_out,
                             dr_stream_t stream) {
    EgesP p = {};
    const int st = eges_sizes(p, n, D, S);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (n == 0) return DR_OK;
    if (eges_bad_inputs(side_table, row_base, side_ids, att, ld_att, att_ids, S) || !out || !dr_aligned16(out)) return DR_EINVAL;
    p.side_table = side_table; p.row_base = row_base; p.side_ids = side_ids; p.att = att; p.ld_att = ld_att; p.att_ids = att_ids;
    p.out = out; p.ld_out = ld_out; p.P = 1;
    return eges_launch<EGES_EMBED>(p, stream);
}
