// LS-PLM, the large-scale piece-wise linear model (Gai et al., Alibaba 2017): a mixture of m logistic experts under a softmax gate over
// sparse features, as one bag-sum + head kernel each way.
//
//   a table row is W = 2 m floats: [u (gate, m) | w (expert, m)]
//   z[b, :] = bias + sum_f mean over the valid ids of field f's bag of table[row_base[f] + id, :]      (K3's pooling; empty bag: nothing)
//   pi = softmax(z[:m]) (max subtracted),  sg_i = sigmoid(z[m + i]),  sn_i = sigmoid(-z[m + i])
//   p = sum_i pi_i sg_i,   q = sum_i pi_i sn_i  (= 1 - p without the subtraction)
//   d_z = d_p [ pi_i (sg_i - p) ; pi_i sg_i sn_i ],   d_rows[b, f, :] = d_z[b, :] for every field (K4 divides by the bag count)
//
// A POWER-OF-TWO GROUP OF G >= m / 2 LANES OWNS ONE EXAMPLE.  Lane l < m / 2 keeps the gate columns (2 l, 2 l + 1) and the expert
// columns (m + 2 l, m + 2 l + 1) of z in registers, so pi_i and sg_i of one region meet in one lane; the m-way max and the three m-way
// sums are xor butterflies inside the group (G / 2 .. 1: every lane ends with the same bits).  No LDS, no atomics, no workspace.  The
// fields are added in ascending order, a bag in column order: the order is a function of (F, m, the bag layout) alone, results are
// bit-identical from run to run and an example's bits depend neither on its batch nor on its place in it.
// sg and sn come from ONE exponential e = exp(-|x|): 1 / (1 + e) and e / (1 + e), so sg + sn is 1 to a rounding and p + q stays within
// a few roundings of 1 whatever m is.
// The forward, the backward (from the stored z) and the one-pass training form share lsplm_head / lsplm_dz: the same z bits give the
// same p, q and d_z bits.
#include "dr_common.h"
#include "dr_sum_partials.h"

namespace {

constexpr int LS_MAX_M = 128;
constexpr int LS_MAX_F = 1024;
constexpr int LS_U = 4;               // rows a lane keeps in flight (single-valued fields)
constexpr float LS_TINY = 1e-30f;     // floor of p and q inside the log and the quotient of the loss form

struct LsP {
    const int64_t* ids; const int32_t* col_start; const int64_t* row_base;
    const float* table; const float* bias;
    const float* z_in; int64_t ld_zin;           // backward: the z the forward stored
    const float* d_p;                            // backward
    const float* labels; const float* sample_weight; float row_scale;   // loss form
    float* z; int64_t ld_z;                      // forward, optional
    float* p; float* q; float* loss;
    float* d_z; int64_t ld_dz;
    float* d_rows; int64_t ld_d;
    int64_t B;
    int32_t F, C, m, W, h;                       // W = 2 m, h = m / 2 lanes that hold columns
};

struct LsZ { float2 u, w; };                     // this lane's two gate and two expert columns

__device__ __forceinline__ float2 ls_ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// z of example b on lane l < h (bias + the pooled rows); lanes l >= h never load
__device__ __forceinline__ LsZ lsplm_pool(const LsP& p, int64_t b, int l) {
    LsZ z;
    z.u = ls_ld2(p.bias + 2 * l);
    z.w = ls_ld2(p.bias + p.m + 2 * l);
    const int64_t* id_row = p.ids + b * p.C;
    const float* col = p.table + 2 * l;
    if (p.col_start == nullptr) {                              // single-valued fields, C == F
        for (int f0 = 0; f0 < p.F; f0 += LS_U) {
            int64_t r[LS_U];
            float2 u[LS_U], w[LS_U];
#pragma unroll
            for (int k = 0; k < LS_U; ++k) {
                r[k] = -1;
                if (f0 + k < p.F) {
                    const int64_t id = id_row[f0 + k];
                    r[k] = id >= 0 ? p.row_base[f0 + k] + id : -1;
                }
            }
#pragma unroll
            for (int k = 0; k < LS_U; ++k) {
                u[k] = make_float2(0.f, 0.f); w[k] = make_float2(0.f, 0.f);
                if (r[k] >= 0) { u[k] = ls_ld2(col + r[k] * p.W); w[k] = ls_ld2(col + r[k] * p.W + p.m); }
            }
#pragma unroll
            for (int k = 0; k < LS_U; ++k) {
                if (r[k] >= 0) { z.u.x += u[k].x; z.u.y += u[k].y; z.w.x += w[k].x; z.w.y += w[k].y; }
            }
        }
        return z;
    }
    for (int f = 0; f < p.F; ++f) {                            // ragged bags: K3's general path
        const int c0 = p.col_start[f], c1 = p.col_start[f + 1];
        const int64_t base = p.row_base[f];
        float2 au = make_float2(0.f, 0.f), aw = make_float2(0.f, 0.f);
        int cnt = 0;
        for (int c = c0; c < c1; ++c) {
            const int64_t id = id_row[c];
            if (id >= 0) {
                const float* row = col + (base + id) * p.W;
                const float2 u = ls_ld2(row), w = ls_ld2(row + p.m);
                au.x += u.x; au.y += u.y; aw.x += w.x; aw.y += w.y;
                ++cnt;
            }
        }
        if (cnt > 1) {                                         // one divide by the count, as K3
            const float n = (float)cnt;
            au.x /= n; au.y /= n; aw.x /= n; aw.y /= n;
        }
        if (cnt > 0) { z.u.x += au.x; z.u.y += au.y; z.w.x += aw.x; z.w.y += aw.y; }
    }
    return z;
}

struct LsHead { float2 pi, sg, sn; float p, q; };

__device__ __forceinline__ void ls_sig(float x, float& sg, float& sn) {
    const float e = expf(-fabsf(x)), t = 1.f + e;
    const float hi = 1.f / t, lo = e / t;
    sg = x >= 0.f ? hi : lo;
    sn = x >= 0.f ? lo : hi;
}

// every lane of the group takes part (lanes l >= h with neutral values); p and q end up identical on all of them
template <int G>
__device__ __forceinline__ LsHead lsplm_head(const LsZ& z, bool holds) {
#pragma clang fp contract(off)        // every instantiation rounds p and q the same way, whether or not it stores them
    LsHead H;
    float mx = holds ? fmaxf(z.u.x, z.u.y) : -INFINITY;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, G));
    const float ex = holds ? expf(z.u.x - mx) : 0.f, ey = holds ? expf(z.u.y - mx) : 0.f;
    float se = ex + ey;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) se += __shfl_xor(se, o, G);
    H.pi = make_float2(ex / se, ey / se);
    H.sg = make_float2(0.f, 0.f); H.sn = make_float2(0.f, 0.f);
    if (holds) { ls_sig(z.w.x, H.sg.x, H.sn.x); ls_sig(z.w.y, H.sg.y, H.sn.y); }
    float pp = H.pi.x * H.sg.x + H.pi.y * H.sg.y, qq = H.pi.x * H.sn.x + H.pi.y * H.sn.y;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) { pp += __shfl_xor(pp, o, G); qq += __shfl_xor(qq, o, G); }
    H.p = pp; H.q = qq;
    return H;
}

// d_z of this lane's columns for the example's d_p
__device__ __forceinline__ LsZ lsplm_dz(const LsHead& H, float d_p) {
#pragma clang fp contract(off)        // sg - p must not fuse with the products p is made of (G = 1 keeps them in one lane)
    LsZ g;
    g.u = make_float2(d_p * (H.pi.x * (H.sg.x - H.p)), d_p * (H.pi.y * (H.sg.y - H.p)));
    g.w = make_float2(d_p * (H.pi.x * (H.sg.x * H.sn.x)), d_p * (H.pi.y * (H.sg.y * H.sn.y)));
    return g;
}

__device__ __forceinline__ void ls_st(float* dst, int m, int l, const LsZ& v) {
    *reinterpret_cast<float2*>(dst + 2 * l) = v.u;
    *reinterpret_cast<float2*>(dst + m + 2 * l) = v.w;
}

__device__ __forceinline__ void lsplm_store_grads(const LsP& p, int64_t b, int l, const LsZ& g) {
    if (p.d_z != nullptr) ls_st(p.d_z + b * p.ld_dz, p.m, l, g);
    if (p.d_rows != nullptr) {
        float* dst = p.d_rows + b * p.ld_d;
        for (int f = 0; f < p.F; ++f) ls_st(dst + (int64_t)f * p.W, p.m, l, g);
    }
}

// MODE 0: forward (z optional, p, q);  1: backward from z_in and d_p;  2: the one-pass training form
template <int G, int MODE>
__global__ __launch_bounds__(256) void lsplm_kernel(const LsP p) {
    constexpr int EPB = 256 / G;                               // examples per block
    const int l = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * EPB + threadIdx.x / G;
    const bool bv = b0 < p.B;
    const int64_t b = bv ? b0 : p.B - 1;                       // a group past the end repeats the last example and stores nothing
    const bool holds = l < p.h;
    LsZ z;
    z.u = make_float2(0.f, 0.f); z.w = make_float2(0.f, 0.f);
    if (holds) {
        if constexpr (MODE == 1) {
            z.u = ls_ld2(p.z_in + b * p.ld_zin + 2 * l);
            z.w = ls_ld2(p.z_in + b * p.ld_zin + p.m + 2 * l);
        } else {
            z = lsplm_pool(p, b, l);
        }
    }
    const LsHead H = lsplm_head<G>(z, holds);
    if (!bv) return;                                           // after the last shuffle
    if constexpr (MODE == 0) {
        if (holds && p.z != nullptr) ls_st(p.z + b * p.ld_z, p.m, l, z);
        if (l == 0) { p.p[b] = H.p; p.q[b] = H.q; }
    } else if constexpr (MODE == 1) {
        if (holds) lsplm_store_grads(p, b, l, lsplm_dz(H, p.d_p[b]));
    } else {
        const float y = p.labels[b], ny = 1.f - y;
        const float wt = p.sample_weight != nullptr ? p.sample_weight[b] : 1.f;
        const float pc = fmaxf(H.p, LS_TINY), qc = fmaxf(H.q, LS_TINY);
        float c = 0.f, ll = 0.f;
        if (y != 0.f) { c = -y / pc; ll = y * logf(pc); }      // a term whose coefficient is exactly 0 is not evaluated
        if (ny != 0.f) { c += ny / qc; ll += ny * logf(qc); }
        if (l == 0) {
            p.p[b] = H.p; p.q[b] = H.q;
            if (p.loss != nullptr) p.loss[b] = -wt * ll;
        }
        if (holds) lsplm_store_grads(p, b, l, lsplm_dz(H, (p.row_scale * wt) * c));
    }
}

// part[chunk, c] = sum over the chunk's rows of d_z[r, c], rows in ascending order; one thread per column
__global__ __launch_bounds__(256) void lsplm_colsum_kernel(const float* __restrict__ d_z, int64_t ld, int64_t B, int32_t W,
                                                           int64_t rows_per_chunk, float* __restrict__ part) {
    const int c = threadIdx.x;
    if (c >= W) return;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = r0 + rows_per_chunk < B ? r0 + rows_per_chunk : B;
    float acc = 0.f;
    for (int64_t r = r0; r < r1; ++r) acc += d_z[r * ld + c];
    part[(int64_t)blockIdx.x * W + c] = acc;
}

int64_t ls_chunks(int64_t B) { return B <= 0 ? 0 : (B + 31) / 32 < 256 ? (B + 31) / 32 : 256; }

// fills the sizes; DR_OK, or DR_EINVAL / DR_ESHAPE outside the domain
int ls_sizes(LsP& p, int64_t B, int32_t F, int32_t m) {
    if (B < 0 || F < 1 || F > LS_MAX_F) return DR_EINVAL;
    if (m < 2 || m > LS_MAX_M || (m & 1)) return DR_ESHAPE;
    p.B = B; p.F = F; p.m = m; p.W = 2 * m; p.h = m >> 1;
    return DR_OK;
}

int ls_pool_args(LsP& p, const int64_t* ids, int32_t C, const int32_t* col_start, const int64_t* row_base, const float* table,
                 const float* bias) {
    if (C < p.F || (col_start == nullptr && C != p.F)) return DR_EINVAL;
    if (p.B == 0) return DR_OK;
    if (!ids || !row_base || !table || !bias || !dr_aligned16(table) || !dr_aligned16(bias)) return DR_EINVAL;
    p.ids = ids; p.C = C; p.col_start = col_start; p.row_base = row_base; p.table = table; p.bias = bias;
    return DR_OK;
}

template <int MODE>
int ls_launch(const LsP& p, dr_stream_t stream) {
    const int g = dr_pow2_ceil(p.h);
    const int64_t grid = (p.B + 256 / g - 1) / (256 / g);
    if (grid > 0x7fffffff) return DR_EINVAL;
    const dim3 gr((unsigned)grid), bl(256);
    switch (g) {
        case 1: return dr_launch(lsplm_kernel<1, MODE>, gr, bl, 0, dr_s(stream), p);
        case 2: return dr_launch(lsplm_kernel<2, MODE>, gr, bl, 0, dr_s(stream), p);
        case 4: return dr_launch(lsplm_kernel<4, MODE>, gr, bl, 0, dr_s(stream), p);
        case 8: return dr_launch(lsplm_kernel<8, MODE>, gr, bl, 0, dr_s(stream), p);
        case 16: return dr_launch(lsplm_kernel<16, MODE>, gr, bl, 0, dr_s(stream), p);
        case 32: return dr_launch(lsplm_kernel<32, MODE>, gr, bl, 0, dr_s(stream), p);
        default: return dr_launch(lsplm_kernel<64, MODE>, gr, bl, 0, dr_s(stream), p);
    }
}

}  // namespace

extern "C" int dr_lsplm_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start, const int64_t* row_base,
                            const float* table, int32_t m, const float* bias, float* z, int64_t ld_z, float* p, float* q,
                            dr_stream_t stream) {
    LsP a = {};
    int st = ls_sizes(a, B, F, m);
    if (st != DR_OK) return st;
    if (z != nullptr && dr_bad_ld(ld_z, a.W)) return DR_EINVAL;
    st = ls_pool_args(a, ids, C, col_start, row_base, table, bias);
    if (st != DR_OK || B == 0) return st;
    if (!p || !q || !dr_aligned16(z)) return DR_EINVAL;
    a.z = z; a.ld_z = ld_z; a.p = p; a.q = q;
    return ls_launch<0>(a, stream);
}

extern "C" int dr_lsplm_bwd(const float* z, int64_t ld_z, const float* d_p, int64_t B, int32_t F, int32_t m, float* d_z,
                            int64_t ld_dz, float* d_rows, int64_t ld_d, dr_stream_t stream) {
    LsP a = {};
    const int st = ls_sizes(a, B, F, m);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_z, a.W) || (d_z != nullptr && dr_bad_ld(ld_dz, a.W)) || (d_rows != nullptr && dr_bad_ld(ld_d, (int64_t)F * a.W)))
        return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!z || !d_p || (!d_z && !d_rows) || !dr_aligned16(z) || !dr_aligned16(d_z) || !dr_aligned16(d_rows)) return DR_EINVAL;
    a.z_in = z; a.ld_zin = ld_z; a.d_p = d_p; a.d_z = d_z; a.ld_dz = ld_dz; a.d_rows = d_rows; a.ld_d = ld_d;
    return ls_launch<1>(a, stream);
}

extern "C" int dr_lsplm_loss_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start,
                                 const int64_t* row_base, const float* table, int32_t m, const float* bias, const float* labels,
                                 const float* sample_weight, float row_scale, float* p, float* q, float* loss, float* d_z,
                                 int64_t ld_dz, float* d_rows, int64_t ld_d, dr_stream_t stream) {
    LsP a = {};
    int st = ls_sizes(a, B, F, m);
    if (st != DR_OK) return st;
    if ((d_z != nullptr && dr_bad_ld(ld_dz, a.W)) || (d_rows != nullptr && dr_bad_ld(ld_d, (int64_t)F * a.W))) return DR_EINVAL;
    st = ls_pool_args(a, ids, C, col_start, row_base, table, bias);
    if (st != DR_OK || B == 0) return st;
    if (!labels || !p || !q || !dr_aligned16(d_z) || !dr_aligned16(d_rows)) return DR_EINVAL;
    a.labels = labels; a.sample_weight = sample_weight; a.row_scale = row_scale; a.p = p; a.q = q; a.loss = loss;
    a.d_z = d_z; a.ld_dz = ld_dz; a.d_rows = d_rows; a.ld_d = ld_d;
    return ls_launch<2>(a, stream);
}

extern "C" int64_t dr_lsplm_bias_grad_workspace_bytes(int64_t B, int32_t m) {
    if (B < 0 || m < 2 || m > LS_MAX_M) return -1;
    return ls_chunks(B) * 2 * m * (int64_t)sizeof(float);
}

extern "C" int dr_lsplm_bias_grad(const float* d_z, int64_t ld_dz, int64_t B, int32_t m, float* d_bias, void* workspace,
                                  int64_t workspace_bytes, dr_stream_t stream) {
    LsP a = {};
    const int st = ls_sizes(a, B, 1, m);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_dz, a.W) || !d_bias) return DR_EINVAL;
    const int64_t chunks = ls_chunks(B);
    if (workspace_bytes < chunks * a.W * (int64_t)sizeof(float)) return DR_EINVAL;
    if (B > 0) {
        if (!d_z || !workspace) return DR_EINVAL;
        const int64_t rpc = (B + chunks - 1) / chunks;
        const int st1 = dr_launch(lsplm_colsum_kernel, dim3((unsigned)chunks), dim3(256), 0, dr_s(stream), d_z, ld_dz, B, a.W, rpc,
                                  static_cast<float*>(workspace));
        if (st1 != DR_OK) return st1;
    }
    // with B == 0 there are no partials and the sum is +0.0
    return dr_sum_partials(static_cast<const float*>(workspace), chunks, d_bias, a.W, nullptr, 0, nullptr, 0, 1, dr_s(stream));
}
