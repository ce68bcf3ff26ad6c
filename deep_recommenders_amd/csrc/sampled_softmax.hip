// The training loss of YoutubeNet (Covington et al., RecSys 2016), which the reference's README lists and ships no code for:
// tf.nn.sampled_softmax_loss with num_true = 1 and no bias -- a softmax over the true class and S sampled classes that the whole
// batch shares, importance-corrected by log Q, accidental hits left out.  dr_sampled_softmax_fwd / dr_sampled_softmax_bwd.
//
// It is csrc/attention.hip with one head, no V and keys shared by every query, and it takes the same answers: the [B, S] score
// matrix is never written (online softmax over 64-column tiles in the forward, recomputation from the saved row_lse in the
// backward), every product is the fp32-input MFMA v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation, no operand
// split), one wave owns 16 rows and keeps them in registers as the B operand of the TRANSPOSED score tile S^T = T U^T, whose
// accumulator layout is the B operand of the product that follows.  The table rows are gathered by id straight into the LDS tile;
// there is no [S, D] copy.
//
// Order of every sum: the columns are cut into `nseg` segments, a function of S alone.  A row-owning block
// starts every segment from fresh accumulators -- (max, sum) in the forward, the d_u sums in the backward -- and the segments are
// combined in ascending order, inside the block when it walks all of them and by a finalize kernel when every segment has a block of
// its own.  Both ways perform the same additions in the same order, so a row's outputs do not depend on B, although the grid does.
// d_sampled is summed over row chunks whose count is a function of (B, S), the chunk partials added in chunk order
// (dr_sum_partials.h).  No float atomics, no waiting between workgroups.
#include "dr_common.h"
#include "dr_sum_partials.h"
#include "dr_score_tile.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int SS_SMALL = 4 * SS_TILE;               // floats of per-row / per-column scalars behind the tile

struct SsPlan {
    int64_t row_tiles;
    int32_t col_tiles, nseg, seg_tiles, groups, chunks, chunk_tiles;
};

// pure functions of (B, S): no device query, so the bits do not depend on the machine
inline SsPlan ss_plan(int64_t B, int64_t S) {
    SsPlan pl;
    pl.row_tiles = (B + SS_TILE - 1) / SS_TILE;
    pl.col_tiles = (int32_t)((S + SS_TILE - 1) / SS_TILE);
    int64_t nseg = std::min<int64_t>(DR_SAMPLED_SOFTMAX_MAX_GROUPS, (S + DR_SAMPLED_SOFTMAX_COL_GROUP - 1) / DR_SAMPLED_SOFTMAX_COL_GROUP);
    pl.seg_tiles = (int32_t)((pl.col_tiles + nseg - 1) / nseg);
    pl.nseg = (pl.col_tiles + pl.seg_tiles - 1) / pl.seg_tiles;
    // one block per (row tile, segment) while the row tiles alone leave CUs idle; else one block walks every segment
    pl.groups = pl.row_tiles <= DR_SAMPLED_SOFTMAX_SPLIT_TILES ? pl.nseg : 1;
    const int64_t want = std::max<int64_t>(1, (512 + pl.col_tiles - 1) / pl.col_tiles);
    int64_t chunks = std::min<int64_t>(std::min<int64_t>(DR_SAMPLED_SOFTMAX_MAX_CHUNKS, want),
                                       std::max<int64_t>(1, (B + DR_SAMPLED_SOFTMAX_ROW_CHUNK - 1) / DR_SAMPLED_SOFTMAX_ROW_CHUNK));
    const int64_t ct = std::max<int64_t>(1, (pl.row_tiles + chunks - 1) / chunks);
    pl.chunk_tiles = (int32_t)std::min<int64_t>(ct, INT32_MAX);
    pl.chunks = (int32_t)std::max<int64_t>(1, (pl.row_tiles + ct - 1) / ct);
    return pl;
}

struct SsP {
    const float *u, *table, *lq_true, *lq_samp, *weight, *t_in, *lse_in;
    const int64_t *labels, *sampled;
    float *t_out, *ml, *scores, *d_u, *d_true, *d_samp, *part_u, *part_s;
    int64_t ld_u, ld_du, B;
    int32_t S, D, rah, col_tiles, nseg, seg_tiles, groups, chunks, chunk_tiles;
    int64_t row_tiles;
    float row_scale;
};

// the ids and log Q of the 64 columns from j0 on (-1: past S or a padding id: the column is left out and its row never read)
__device__ __forceinline__ void ss_stage_cols(const SsP& p, int64_t j0, int* sid, float* lqs) {
    if (threadIdx.x < SS_TILE) {
        const int64_t j = j0 + threadIdx.x;
        int id = -1;
        float lq = 0.f;
        if (j < p.S) {
            const int64_t s = p.sampled[j];
            if (s >= 0) {
                id = (int)s;
                if (p.lq_samp) lq = p.lq_samp[j];
            }
        }
        sid[threadIdx.x] = id;
        lqs[threadIdx.x] = lq;
    }
}

// g_i = c_i (exp(t_i - lse_i) - 1), c_i = row_scale w_i; both 0 for a padding row
__device__ __forceinline__ float ss_row_c(const SsP& p, int64_t i) { return p.weight ? p.row_scale * p.weight[i] : p.row_scale; }
__device__ __forceinline__ float ss_row_g(float c, float t, float lse) { return c * (expf(t - lse) - 1.f); }

// ---- forward: a block owns 64 rows of u and walks the column tiles of its segments ---------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void ss_fwd_kernel(const SsP p) {
    constexpr int LS = DP + 4;
    extern __shared__ __attribute__((aligned(16))) float ss_lds[];
    float* Ts = ss_lds;
    int* sid = reinterpret_cast<int*>(Ts + SS_TILE * LS);
    float* lqs = reinterpret_cast<float*>(sid + SS_TILE);
    const int64_t rt = blockIdx.x / p.groups;
    const int grp = (int)(blockIdx.x - rt * p.groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int64_t i = rt * SS_TILE + wave * 16 + i16;
    const bool inb = i < p.B;
    const int64_t lab64 = inb ? p.labels[i] : -1;
    const bool rok = lab64 >= 0;
    const int lab = rok ? (int)lab64 : -1;
    float ureg[DP / 4];
    ss_load_frag<DP>(ureg, rok ? p.u + i * p.ld_u : nullptr, p.D, g);
    if (grp == 0) {
        float t = ss_true_dot<DP>(rok ? p.table + (int64_t)lab * p.D : nullptr, ureg, p.D, i16, g);
        if (rok && p.lq_true) t -= p.lq_true[i];
        if (inb && g == 0) p.t_out[i] = rok ? t : 0.f;
    }
    const int seg0 = p.groups == 1 ? 0 : grp, seg1 = p.groups == 1 ? p.nseg : grp + 1;
    for (int seg = seg0; seg < seg1; ++seg) {
        float m = -INFINITY, l = 0.f;
        const int kt1 = min((seg + 1) * p.seg_tiles, p.col_tiles);
        for (int kt = seg * p.seg_tiles; kt < kt1; ++kt) {
            const int64_t j0 = (int64_t)kt * SS_TILE;
            __syncthreads();
            ss_stage_cols(p, j0, sid, lqs);
            __syncthreads();
            ss_load_tile<DP>(Ts, p.table, p.D, sid, p.D);
            __syncthreads();
            dr_f32x4 s[4];
            ss_tile_dot<DP>(Ts, ureg, i16, g, s);
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * t + 4 * g + r;
                    const int id = sid[jl];
                    const bool keep = id >= 0 && !(p.rah && id == lab);
                    s[t][r] = keep ? s[t][r] - lqs[jl] : -INFINITY;
                    mx = fmaxf(mx, s[t][r]);
                }
            if (p.scores && inb) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t j = j0 + 16 * t + 4 * g + r;
                        if (j < p.S) p.scores[i * p.S + j] = s[t][r];
                    }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);
            const float mref = mn == -INFINITY ? 0.f : mn;      // nothing kept so far: every exp below is exp(-inf) = 0
            float ls = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) ls += expf(s[t][r] - mref);
            ls += __shfl_xor(ls, 16, 64);
            ls += __shfl_xor(ls, 32, 64);
            l = l * expf(m - mref) + ls;
            m = mn;
        }
        if (inb && g == 0) {
            float* ml = p.ml + 2 * ((int64_t)seg * p.B + i);
            ml[0] = m;
            ml[1] = l;
        }
    }
}

// lse_i = log(exp(t_i) + sum over the segments in ascending order); loss_i = w_i (lse_i - t_i); a padding row: 0, 0
__global__ __launch_bounds__(256) void ss_fwd_finalize_kernel(const SsP p, float* __restrict__ row_lse, float* __restrict__ row_loss) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.B; i += stride) {
        if (p.labels[i] < 0) {
            row_lse[i] = 0.f;
            row_loss[i] = 0.f;
            continue;
        }
        const float t = p.t_out[i];
        float M = t;
        for (int seg = 0; seg < p.nseg; ++seg) M = fmaxf(M, p.ml[2 * ((int64_t)seg * p.B + i)]);
        float acc = expf(t - M);
        for (int seg = 0; seg < p.nseg; ++seg) {
            const float* ml = p.ml + 2 * ((int64_t)seg * p.B + i);
            acc += ml[1] * expf(ml[0] - M);
        }
        const float lse = M + logf(acc);
        row_lse[i] = lse;
        row_loss[i] = (p.weight ? p.weight[i] : 1.f) * (lse - t);
    }
}

// ---- backward, the row-owning sweep: d_u (and d_true) -------------------------------------------------------------------------------
// tot = ((0 + seg_0) + seg_1) + ...  SPLIT: one block per (row tile, segment); the segment's sum is the partial, and
// ss_bwd_rows_finalize_kernel adds the partials in the same order.  Without the running total the D 256 form runs two waves per SIMD.
template <int DP, bool SPLIT>
__device__ __forceinline__ void ss_bwd_rows_body(const SsP& p) {
    constexpr int LS = DP + 4, NC = DP / 16, NT = SPLIT ? 1 : NC;
    extern __shared__ __attribute__((aligned(16))) float ss_lds[];
    float* Ts = ss_lds;
    int* sid = reinterpret_cast<int*>(Ts + SS_TILE * LS);
    float* lqs = reinterpret_cast<float*>(sid + SS_TILE);
    const int64_t rt = blockIdx.x / p.groups;
    const int grp = (int)(blockIdx.x - rt * p.groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int64_t i = rt * SS_TILE + wave * 16 + i16;
    const bool inb = i < p.B;
    const int64_t lab64 = inb ? p.labels[i] : -1;
    const bool rok = lab64 >= 0;
    const int lab = rok ? (int)lab64 : -1;
    float ureg[DP / 4];
    ss_load_frag<DP>(ureg, rok ? p.u + i * p.ld_u : nullptr, p.D, g);
    const float lse = rok ? p.lse_in[i] : 0.f;
    const float c = rok ? ss_row_c(p, i) : 0.f;
    dr_f32x4 tot[NT], acc[NC];               // SPLIT: the block's one segment is its total, no second set of accumulators
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) tot[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int seg0 = SPLIT ? grp : 0, seg1 = SPLIT ? grp + 1 : p.nseg;
    for (int seg = seg0; seg < seg1; ++seg) {
#pragma unroll
        for (int dt = 0; dt < NC; ++dt) acc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
        const int kt1 = min((seg + 1) * p.seg_tiles, p.col_tiles);
        for (int kt = seg * p.seg_tiles; kt < kt1; ++kt) {
            __syncthreads();
            ss_stage_cols(p, (int64_t)kt * SS_TILE, sid, lqs);
            __syncthreads();
            ss_load_tile<DP>(Ts, p.table, p.D, sid, p.D);
            __syncthreads();
            dr_f32x4 s[4];
            ss_tile_dot<DP>(Ts, ureg, i16, g, s);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * t + 4 * g + r;
                    const int id = sid[jl];
                    const bool keep = rok && id >= 0 && !(p.rah && id == lab);
                    s[t][r] = keep ? c * expf((s[t][r] - lqs[jl]) - lse) : 0.f;
                }
            ss_tile_acc<DP>(Ts, s, i16, g, acc);
        }
        if constexpr (!SPLIT) {
#pragma unroll
            for (int dt = 0; dt < NC; ++dt) tot[dt] += acc[dt];
        }
    }
    if (!inb) return;
    if constexpr (SPLIT) {                    // 0 + acc is acc up to the sign of a zero, which the finalize kernel's 0 + ... absorbs
        float* dst = p.part_u + ((int64_t)grp * p.B + i) * p.D;
#pragma unroll
        for (int dt = 0; dt < NC; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            if (d0 < p.D) *reinterpret_cast<dr_f32x4*>(dst + d0) = acc[dt];
        }
    } else {
        const float gi = rok ? ss_row_g(c, p.t_in[i], lse) : 0.f;
        const float* trow = rok ? p.table + (int64_t)lab * p.D : nullptr;
#pragma unroll
        for (int dt = 0; dt < NC; ++dt) {
            const int d0 = 16 * dt + 4 * g;
            if (d0 >= p.D) continue;
            dr_f32x4 tr = {0.f, 0.f, 0.f, 0.f};
            if (trow) tr = *reinterpret_cast<const dr_f32x4*>(trow + d0);
            dr_f32x4 du, dtv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                du[e] = fmaf(gi, tr[e], tot[dt][e]);
                dtv[e] = gi * ureg[4 * dt + e];
            }
            *reinterpret_cast<dr_f32x4*>(p.d_u + i * p.ld_du + d0) = du;
            *reinterpret_cast<dr_f32x4*>(p.d_true + i * p.D + d0) = dtv;
        }
    }
}

template <int DP>
__global__ __launch_bounds__(256) void ss_bwd_rows_kernel(const SsP p) { ss_bwd_rows_body<DP, false>(p); }
template <int DP>
__global__ __launch_bounds__(256) void ss_bwd_rows_split_kernel(const SsP p) { ss_bwd_rows_body<DP, true>(p); }

// the split form's second launch: d_u = fma(g_i, table[label_i], 0 + part_0 + part_1 + ...), d_true = g_i u_i
__global__ __launch_bounds__(256) void ss_bwd_rows_finalize_kernel(const SsP p) {
    const int C4 = p.D / 4;
    const int64_t total = p.B * C4, stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / C4;
        const int d0 = (int)(e - i * C4) * 4;
        const int64_t lab = p.labels[i];
        dr_f32x4 du = {0.f, 0.f, 0.f, 0.f}, dtv = {0.f, 0.f, 0.f, 0.f};
        if (lab >= 0) {
            const float gi = ss_row_g(ss_row_c(p, i), p.t_in[i], p.lse_in[i]);
            for (int k = 0; k < p.groups; ++k) du += *reinterpret_cast<const dr_f32x4*>(p.part_u + ((int64_t)k * p.B + i) * p.D + d0);
            const dr_f32x4 tr = *reinterpret_cast<const dr_f32x4*>(p.table + lab * p.D + d0);
            const dr_f32x4 uv = *reinterpret_cast<const dr_f32x4*>(p.u + i * p.ld_u + d0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                du[q] = fmaf(gi, tr[q], du[q]);
                dtv[q] = gi * uv[q];
            }
        }
        *reinterpret_cast<dr_f32x4*>(p.d_u + i * p.ld_du + d0) = du;
        *reinterpret_cast<dr_f32x4*>(p.d_true + i * p.D + d0) = dtv;
    }
}

// ---- backward, the column-owning sweep: d_sampled -----------------------------------------------------------------------------------
// a block owns 64 sampled rows and walks the row tiles of its chunk
template <int DP>
__global__ __launch_bounds__(256) void ss_bwd_cols_kernel(const SsP p) {
    constexpr int LS = DP + 4, NC = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float ss_lds[];
    float* Us = ss_lds;
    int* labs = reinterpret_cast<int*>(Us + SS_TILE * LS);
    int* rows = labs + SS_TILE;
    float* lses = reinterpret_cast<float*>(rows + SS_TILE);
    float* cs = lses + SS_TILE;
    const int ct = blockIdx.x / p.chunks, ch = blockIdx.x - ct * p.chunks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int64_t j = (int64_t)ct * SS_TILE + wave * 16 + i16;
    const bool jin = j < p.S;
    const int64_t id64 = jin ? p.sampled[j] : -1;
    const bool cok = id64 >= 0;
    const int id = cok ? (int)id64 : -1;
    float vreg[DP / 4];
    ss_load_frag<DP>(vreg, cok ? p.table + (int64_t)id * p.D : nullptr, p.D, g);
    const float lq = (cok && p.lq_samp) ? p.lq_samp[j] : 0.f;
    dr_f32x4 acc[NC];
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) acc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t it1 = std::min<int64_t>((int64_t)(ch + 1) * p.chunk_tiles, p.row_tiles);
    for (int64_t it = (int64_t)ch * p.chunk_tiles; it < it1; ++it) {
        const int64_t i0 = it * SS_TILE;
        __syncthreads();
        if (threadIdx.x < SS_TILE) {
            const int64_t i = i0 + threadIdx.x;
            int lab = -1;
            float lse = 0.f, c = 0.f;
            if (i < p.B) {
                const int64_t l64 = p.labels[i];
                if (l64 >= 0) {
                    lab = (int)l64;
                    lse = p.lse_in[i];
                    c = ss_row_c(p, i);
                }
            }
            labs[threadIdx.x] = lab;
            rows[threadIdx.x] = lab >= 0 ? (int)threadIdx.x : -1;
            lses[threadIdx.x] = lse;
            cs[threadIdx.x] = c;
        }
        __syncthreads();
        ss_load_tile<DP>(Us, p.u + i0 * p.ld_u, p.ld_u, rows, p.D);
        __syncthreads();
        dr_f32x4 s[4];
        ss_tile_dot<DP>(Us, vreg, i16, g, s);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * t + 4 * g + r;
                const int lab = labs[il];
                const bool keep = cok && lab >= 0 && !(p.rah && id == lab);
                s[t][r] = keep ? cs[il] * expf((s[t][r] - lq) - lses[il]) : 0.f;
            }
        ss_tile_acc<DP>(Us, s, i16, g, acc);
    }
    if (!jin) return;
    float* dst = (p.chunks > 1 ? p.part_s + (int64_t)ch * p.S * p.D : p.d_samp) + j * p.D;
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 < p.D) *reinterpret_cast<dr_f32x4*>(dst + d0) = acc[dt];
    }
}

template <int DP>
constexpr size_t ss_lds_bytes() { return (size_t)(SS_TILE * (DP + 4) + SS_SMALL) * sizeof(float); }

#define SS_DISPATCH(st, KERNEL, grid, stream, p)                                                                                   \
    do {                                                                                                                           \
        if (p.D <= 16) st = dr_launch(KERNEL<16>, dim3(grid), dim3(256), ss_lds_bytes<16>(), dr_s(stream), p);                     \
        else if (p.D <= 32) st = dr_launch(KERNEL<32>, dim3(grid), dim3(256), ss_lds_bytes<32>(), dr_s(stream), p);                \
        else if (p.D <= 64) st = dr_launch(KERNEL<64>, dim3(grid), dim3(256), ss_lds_bytes<64>(), dr_s(stream), p);                \
        else if (p.D <= 128) st = dr_launch(KERNEL<128>, dim3(grid), dim3(256), ss_lds_bytes<128>(), dr_s(stream), p);             \
        else st = dr_launch(KERNEL<256>, dim3(grid), dim3(256), ss_lds_bytes<256>(), dr_s(stream), p);                             \
    } while (0)

inline int ss_domain(int64_t B, int64_t S, int64_t V, int32_t D) {
    if (B < 0 || S < 1 || V < 1) return DR_EINVAL;
    if (D % 4 != 0 || D < 4 || D > 256 || S >= (int64_t)1 << 31 || V >= (int64_t)1 << 31) return DR_ESHAPE;
    const SsPlan pl = ss_plan(B, S);
    if (pl.row_tiles * pl.groups >= (int64_t)1 << 31 || (int64_t)pl.col_tiles * pl.chunks >= (int64_t)1 << 31) return DR_ESHAPE;
    return DR_OK;
}

// workspace: [nseg][B] (max, sum) pairs | [groups][B][D] d_u partials when split | [chunks][S][D] d_sampled partials when chunked
inline int64_t ss_ml_floats(const SsPlan& pl, int64_t B) { return ((int64_t)pl.nseg * B * 2 + 3) / 4 * 4; }
inline int64_t ss_pu_floats(const SsPlan& pl, int64_t B, int32_t D) { return pl.groups > 1 ? (int64_t)pl.groups * B * D : 0; }
inline int64_t ss_ps_floats(const SsPlan& pl, int64_t S, int32_t D) { return pl.chunks > 1 ? (int64_t)pl.chunks * S * D : 0; }

inline void ss_fill(SsP& p, const SsPlan& pl, int64_t B, int64_t S, int32_t D) {
    p.B = B; p.S = (int32_t)S; p.D = D;
    p.row_tiles = pl.row_tiles; p.col_tiles = pl.col_tiles; p.nseg = pl.nseg; p.seg_tiles = pl.seg_tiles; p.groups = pl.groups;
    p.chunks = pl.chunks; p.chunk_tiles = pl.chunk_tiles;
}

}  // namespace

extern "C" int64_t dr_sampled_softmax_workspace_bytes(int64_t B, int64_t S, int32_t D) {
    const int st = ss_domain(B, S, 1, D);
    if (st != DR_OK) return st;
    const SsPlan pl = ss_plan(B, S);
    return (ss_ml_floats(pl, B) + ss_pu_floats(pl, B, D) + ss_ps_floats(pl, S, D)) * (int64_t)sizeof(float);
}

extern "C" int32_t dr_sampled_softmax_col_groups(int64_t B, int64_t S, int32_t D) {
    const int st = ss_domain(B, S, 1, D);
    return st != DR_OK ? st : ss_plan(B, S).groups;
}

extern "C" int32_t dr_sampled_softmax_row_chunks(int64_t B, int64_t S, int32_t D) {
    const int st = ss_domain(B, S, 1, D);
    return st != DR_OK ? st : ss_plan(B, S).chunks;
}

extern "C" int dr_sampled_softmax_fwd(const float* u, int64_t ld_u, const float* table, int64_t V, int32_t D, const int64_t* labels, int64_t B,
                                      const int64_t* sampled, int64_t S, const float* log_q_true, const float* log_q_sampled,
                                      const float* sample_weight, int32_t remove_accidental_hits, float* true_logit, float* row_lse,
                                      float* row_loss, float* scores, void* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    const int dom = ss_domain(B, S, V, D);
    if (dom != DR_OK) return dom;
    if (dr_bad_ld(ld_u, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!u || !table || !labels || !sampled || !true_logit || !row_lse || !row_loss || !workspace) return DR_EINVAL;
    if (!dr_aligned16(u) || !dr_aligned16(table) || !dr_aligned16(workspace)) return DR_EINVAL;
    if (workspace_bytes < dr_sampled_softmax_workspace_bytes(B, S, D)) return DR_EINVAL;
    const SsPlan pl = ss_plan(B, S);
    SsP p = {};
    ss_fill(p, pl, B, S, D);
    p.u = u; p.ld_u = ld_u; p.table = table; p.labels = labels; p.sampled = sampled; p.lq_true = log_q_true; p.lq_samp = log_q_sampled;
    p.weight = sample_weight; p.rah = remove_accidental_hits ? 1 : 0; p.t_out = true_logit; p.scores = scores;
    p.ml = static_cast<float*>(workspace);
    int st = DR_OK;
    SS_DISPATCH(st, ss_fwd_kernel, (unsigned)(pl.row_tiles * pl.groups), stream, p);
    if (st != DR_OK) return st;
    return dr_launch(ss_fwd_finalize_kernel, dim3(dr_grid_for(B, 256)), dim3(256), 0, dr_s(stream), p, row_lse, row_loss);
}

extern "C" int dr_sampled_softmax_bwd(const float* u, int64_t ld_u, const float* table, int64_t V, int32_t D, const int64_t* labels, int64_t B,
                                      const int64_t* sampled, int64_t S, const float* log_q_sampled, const float* sample_weight,
                                      int32_t remove_accidental_hits, float row_scale, const float* true_logit, const float* row_lse,
                                      float* d_u, int64_t ld_du, float* d_true, float* d_sampled, void* workspace,
                                      int64_t workspace_bytes, dr_stream_t stream) {
    const int dom = ss_domain(B, S, V, D);
    if (dom != DR_OK) return dom;
    if (dr_bad_ld(ld_u, D) || dr_bad_ld(ld_du, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!u || !table || !labels || !sampled || !true_logit || !row_lse || !d_u || !d_true || !d_sampled || !workspace) return DR_EINVAL;
    if (!dr_aligned16(u) || !dr_aligned16(table) || !dr_aligned16(d_u) || !dr_aligned16(d_true) || !dr_aligned16(d_sampled) ||
        !dr_aligned16(workspace))
        return DR_EINVAL;
    if (workspace_bytes < dr_sampled_softmax_workspace_bytes(B, S, D)) return DR_EINVAL;
    const SsPlan pl = ss_plan(B, S);
    SsP p = {};
    ss_fill(p, pl, B, S, D);
    p.u = u; p.ld_u = ld_u; p.table = table; p.labels = labels; p.sampled = sampled; p.lq_samp = log_q_sampled; p.weight = sample_weight;
    p.rah = remove_accidental_hits ? 1 : 0; p.row_scale = row_scale; p.t_in = true_logit; p.lse_in = row_lse;
    p.d_u = d_u; p.ld_du = ld_du; p.d_true = d_true; p.d_samp = d_sampled;
    p.part_u = static_cast<float*>(workspace) + ss_ml_floats(pl, B);
    p.part_s = p.part_u + ss_pu_floats(pl, B, D);
    int st = DR_OK;
    if (pl.groups > 1) SS_DISPATCH(st, ss_bwd_rows_split_kernel, (unsigned)(pl.row_tiles * pl.groups), stream, p);
    else SS_DISPATCH(st, ss_bwd_rows_kernel, (unsigned)pl.row_tiles, stream, p);
    if (st != DR_OK) return st;
    if (pl.groups > 1) {
        st = dr_launch(ss_bwd_rows_finalize_kernel, dim3(dr_grid_for(B * (D / 4), 256)), dim3(256), 0, dr_s(stream), p);
        if (st != DR_OK) return st;
    }
    SS_DISPATCH(st, ss_bwd_cols_kernel, (unsigned)((int64_t)pl.col_tiles * pl.chunks), stream, p);
    if (st != DR_OK) return st;
    if (pl.chunks > 1)
        return dr_sum_partials(p.part_s, pl.chunks, d_sampled, S * D, nullptr, 0, nullptr, 0, (unsigned)dr_grid_for(S * D, 256), dr_s(stream));
    return DR_OK;
}
