// The training loss of EBR (Huang et al., "Embedding-based Retrieval in Facebook Search", KDD 2020), which the reference's README lists
// and ships no code for: a margin ranking (triplet) loss over cosine similarities against a negative matrix the whole batch shares --
// in-batch: the positives of the other rows -- optionally over each row's num_hard hardest negatives.  dr_margin_rank_fwd / _bwd.
//
// A sibling of csrc/sampled_softmax.hip on the same tile helpers (dr_score_tile.h): the [B, S] score matrix is never written, every
// product is the fp32-input MFMA on the RAW rows, one wave owns 16 rows as the B operand of the transposed score tile.  The L2
// normalisation is folded in: a prologue leaves r = (max(sum x^2, eps))^(-1/2) and pi = [sum x^2 >= eps] of every row in the
// workspace, the score tile is (raw r_q) r_n, the second product takes the weights a_ij r_nj (a_ij r_qi in the column sweep), and
// the finalize kernels apply the derivative of the normalisation.  Metric dot is r = 1, pi = 0 through the same code.
//
// Order of every sum.  A lane (i16, g) of the wave that owns row i sees the columns 16t + 4g + r of every tile;
// it adds its terms (hinge, c, e) in column order over the tiles of a segment, the four lanes of a row are combined as
// (l0 + l1) + (l2 + l3) at the segment's end, and the segments are added in ascending order from 0 -- by the block that walked them
// or by the finalize kernel when every segment had a block of its own.  The hard-mode forward keeps a sorted (score, j) list of 8 per
// lane, merges the four lanes at the segment's end and the segments in the finalize kernel; the order of the list is total (score
// falling, then j rising), so the set does not depend on any of this; the hinge terms of the selected columns are then added in the
// same order as above (mr_fwd_finalize_kernel), which makes num_hard >= #kept the bits of num_hard == 0.  d_neg and f_j are summed
// over row chunks, the partials added in chunk order (dr_sum_partials.h).  No float atomics, no waiting between workgroups.
#include "dr_common.h"
#include "dr_sum_partials.h"
#include "dr_score_tile.h"
#include <math.h>
#include <limits.h>
#include <algorithm>

// No contraction in this file: the score (raw r_q) r_n and the hinge h = (margin - t) + s are evaluated in the forward, in its finalize
// kernel (from a stored score, where nothing could be fused), in the row sweep and in the column sweep, and all of them must round
// alike -- both sweeps decide every hinge as the forward did, and a list as long as the kept columns gives the bits of no list.  With
// the compiler free to fuse a multiply into an add in some of those places and not in others that would hold by luck.  Where a fused
// multiply-add is meant it is written as fmaf.
#pragma clang fp contract(off)

namespace {

constexpr int MR_K = DR_MARGIN_RANK_MAX_HARD;
constexpr int MR_SMALL = 1024;                      // floats of per-row / per-column scalars behind the tile
static_assert(MR_K == 8, "the lists and their sorting network are written for 8 entries");

struct MrPlan {
    int64_t row_tiles;
    int32_t col_tiles, nseg, seg_tiles, groups, chunks, chunk_tiles;
};

// pure functions of (B, S): no device query, so the bits do not depend on the machine
inline MrPlan mr_plan(int64_t B, int64_t S) {
    MrPlan pl;
    pl.row_tiles = (B + SS_TILE - 1) / SS_TILE;
    pl.col_tiles = (int32_t)((S + SS_TILE - 1) / SS_TILE);
    int64_t nseg = std::min<int64_t>(DR_MARGIN_RANK_MAX_GROUPS, (S + DR_MARGIN_RANK_COL_GROUP - 1) / DR_MARGIN_RANK_COL_GROUP);
    pl.seg_tiles = (int32_t)((pl.col_tiles + nseg - 1) / nseg);
    pl.nseg = (pl.col_tiles + pl.seg_tiles - 1) / pl.seg_tiles;
    // one block per (row tile, segment) while the row tiles alone leave CUs idle; else one block walks every segment
    pl.groups = pl.row_tiles <= DR_MARGIN_RANK_SPLIT_TILES ? pl.nseg : 1;
    const int64_t want = std::max<int64_t>(1, (512 + pl.col_tiles - 1) / pl.col_tiles);
    int64_t chunks = std::min<int64_t>(std::min<int64_t>(DR_MARGIN_RANK_MAX_CHUNKS, want),
                                       std::max<int64_t>(1, (B + DR_MARGIN_RANK_ROW_CHUNK - 1) / DR_MARGIN_RANK_ROW_CHUNK));
    const int64_t ct = std::max<int64_t>(1, (pl.row_tiles + chunks - 1) / chunks);
    pl.chunk_tiles = (int32_t)std::min<int64_t>(ct, INT32_MAX);
    pl.chunks = (int32_t)std::max<int64_t>(1, (pl.row_tiles + ct - 1) / ct);
    return pl;
}

struct MrP {
    const float *q, *pos, *neg, *weight, *t_in;
    const int64_t *pos_ids, *neg_ids;
    const int32_t* hard_in;
    float *t_out, *row_loss, *scores, *d_q, *d_pos, *d_neg;
    int32_t *row_active, *hard_out;
    float *rq, *piq, *rp, *pip, *rn, *pin;          // the prologue's inverse norms and projection flags
    float *seg_loss, *seg_ls, *ce, *part_q, *part_n, *nsum, *fsum;
    int32_t *seg_act, *seg_li;
    int64_t ld_q, ld_p, ld_n, ld_dq, B, row_tiles, S4;          // S4: S rounded up to 4 (it can pass 2^31 - 1 where S does not)
    int32_t S, D, K, metric, in_batch, col_tiles, nseg, seg_tiles, groups, chunks, chunk_tiles;
    float margin, eps, row_scale;
};

__device__ __forceinline__ bool mr_row_valid(const MrP& p, int64_t i) { return i < p.B && (!p.pos_ids || p.pos_ids[i] >= 0); }
__device__ __forceinline__ bool mr_col_ok(const MrP& p, int64_t j) { return j < p.S && (!p.neg_ids || p.neg_ids[j] >= 0); }
__device__ __forceinline__ float mr_row_c(const MrP& p, int64_t i) { return p.weight ? p.row_scale * p.weight[i] : p.row_scale; }
// (l0 + l1) + (l2 + l3) over the four lanes (g = 0 .. 3) that share a row, on each of them
__device__ __forceinline__ float mr_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// ---- prologue: r and pi of every row of q, pos and neg; 16 lanes per row -------------------------------------------------------------
__global__ __launch_bounds__(256) void mr_norms_kernel(const MrP p) {
    const int64_t total = 2 * p.B + p.S, stride = (int64_t)gridDim.x * 16;
    const int l16 = threadIdx.x & 15;
    for (int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); row < total; row += stride) {
        const int which = row < p.B ? 0 : row < 2 * p.B ? 1 : 2;
        const int64_t idx = which == 0 ? row : which == 1 ? row - p.B : row - 2 * p.B;
        const bool ok = which == 2 ? mr_col_ok(p, idx) : mr_row_valid(p, idx);
        const float* src = which == 0 ? p.q + idx * p.ld_q : which == 1 ? p.pos + idx * p.ld_p : p.neg + idx * p.ld_n;
        float ss = 0.f;
        if (ok && p.metric == 1) {
            for (int d = 4 * l16; d < p.D; d += 64) {
                const dr_f32x4 v = *reinterpret_cast<const dr_f32x4*>(src + d);
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = fmaf(v[e], v[e], ss);
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        float r = 0.f, pi = 0.f;
        if (ok) {
            r = p.metric == 1 ? 1.f / sqrtf(fmaxf(ss, p.eps)) : 1.f;
            pi = (p.metric == 1 && ss >= p.eps) ? 1.f : 0.f;
        }
        if (l16 == 0) {
            (which == 0 ? p.rq : which == 1 ? p.rp : p.rn)[idx] = r;
            (which == 0 ? p.piq : which == 1 ? p.pip : p.pin)[idx] = pi;
        }
    }
}

// ---- the sorted list of 8 (score, j): score falling, ties to the smaller j; j < 0 is an empty slot ------------------------------------
__device__ __forceinline__ bool mr_beats(float v, int j, float s, int sj) { return sj < 0 || v > s || (v == s && j < sj); }
__device__ __forceinline__ void mr_insert(float (&ls)[MR_K], int (&li)[MR_K], float v, int j) {
    if (j < 0 || !mr_beats(v, j, ls[MR_K - 1], li[MR_K - 1])) return;
#pragma unroll
    for (int k = 0; k < MR_K; ++k) {
        const bool b = j >= 0 && mr_beats(v, j, ls[k], li[k]);
        const float ts = ls[k];
        const int ti = li[k];
        ls[k] = b ? v : ts;
        li[k] = b ? j : ti;
        v = b ? ts : v;
        j = b ? ti : j;
    }
}

// the staging of a column tile: which rows of neg to load, their inverse norms and ids
struct MrCols {
    int* sel;           // [64] the row of the tile to load, -1: past S or a padding id (never read)
    float* rn;          // [64]
    int64_t* nid;       // [64]
};
__device__ __forceinline__ MrCols mr_cols_at(float* small) {
    MrCols c;
    c.nid = reinterpret_cast<int64_t*>(small);
    c.sel = reinterpret_cast<int*>(small + 2 * SS_TILE);
    c.rn = small + 3 * SS_TILE;
    return c;
}
__device__ __forceinline__ void mr_stage_cols(const MrP& p, int64_t j0, const MrCols& c) {
    if (threadIdx.x < SS_TILE) {
        const int64_t j = j0 + threadIdx.x;
        const bool ok = mr_col_ok(p, j);
        c.sel[threadIdx.x] = ok ? (int)threadIdx.x : -1;
        c.rn[threadIdx.x] = ok ? p.rn[j] : 0.f;
        c.nid[threadIdx.x] = (ok && p.neg_ids) ? p.neg_ids[j] : 0;
    }
}

// what a lane of a row-owning wave knows of its row
struct MrRow {
    int64_t i, pid;
    bool inb, valid;
    float rq, t, mt;
};
template <int DP>
__device__ __forceinline__ MrRow mr_own_row(const MrP& p, int64_t i, float (&qreg)[DP / 4], int i16, int g, bool fwd) {
    MrRow r;
    r.i = i;
    r.inb = i < p.B;
    r.valid = mr_row_valid(p, i);
    r.pid = (r.valid && p.pos_ids) ? p.pos_ids[i] : 0;
    ss_load_frag<DP>(qreg, r.valid ? p.q + i * p.ld_q : nullptr, p.D, g);
    r.rq = r.valid ? p.rq[i] : 0.f;
    if (fwd) {
        const float raw = ss_true_dot<DP>(r.valid ? p.pos + i * p.ld_p : nullptr, qreg, p.D, i16, g);
        r.t = r.valid ? (raw * r.rq) * p.rp[i] : 0.f;
    } else {
        r.t = r.valid ? p.t_in[i] : 0.f;
    }
    r.mt = p.margin - r.t;
    return r;
}
__device__ __forceinline__ bool mr_keep(const MrP& p, const MrRow& r, const MrCols& c, int jl, int64_t j) {
    return r.valid && c.sel[jl] >= 0 && !(p.in_batch && j == r.i) && !(p.pos_ids && p.neg_ids && c.nid[jl] == r.pid);
}

// ---- forward: a block owns 64 rows of q and walks the column tiles of its segments ---------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void mr_fwd_kernel(const MrP p) {
    constexpr int LS = DP + 4;
    extern __shared__ __attribute__((aligned(16))) float mr_lds[];
    float* Ts = mr_lds;
    const MrCols cols = mr_cols_at(Ts + SS_TILE * LS);
    const int64_t rt = blockIdx.x / p.groups;
    const int grp = (int)(blockIdx.x - rt * p.groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    float qreg[DP / 4];
    const MrRow row = mr_own_row<DP>(p, rt * SS_TILE + wave * 16 + i16, qreg, i16, g, true);
    if (grp == 0 && row.inb && g == 0) p.t_out[row.i] = row.t;
    const int seg0 = p.groups == 1 ? 0 : grp, seg1 = p.groups == 1 ? p.nseg : grp + 1;
    for (int seg = seg0; seg < seg1; ++seg) {
        float l = 0.f;
        int cnt = 0;
        float ls[MR_K];
        int li[MR_K];
#pragma unroll
        for (int k = 0; k < MR_K; ++k) {
            ls[k] = -INFINITY;
            li[k] = -1;
        }
        const int kt1 = min((seg + 1) * p.seg_tiles, p.col_tiles);
        for (int kt = seg * p.seg_tiles; kt < kt1; ++kt) {
            const int64_t j0 = (int64_t)kt * SS_TILE;
            __syncthreads();
            mr_stage_cols(p, j0, cols);
            __syncthreads();
            ss_load_tile<DP>(Ts, p.neg + j0 * p.ld_n, p.ld_n, cols.sel, p.D);
            __syncthreads();
            dr_f32x4 s[4];
            ss_tile_dot<DP>(Ts, qreg, i16, g, s);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * t + 4 * g + r;
                    const int64_t j = j0 + jl;
                    const bool keep = mr_keep(p, row, cols, jl, j);
                    const float sc = (s[t][r] * row.rq) * cols.rn[jl];
                    if (p.scores && row.inb && j < p.S) p.scores[row.i * p.S + j] = keep ? sc : -INFINITY;
                    if (p.K == 0) {
                        const float h = row.mt + sc;
                        if (keep && h > 0.f) {
                            l += h;
                            ++cnt;
                        }
                    } else if (keep) {
                        mr_insert(ls, li, sc, (int)j);
                    }
                }
        }
        if (p.K == 0) {
            l = mr_sum4(l);
            cnt += __shfl_xor(cnt, 16, 64);
            cnt += __shfl_xor(cnt, 32, 64);
            if (row.inb && g == 0) {
                p.seg_loss[(int64_t)seg * p.B + row.i] = l;
                p.seg_act[(int64_t)seg * p.B + row.i] = cnt;
            }
        } else {
            // the four lanes of a row: every lane takes the other three lists (the order of the list is total: the same list on each)
            float os[MR_K];
            int oi[MR_K];
#pragma unroll
            for (int k = 0; k < MR_K; ++k) {
                os[k] = ls[k];
                oi[k] = li[k];
            }
#pragma unroll
            for (int x = 16; x < 64; x += 16)
#pragma unroll
                for (int k = 0; k < MR_K; ++k) mr_insert(ls, li, __shfl_xor(os[k], x, 64), __shfl_xor(oi[k], x, 64));
            if (row.inb && g == 0) {
                float* dl = p.seg_ls + ((int64_t)seg * p.B + row.i) * MR_K;
                int32_t* di = p.seg_li + ((int64_t)seg * p.B + row.i) * MR_K;
#pragma unroll
                for (int k = 0; k < MR_K; ++k) {
                    dl[k] = ls[k];
                    di[k] = li[k];
                }
            }
        }
    }
}

// row_loss, row_active and hard_idx from the segments' partials, in segment order
__global__ __launch_bounds__(256) void mr_fwd_finalize_kernel(const MrP p) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.B; i += stride) {
        const bool valid = mr_row_valid(p, i);
        float loss = 0.f;
        int act = 0;
        if (p.K == 0) {
            if (valid)
                for (int seg = 0; seg < p.nseg; ++seg) {
                    loss += p.seg_loss[(int64_t)seg * p.B + i];
                    act += p.seg_act[(int64_t)seg * p.B + i];
                }
        } else {
            float ls[MR_K];
            int li[MR_K];
#pragma unroll
            for (int k = 0; k < MR_K; ++k) {
                ls[k] = -INFINITY;
                li[k] = -1;
            }
            if (valid)
                for (int seg = 0; seg < p.nseg; ++seg) {
                    const float* sl = p.seg_ls + ((int64_t)seg * p.B + i) * MR_K;
                    const int32_t* si = p.seg_li + ((int64_t)seg * p.B + i) * MR_K;
#pragma unroll
                    for (int k = 0; k < MR_K; ++k) mr_insert(ls, li, sl[k], si[k]);
                }
            const float mt = p.margin - p.t_out[i];
            float hv[MR_K];
            int key[MR_K];
#pragma unroll
            for (int k = 0; k < MR_K; ++k) {
                const bool in = k < p.K && li[k] >= 0;
                if (k < p.K) p.hard_out[i * p.K + k] = in ? li[k] : -1;
                const float h = mt + ls[k];
                const bool on = in && h > 0.f;
                hv[k] = on ? h : 0.f;
                key[k] = on ? li[k] : INT_MAX;
                act += on ? 1 : 0;
            }
            // the hinge terms in the order the num_hard == 0 form adds them: by column (a sorting network on j), per lane class
            // g = (j / 4) % 4, the four classes as (l0 + l1) + (l2 + l3) per segment, the segments from 0 upwards
#pragma unroll
            for (int a = 0; a < MR_K - 1; ++a)
#pragma unroll
                for (int b = 0; b < MR_K - 1 - a; ++b) {
                    const bool sw = key[b] > key[b + 1];
                    const int k0 = key[b], k1 = key[b + 1];
                    const float h0 = hv[b], h1 = hv[b + 1];
                    key[b] = sw ? k1 : k0;
                    key[b + 1] = sw ? k0 : k1;
                    hv[b] = sw ? h1 : h0;
                    hv[b + 1] = sw ? h0 : h1;
                }
            if (act > 0)
                for (int seg = 0; seg < p.nseg; ++seg) {
                    float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
#pragma unroll
                    for (int k = 0; k < MR_K; ++k) {
                        if (key[k] == INT_MAX || (key[k] / SS_TILE) / p.seg_tiles != seg) continue;
                        const int gg = (key[k] >> 2) & 3;
                        if (gg == 0) l0 += hv[k];
                        else if (gg == 1) l1 += hv[k];
                        else if (gg == 2) l2 += hv[k];
                        else l3 += hv[k];
                    }
                    loss += (l0 + l1) + (l2 + l3);
                }
        }
        p.row_loss[i] = valid ? (p.weight ? p.weight[i] : 1.f) * loss : 0.f;
        p.row_active[i] = act;
    }
}

// ---- backward, the row-owning sweep: sum_j a_ij r_nj n_j, c_i and e_i ------------------------------------------------------------------
// tot = ((0 + seg_0) + seg_1) + ...  SPLIT: one block per (row tile, segment); the segment's sums are the partials, and
// mr_bwd_rows_finalize_kernel adds them in the same order.  The other form leaves its totals in d_q and ce for the same kernel.
template <int DP, bool SPLIT>
__device__ __forceinline__ void mr_bwd_rows_body(const MrP& p) {
    constexpr int LS = DP + 4, NC = DP / 16, NT = SPLIT ? 1 : NC;
    extern __shared__ __attribute__((aligned(16))) float mr_lds[];
    float* Ts = mr_lds;
    const MrCols cols = mr_cols_at(Ts + SS_TILE * LS);
    const int64_t rt = blockIdx.x / p.groups;
    const int grp = (int)(blockIdx.x - rt * p.groups);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    float qreg[DP / 4];
    const MrRow row = mr_own_row<DP>(p, rt * SS_TILE + wave * 16 + i16, qreg, i16, g, false);
    const float cw = row.valid ? mr_row_c(p, row.i) : 0.f;
    int hi[MR_K];
#pragma unroll
    for (int k = 0; k < MR_K; ++k) hi[k] = (row.valid && k < p.K) ? p.hard_in[row.i * p.K + k] : -1;
    dr_f32x4 tot[NT], acc[NC];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) tot[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    float c_tot = 0.f, e_tot = 0.f;
    const int seg0 = SPLIT ? grp : 0, seg1 = SPLIT ? grp + 1 : p.nseg;
    for (int seg = seg0; seg < seg1; ++seg) {
#pragma unroll
        for (int dt = 0; dt < NC; ++dt) acc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
        float cl = 0.f, el = 0.f;
        const int kt1 = min((seg + 1) * p.seg_tiles, p.col_tiles);
        for (int kt = seg * p.seg_tiles; kt < kt1; ++kt) {
            const int64_t j0 = (int64_t)kt * SS_TILE;
            __syncthreads();
            mr_stage_cols(p, j0, cols);
            __syncthreads();
            ss_load_tile<DP>(Ts, p.neg + j0 * p.ld_n, p.ld_n, cols.sel, p.D);
            __syncthreads();
            dr_f32x4 s[4];
            ss_tile_dot<DP>(Ts, qreg, i16, g, s);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jl = 16 * t + 4 * g + r;
                    const int64_t j = j0 + jl;
                    bool member = p.K == 0;
#pragma unroll
                    for (int k = 0; k < MR_K; ++k) member |= hi[k] == (int)j;
                    const float sc = (s[t][r] * row.rq) * cols.rn[jl];
                    const float h = row.mt + sc;
                    const float a = (mr_keep(p, row, cols, jl, j) && member && h > 0.f) ? cw : 0.f;
                    cl += a;
                    el += a * sc;
                    s[t][r] = a * cols.rn[jl];
                }
            ss_tile_acc<DP>(Ts, s, i16, g, acc);
        }
        cl = mr_sum4(cl);
        el = mr_sum4(el);
        if constexpr (SPLIT) {
            c_tot = cl;
            e_tot = el;
        } else {
            c_tot += cl;
            e_tot += el;
#pragma unroll
            for (int dt = 0; dt < NC; ++dt) tot[dt] += acc[dt];
        }
    }
    if (!row.inb) return;
    float* dst = SPLIT ? p.part_q + ((int64_t)grp * p.B + row.i) * p.D : p.d_q + row.i * p.ld_dq;
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 < p.D) *reinterpret_cast<dr_f32x4*>(dst + d0) = SPLIT ? acc[dt] : tot[SPLIT ? 0 : dt];
    }
    if (g == 0) {
        float* ce = p.ce + 2 * ((int64_t)(SPLIT ? grp : 0) * p.B + row.i);
        ce[0] = c_tot;
        ce[1] = e_tot;
    }
}

template <int DP>
__global__ __launch_bounds__(256) void mr_bwd_rows_kernel(const MrP p) { mr_bwd_rows_body<DP, false>(p); }
template <int DP>
__global__ __launch_bounds__(256) void mr_bwd_rows_split_kernel(const MrP p) { mr_bwd_rows_body<DP, true>(p); }

// d_q = r_q [ sum - c p^ - pi_q (e - c t) q^ ],  d_pos = -c r_p (q^ - pi_p t p^); the sums are 0 + part_0 + part_1 + ... of the split
// form or what the other form left in d_q and ce
__global__ __launch_bounds__(256) void mr_bwd_rows_finalize_kernel(const MrP p) {
    const int C4 = p.D / 4;
    const int64_t total = p.B * C4, stride = (int64_t)gridDim.x * 256;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += stride) {
        const int64_t i = x / C4;
        const int d0 = (int)(x - i * C4) * 4;
        dr_f32x4 dq = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
        if (mr_row_valid(p, i)) {
            dr_f32x4 sum = {0.f, 0.f, 0.f, 0.f};
            float c = 0.f, e = 0.f;
            if (p.groups > 1) {
                for (int k = 0; k < p.groups; ++k) {
                    sum += *reinterpret_cast<const dr_f32x4*>(p.part_q + ((int64_t)k * p.B + i) * p.D + d0);
                    c += p.ce[2 * ((int64_t)k * p.B + i)];
                    e += p.ce[2 * ((int64_t)k * p.B + i) + 1];
                }
            } else {
                sum = *reinterpret_cast<const dr_f32x4*>(p.d_q + i * p.ld_dq + d0);
                c = p.ce[2 * i];
                e = p.ce[2 * i + 1];
            }
            const float t = p.t_in[i], rq = p.rq[i], rp = p.rp[i];
            const float coef = p.piq[i] * (e - c * t), pt = p.pip[i] * t, mc = -c * rp;
            const dr_f32x4 qv = *reinterpret_cast<const dr_f32x4*>(p.q + i * p.ld_q + d0);
            const dr_f32x4 pv = *reinterpret_cast<const dr_f32x4*>(p.pos + i * p.ld_p + d0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float qh = qv[u] * rq, ph = pv[u] * rp;
                dq[u] = rq * ((sum[u] - c * ph) - coef * qh);
                dp[u] = mc * (qh - pt * ph);
            }
        }
        *reinterpret_cast<dr_f32x4*>(p.d_q + i * p.ld_dq + d0) = dq;
        *reinterpret_cast<dr_f32x4*>(p.d_pos + i * p.D + d0) = dp;
    }
}

// ---- backward, the column-owning sweep: sum_i a_ij r_qi q_i and f_j ---------------------------------------------------------------------
// a block owns 64 rows of neg and walks the row tiles of its chunk
template <int DP>
__global__ __launch_bounds__(256) void mr_bwd_cols_kernel(const MrP p) {
    constexpr int LS = DP + 4, NC = DP / 16;
    extern __shared__ __attribute__((aligned(16))) float mr_lds[];
    float* Us = mr_lds;
    float* small = Us + SS_TILE * LS;
    int64_t* pids = reinterpret_cast<int64_t*>(small);
    int* rows = reinterpret_cast<int*>(small + 2 * SS_TILE);
    float* rqs = small + 3 * SS_TILE;
    float* mts = small + 4 * SS_TILE;
    float* cws = small + 5 * SS_TILE;
    int* hard = reinterpret_cast<int*>(small + 6 * SS_TILE);          // [64][8]
    const int ct = blockIdx.x / p.chunks, ch = blockIdx.x - ct * p.chunks;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int64_t j = (int64_t)ct * SS_TILE + wave * 16 + i16;
    const bool cok = mr_col_ok(p, j);
    const int64_t nid = (cok && p.neg_ids) ? p.neg_ids[j] : 0;
    float nreg[DP / 4];
    ss_load_frag<DP>(nreg, cok ? p.neg + j * p.ld_n : nullptr, p.D, g);
    const float rn = cok ? p.rn[j] : 0.f;
    dr_f32x4 acc[NC];
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) acc[dt] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    float fl = 0.f;
    const int64_t it1 = std::min<int64_t>((int64_t)(ch + 1) * p.chunk_tiles, p.row_tiles);
    for (int64_t it = (int64_t)ch * p.chunk_tiles; it < it1; ++it) {
        const int64_t i0 = it * SS_TILE;
        __syncthreads();
        if (threadIdx.x < SS_TILE) {
            const int64_t i = i0 + threadIdx.x;
            const bool valid = mr_row_valid(p, i);
            rows[threadIdx.x] = valid ? (int)threadIdx.x : -1;
            pids[threadIdx.x] = (valid && p.pos_ids) ? p.pos_ids[i] : 0;
            rqs[threadIdx.x] = valid ? p.rq[i] : 0.f;
            mts[threadIdx.x] = valid ? p.margin - p.t_in[i] : 0.f;
            cws[threadIdx.x] = valid ? mr_row_c(p, i) : 0.f;
            for (int k = 0; k < p.K; ++k) hard[threadIdx.x * MR_K + k] = valid ? p.hard_in[i * p.K + k] : -1;
        }
        __syncthreads();
        ss_load_tile<DP>(Us, p.q + i0 * p.ld_q, p.ld_q, rows, p.D);
        __syncthreads();
        dr_f32x4 s[4];
        ss_tile_dot<DP>(Us, nreg, i16, g, s);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * t + 4 * g + r;
                bool member = p.K == 0;
                for (int k = 0; k < p.K; ++k) member |= hard[il * MR_K + k] == (int)j;
                const bool keep = cok && rows[il] >= 0 && !(p.in_batch && i0 + il == j) && !(p.pos_ids && p.neg_ids && nid == pids[il]);
                const float sc = (s[t][r] * rqs[il]) * rn;
                const float h = mts[il] + sc;
                const float a = (keep && member && h > 0.f) ? cws[il] : 0.f;
                fl += a * sc;
                s[t][r] = a * rqs[il];
            }
        ss_tile_acc<DP>(Us, s, i16, g, acc);
    }
    fl = mr_sum4(fl);
    float* base = p.chunks > 1 ? p.part_n + (int64_t)ch * ((int64_t)p.S * p.D + p.S4) : p.nsum;
    if (g == 0 && j < p.S4) base[(int64_t)p.S * p.D + j] = fl;
    if (j >= p.S) return;
#pragma unroll
    for (int dt = 0; dt < NC; ++dt) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 < p.D) *reinterpret_cast<dr_f32x4*>(base + j * p.D + d0) = acc[dt];
    }
}

// d_neg = r_n [ sum - pi_n f n^ ] from nsum | fsum (the chunks' partials already added in chunk order)
__global__ __launch_bounds__(256) void mr_bwd_cols_finalize_kernel(const MrP p) {
    const int C4 = p.D / 4;
    const int64_t total = (int64_t)p.S * C4, stride = (int64_t)gridDim.x * 256;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += stride) {
        const int64_t j = x / C4;
        const int d0 = (int)(x - j * C4) * 4;
        dr_f32x4 dn = {0.f, 0.f, 0.f, 0.f};
        if (mr_col_ok(p, j)) {
            const dr_f32x4 sum = *reinterpret_cast<const dr_f32x4*>(p.nsum + j * p.D + d0);
            const dr_f32x4 nv = *reinterpret_cast<const dr_f32x4*>(p.neg + j * p.ld_n + d0);
            const float rn = p.rn[j], pf = p.pin[j] * p.fsum[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) dn[u] = rn * (sum[u] - pf * (nv[u] * rn));
        }
        *reinterpret_cast<dr_f32x4*>(p.d_neg + j * p.D + d0) = dn;
    }
}

template <int DP>
constexpr size_t mr_lds_bytes() { return (size_t)(SS_TILE * (DP + 4) + MR_SMALL) * sizeof(float); }

// no 16-wide instance: at DP 16 the compiler's schedule of the row sweep spills (190 VGPRs to scratch); D <= 16 runs the 32-wide form,
// whose zero columns add 0 * 0 to every chain
#define MR_DISPATCH(st, KERNEL, grid, stream, p)                                                                                   \
    do {                                                                                                                           \
        if (p.D <= 32) st = dr_launch(KERNEL<32>, dim3(grid), dim3(256), mr_lds_bytes<32>(), dr_s(stream), p);                \
        else if (p.D <= 64) st = dr_launch(KERNEL<64>, dim3(grid), dim3(256), mr_lds_bytes<64>(), dr_s(stream), p);                \
        else if (p.D <= 128) st = dr_launch(KERNEL<128>, dim3(grid), dim3(256), mr_lds_bytes<128>(), dr_s(stream), p);             \
        else st = dr_launch(KERNEL<256>, dim3(grid), dim3(256), mr_lds_bytes<256>(), dr_s(stream), p);                             \
    } while (0)

inline int mr_domain(int64_t B, int64_t S, int32_t D) {
    if (B < 0 || S < 1) return DR_EINVAL;
    if (D % 4 != 0 || D < 4 || D > 256 || S >= (int64_t)1 << 31) return DR_ESHAPE;
    const MrPlan pl = mr_plan(B, S);
    if (pl.row_tiles * pl.groups >= (int64_t)1 << 31 || (int64_t)pl.col_tiles * pl.chunks >= (int64_t)1 << 31) return DR_ESHAPE;
    return DR_OK;
}
inline int mr_options(int64_t B, int64_t S, int32_t metric, int32_t in_batch, int32_t num_hard) {
    if (num_hard < 0 || num_hard > MR_K || (metric != 0 && metric != 1)) return DR_EINVAL;
    if (in_batch && S != B) return DR_ESHAPE;
    return DR_OK;
}

inline int64_t mr_up4(int64_t n) { return (n + 3) / 4 * 4; }

// the workspace, in floats: r and pi of q, pos, neg | the forward's segment partials | the backward's partials
struct MrWs {
    int64_t rq, piq, rp, pip, rn, pin, seg_loss, seg_act, seg_ls, seg_li, ce, part_q, part_n, nsum, total;
};
inline MrWs mr_ws(const MrPlan& pl, int64_t B, int64_t S, int32_t D, int32_t K) {
    MrWs w;
    int64_t at = 0;
    const int64_t B4 = mr_up4(B), S4 = mr_up4(S);
    w.rq = at; at += B4;
    w.piq = at; at += B4;
    w.rp = at; at += B4;
    w.pip = at; at += B4;
    w.rn = at; at += S4;
    w.pin = at; at += S4;
    w.seg_loss = at; at += mr_up4((int64_t)pl.nseg * B);
    w.seg_act = at; at += mr_up4((int64_t)pl.nseg * B);
    w.seg_ls = at; at += K > 0 ? (int64_t)pl.nseg * B * MR_K : 0;
    w.seg_li = at; at += K > 0 ? (int64_t)pl.nseg * B * MR_K : 0;
    w.ce = at; at += mr_up4((int64_t)pl.groups * B * 2);
    w.part_q = at; at += pl.groups > 1 ? (int64_t)pl.groups * B * D : 0;
    w.part_n = at; at += pl.chunks > 1 ? (int64_t)pl.chunks * (S * D + S4) : 0;
    w.nsum = at; at += S * D + S4;
    w.total = at;
    return w;
}

struct MrArgs {
    const float *q, *pos, *neg, *weight;
    const int64_t *pos_ids, *neg_ids;
    int64_t ld_q, ld_p, ld_n, B, S;
    int32_t D, metric, in_batch, K;
    float margin, eps;
};

// the checks both entry points share and the parameter block they start from; DR_OK with B == 0 is the caller's early return
inline int mr_prepare(const MrArgs& a, void* workspace, int64_t workspace_bytes, MrP& p, MrPlan& pl) {
    const int dom = mr_domain(a.B, a.S, a.D);
    if (dom != DR_OK) return dom;
    const int opt = mr_options(a.B, a.S, a.metric, a.in_batch, a.K);
    if (opt != DR_OK) return opt;
    if (dr_bad_ld(a.ld_q, a.D) || dr_bad_ld(a.ld_p, a.D) || dr_bad_ld(a.ld_n, a.D)) return DR_EINVAL;
    if (a.B == 0) return DR_OK;
    if (!a.q || !a.pos || !a.neg || !workspace) return DR_EINVAL;
    if (!dr_aligned16(a.q) || !dr_aligned16(a.pos) || !dr_aligned16(a.neg) || !dr_aligned16(workspace)) return DR_EINVAL;
    if (workspace_bytes < dr_margin_rank_workspace_bytes(a.B, a.S, a.D, a.K)) return DR_EINVAL;
    pl = mr_plan(a.B, a.S);
    const MrWs w = mr_ws(pl, a.B, a.S, a.D, a.K);
    float* ws = static_cast<float*>(workspace);
    p = MrP{};
    p.q = a.q; p.pos = a.pos; p.neg = a.neg; p.weight = a.weight; p.pos_ids = a.pos_ids; p.neg_ids = a.neg_ids;
    p.ld_q = a.ld_q; p.ld_p = a.ld_p; p.ld_n = a.ld_n; p.B = a.B; p.S = (int32_t)a.S; p.S4 = mr_up4(a.S);
    p.D = a.D; p.K = a.K; p.metric = a.metric; p.in_batch = a.in_batch ? 1 : 0; p.margin = a.margin; p.eps = a.eps;
    p.row_tiles = pl.row_tiles; p.col_tiles = pl.col_tiles; p.nseg = pl.nseg; p.seg_tiles = pl.seg_tiles; p.groups = pl.groups;
    p.chunks = pl.chunks; p.chunk_tiles = pl.chunk_tiles;
    p.rq = ws + w.rq; p.piq = ws + w.piq; p.rp = ws + w.rp; p.pip = ws + w.pip; p.rn = ws + w.rn; p.pin = ws + w.pin;
    p.seg_loss = ws + w.seg_loss; p.seg_act = reinterpret_cast<int32_t*>(ws + w.seg_act);
    p.seg_ls = ws + w.seg_ls; p.seg_li = reinterpret_cast<int32_t*>(ws + w.seg_li);
    p.ce = ws + w.ce; p.part_q = ws + w.part_q; p.part_n = ws + w.part_n; p.nsum = ws + w.nsum;
    p.fsum = p.nsum + a.S * a.D;
    return DR_OK;
}

}  // namespace

extern "C" int64_t dr_margin_rank_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t num_hard) {
    const int st = mr_domain(B, S, D);
    if (st != DR_OK) return st;
    if (num_hard < 0 || num_hard > MR_K) return DR_EINVAL;
    return mr_ws(mr_plan(B, S), B, S, D, num_hard).total * (int64_t)sizeof(float);
}

extern "C" int32_t dr_margin_rank_col_groups(int64_t B, int64_t S, int32_t D) {
    const int st = mr_domain(B, S, D);
    return st != DR_OK ? st : mr_plan(B, S).groups;
}

extern "C" int32_t dr_margin_rank_col_segments(int64_t B, int64_t S, int32_t D) {
    const int st = mr_domain(B, S, D);
    return st != DR_OK ? st : mr_plan(B, S).nseg;
}

extern "C" int32_t dr_margin_rank_row_chunks(int64_t B, int64_t S, int32_t D) {
    const int st = mr_domain(B, S, D);
    return st != DR_OK ? st : mr_plan(B, S).chunks;
}

extern "C" int dr_margin_rank_fwd(const float* q, int64_t ld_q, const float* pos, int64_t ld_p, const float* neg, int64_t ld_n, int32_t D,
                                  int64_t B, int64_t S, const int64_t* pos_ids, const int64_t* neg_ids, const float* sample_weight,
                                  float margin, int32_t metric, int32_t in_batch, int32_t num_hard, float eps, float* pos_score,
                                  float* row_loss, int32_t* row_active, int32_t* hard_idx, float* scores, void* workspace,
                                  int64_t workspace_bytes, dr_stream_t stream) {
    const MrArgs a = {q, pos, neg, sample_weight, pos_ids, neg_ids, ld_q, ld_p, ld_n, B, S, D, metric, in_batch, num_hard, margin, eps};
    MrP p;
    MrPlan pl;
    int st = mr_prepare(a, workspace, workspace_bytes, p, pl);
    if (st != DR_OK || B == 0) return st;
    if (!pos_score || !row_loss || !row_active || (num_hard > 0 && !hard_idx)) return DR_EINVAL;
    p.t_out = pos_score; p.row_loss = row_loss; p.row_active = row_active; p.hard_out = hard_idx; p.scores = scores;
    st = dr_launch(mr_norms_kernel, dim3(dr_grid_for(2 * B + S, 16)), dim3(256), 0, dr_s(stream), p);
    if (st != DR_OK) return st;
    MR_DISPATCH(st, mr_fwd_kernel, (unsigned)(pl.row_tiles * pl.groups), stream, p);
    if (st != DR_OK) return st;
    return dr_launch(mr_fwd_finalize_kernel, dim3(dr_grid_for(B, 256)), dim3(256), 0, dr_s(stream), p);
}

extern "C" int dr_margin_rank_bwd(const float* q, int64_t ld_q, const float* pos, int64_t ld_p, const float* neg, int64_t ld_n, int32_t D,
                                  int64_t B, int64_t S, const int64_t* pos_ids, const int64_t* neg_ids, const float* sample_weight,
                                  float margin, int32_t metric, int32_t in_batch, int32_t num_hard, float eps, float row_scale,
                                  const float* pos_score, const int32_t* hard_idx, float* d_q, int64_t ld_dq, float* d_pos, float* d_neg,
                                  void* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    const MrArgs a = {q, pos, neg, sample_weight, pos_ids, neg_ids, ld_q, ld_p, ld_n, B, S, D, metric, in_batch, num_hard, margin, eps};
    MrP p;
    MrPlan pl;
    int st = mr_prepare(a, workspace, workspace_bytes, p, pl);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_dq, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!pos_score || (num_hard > 0 && !hard_idx) || !d_q || !d_pos || !d_neg) return DR_EINVAL;
    if (!dr_aligned16(d_q) || !dr_aligned16(d_pos) || !dr_aligned16(d_neg)) return DR_EINVAL;
    p.t_in = pos_score; p.hard_in = hard_idx; p.row_scale = row_scale; p.d_q = d_q; p.ld_dq = ld_dq; p.d_pos = d_pos; p.d_neg = d_neg;
    st = dr_launch(mr_norms_kernel, dim3(dr_grid_for(2 * B + S, 16)), dim3(256), 0, dr_s(stream), p);
    if (st != DR_OK) return st;
    if (pl.groups > 1) MR_DISPATCH(st, mr_bwd_rows_split_kernel, (unsigned)(pl.row_tiles * pl.groups), stream, p);
    else MR_DISPATCH(st, mr_bwd_rows_kernel, (unsigned)pl.row_tiles, stream, p);
    if (st != DR_OK) return st;
    st = dr_launch(mr_bwd_rows_finalize_kernel, dim3(dr_grid_for(B * (D / 4), 256)), dim3(256), 0, dr_s(stream), p);
    if (st != DR_OK) return st;
    MR_DISPATCH(st, mr_bwd_cols_kernel, (unsigned)((int64_t)pl.col_tiles * pl.chunks), stream, p);
    if (st != DR_OK) return st;
    if (pl.chunks > 1) {
        const int64_t n = S * D + p.S4;
        st = dr_sum_partials(p.part_n, pl.chunks, p.nsum, n, nullptr, 0, nullptr, 0, (unsigned)dr_grid_for(n, 256), dr_s(stream));
        if (st != DR_OK) return st;
    }
    return dr_launch(mr_bwd_cols_finalize_kernel, dim3(dr_grid_for(S * (D / 4), 256)), dim3(256), 0, dr_s(stream), p);
}
