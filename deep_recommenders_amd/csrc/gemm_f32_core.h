// The fp32 MFMA GEMM template with fused epilogues, its argument block and its launcher: shared by dense.hip (tower linears),
// dense_cross.hip (DCN cross layer), dense_head.hip (fused tower head) and dense_scores.hip (two-tower score passes).  Each of
// those instantiates its own epilogues; no instantiation is emitted twice.
//
// One kernel template.  C[i][j] = sum_r A(i,r) * B(r,j), block tile 128 x 128 x 32, 4 waves in a
// 2 x 2 arrangement, each wave owns 64 x 64 = 2 x 2 MFMA tiles of 32 x 32 (64 accumulator registers).
// Operands are staged HBM -> registers -> LDS with the next tile's global loads issued before the
// current tile's MFMAs (register double buffering).  The LDS image is always [r][i] (reduction-major):
//   - an operand whose memory layout is reduction-contiguous (a[i*ld + r], "RC": x in fwd, dy and W
//     in bwd_dx) is transposed on the way in: float4 global loads along r, four ds_write_b32 with row
//     pitch 129 floats (129 % 32 == 1 makes the 4 x 8 (i, r4) lanes of a write group hit 32 banks);
//   - an operand already reduction-major (a[r*ld + i]: W in fwd, x and dy in bwd_dw) goes in with
//     ds_write_b128 at pitch 132 floats.
// Fragment reads are ds_read_b32 of 32 consecutive floats per half-wave: conflict-free in both cases.
// (bf16x3 mode keeps three bf16 planes [i][k] instead, see put4_bf3 below.)
// Consecutive workgroup ids are remapped so that the tiles sharing an A row-panel run on the same XCD
// (same L2): dispatch places block b on XCD b % 8.
#pragma once
#include "dr_common.h"
#include "bf3_rs_core.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

using bf3::bf16x2;
using bf3::bf16x4;
using bf3::bf16x8;
using bf3::f32x2;
using drrs::f32x16;

constexpr int BM = 128, BN = 128, BK = 32;   // wide configuration; the narrow one is 128 x 32 (template NARROW)
constexpr int LD_T = 129;   // pitch of a transposed-in operand tile
constexpr int LD_D = 132;   // pitch of a direct operand tile

enum Epi { EPI_BIAS_ACT = 0, EPI_CROSS = 1, EPI_MASK = 2, EPI_ATOMIC = 3, EPI_FMGRAD = 4, EPI_LSE = 5, EPI_SMGRAD = 6, EPI_HEAD = 7, EPI_FILTER = 8 };
constexpr int HEAD_PART = 34;   // per-block partials of the fused tower head: dw2[32], db2, loss

struct GemmArgs {
    const float* A; int64_t lda;
    const float* B; int64_t ldb;
    int64_t M;      // rows of C (i)
    int32_t N;      // cols of C (j)
    int64_t R;      // reduction length
    float* C; int64_t ldc;
    // epilogue operands
    const float* bias;        // [N]            (BIAS_ACT, CROSS)
    int32_t act;              // 0 / 1          (BIAS_ACT)
    const float* e0; int64_t lde0;   // CROSS: x0 ; MASK: relu_src
    const float* e1; int64_t lde1;   // CROSS: x
    float* aux; int64_t ldaux;       // CROSS: prod_out (may be null)
    float alpha;              // CROSS: diag_scale ; ATOMIC: scale
    int32_t accumulate;       // MASK: add to existing C
    float* colsum_dst;        // ATOMIC: dstb (may be null)
    int32_t split;            // ATOMIC: number of reduction splits (gridDim.y)
    int64_t per;              // ATOMIC: reduction rows per split (multiple of BK)
    float* partial;           // ATOMIC: if non-null, block (tile, y) stores its tile to partial[y][M][N] instead of atomics
    int32_t a_vec, b_vec;     // dead: written and read by nobody, kept so that every later field stays at its offset
    // FMGRAD: C = acc + dl[i] * (S[i][j % fm_D] - x[i][j]) for j < fm_FD   (e0 = x, e1 = S [M, fm_D])
    const float* vec; int32_t fm_D, fm_FD;
    // LSE / SMGRAD (in-batch softmax, Retrieval.call): score s_ij = (acc - log p_j + dupmask_ij * MIN_FLOAT) * inv_t
    const float* cand_prob;       // [N] or null
    const int64_t* cand_ids;      // [N] or null (N == M)
    float inv_t;
    float* part_m; float* part_l; // LSE: partial row max / sum-exp, [2*tiles_n][M]
    float* pos;                   // LSE: s_ii
    const float* lse;             // SMGRAD: row log-sum-exp ; vec = sample_weight (or null) ; alpha = d_loss
    // HEAD (narrow tile only): y = act(acc + bias) is the last hidden layer [M, N<=32]; logit = y . head_w + head_b + extra;
    // loss / gradient per example (dr_bce_terms), d_h = d_logit * head_w * act'(y); C (h itself) optional
    const float* head_w; int64_t ld_head_w;
    const float* head_b;
    const float* head_extra;      // [M] or null (the FM logit)
    const float* labels;          // [M]
    int32_t loss_mode;
    float inv_n;
    float* prob; float* d_logit;  // [M] (either may be null)
    float* d_h; int64_t ld_dh;    // [M, N] or null
    float* head_partial;          // [gridDim.x][HEAD_PART]
    // FILTER (top-K scan): a score is kept only if it beats its row's current k-th best `tau[row]`; kept scores are
    // appended to the row's candidate list (one atomic per 32-column group that has any) instead of writing C
    const float* tau;             // [M]
    float* cand_s; int32_t* cand_c;   // [M][cand_cap] scores / column numbers
    int32_t* cand_cnt;            // [M] append cursors (may exceed cand_cap: the consumer clamps; cap == N never overflows)
    int64_t cand_cap;
    // grouped launches (template GRP, gridDim.z = groups): block z offsets every operand by z times its group stride; with
    // `partial` set, the EPI_ATOMIC column sums go to partial[split][M][N] + [split][N] (summed by the grouped reduce)
    int32_t groups;
    int64_t a_gs, b_gs, c_gs, bias_gs, e0_gs, cs_gs, part_gs;
};

// exp() of a non-positive softmax argument; masked logits sit at ~-5e36 (MIN_FLOAT / temperature), far outside the
// range the libm range reduction is exact for, so anything below -87 (exp < FLT_MIN) is taken as exactly 0
__device__ __forceinline__ float safe_exp(float d) { return d < -87.f ? 0.f : expf(d); }

// Branch-free edge-safe float4 load of an operand tile element (row, col..col+3) of a [nrows, ncols] matrix with
// pitch ld (ncols >= 4).  Out-of-range rows are clamped to the last row, a vector that would run past the last
// valid column is shifted left so that it ends exactly at ncols (a dword-aligned, possibly 16-byte-unaligned
// global_load_dwordx4), and the components are rotated back / zeroed with selects.  No control flow: hipcc keeps
// all eight loads of a k-tile in flight across the MFMA block (with exec-mask branches it drains them first).
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
struct EdgeFix { int shift; bool ok; };
__device__ __forceinline__ EdgeFix edge_of(int64_t row, int64_t nrows, int64_t col, int64_t ncols) {
    const int64_t over = col + 4 - ncols;
    EdgeFix e;
    e.shift = over <= 0 ? 0 : (over >= 4 ? 4 : (int)over);
    e.ok = row < nrows;
    return e;
}
// raw load at the clamped address (no dependence on the loaded data -> stays in flight)
__device__ __forceinline__ f4u ld4_raw(const float* __restrict__ p, int64_t ld, int64_t row, int64_t nrows, int64_t col,
                                       int64_t ncols) {
    const int64_t rr = row < nrows ? row : nrows - 1;
    const int64_t over = col + 4 - ncols;
    const int shift = over <= 0 ? 0 : (over >= 4 ? 4 : (int)over);
    const int64_t cc = (col < ncols ? col : ncols) - shift;
    return *reinterpret_cast<const f4u*>(p + rr * ld + cc);
}
// applied when the tile is written to LDS, i.e. after the MFMA block the load was hidden under
__device__ __forceinline__ float4 fix4(f4u v, EdgeFix e) {
    float4 o;
    const int s = e.shift;
    o.x = !e.ok ? 0.f : (s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : s == 3 ? v.w : 0.f);
    o.y = !e.ok ? 0.f : (s == 0 ? v.y : s == 1 ? v.z : s == 2 ? v.w : 0.f);
    o.z = !e.ok ? 0.f : (s == 0 ? v.z : s == 1 ? v.w : 0.f);
    o.w = !e.ok ? 0.f : (s == 0 ? v.w : 0.f);
    return o;
}

// ---- fp32 product emulation on the bf16 matrix pipe ("bf16x3", 6 of the 9 cross products) --------------------------
// x = x0 + x1 + x2 with x0 = bf16_rn(x), x1 = bf16_rn(x - x0), x2 = bf16_rn(x - x0 - x1): |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|,
// the two subtractions are exact in fp32.  a * b ~= a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0); every bf16 x bf16 product
// is exact in the MFMA's fp32 accumulator and the dropped terms (a1b2, a2b1, a2b2) are below 2^-24 |ab|.
// LDS image of an operand tile in bf16x3 mode: three planes [rows][PK] of bf16, k-contiguous.  PK = 40 (80-byte rows): the
// ds_read_b128 fragment reads (lane -> row lane & 31, 16 bytes) are conflict-free for that instruction's 16-lane groups
// (20 * row mod 64 is a permutation of the 4-bank slots over each group, MI355X_MICROARCH.md LDS table).
constexpr int PK = 40;
// four k-consecutive fp32 values of one row -> 4 bf16 in each plane (one ds_write_b64 per plane).  The arithmetic is bf3::split4's with
// its two halves interleaved; calling split4 here gives the eleven bf16x3 kernels other register numbers.
__device__ __forceinline__ void put4_bf3(__bf16* __restrict__ plane0, int plane_stride, int row, int k, float v0, float v1,
                                         float v2, float v3) {
    const f32x2 a = {v0, v1}, b = {v2, v3};
    const bf16x2 a0 = __builtin_convertvector(a, bf16x2), b0 = __builtin_convertvector(b, bf16x2);
    const f32x2 ra = a - __builtin_convertvector(a0, f32x2), rb = b - __builtin_convertvector(b0, f32x2);
    const bf16x2 a1 = __builtin_convertvector(ra, bf16x2), b1 = __builtin_convertvector(rb, bf16x2);
    const f32x2 sa = ra - __builtin_convertvector(a1, f32x2), sb = rb - __builtin_convertvector(b1, f32x2);
    const bf16x2 a2 = __builtin_convertvector(sa, bf16x2), b2 = __builtin_convertvector(sb, bf16x2);
    __bf16* d = plane0 + row * PK + k;
    *reinterpret_cast<bf16x4*>(d) = bf16x4{a0[0], a0[1], b0[0], b0[1]};
    *reinterpret_cast<bf16x4*>(d + plane_stride) = bf16x4{a1[0], a1[1], b1[0], b1[1]};
    *reinterpret_cast<bf16x4*>(d + 2 * plane_stride) = bf16x4{a2[0], a2[1], b2[0], b2[1]};
}

// bf16x3 mode: one operand's four float4's `t[4]` -> its three planes.  A reduction-contiguous operand goes in row by row, a
// reduction-major one is transposed in registers (component c of the four float4's = four k-consecutive values of column
// dr_c4 * 4 + c).  A macro over the kernel's per-thread coordinates: as a function or a lambda, by value or by reference, the
// bf16x3 kernels come out with other register numbers and up to 8 % more instructions.
#define GEMM_STAGE_BF3(planes, plane_stride, rc, t)                                                                          \
    do {                                                                                                                     \
        if (rc) {                                                                                                            \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                                    \
                put4_bf3(planes, plane_stride, rc_i + RCS * q, rc_r4 * 4, t[q].x, t[q].y, t[q].z, t[q].w);                   \
        } else {                                                                                                             \
            put4_bf3(planes, plane_stride, dr_c4 * 4 + 0, dr_r0, t[0].x, t[1].x, t[2].x, t[3].x);                            \
            put4_bf3(planes, plane_stride, dr_c4 * 4 + 1, dr_r0, t[0].y, t[1].y, t[2].y, t[3].y);                            \
            put4_bf3(planes, plane_stride, dr_c4 * 4 + 2, dr_r0, t[0].z, t[1].z, t[2].z, t[3].z);                            \
            put4_bf3(planes, plane_stride, dr_c4 * 4 + 3, dr_r0, t[0].w, t[1].w, t[2].w, t[3].w);                            \
        }                                                                                                                    \
    } while (0)

// Occupancy: 3 blocks per CU for the wide tile (168 VGPRs).  At 4 (128 VGPRs) the next k-tile's 8 prefetch registers
// cannot stay live across the MFMA block without spilling, so the compiler sinks the global loads BELOW the 64 MFMAs
// and their latency is exposed in front of every barrier; pinned ahead of the MFMAs at 3 blocks/CU is 2-4 % faster.
template <bool A_RC, bool B_RC, int EPI, bool NARROW, bool OCC4 = false, bool BF3 = false, bool GRP = false>
__global__ __launch_bounds__(256, BF3 ? 2 : ((NARROW || OCC4) ? 4 : 3)) void gemm_f32_mfma_kernel(GemmArgs g) {
    if constexpr (GRP) {
        const int64_t z = blockIdx.z;
        g.A += z * g.a_gs; g.B += z * g.b_gs; g.C += z * g.c_gs;
        if (g.bias != nullptr) g.bias += z * g.bias_gs;
        if (g.e0 != nullptr) g.e0 += z * g.e0_gs;
        if (g.colsum_dst != nullptr) g.colsum_dst += z * g.cs_gs;
        if (g.partial != nullptr) g.partial += z * g.part_gs;
    }
    // wide: 2 x 2 waves, each 2 x 2 MFMA tiles (128 x 128);  narrow: 4 x 1 waves, each 1 x 1 tile (128 x 32)
    constexpr int BN = NARROW ? 32 : 128;
    constexpr int TM = NARROW ? 1 : 2, TN = NARROW ? 1 : 2;
    constexpr int RCS = 32;                                  // rows between a thread's float4's of a reduction-contiguous operand
    constexpr int NQB = NARROW ? 1 : 4;                      // float4's of the B tile per thread
    constexpr int LDA = A_RC ? LD_T : LD_D;
    constexpr int LDB = B_RC ? (NARROW ? 33 : LD_T) : (NARROW ? 36 : LD_D);
    static_assert(!(BF3 && NARROW), "bf16x3 mode uses the wide tile");
    constexpr int PLANE_A = BM * PK, PLANE_B = BN * PK;       // bf16 elements per plane (bf16x3 mode)
    constexpr int BF3_BUF = 3 * (PLANE_A + PLANE_B);          // bf16 elements of the tile image
    constexpr int SMEM_FLOATS = BF3 ? BF3_BUF / 2 : BK * LDA + BK * LDB;       // bf16x3: 60 KB, two blocks per CU
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    float* As = smem;
    float* Bs = smem + (BF3 ? 0 : BK * LDA);
    __bf16* const Ap = reinterpret_cast<__bf16*>(smem);       // bf16x3: [3][BM][PK] then [3][BN][PK]
    __bf16* const Bp = Ap + 3 * PLANE_A;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = NARROW ? wave : (wave >> 1), wn = NARROW ? 0 : (wave & 1);

    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_m = (int)((g.M + BM - 1) / BM);
    const int nwg = tiles_m * tiles_n;
    const int lid = drrs::xcd_remap(blockIdx.x, nwg);
    const int64_t m0 = (int64_t)(lid / tiles_n) * BM;
    const int n0 = (lid % tiles_n) * BN;

    // reduction range of this block (split-K only for EPI_ATOMIC)
    int64_t r_begin = 0, r_end = g.R;
    if (EPI == EPI_ATOMIC) {
        const int64_t per = g.per;                                // host-computed: every launched slice is non-empty
        r_begin = (int64_t)blockIdx.y * per;
        r_end = r_begin + per < g.R ? r_begin + per : g.R;
        if (r_begin >= r_end) return;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[a][b][k] = 0.f;

    // per-thread coordinates of its float4's.  RC operand: (i = tid>>3 (+32q), r4 = tid&7); reduction-major operand, wide:
    // (r = tid>>5 (+8q), c4 = tid&31), narrow B (32 columns): (r = tid>>3, c4 = tid&7), one float4 per thread.
    const int rc_i = tid >> 3, rc_r4 = tid & 7;
    // bf16x3 mode, reduction-major operand: each thread owns a 4 (k) x 4 (i) block so that it can write k-contiguous bf16
    // quads; a 16-lane group spans 4 column-quads x 4 k-quads (64-byte global segments, 2-way LDS store conflicts at most)
    const int t_kq = (tid >> 7) * 4 + ((tid & 15) >> 2), t_c4 = ((tid >> 4) & 7) * 4 + (tid & 3);
    const int dr_r0 = BF3 ? 4 * t_kq : (tid >> 5), dr_rs = BF3 ? 1 : 8;     // row of float4 q: dr_r0 + dr_rs * q
    const int dr_c4 = BF3 ? t_c4 : (tid & 31);
    const int nb_r = tid >> 3, nb_c4 = tid & 7;
    f4u va[4], vb[NQB];
    auto load_tiles = [&](f4u (&va)[4], f4u (&vb)[NQB], int64_t r0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (A_RC) va[q] = ld4_raw(g.A, g.lda, m0 + rc_i + RCS * q, g.M, r0 + rc_r4 * 4, r_end);
            else      va[q] = ld4_raw(g.A, g.lda, r0 + dr_r0 + dr_rs * q, r_end, m0 + dr_c4 * 4, g.M);
        }
#pragma unroll
        for (int q = 0; q < NQB; ++q) {
            if (B_RC) vb[q] = ld4_raw(g.B, g.ldb, (int64_t)n0 + rc_i + RCS * q, g.N, r0 + rc_r4 * 4, r_end);
            else if (NARROW) vb[q] = ld4_raw(g.B, g.ldb, r0 + nb_r, r_end, (int64_t)n0 + nb_c4 * 4, g.N);
            else      vb[q] = ld4_raw(g.B, g.ldb, r0 + dr_r0 + dr_rs * q, r_end, (int64_t)n0 + dr_c4 * 4, g.N);
        }
    };
    auto store_tiles = [&](const f4u (&va)[4], const f4u (&vb)[NQB], int64_t r0) {     // r0 = offset the set was loaded for
        if constexpr (BF3) {
            float4 ta[4], tb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (A_RC) ta[q] = fix4(va[q], edge_of(m0 + rc_i + RCS * q, g.M, r0 + rc_r4 * 4, r_end));
                else      ta[q] = fix4(va[q], edge_of(r0 + dr_r0 + dr_rs * q, r_end, m0 + dr_c4 * 4, g.M));
                if (B_RC) tb[q] = fix4(vb[q], edge_of((int64_t)n0 + rc_i + RCS * q, g.N, r0 + rc_r4 * 4, r_end));
                else      tb[q] = fix4(vb[q], edge_of(r0 + dr_r0 + dr_rs * q, r_end, (int64_t)n0 + dr_c4 * 4, g.N));
            }
            GEMM_STAGE_BF3(Ap, PLANE_A, A_RC, ta);
            GEMM_STAGE_BF3(Bp, PLANE_B, B_RC, tb);
            return;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (A_RC) {
                const float4 t = fix4(va[q], edge_of(m0 + rc_i + RCS * q, g.M, r0 + rc_r4 * 4, r_end));
                float* d = As + (rc_r4 * 4) * LDA + rc_i + RCS * q;
                d[0] = t.x; d[LDA] = t.y; d[2 * LDA] = t.z; d[3 * LDA] = t.w;
            } else {
                const float4 t = fix4(va[q], edge_of(r0 + dr_r0 + dr_rs * q, r_end, m0 + dr_c4 * 4, g.M));
                *reinterpret_cast<float4*>(&As[(dr_r0 + dr_rs * q) * LDA + dr_c4 * 4]) = t;
            }
        }
#pragma unroll
        for (int q = 0; q < NQB; ++q) {
            if (B_RC) {
                const float4 t = fix4(vb[q], edge_of((int64_t)n0 + rc_i + RCS * q, g.N, r0 + rc_r4 * 4, r_end));
                float* d = Bs + (rc_r4 * 4) * LDB + rc_i + RCS * q;
                d[0] = t.x; d[LDB] = t.y; d[2 * LDB] = t.z; d[3 * LDB] = t.w;
            } else if (NARROW) {
                const float4 t = fix4(vb[q], edge_of(r0 + nb_r, r_end, (int64_t)n0 + nb_c4 * 4, g.N));
                *reinterpret_cast<float4*>(&Bs[nb_r * LDB + nb_c4 * 4]) = t;
            } else {
                const float4 t = fix4(vb[q], edge_of(r0 + dr_r0 + dr_rs * q, r_end, (int64_t)n0 + dr_c4 * 4, g.N));
                *reinterpret_cast<float4*>(&Bs[(dr_r0 + dr_rs * q) * LDB + dr_c4 * 4]) = t;
            }
        }
    };

    float colsum = 0.f;   // EPI_ATOMIC: column sums of B (dy) accumulated by the m-tile-0 blocks
    const bool do_colsum = (EPI == EPI_ATOMIC) && g.colsum_dst != nullptr && m0 == 0 && tid < BN;

    const float* as = As + (lane >> 5) * LDA + wm * (TM * 32) + (lane & 31);
    const float* bs = Bs + (lane >> 5) * LDB + wn * (TN * 32) + (lane & 31);
    auto mfma_block = [&]() {
        if constexpr (BF3) {
            if (do_colsum) {   // column sums of the B tile from its three planes (x0 + x1 + x2 == x up to 2^-24)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int c = 0; c < BK / 8; ++c) {
                        const bf16x8 v = *reinterpret_cast<const bf16x8*>(Bp + pl * PLANE_B + tid * PK + 8 * c);
#pragma unroll
                        for (int j = 0; j < 8; ++j) colsum += (float)v[j];
                    }
            }
            // fragment of a 32 x 16 sub-tile: lane (row = lane & 31, kg = lane >> 5) takes k = k0 + 8 * kg + 0..7, one ds_read_b128 per plane
            const __bf16* ap = Ap + (wm * (TM * 32) + (lane & 31)) * PK + 8 * (lane >> 5);
            const __bf16* bp = Bp + (wn * (TN * 32) + (lane & 31)) * PK + 8 * (lane >> 5);
#pragma unroll
            for (int k0 = 0; k0 < BK; k0 += 16) {
                bf16x8 af[3][TM], bf[3][TN];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                    for (int t = 0; t < TM; ++t) af[pl][t] = *reinterpret_cast<const bf16x8*>(ap + pl * PLANE_A + t * 32 * PK + k0);
#pragma unroll
                    for (int t = 0; t < TN; ++t) bf[pl][t] = *reinterpret_cast<const bf16x8*>(bp + pl * PLANE_B + t * 32 * PK + k0);
                }
                // smallest terms first; the four accumulators are interleaved so that back-to-back MFMAs are independent
#pragma unroll
                for (int term = 0; term < 6; ++term) {
                    constexpr int PA[6] = {0, 1, 2, 0, 1, 0}, PB[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
                    for (int a = 0; a < TM; ++a)
#pragma unroll
                        for (int b = 0; b < TN; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[term]][a], bf[PB[term]][b], acc[a][b], 0, 0, 0);
                }
            }
            return;
        }
        if (do_colsum) {
#pragma unroll 8
            for (int r = 0; r < BK; ++r) colsum += Bs[r * LDB + tid];
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float af[TM], bf[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) af[t] = as[kk * LDA + 32 * t];
#pragma unroll
            for (int t = 0; t < TN; ++t) bf[t] = bs[kk * LDB + 32 * t];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
    };
    // ---- lean path for interior blocks: raw pointer-bumped dwordx4 loads, direct LDS stores, no edge logic.
    // (PMC, tools/exp/gemm_only.py: the clamped loader + fix-up costs ~600 SALU/VALU instructions per wave per k-tile,
    // as long as the 64-MFMA block itself; the lean loop issues ~60.)
    // Row / column edges of the OUTPUT tile need no masking here: an operand row (RC) or column (reduction-major)
    // that lies outside the matrix only feeds accumulator rows / columns the epilogue never stores, so its address is
    // simply clamped into the matrix (computed once, outside the loop).  Only the reduction tail needs zero fill.
    const int64_t nfull = (r_end - r_begin) / BK;             // whole k-tiles
    const bool has_tail = r_begin + nfull * BK < r_end;
    // a float4 that straddles the last column of a reduction-major operand is loaded unshifted, which is only legal
    // when the row pitch covers it (padded buffers); a tight pitch sends that edge block down the clamped slow path
    const bool a_tight = !A_RC && (m0 + BM > g.M) && (g.M & 3) && g.lda < ((g.M + 3) & ~(int64_t)3);
    const bool b_tight = !B_RC && (n0 + BN > g.N) && (g.N & 3) && g.ldb < (((int64_t)g.N + 3) & ~(int64_t)3);
    if (nfull > 0 && !a_tight && !b_tight) {
        const float* pa[4];
        const float* pb[NQB];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (A_RC) {
                int64_t row = m0 + rc_i + RCS * q;
                row = row < g.M ? row : g.M - 1;
                pa[q] = g.A + row * g.lda + r_begin + rc_r4 * 4;
            } else {
                int64_t col = m0 + dr_c4 * 4;
                col = col < g.M ? col : g.M - 4;             // fully outside -> anywhere legal; straddling -> unshifted
                pa[q] = g.A + (r_begin + dr_r0 + dr_rs * q) * g.lda + col;
            }
        }
#pragma unroll
        for (int q = 0; q < NQB; ++q) {
            if (B_RC) {
                int64_t row = (int64_t)n0 + rc_i + RCS * q;
                row = row < g.N ? row : g.N - 1;
                pb[q] = g.B + row * g.ldb + r_begin + rc_r4 * 4;
            } else {
                int64_t col = (int64_t)n0 + (NARROW ? nb_c4 : dr_c4) * 4;
                col = col < g.N ? col : g.N - 4;
                pb[q] = g.B + (r_begin + (NARROW ? nb_r : dr_r0 + dr_rs * q)) * g.ldb + col;
            }
        }
        const int64_t a_it = A_RC ? (int64_t)BK : BK * g.lda;
        const int64_t b_it = B_RC ? (int64_t)BK : BK * g.ldb;
        auto load_fast = [&](f4u (&va)[4], f4u (&vb)[NQB]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                va[q] = *reinterpret_cast<const f4u*>(pa[q]);
                pa[q] += a_it;
            }
#pragma unroll
            for (int q = 0; q < NQB; ++q) {
                vb[q] = *reinterpret_cast<const f4u*>(pb[q]);
                pb[q] += b_it;
            }
        };
        auto store_fast = [&](const f4u (&va)[4], const f4u (&vb)[NQB]) {
            if constexpr (BF3) {
                GEMM_STAGE_BF3(Ap, PLANE_A, A_RC, va);
                GEMM_STAGE_BF3(Bp, PLANE_B, B_RC, vb);
                return;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (A_RC) {
                    float* d = As + (rc_r4 * 4) * LDA + rc_i + RCS * q;
                    d[0] = va[q].x; d[LDA] = va[q].y; d[2 * LDA] = va[q].z; d[3 * LDA] = va[q].w;
                } else {
                    *reinterpret_cast<f4u*>(&As[(dr_r0 + dr_rs * q) * LDA + dr_c4 * 4]) = va[q];
                }
            }
#pragma unroll
            for (int q = 0; q < NQB; ++q) {
                if (B_RC) {
                    float* d = Bs + (rc_r4 * 4) * LDB + rc_i + RCS * q;
                    d[0] = vb[q].x; d[LDB] = vb[q].y; d[2 * LDB] = vb[q].z; d[3 * LDB] = vb[q].w;
                } else if (NARROW) {
                    *reinterpret_cast<f4u*>(&Bs[nb_r * LDB + nb_c4 * 4]) = vb[q];
                } else {
                    *reinterpret_cast<f4u*>(&Bs[(dr_r0 + dr_rs * q) * LDB + dr_c4 * 4]) = vb[q];
                }
            }
        };
        if constexpr (BF3) {
            // Two register sets, so that a tile's global loads are issued two k-tiles before they are needed: with one set
            // they have only the 48-MFMA block (~2000 cycles) to land and the store phase waits 1000-2000 cycles for them
            // in most iterations (tools/exp/bf3_phases.py: clock64 timeline of one block).
            f4u wa[4], wb[NQB];
            load_fast(va, vb);                                 // tile 0
            if (nfull > 1) load_fast(wa, wb);                  // tile 1
            int64_t t = 0;
            for (; t + 3 < nfull; t += 2) {
                store_fast(va, vb);                            // tile t
                __syncthreads();
                load_fast(va, vb);                             // tile t + 2
                __builtin_amdgcn_sched_barrier(0);
                mfma_block();
                __syncthreads();
                store_fast(wa, wb);                            // tile t + 1
                __syncthreads();
                load_fast(wa, wb);                             // tile t + 3
                __builtin_amdgcn_sched_barrier(0);
                mfma_block();
                __syncthreads();
            }
            // up to three whole tiles left: t (in va / vb), t + 1 (in wa / wb), t + 2 (not loaded yet), then the tail
            const int64_t left = nfull - t;                    // 1, 2 or 3
            store_fast(va, vb);
            __syncthreads();
            if (left == 3) load_fast(va, vb);
            else if (left == 1 && has_tail) load_tiles(va, vb, r_begin + nfull * BK);
            mfma_block();
            __syncthreads();
            if (left >= 2) {
                store_fast(wa, wb);
                __syncthreads();
                if (left == 2 && has_tail) load_tiles(wa, wb, r_begin + nfull * BK);
                mfma_block();
                __syncthreads();
            }
            if (left == 3) {
                store_fast(va, vb);
                __syncthreads();
                if (has_tail) load_tiles(wa, wb, r_begin + nfull * BK);
                mfma_block();
                __syncthreads();
            }
            if (has_tail) {
                if (left == 1) store_tiles(va, vb, r_begin + nfull * BK); else store_tiles(wa, wb, r_begin + nfull * BK);
                __syncthreads();
                mfma_block();
                __syncthreads();
            }
        } else {
        load_fast(va, vb);
        for (int64_t t = 0; t + 1 < nfull; ++t) {
            store_fast(va, vb);
            __syncthreads();
            load_fast(va, vb);
            if (!OCC4) __builtin_amdgcn_sched_barrier(0);    // keep the global loads AHEAD of the MFMA block (needs > 128 VGPRs)
            mfma_block();
            __syncthreads();
        }
        // last whole tile (+ the clamped tail tile, if any), straight-line
        store_fast(va, vb);
        __syncthreads();
        if (has_tail) load_tiles(va, vb, r_begin + nfull * BK);
        mfma_block();
        __syncthreads();
        if (has_tail) {
            store_tiles(va, vb, r_begin + nfull * BK);
            __syncthreads();
            mfma_block();
            __syncthreads();
        }
        }
    } else {
        load_tiles(va, vb, r_begin);
        for (int64_t r0 = r_begin; r0 < r_end; r0 += BK) {
            store_tiles(va, vb, r0);
            __syncthreads();
            if (r0 + BK < r_end) load_tiles(va, vb, r0 + BK);
            mfma_block();
            __syncthreads();
        }
    }

    if constexpr ((EPI == EPI_LSE || EPI == EPI_SMGRAD) && !NARROW) {
        constexpr float MIN_FLOAT = -3.4028234663852886e36f;   // np.finfo(np.float32).min / 100 (sbcnm.py:10)
        static_assert(!((EPI == EPI_LSE || EPI == EPI_SMGRAD) && NARROW), "softmax epilogues use the wide tile");
        float colcorr[2];
        int64_t colid[2];
        int colj[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            colj[ni] = n0 + wn * 64 + ni * 32 + (lane & 31);
            const bool cv = colj[ni] < g.N;
            colcorr[ni] = (cv && g.cand_prob != nullptr) ? -logf(g.cand_prob[colj[ni]]) : 0.f;
            colid[ni] = (cv && g.cand_ids != nullptr) ? g.cand_ids[colj[ni]] : 0;
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t row = m0 + wm * 64 + mi * 32 + 4 * (lane >> 5) + (reg & 3) + 8 * (reg >> 2);
                const bool rv = row < g.M;
                const int64_t rid = (rv && g.cand_ids != nullptr) ? g.cand_ids[row] : 0;
                float sv[2];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    float v = acc[mi][ni][reg] + colcorr[ni];
                    if (g.cand_ids != nullptr && rid == colid[ni] && row != colj[ni]) v += MIN_FLOAT;
                    sv[ni] = v * g.inv_t;
                }
                if (EPI == EPI_LSE) {
                    float m = -INFINITY;
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        if (colj[ni] < g.N) m = fmaxf(m, sv[ni]);
#pragma unroll
                    for (int o = 1; o < 32; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                    float l = 0.f;
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        if (colj[ni] < g.N) l += safe_exp(sv[ni] - m);
#pragma unroll
                    for (int o = 1; o < 32; o <<= 1) l += __shfl_xor(l, o, 64);
                    if (rv && (lane & 31) == 0) {
                        const int64_t pc = (int64_t)((n0 / BN) * 2 + wn);
                        g.part_m[pc * g.M + row] = m;
                        g.part_l[pc * g.M + row] = l;
                    }
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        if (rv && row == colj[ni]) g.pos[row] = sv[ni];
                } else {
                    if (!rv) continue;
                    const float w = g.vec != nullptr ? g.vec[row] : 1.f;
                    const float lse = g.lse[row];
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        if (colj[ni] >= g.N) continue;
                        const float pr = safe_exp(sv[ni] - lse) - (row == colj[ni] ? 1.f : 0.f);
                        g.C[row * g.ldc + colj[ni]] = w * pr * g.inv_t * g.alpha;
                    }
                }
            }
        }
        return;
    }
    if constexpr (EPI == EPI_FILTER && !NARROW) {
        const int c31 = lane & 31, hh = lane >> 5;
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t row = m0 + wm * (TM * 32) + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                const bool rv = row < g.M;
                const float t = rv ? g.tau[row] : INFINITY;
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int col = n0 + wn * (TN * 32) + ni * 32 + c31;
                    const float v = acc[mi][ni][reg];
                    const bool pass = rv && col < g.N && v > t;
                    const unsigned half = (unsigned)((__ballot(pass) >> (32 * hh)) & 0xffffffffull);
                    if (half != 0u) {                      // rare once tau has warmed up: one atomic per (row, 32 columns)
                        const int leader = 32 * hh + __ffs((int)half) - 1;
                        int base = 0;
                        if (lane == leader) base = atomicAdd(g.cand_cnt + row, __popc(half));
                        base = __shfl(base, leader, 64);
                        if (pass) {
                            const int64_t pos = base + __popc(half & ((1u << c31) - 1u));
                            if (pos < g.cand_cap) {
                                g.cand_s[row * g.cand_cap + pos] = v;
                                g.cand_c[row * g.cand_cap + pos] = col;
                            }
                        }
                    }
                }
            }
        }
        return;
    }
    if constexpr (EPI == EPI_HEAD && NARROW) {
        // Fused tower head (the Dense(1) that follows the last hidden layer, the loss, and their backward):
        // lane (col, half) holds 16 rows of column col of y; the Dense(1) dot product is a butterfly over the 32 columns.
        const int col = lane & 31, hh = lane >> 5;
        const bool cv = col < g.N;
        const int colc = cv ? col : g.N - 1;
        const float bj = g.bias != nullptr ? g.bias[colc] : 0.f;
        const float wj = cv ? g.head_w[(int64_t)colc * g.ld_head_w] : 0.f;
        const float b2 = g.head_b != nullptr ? g.head_b[0] : 0.f;
        const int64_t row_b = m0 + wm * 32 + 4 * hh;
        float dw_acc = 0.f, db_acc = 0.f, loss_acc = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int ro = (reg & 3) + 8 * (reg >> 2);
            const int64_t row = row_b + ro;
            const bool rv = row < g.M;
            const int64_t rc = rv ? row : g.M - 1;
            float v = acc[0][0][reg] + bj;
            if (g.act == 1) v = fmaxf(v, 0.f);
            if (!cv) v = 0.f;
            float dot = v * wj;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) dot += __shfl_xor(dot, o, 64);
            const float x = (dot + b2) + (g.head_extra != nullptr ? g.head_extra[rc] : 0.f);
            float p, l, gr;
            dr_bce_terms(x, g.labels[rc], g.loss_mode, p, l, gr);
            float gs = gr * g.inv_n;
            if (!rv) { l = 0.f; gs = 0.f; }
            if (rv && col == 0) {
                if (g.prob != nullptr) g.prob[row] = p;
                if (g.d_logit != nullptr) g.d_logit[row] = gs;
            }
            if (rv && cv) {
                if (g.d_h != nullptr) g.d_h[row * g.ld_dh + col] = (g.act == 1 && !(v > 0.f)) ? 0.f : gs * wj;
                if (g.C != nullptr) g.C[row * g.ldc + col] = v;
            }
            dw_acc = fmaf(v, gs, dw_acc);
            if (col == 0) { db_acc += gs; loss_acc += l; }
        }
        __syncthreads();                                   // every wave is done with the operand tiles
        float* red = smem;                                 // [8 = wave * 2 + half][HEAD_PART]
        red[(wave * 2 + hh) * HEAD_PART + col] = dw_acc;
        if (col == 0) {
            red[(wave * 2 + hh) * HEAD_PART + 32] = db_acc;
            red[(wave * 2 + hh) * HEAD_PART + 33] = loss_acc;
        }
        __syncthreads();
        if (tid < HEAD_PART) {
            float sacc = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) sacc += red[i * HEAD_PART + tid];
            g.head_partial[(int64_t)blockIdx.x * HEAD_PART + tid] = sacc;
        }
        return;
    }
    // ---- epilogue: C/D layout of 32x32 MFMA: col = lane & 31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    const bool full = (m0 + BM <= g.M) && (n0 + BN <= g.N);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int col = n0 + wn * (TN * 32) + ni * 32 + (lane & 31);
            if (!full && col >= g.N) continue;
            float bj = 0.f;
            if ((EPI == EPI_BIAS_ACT || EPI == EPI_CROSS) && g.bias != nullptr) bj = g.bias[col];
            int cmod = 0;
            if (EPI == EPI_FMGRAD) cmod = col % g.fm_D;
            const int64_t row_b = m0 + wm * (TM * 32) + mi * 32 + 4 * (lane >> 5);
            float* cp = g.C + row_b * g.ldc + col;
            const float* e0p = (EPI == EPI_CROSS || EPI == EPI_MASK || EPI == EPI_FMGRAD) && g.e0 != nullptr
                                   ? g.e0 + row_b * g.lde0 + col : nullptr;
            const float* e1p = (EPI == EPI_CROSS) ? g.e1 + row_b * g.lde1 + col
                               : (EPI == EPI_FMGRAD ? g.e1 + row_b * g.lde1 + cmod : nullptr);
            float* auxp = (EPI == EPI_CROSS && g.aux != nullptr) ? g.aux + row_b * g.ldaux + col : nullptr;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int ro = (reg & 3) + 8 * (reg >> 2);
                if (!full && row_b + ro >= g.M) continue;
                float v = acc[mi][ni][reg];
                if (EPI == EPI_BIAS_ACT) {
                    v += bj;
                    if (g.act == 1) v = fmaxf(v, 0.f);
                    cp[ro * g.ldc] = v;
                } else if (EPI == EPI_CROSS) {
                    const float xv = e1p[ro * g.lde1];
                    const float prod = v + bj + g.alpha * xv;
                    if (auxp != nullptr) auxp[ro * g.ldaux] = prod;
                    cp[ro * g.ldc] = e0p[ro * g.lde0] * prod + xv;
                } else if (EPI == EPI_FMGRAD) {
                    if (col < g.fm_FD) v += g.vec[row_b + ro] * (e1p[ro * g.lde1] - e0p[ro * g.lde0]);
                    cp[ro * g.ldc] = v;
                } else if (EPI == EPI_MASK) {
                    if (e0p != nullptr && !(e0p[ro * g.lde0] > 0.f)) v = 0.f;
                    if (g.accumulate) v += cp[ro * g.ldc];
                    cp[ro * g.ldc] = v;
                } else {
                    if (g.partial != nullptr)
                        g.partial[((int64_t)blockIdx.y * g.M + row_b + ro) * g.N + col] = v;
                    else
                        unsafeAtomicAdd(cp + ro * g.ldc, g.alpha * v);
                }
            }
        }
    }
    if (do_colsum && n0 + tid < g.N) {
        if (GRP && g.partial != nullptr)
            g.partial[(int64_t)g.split * g.M * g.N + (int64_t)blockIdx.y * g.N + n0 + tid] = colsum;
        else
            unsafeAtomicAdd(g.colsum_dst + n0 + tid, g.alpha * colsum);
    }
}

#undef GEMM_STAGE_BF3

template <bool A_RC, bool B_RC, int EPI, bool GRP = false>
int launch(GemmArgs& g, hipStream_t s) {
    const bool narrow = g.N <= 32 && (EPI == EPI_BIAS_ACT || EPI == EPI_MASK || EPI == EPI_ATOMIC || EPI == EPI_HEAD);
    const int bn = narrow ? 32 : BN;
    const int tiles_n = (g.N + bn - 1) / bn;
    const int64_t tiles_m = (g.M + BM - 1) / BM;
    if (tiles_m * tiles_n > 0x7fffffff) return DR_EINVAL;
    dim3 grid((unsigned)(tiles_m * tiles_n), EPI == EPI_ATOMIC ? g.split : 1, GRP ? g.groups : 1);
    if (narrow) {
        if constexpr (EPI == EPI_BIAS_ACT || EPI == EPI_MASK || EPI == EPI_ATOMIC || EPI == EPI_HEAD)
            hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, true, false, false, GRP>), grid, dim3(256), 0, s, g);
    } else {
        if constexpr (EPI == EPI_HEAD) return DR_ESHAPE;
        else if constexpr (EPI == EPI_FILTER || EPI == EPI_LSE || EPI == EPI_SMGRAD) {
            // short reductions with heavy epilogues (the two-tower rows: K = 128 = 4 k-tiles per output tile): the per-tile
            // prologue / epilogue weigh more than the steady-state loop, so a fourth resident block per CU beats the pinned
            // prefetch (measured: in-batch softmax forward 0.343 -> 0.320 ms, top-K scan 26.65 -> 25.65 ms; plain scores: no)
            // the top-K scan follows the GEMM mode (bf16x3 products: 25.7 -> 23.3 ms at 8192 x 1 M x 128) together with
            // dr_scores_nt, which scores its first chunk: equal candidates must tie bit-exactly across the two kernels.
            // The in-batch softmax pair (LSE forward / gradient) stays on the fp32 MFMA (bf16x3 measured 3 % slower there).
            if (EPI == EPI_FILTER && dr_get_gemm_mode() == DR_GEMM_BF16X3) {
                if constexpr (EPI == EPI_FILTER)
                    hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, false, false, true, GRP>), grid, dim3(256), 0, s, g);
            } else if (g.R <= 256)
                hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, false, true, false, GRP>), grid, dim3(256), 0, s, g);
            else
                hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, false, false, false, GRP>), grid, dim3(256), 0, s, g);
        } else {
            // the tower / cross-layer GEMMs: fp32 products on the bf16 matrix pipe unless the caller asked for the native one
            if (dr_get_gemm_mode() == DR_GEMM_BF16X3)
                hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, false, false, true, GRP>), grid, dim3(256), 0, s, g);
            else
                hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_RC, B_RC, EPI, false, false, false, GRP>), grid, dim3(256), 0, s, g);
        }
    }
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// the operands and the output of C = A x B; every epilogue operand zero / null, no split
GemmArgs gemm_args(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int32_t N, int64_t R, float* C, int64_t ldc) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.R = R; g.C = C; g.ldc = ldc; g.split = 1;
    return g;
}

// argument checks of the entry points
bool bad_ld(int64_t ld, int64_t min) { return ld < min; }
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

}  // namespace
