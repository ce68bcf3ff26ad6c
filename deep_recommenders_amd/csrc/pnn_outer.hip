// PNN's outer-product layer (Qu et al., ICDM 2016), forward and backward.
//
//   u[b, d] = sum_i emb[b, i D + d]  (i ascending);   out[b, n] = sum_{d,e} u[b,d] u[b,e] W[d D + e, n] (+ addend[b, n])
//   backward from g = d_out:   dW[d D + e, n] = sum_b u[b,d] u[b,e] g[b,n]
//                              S[b,d,e] = sum_n g[b,n] W[d D + e, n];  du[b,d] = sum_e (S[b,d,e] + S[b,e,d]) u[b,e];  d_emb[b, i D + d] = du[b,d]
//
// THREE BLOCK-TILED GEMMS ON v_mfma_f32_32x32x2_f32 WHOSE [B, D^2] OPERAND IS NEVER WRITTEN.  256 threads, 2 x 2 waves, k-tiles of 16
// staged HBM -> registers -> LDS with the next tile's global loads issued ahead of the MFMAs (as gemm_f32_core.h does).
// FORWARD   pnn_usum_kernel writes u; pnn_fwd_kernel is the GEMM M = B, K = D^2, N.  Block tile 128 x 128 (64 x 64 for grids below one
//           tile per CU).  The row tile's u sits in LDS transposed ([D][132]) for the whole K loop; the A fragment of k = (d, e) is ut[d][i] * ut[e][i], one multiply per lane.
//           W is the streamed operand ([16][132] per k-tile).  k runs upward in every accumulator: an example's bits do not depend on
//           its row in the tile.
// dW        the same GEMM transposed: M = D^2 is generated (lane i of the A fragment owns one (d, e) for the whole loop), K = B.  The
//           batch is cut into `parts` runs of `per` examples (pnn_parts: a function of B alone); block (tile, part) writes its tile of
//           partial[part] to the workspace and pnn_dw_reduce_kernel adds the partials in part order.
// du        g W^T with W symmetrised on the way into LDS (W[(d,e)] + W[(e,d)]), so that du[b,d] needs the D columns (d, .) only.  A
//           block owns 64 examples and walks the D^2 columns in chunks of 128: the accumulator tile passes through LDS once and the
//           thread that owns (b, d) adds its columns, e ascending, onto du in LDS.  Chunks are separated by barriers, so every du has one
//           owner at a time and a fixed order.  At the end the block writes du to the F rows of d_emb (one thread per element).
// No float atomics, no allocation, no copy, no environment variable.
#include "dr_common.h"

namespace {

constexpr int PNN_MAX_F = 64;
constexpr int PNN_MAX_D = 128;
constexpr int PNN_MAX_N = 4096;
constexpr int PNN_BK = 16;            // D^2 is a multiple of 16 for every D % 4 == 0
constexpr int PNN_LD = 132;           // pitch of a 128-wide LDS tile read along its row
constexpr int PNN_LDT = 129;          // pitch of a 128-wide LDS tile written transposed / read down its columns
constexpr int PNN_DU_BM = 64;         // examples per block of the du kernel
constexpr int PNN_MAX_PARTS = 64;
constexpr int PNN_FWD_MIN_BLOCKS = 256;   // fewer 128 x 128 tiles than this (one per CU) and the forward takes 64 x 64 tiles

struct PnnP {
    const float* u_in; const float* W; int64_t ld_w;
    const float* addend; int64_t ld_add;
    const float* g; int64_t ld_g;
    float* out; int64_t ld_out;
    float* d_emb; int64_t ld_demb;
    float* part;
    int64_t ld_u, B, per;
    int32_t F, D, N, Npad, accumulate;
};

__global__ __launch_bounds__(256) void pnn_usum_kernel(const float* __restrict__ emb, int64_t ld_emb, int64_t B, int F, int D,
                                                       float* __restrict__ u, int64_t ld_u) {
    const int n4 = D >> 2;
    const int64_t total = B * n4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / n4;
        const int k = (int)(idx - b * n4) << 2;
        const float* src = emb + b * ld_emb + k;
        float4 a = *reinterpret_cast<const float4*>(src);
        for (int i = 1; i < F; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)i * D);
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        *reinterpret_cast<float4*>(u + b * ld_u + k) = a;
    }
}

// out tile BT x BT, BT = 64 T (2 x 2 waves of T x T MFMA tiles).  LDS: ut [D][BT + 4] (u of the BT rows, transposed), Ws [16][BT + 4].
// T = 2 is the steady-state tile; T = 1 is for grids that would leave CUs idle (pnn_fwd_small).  Both add k upward on the same
// instruction, so an element's bits do not depend on the tile it falls into.
template <int T>
__global__ __launch_bounds__(256, 2) void pnn_fwd_kernel(const PnnP p) {
    extern __shared__ __attribute__((aligned(16))) float pnn_lds[];
    constexpr int BT = 64 * T, LDP = BT + 4, C4 = BT / 4, WROWS = 256 / C4;      // W's k-tile: T float4's per thread, rows WROWS apart
    const int D = p.D, N = p.N;
    float* ut = pnn_lds;
    float* Ws = pnn_lds + D * LDP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hh = lane >> 5;
    const int tiles_n = (N + BT - 1) / BT;
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * BT;
    const int n0 = (int)(blockIdx.x % tiles_n) * BT;

    const int n4 = D >> 2;
    for (int idx = tid; idx < BT * n4; idx += 256) {
        const int i = idx & (BT - 1), k = (idx / BT) << 2;
        int64_t row = m0 + i;
        row = row < p.B ? row : p.B - 1;                       // rows past B feed accumulator rows nobody stores
        const float4 v = *reinterpret_cast<const float4*>(p.u_in + row * p.ld_u + k);
        ut[(k + 0) * LDP + i] = v.x; ut[(k + 1) * LDP + i] = v.y; ut[(k + 2) * LDP + i] = v.z; ut[(k + 3) * LDP + i] = v.w;
    }

    // W's k-tile: rows tid / C4 + WROWS q, float4 column tid % C4.  A column quad past N is clamped to the last quad inside the pitch
    // (ld_w >= 4 ceil(N / 4)); what it holds feeds accumulator columns nobody stores.
    const int wr = tid / C4, wc4 = tid % C4;
    int wcol = n0 + wc4 * 4;
    wcol = wcol < p.Npad ? wcol : p.Npad - 4;
    const float* wp = p.W + (int64_t)wr * p.ld_w + wcol;
    const int64_t w_q = WROWS * p.ld_w, w_it = (int64_t)PNN_BK * p.ld_w;

    dr_f32x16 acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = D * D / PNN_BK;
    float4 vb0, vb1 = dr_zero4();
    vb0 = *reinterpret_cast<const float4*>(wp);
    if (T == 2) vb1 = *reinterpret_cast<const float4*>(wp + w_q);
    wp += w_it;
    const float* ub = ut + wm * (32 * T) + l31;
    const float* bs = Ws + hh * LDP + wn * (32 * T) + l31;
    int d = 0, e = 0;                                          // k = d D + e of the k-tile's first row (uniform)
    for (int t = 0; t < nk; ++t) {
        *reinterpret_cast<float4*>(&Ws[wr * LDP + wc4 * 4]) = vb0;
        if (T == 2) *reinterpret_cast<float4*>(&Ws[(wr + WROWS) * LDP + wc4 * 4]) = vb1;
        __syncthreads();
        if (t + 1 < nk) {
            vb0 = *reinterpret_cast<const float4*>(wp);
            if (T == 2) vb1 = *reinterpret_cast<const float4*>(wp + w_q);
            wp += w_it;
        }
#pragma unroll
        for (int kk = 0; kk < PNN_BK; kk += 2) {
            const float* ud = ub + d * LDP;
            const float* ue = ub + (e + hh) * LDP;
            float af[T], bf[T];
#pragma unroll
            for (int a = 0; a < T; ++a) af[a] = ud[32 * a] * ue[32 * a];
#pragma unroll
            for (int b = 0; b < T; ++b) bf[b] = bs[kk * LDP + 32 * b];
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
            e += 2;
            if (e >= D) { e = 0; ++d; }
        }
        __syncthreads();
    }

    // C layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int mi = 0; mi < T; ++mi)
#pragma unroll
        for (int ni = 0; ni < T; ++ni) {
            const int col = n0 + wn * (32 * T) + ni * 32 + l31;
            if (col >= N) continue;
            const int64_t row_b = m0 + wm * (32 * T) + mi * 32 + 4 * hh;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t row = row_b + (reg & 3) + 8 * (reg >> 2);
                if (row >= p.B) continue;
                float v = acc[mi][ni][reg];
                if (p.addend != nullptr) v += p.addend[row * p.ld_add + col];
                p.out[row * p.ld_out + col] = v;
            }
        }
}

// partial[part] tile 128 (d, e) x 128 n over the examples [part * per, min(B, (part + 1) * per)).
__global__ __launch_bounds__(256, 2) void pnn_dw_kernel(const PnnP p) {
    __shared__ __attribute__((aligned(16))) float us[PNN_BK * PNN_LD];     // [16][D + 4]
    __shared__ __attribute__((aligned(16))) float gs[PNN_BK * PNN_LD];     // [16][PNN_LD]
    const int D = p.D, N = p.N, DD = D * D, PU = D + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hh = lane >> 5;
    const int tiles_n = (N + 127) >> 7;
    const int m0 = (int)(blockIdx.x / tiles_n) * 128;
    const int n0 = (int)(blockIdx.x % tiles_n) * 128;
    const int64_t b_begin = (int64_t)blockIdx.y * p.per;
    const int64_t b_end = b_begin + p.per < p.B ? b_begin + p.per : p.B;

    int dt[2], et[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        int m = m0 + wm * 64 + 32 * a + l31;
        m = m < DD ? m : DD - 1;                               // rows past D^2 are not stored
        dt[a] = m / D;
        et[a] = m - dt[a] * D;
    }

    // u's k-tile: 16 examples x D / 4 float4's (at most 512), thread tid takes idx = tid and tid + 256;  g's: rows (tid >> 5) + 8 q
    const int n4 = D >> 2;
    int ur[2], uk[2]; bool uv[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int idx = tid + 256 * q;
        uv[q] = idx < PNN_BK * n4;
        ur[q] = uv[q] ? idx / n4 : 0;
        uk[q] = uv[q] ? (idx - ur[q] * n4) << 2 : 0;
    }
    const int gr = tid >> 5, gc4 = tid & 31;
    int gcol = n0 + gc4 * 4;
    gcol = gcol < p.Npad ? gcol : p.Npad - 4;

    float4 vu[2], vg[2];
    auto load = [&](int64_t bb) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t bu = bb + ur[q], bg = bb + gr + 8 * q;
            vu[q] = dr_zero4();
            vg[q] = dr_zero4();
            if (uv[q] && bu < b_end) vu[q] = *reinterpret_cast<const float4*>(p.u_in + bu * p.ld_u + uk[q]);
            if (bg < b_end) vg[q] = *reinterpret_cast<const float4*>(p.g + bg * p.ld_g + gcol);
        }
    };

    dr_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    load(b_begin);
    for (int64_t bb = b_begin; bb < b_end; bb += PNN_BK) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (uv[q]) *reinterpret_cast<float4*>(&us[ur[q] * PU + uk[q]]) = vu[q];
            *reinterpret_cast<float4*>(&gs[(gr + 8 * q) * PNN_LD + gc4 * 4]) = vg[q];
        }
        __syncthreads();
        if (bb + PNN_BK < b_end) load(bb + PNN_BK);
#pragma unroll
        for (int kk = 0; kk < PNN_BK; kk += 2) {
            const float* ux = us + (kk + hh) * PU;
            float af[2], bf[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) af[a] = ux[dt[a]] * ux[et[a]];
#pragma unroll
            for (int b = 0; b < 2; ++b) bf[b] = gs[(kk + hh) * PNN_LD + wn * 64 + 32 * b + l31];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    float* dst = p.part + (int64_t)blockIdx.y * DD * p.Npad;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = n0 + wn * 64 + ni * 32 + l31;
            if (col >= N) continue;
            const int row_b = m0 + wm * 64 + mi * 32 + 4 * hh;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = row_b + (reg & 3) + 8 * (reg >> 2);
                if (row < DD) dst[(int64_t)row * p.Npad + col] = acc[mi][ni][reg];
            }
        }
}

// dW[m, n] = partial[0][m, n] + partial[1][m, n] + ... in part order; writes N columns of every row
__global__ __launch_bounds__(256) void pnn_dw_reduce_kernel(const float* __restrict__ part, int parts, int DD, int N, int Npad,
                                                            float* __restrict__ dW, int64_t ld_dw) {
    const int n4 = Npad >> 2;
    const int64_t total = (int64_t)DD * n4, plane = (int64_t)DD * Npad;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int m = (int)(idx / n4), c = (int)(idx - (int64_t)m * n4) << 2;
        const float* src = part + (int64_t)m * Npad + c;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < parts; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < N) s[j] = q == 0 ? src[j] : s[j] + src[j];
            src += plane;
        }
        float* dst = dW + (int64_t)m * ld_dw + c;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < N) dst[j] = s[j];
    }
}

// A block owns 64 examples.  LDS: St [64][129], du [64][D + 1], ul [64][D + 1], As [16][65], Bs [16][129].
__global__ __launch_bounds__(256, 2) void pnn_du_kernel(const PnnP p) {
    extern __shared__ __attribute__((aligned(16))) float pnn_lds[];
    const int D = p.D, N = p.N, DD = D * D, PD = D + 1;
    constexpr int LA = PNN_DU_BM + 1;
    float* St = pnn_lds;
    float* du = St + PNN_DU_BM * PNN_LDT;
    float* ul = du + PNN_DU_BM * PD;
    float* As = ul + PNN_DU_BM * PD;
    float* Bs = As + PNN_BK * LA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * PNN_DU_BM;

    const int n4 = D >> 2;
    for (int idx = tid; idx < PNN_DU_BM * n4; idx += 256) {
        const int r = idx / n4, k = (idx - r * n4) << 2;
        int64_t row = m0 + r;
        row = row < p.B ? row : p.B - 1;
        const float4 v = *reinterpret_cast<const float4*>(p.u_in + row * p.ld_u + k);
        float* dst = ul + r * PD + k;
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        float* z = du + r * PD + k;
        z[0] = 0.f; z[1] = 0.f; z[2] = 0.f; z[3] = 0.f;
    }

    // operand coordinates: row tid >> 2 (+ 64 for W's second float4), n quad tid & 3 of the k-tile
    const int oi = tid >> 2, or4 = (tid & 3) << 2;
    int64_t grow = m0 + oi;
    grow = grow < p.B ? grow : p.B - 1;
    const float* gp = p.g + grow * p.ld_g;

    for (int c0 = 0; c0 < DD; c0 += 128) {
        const float* wa[2];
        const float* wb[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            int c = c0 + oi + 64 * q;
            c = c < DD ? c : DD - 1;                           // columns past D^2 are not used
            const int dd = c / D, ee = c - dd * D;
            wa[q] = p.W + (int64_t)c * p.ld_w;
            wb[q] = p.W + (int64_t)(ee * D + dd) * p.ld_w;
        }
        float4 vg, vw[2];
        // an element at or past N is zero in BOTH operands: the padding of d_out and W may hold anything
        auto load = [&](int nn) {
            const int n = nn + or4;
            vg = dr_zero4(); vw[0] = dr_zero4(); vw[1] = dr_zero4();
            if (n < N) {
                vg = *reinterpret_cast<const float4*>(gp + n);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float4 x = *reinterpret_cast<const float4*>(wa[q] + n);
                    const float4 y = *reinterpret_cast<const float4*>(wb[q] + n);
                    vw[q] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
                }
                if (n + 1 >= N) { vg.y = 0.f; vw[0].y = 0.f; vw[1].y = 0.f; }
                if (n + 2 >= N) { vg.z = 0.f; vw[0].z = 0.f; vw[1].z = 0.f; }
                if (n + 3 >= N) { vg.w = 0.f; vw[0].w = 0.f; vw[1].w = 0.f; }
            }
        };

        dr_f32x16 acc[2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

        load(0);
        for (int nn = 0; nn < N; nn += PNN_BK) {
            float* a = As + or4 * LA + oi;
            a[0] = vg.x; a[LA] = vg.y; a[2 * LA] = vg.z; a[3 * LA] = vg.w;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float* b = Bs + or4 * PNN_LDT + oi + 64 * q;
                b[0] = vw[q].x; b[PNN_LDT] = vw[q].y; b[2 * PNN_LDT] = vw[q].z; b[3 * PNN_LDT] = vw[q].w;
            }
            __syncthreads();
            if (nn + PNN_BK < N) load(nn + PNN_BK);
#pragma unroll
            for (int kk = 0; kk < PNN_BK; kk += 2) {
                const float af = As[(kk + hh) * LA + wm * 32 + l31];
                float bf[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) bf[b] = Bs[(kk + hh) * PNN_LDT + wn * 64 + 32 * b + l31];
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf[b], acc[b], 0, 0, 0);
            }
            __syncthreads();
        }

        // S^T + S of the chunk -> LDS; then thread (r, d) adds the chunk's columns of row d, e ascending
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                St[(wm * 32 + 4 * hh + (reg & 3) + 8 * (reg >> 2)) * PNN_LDT + wn * 64 + ni * 32 + l31] = acc[ni][reg];
        __syncthreads();
        const int c_end = c0 + 128 < DD ? c0 + 128 : DD;
        const int d_lo = c0 / D, nd = (c_end - 1) / D - d_lo + 1;
        for (int idx = tid; idx < PNN_DU_BM * nd; idx += 256) {
            const int r = idx & (PNN_DU_BM - 1), dd = d_lo + (idx >> 6);
            const int cs = dd * D > c0 ? dd * D : c0;
            const int ce = (dd + 1) * D < c_end ? (dd + 1) * D : c_end;
            const float* sp = St + r * PNN_LDT - c0;
            const float* up = ul + r * PD - dd * D;
            float s = du[r * PD + dd];
            for (int c = cs; c < ce; ++c) s = fmaf(sp[c], up[c], s);
            du[r * PD + dd] = s;
        }
        __syncthreads();
    }

    const int fn4 = p.F * n4;
    for (int idx = tid; idx < PNN_DU_BM * fn4; idx += 256) {
        const int r = idx / fn4, rem = idx - r * fn4;
        const int i = rem / n4, k = (rem - i * n4) << 2;
        const int64_t row = m0 + r;
        if (row >= p.B) continue;
        const float* s = du + r * PD + k;
        float4 v = make_float4(s[0], s[1], s[2], s[3]);
        float* dst = p.d_emb + row * p.ld_demb + (int64_t)i * D + k;
        if (p.accumulate) {
            const float4 o = *reinterpret_cast<const float4*>(dst);
            v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        *reinterpret_cast<float4*>(dst) = v;
    }
}

int pnn_domain(int64_t B, int32_t F, int32_t D, int32_t N) {
    if (B < 0 || F < 1 || F > PNN_MAX_F || D < 4 || D > PNN_MAX_D || (D & 3) || N < 1 || N > PNN_MAX_N) return DR_EINVAL;
    if (B > ((int64_t)1 << 31)) return DR_ESHAPE;              // keeps every grid below 2^31 blocks
    return DR_OK;
}

// the batch split of dW: runs of `per` examples, a multiple of 128; at most 64 of them
void pnn_parts(int64_t B, int64_t& per, int& parts) {
    per = 128 * ((B + 128 * PNN_MAX_PARTS - 1) / (128 * PNN_MAX_PARTS));
    if (per < 128) per = 128;
    parts = (int)((B + per - 1) / per);
    if (parts < 1) parts = 1;
}

}  // namespace

extern "C" int dr_pnn_outer_fwd(const float* emb, int64_t ld_emb, const float* W, int64_t ld_w, const float* addend, int64_t ld_add,
                                int64_t B, int32_t F, int32_t D, int32_t N, float* u, int64_t ld_u, float* out, int64_t ld_out,
                                dr_stream_t stream) {
    const int st = pnn_domain(B, F, D, N);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_emb, (int64_t)F * D) || dr_bad_ld(ld_w, N) || dr_bad_ld(ld_u, D) || dr_bad_ld(ld_out, N)) return DR_EINVAL;
    if (addend != nullptr && dr_bad_ld(ld_add, N)) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!emb || !W || !u || !out) return DR_EINVAL;
    if (!dr_aligned16(emb) || !dr_aligned16(W) || !dr_aligned16(addend) || !dr_aligned16(u) || !dr_aligned16(out)) return DR_EINVAL;
    hipLaunchKernelGGL(pnn_usum_kernel, dim3(dr_grid_for(B * (D >> 2), 256)), dim3(256), 0, dr_s(stream), emb, ld_emb, B, F, D, u, ld_u);
    DR_CHECK_LAUNCH();
    PnnP p = {};
    p.u_in = u; p.ld_u = ld_u; p.W = W; p.ld_w = ld_w; p.addend = addend; p.ld_add = ld_add; p.out = out; p.ld_out = ld_out;
    p.B = B; p.F = F; p.D = D; p.N = N; p.Npad = (N + 3) & ~3;
    const int64_t grid = ((B + 127) / 128) * ((N + 127) / 128);
    if (grid >= PNN_FWD_MIN_BLOCKS)
        return dr_launch(pnn_fwd_kernel<2>, dim3((unsigned)grid), dim3(256), (size_t)(D + PNN_BK) * 132 * sizeof(float), dr_s(stream), p);
    const int64_t small = ((B + 63) / 64) * ((N + 63) / 64);
    return dr_launch(pnn_fwd_kernel<1>, dim3((unsigned)small), dim3(256), (size_t)(D + PNN_BK) * 68 * sizeof(float), dr_s(stream), p);
}

extern "C" int64_t dr_pnn_outer_bwd_workspace_bytes(int64_t B, int32_t F, int32_t D, int32_t N) {
    const int st = pnn_domain(B, F, D, N);
    if (st != DR_OK) return st;
    int64_t per; int parts;
    pnn_parts(B, per, parts);
    return (int64_t)sizeof(float) * parts * D * D * ((N + 3) & ~3);
}

extern "C" int dr_pnn_outer_bwd(const float* u, int64_t ld_u, const float* W, int64_t ld_w, const float* d_out, int64_t ld_dout,
                                int64_t B, int32_t F, int32_t D, int32_t N, float* d_emb, int64_t ld_demb, int32_t accumulate,
                                float* dW, int64_t ld_dw, void* ws, int64_t ws_bytes, dr_stream_t stream) {
    const int st = pnn_domain(B, F, D, N);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_u, D) || dr_bad_ld(ld_w, N) || dr_bad_ld(ld_dout, N) || dr_bad_ld(ld_demb, (int64_t)F * D) || dr_bad_ld(ld_dw, N))
        return DR_EINVAL;
    if (accumulate != 0 && accumulate != 1) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!u || !W || !d_out || !d_emb || !dW || !ws) return DR_EINVAL;
    if (!dr_aligned16(u) || !dr_aligned16(W) || !dr_aligned16(d_out) || !dr_aligned16(d_emb) || !dr_aligned16(dW) || !dr_aligned16(ws))
        return DR_EINVAL;
    int64_t per; int parts;
    pnn_parts(B, per, parts);
    const int DD = D * D, Npad = (N + 3) & ~3;
    if (ws_bytes < (int64_t)sizeof(float) * parts * DD * Npad) return DR_EINVAL;
    PnnP p = {};
    p.u_in = u; p.ld_u = ld_u; p.W = W; p.ld_w = ld_w; p.g = d_out; p.ld_g = ld_dout; p.d_emb = d_emb; p.ld_demb = ld_demb;
    p.part = static_cast<float*>(ws); p.per = per; p.accumulate = accumulate;
    p.B = B; p.F = F; p.D = D; p.N = N; p.Npad = Npad;
    const int tiles = ((DD + 127) / 128) * ((N + 127) / 128);
    int rc = dr_launch(pnn_dw_kernel, dim3((unsigned)tiles, (unsigned)parts), dim3(256), 0, dr_s(stream), p);
    if (rc != DR_OK) return rc;
    hipLaunchKernelGGL(pnn_dw_reduce_kernel, dim3(dr_grid_for((int64_t)DD * (Npad >> 2), 256)), dim3(256), 0, dr_s(stream), p.part, parts,
                       DD, N, Npad, dW, ld_dw);
    DR_CHECK_LAUNCH();
    const size_t lds = (size_t)(PNN_DU_BM * PNN_LDT + 2 * PNN_DU_BM * (D + 1) + PNN_BK * (PNN_DU_BM + 1) + PNN_BK * PNN_LDT) * sizeof(float);
    return dr_launch(pnn_du_kernel, dim3((unsigned)((B + PNN_DU_BM - 1) / PNN_DU_BM)), dim3(256), lds, dr_s(stream), p);
}
