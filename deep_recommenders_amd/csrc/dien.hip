// DIEN's recurrences (Zhou et al., AAAI 2019): a GRU / AUGRU over a behaviour sequence, forward and backward, and the masked softmax
// attention of the interest-evolution layer.
//
//   step t < len[b]:  g = h_{t-1} U [3H] (columns [u | r | c]);  u = sigmoid(xp_u + g_u);  r = sigmoid(xp_r + g_r);  c = tanh(xp_c + r g_c)
//                     u' = att[b, t] u (u' = u without att);  h_t = h_{t-1} + u' (c - h_{t-1});  hs[b, t] = h_t
//   step t >= len[b]: h_t = h_{t-1}, hs[b, t] = 0; xp[b, t] and att[b, t] are not read.
//
// ONE BLOCK OWNS A TILE OF 16 EXAMPLES and runs the time loop itself.  g = h U is v_mfma_f32_16x16x4_f32 with the example on the row:
// A operand h[example c][k] as float4 from LDS (k = 16 s + 4 (lane >> 4) + e in step e of chunk s, for both operands alike), B operand
// U[k][column], held IN REGISTERS for all T steps: wave w owns the column tiles jt = w, w + NW, ... of 16 units and, for each, the three
// gate columns u, r, c of those units, so lane (c, q4) ends up with g_u, g_r, g_c of unit j = 16 jt + c for the examples 4 q4 + 0..3 and
// the whole gate arithmetic is lane-local.  h_t goes to the other half of a double-buffered [16][H16 + 4] LDS tile: one barrier per step.
// The next step's xp values are loaded before the current step's products.
// BACKWARD walks t downward, recomputes g, u, r, c from xp, U and the saved hs, and runs a second product dh_prev += dg U^T with the
// example on the row again: A operand dg[example][column] from a [16][3 H16 + 4] LDS tile, B operand U[j][column] in a second set of
// registers.  d_att[b, t] = sum_j du'_j u_j: 16-lane xor sums, then the waves' parts are added in wave order by one lane.  dg is written
// to the workspace (rows t = 0 apart, rows t >= 1 shifted by one so that row s pairs with hs[b, s]); dU = sum h_{t-1}^T dg is then
// dr_linear_bwd_dw over hs (and once more over h0), which adds in a fixed order.  No float atomics anywhere.
#include "dr_common.h"

namespace {


constexpr int GRU_MAX_H = 128;
constexpr int GRU_MAX_BLOCKS = 512;

struct GruP {
    const float* xp; int64_t ld_xp;
    const float* U; const float* h0; const int32_t* lengths; const float* att;
    const float* hs_in; const float* d_hs; int64_t ld_dhs; const float* d_h_last;      // backward
    float* hs; int64_t ld_hs; float* h_last;                                            // forward (ld_hs shared)
    float* d_xp; int64_t ld_dxp; float* d_h0; float* d_att; float* dg0; float* dgs;
    int64_t B, ntiles;
    int32_t T, H;
};


// ureg[tp][g][s][e] = U[k = 16 s + 4 q4 + e][g H + 16 jt + c] (zero beyond H), jt = wave + NW tp
template <int JT, int NW, int TPW>
__device__ __forceinline__ void gru_load_u(const GruP& p, int wave, int c, int q4, float (&ureg)[TPW][3][JT][4]) {
    const int H = p.H;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
        const int jt = wave + NW * tp, j = 16 * jt + c;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int s = 0; s < JT; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * s + 4 * q4 + e;
                    ureg[tp][g][s][e] = (jt < JT && j < H && k < H) ? p.U[(int64_t)k * 3 * H + g * H + j] : 0.f;
                }
    }
}

// acc[tp][g] = rows of hl times the wave's columns of U
template <int JT, int TPW>
__device__ __forceinline__ void gru_h_times_u(const float* hl, int PH, int c, int q4, const float (&ureg)[TPW][3][JT][4],
                                              dr_f32x4 (&acc)[TPW][3]) {
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[tp][g] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < JT; ++s) {
        const float4 a4 = *reinterpret_cast<const float4*>(hl + c * PH + 16 * s + 4 * q4);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    acc[tp][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], ureg[tp][g][s][e], acc[tp][g], 0, 0, 0);
    }
}

template <int JT>
__global__ __launch_bounds__(256) void gru_fwd_kernel(const GruP p) {
    constexpr int NW = JT < 4 ? JT : 4, TPW = (JT + NW - 1) / NW, H16 = 16 * JT, PH = H16 + 4;
    __shared__ float hl[2][16 * PH];
    __shared__ int lens[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q4 = lane >> 4;
    const int H = p.H, T = p.T;
    float ureg[TPW][3][JT][4];
    gru_load_u<JT, NW, TPW>(p, wave, c, q4, ureg);
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * 16;
        __syncthreads();                                       // the previous tile's lens and rows are read
        if (threadIdx.x < 16) {
            const int64_t b = b0 + threadIdx.x;
            int l = 0;
            if (b < p.B) l = p.lengths != nullptr ? min(max(p.lengths[b], 0), T) : T;
            lens[threadIdx.x] = l;
        }
        __syncthreads();
        int len[4], lmax = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) len[r] = lens[4 * q4 + r];
        for (int i = 0; i < 16; ++i) lmax = max(lmax, lens[i]);
        float h[TPW][4];
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int jt = wave + NW * tp, j = 16 * jt + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                h[tp][r] = (jt < JT && j < H && b < p.B && p.h0 != nullptr) ? p.h0[b * H + j] : 0.f;
                if (jt < JT) hl[0][(4 * q4 + r) * PH + j] = h[tp][r];
            }
        }
        float xn[TPW][3][4], an[4];
        auto prefetch = [&](int t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                const bool on = t < len[r];
                an[r] = (on && p.att != nullptr) ? p.att[b * T + t] : 1.f;
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) {
                    const int jt = wave + NW * tp, j = 16 * jt + c;
                    const float* src = p.xp + (b * T + t) * p.ld_xp + j;
#pragma unroll
                    for (int g = 0; g < 3; ++g) xn[tp][g][r] = (on && jt < JT && j < H) ? src[g * H] : 0.f;
                }
            }
        };
        if (lmax > 0) prefetch(0);
        __syncthreads();
        for (int t = 0; t < lmax; ++t) {
            const int cur = t & 1;
            float x[TPW][3][4], a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a[r] = an[r];
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
                    for (int g = 0; g < 3; ++g) x[tp][g][r] = xn[tp][g][r];
            }
            if (t + 1 < lmax) prefetch(t + 1);
            dr_f32x4 acc[TPW][3];
            gru_h_times_u<JT, TPW>(hl[cur], PH, c, q4, ureg, acc);
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) {
                const int jt = wave + NW * tp, j = 16 * jt + c;
                if (jt >= JT) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t b = b0 + 4 * q4 + r;
                    if (j < H && b < p.B) {
                        float out = 0.f;
                        if (t < len[r]) {
                            const float u = dr_sigmoidf(x[tp][0][r] + acc[tp][0][r]);
                            const float rg = dr_sigmoidf(x[tp][1][r] + acc[tp][1][r]);
                            const float cc = tanhf(fmaf(rg, acc[tp][2][r], x[tp][2][r]));
                            const float up = p.att != nullptr ? a[r] * u : u;
                            h[tp][r] = fmaf(up, cc - h[tp][r], h[tp][r]);
                            out = h[tp][r];
                        }
                        p.hs[(b * T + t) * p.ld_hs + j] = out;
                    }
                    hl[cur ^ 1][(4 * q4 + r) * PH + j] = h[tp][r];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int jt = wave + NW * tp, j = 16 * jt + c;
            if (jt >= JT || j >= H) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                if (b >= p.B) continue;
                for (int t = lmax; t < T; ++t) p.hs[(b * T + t) * p.ld_hs + j] = 0.f;
                p.h_last[b * H + j] = h[tp][r];
            }
        }
    }
}

template <int JT>
__global__ __launch_bounds__(256) void gru_bwd_kernel(const GruP p) {
    constexpr int NW = JT < 4 ? JT : 4, TPW = (JT + NW - 1) / NW, H16 = 16 * JT, PH = H16 + 4, PG = 3 * H16 + 4;
    __shared__ float hl[2][16 * PH];
    __shared__ float dgl[16 * PG];
    __shared__ float red[4][16];
    __shared__ int lens[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q4 = lane >> 4;
    const int H = p.H, T = p.T;
    float ureg[TPW][3][JT][4];
    gru_load_u<JT, NW, TPW>(p, wave, c, q4, ureg);
    // utreg[tp][g][s][e] = U[j = 16 jt + c][g H + 16 s + 4 q4 + e] (zero beyond H)
    float utreg[TPW][3][JT][4];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
        const int jt = wave + NW * tp, j = 16 * jt + c;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int s = 0; s < JT; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * s + 4 * q4 + e;
                    utreg[tp][g][s][e] = (jt < JT && j < H && k < H) ? p.U[(int64_t)j * 3 * H + g * H + k] : 0.f;
                }
    }
    for (int64_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * 16;
        __syncthreads();
        if (threadIdx.x < 16) {
            const int64_t b = b0 + threadIdx.x;
            int l = 0;
            if (b < p.B) l = p.lengths != nullptr ? min(max(p.lengths[b], 0), T) : T;
            lens[threadIdx.x] = l;
        }
        __syncthreads();
        int len[4], lmax = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) len[r] = lens[4 * q4 + r];
        for (int i = 0; i < 16; ++i) lmax = max(lmax, lens[i]);
        float dh[TPW][4];
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int jt = wave + NW * tp, j = 16 * jt + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                dh[tp][r] = (jt < JT && j < H && b < p.B && p.d_h_last != nullptr) ? p.d_h_last[b * H + j] : 0.f;
            }
        }
        // the [16][H16] tile of h_{t-1}: thread -> float4 idx = tid + 64 NW i of row idx / (4 JT); zero for a masked row and beyond H
        float4 pf[TPW];
        auto load_hprev = [&](int t) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int idx = threadIdx.x + 64 * NW * i, row = idx / (4 * JT), col = 4 * (idx - row * 4 * JT);
                pf[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx < 64 * JT && col < H && t < lens[row]) {
                    const int64_t b = b0 + row;
                    if (t > 0) pf[i] = *reinterpret_cast<const float4*>(p.hs_in + (b * T + t - 1) * p.ld_hs + col);
                    else if (p.h0 != nullptr) pf[i] = *reinterpret_cast<const float4*>(p.h0 + b * H + col);
                }
            }
        };
        auto store_hprev = [&](int buf) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int idx = threadIdx.x + 64 * NW * i, row = idx / (4 * JT), col = 4 * (idx - row * 4 * JT);
                if (idx < 64 * JT) *reinterpret_cast<float4*>(&hl[buf][row * PH + col]) = pf[i];
            }
        };
        float xn[TPW][3][4], dn[TPW][4], an[4];
        auto prefetch = [&](int t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                const bool on = t < len[r];
                an[r] = (on && p.att != nullptr) ? p.att[b * T + t] : 1.f;
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) {
                    const int jt = wave + NW * tp, j = 16 * jt + c;
                    const bool ok = on && jt < JT && j < H;
                    const float* src = p.xp + (b * T + t) * p.ld_xp + j;
#pragma unroll
                    for (int g = 0; g < 3; ++g) xn[tp][g][r] = ok ? src[g * H] : 0.f;
                    dn[tp][r] = (ok && p.d_hs != nullptr) ? p.d_hs[(b * T + t) * p.ld_dhs + j] : 0.f;
                }
            }
        };
        // row t of example b in the workspace: t = 0 in dg0, t >= 1 at row t - 1 of dgs (so that it pairs with hs[b, t - 1])
        auto dg_row = [&](int64_t b, int t) { return t == 0 ? p.dg0 + b * 3 * H : p.dgs + (b * T + t - 1) * 3 * H; };
        if (lmax > 0) {
            load_hprev(lmax - 1);
            store_hprev((lmax - 1) & 1);
            prefetch(lmax - 1);
        }
        __syncthreads();
        for (int t = lmax - 1; t >= 0; --t) {
            const int cur = t & 1;
            float x[TPW][3][4], dv[TPW][4], a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a[r] = an[r];
#pragma unroll
                for (int tp = 0; tp < TPW; ++tp) {
                    dv[tp][r] = dn[tp][r];
#pragma unroll
                    for (int g = 0; g < 3; ++g) x[tp][g][r] = xn[tp][g][r];
                }
            }
            if (t > 0) {
                prefetch(t - 1);
                load_hprev(t - 1);
            }
            dr_f32x4 acc[TPW][3];
            gru_h_times_u<JT, TPW>(hl[cur], PH, c, q4, ureg, acc);
            float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) {
                const int jt = wave + NW * tp, j = 16 * jt + c;
                if (jt >= JT) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ex = 4 * q4 + r;
                    const int64_t b = b0 + ex;
                    float dgv[3] = {0.f, 0.f, 0.f};
                    if (j < H && b < p.B) {
                        float dx[3] = {0.f, 0.f, 0.f};
                        if (t < len[r]) {
                            const float hp = hl[cur][ex * PH + j];
                            const float gc = acc[tp][2][r];
                            const float u = dr_sigmoidf(x[tp][0][r] + acc[tp][0][r]);
                            const float rg = dr_sigmoidf(x[tp][1][r] + acc[tp][1][r]);
                            const float cc = tanhf(fmaf(rg, gc, x[tp][2][r]));
                            const float up = p.att != nullptr ? a[r] * u : u;
                            const float d = dh[tp][r] + dv[tp][r];
                            const float dc = d * up, dup = d * (cc - hp);
                            dh[tp][r] = d * (1.f - up);
                            part[r] = fmaf(dup, u, part[r]);
                            const float du = p.att != nullptr ? a[r] * dup : dup;
                            const float dpc = dc * (1.f - cc * cc);
                            dx[0] = du * u * (1.f - u);
                            dx[1] = dpc * gc * rg * (1.f - rg);
                            dx[2] = dpc;
                            dgv[0] = dx[0]; dgv[1] = dx[1]; dgv[2] = dpc * rg;
                        }
                        float* dxp = p.d_xp + (b * T + t) * p.ld_dxp + j;
                        float* dgw = dg_row(b, t) + j;
#pragma unroll
                        for (int g = 0; g < 3; ++g) {
                            dxp[g * H] = dx[g];
                            dgw[g * H] = dgv[g];
                        }
                    }
#pragma unroll
                    for (int g = 0; g < 3; ++g) dgl[ex * PG + g * H16 + j] = dgv[g];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) part[r] += __shfl_xor(part[r], o, 64);
                if (c == 0) red[wave][4 * q4 + r] = part[r];
            }
            if (t > 0) store_hprev(cur ^ 1);
            __syncthreads();                                   // dgl, red and the next h_{t-1} are written
            if (threadIdx.x < 16 && p.d_att != nullptr && b0 + threadIdx.x < p.B) {
                float s = 0.f;
                if (t < lens[threadIdx.x]) {
                    s = red[0][threadIdx.x];
                    for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
                }
                p.d_att[(b0 + threadIdx.x) * T + t] = s;
            }
            // dh_prev += dg U^T
            dr_f32x4 acc2[TPW];
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) acc2[tp] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int s = 0; s < JT; ++s) {
                    const float4 a4 = *reinterpret_cast<const float4*>(dgl + c * PG + g * H16 + 16 * s + 4 * q4);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int tp = 0; tp < TPW; ++tp)
                            acc2[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], utreg[tp][g][s][e], acc2[tp], 0, 0, 0);
                }
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t < len[r]) dh[tp][r] += acc2[tp][r];
            __syncthreads();                                   // dgl and red are read
        }
        // masked steps beyond the tile's longest example, the workspace's row T, and d_h0
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int jt = wave + NW * tp, j = 16 * jt + c;
            if (jt >= JT || j >= H) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = b0 + 4 * q4 + r;
                if (b >= p.B) continue;
                for (int t = lmax; t <= T; ++t) {
                    float* dgw = dg_row(b, t) + j;
                    dgw[0] = 0.f; dgw[H] = 0.f; dgw[2 * H] = 0.f;
                    if (t < T) {
                        float* dxp = p.d_xp + (b * T + t) * p.ld_dxp + j;
                        dxp[0] = 0.f; dxp[H] = 0.f; dxp[2 * H] = 0.f;
                    }
                }
                if (p.d_h0 != nullptr) p.d_h0[b * H + j] = dh[tp][r];
            }
        }
        if (threadIdx.x < 16 && p.d_att != nullptr && b0 + threadIdx.x < p.B)
            for (int t = lmax; t < T; ++t) p.d_att[(b0 + threadIdx.x) * T + t] = 0.f;
    }
}

// ---- the evolution layer's attention: a[b, t] = softmax over t < len[b] of <hs[b, t], q[b]>, 0 at masked steps -----------------------
// One wave per example.  Forward: lane t mod 64 owns step t (the dot product runs over j in order), the scores pass through a.
__global__ __launch_bounds__(256) void seq_attn_fwd_kernel(const float* __restrict__ hs, int64_t ld_hs, const float* __restrict__ q,
                                                           const int32_t* __restrict__ lengths, int64_t B, int T, int H,
                                                           float* __restrict__ a) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += nwaves) {
        const int len = lengths != nullptr ? min(max(lengths[b], 0), T) : T;
        const float* qb = q + b * H;
        float* ab = a + b * T;
        float m = -INFINITY;
        for (int t = lane; t < len; t += 64) {
            const float* row = hs + (b * T + t) * ld_hs;
            float s = 0.f;
            for (int j = 0; j < H; j += 4) {
                const float4 hv = *reinterpret_cast<const float4*>(row + j);
                const float4 qv = *reinterpret_cast<const float4*>(qb + j);
                s = fmaf(hv.x, qv.x, s); s = fmaf(hv.y, qv.y, s); s = fmaf(hv.z, qv.z, s); s = fmaf(hv.w, qv.w, s);
            }
            ab[t] = s;
            m = fmaxf(m, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float l = 0.f;
        for (int t = lane; t < len; t += 64) {                 // the lane reads back what it wrote
            const float e = expf(ab[t] - m);
            ab[t] = e;
            l += e;
        }
        l = dr_wave_sum(l);
        for (int t = lane; t < T; t += 64) ab[t] = t < len ? ab[t] / l : 0.f;
    }
}

// ds_t = a_t (d_a_t - sum_t' a_t' d_a_t');  d_hs[b, t] = ds_t q[b] (0 at masked steps);  d_q[b] = sum_t ds_t hs[b, t].  The lane owns the
// columns j = lane, lane + 64 and adds over t in order.
__global__ __launch_bounds__(256) void seq_attn_bwd_kernel(const float* __restrict__ hs, int64_t ld_hs, const float* __restrict__ q,
                                                           const int32_t* __restrict__ lengths, const float* __restrict__ a,
                                                           const float* __restrict__ d_a, int64_t B, int T, int H,
                                                           float* __restrict__ d_hs, int64_t ld_dhs, float* __restrict__ d_q) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += nwaves) {
        const int len = lengths != nullptr ? min(max(lengths[b], 0), T) : T;
        const float* ab = a + b * T;
        const float* db = d_a + b * T;
        float dot = 0.f;
        for (int t = lane; t < len; t += 64) dot = fmaf(ab[t], db[t], dot);
        dot = dr_wave_sum(dot);
        const int j0 = lane, j1 = lane + 64;
        const float q0 = j0 < H ? q[b * H + j0] : 0.f, q1 = j1 < H ? q[b * H + j1] : 0.f;
        float dq0 = 0.f, dq1 = 0.f;
        for (int t = 0; t < T; ++t) {
            const int64_t row = b * T + t;
            if (t < len) {
                const float ds = ab[t] * (db[t] - dot);
                if (j0 < H) { d_hs[row * ld_dhs + j0] = ds * q0; dq0 = fmaf(ds, hs[row * ld_hs + j0], dq0); }
                if (j1 < H) { d_hs[row * ld_dhs + j1] = ds * q1; dq1 = fmaf(ds, hs[row * ld_hs + j1], dq1); }
            } else {
                if (j0 < H) d_hs[row * ld_dhs + j0] = 0.f;
                if (j1 < H) d_hs[row * ld_dhs + j1] = 0.f;
            }
        }
        if (j0 < H) d_q[b * H + j0] = dq0;
        if (j1 < H) d_q[b * H + j1] = dq1;
    }
}

// DR_OK inside the domain of all five entry points
int gru_domain(int64_t B, int32_t T, int32_t H) {
    if (B < 0 || T < 1 || H < 4 || (H & 3)) return DR_EINVAL;
    if (H > GRU_MAX_H || B * (int64_t)T > (int64_t)1 << 40) return DR_ESHAPE;
    return DR_OK;
}

int64_t gru_dw_ws_bytes(int64_t B, int32_t T, int32_t H) {
    const int64_t a = dr_linear_bwd_dw_workspace_bytes(B * T, H, 3 * H), b = dr_linear_bwd_dw_workspace_bytes(B, H, 3 * H);
    return ((a > b ? a : b) + 15) / 16 * 16;
}

template <typename K>
int gru_launch(K kernel, int JT, const GruP& p, dr_stream_t stream) {
    const int nw = JT < 4 ? JT : 4;
    const int64_t grid = p.ntiles < GRU_MAX_BLOCKS ? p.ntiles : GRU_MAX_BLOCKS;
    return dr_launch(kernel, dim3((unsigned)grid), dim3(64 * nw), 0, dr_s(stream), p);
}

}  // namespace

#define GRU_CASE(name, jt) \
    case jt: return gru_launch(name<jt>, jt, p, stream)
#define GRU_DISPATCH(name)                                                                      \
    switch ((p.H + 15) / 16) {                                                                  \
        GRU_CASE(name, 1); GRU_CASE(name, 2); GRU_CASE(name, 3); GRU_CASE(name, 4);             \
        GRU_CASE(name, 5); GRU_CASE(name, 6); GRU_CASE(name, 7); GRU_CASE(name, 8);             \
    }                                                                                           \
    return DR_ESHAPE

static int gru_fwd_dispatch(const GruP& p, dr_stream_t stream) { GRU_DISPATCH(gru_fwd_kernel); }
static int gru_bwd_dispatch(const GruP& p, dr_stream_t stream) { GRU_DISPATCH(gru_bwd_kernel); }

extern "C" int dr_gru_seq_fwd(const float* xp, int64_t ld_xp, const float* U, const float* h0, const int32_t* lengths, const float* att,
                              int64_t B, int32_t T, int32_t H, float* hs, int64_t ld_hs, float* h_last, dr_stream_t stream) {
    const int st = gru_domain(B, T, H);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_xp, 3 * H) || dr_bad_ld(ld_hs, H)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!xp || !U || !hs || !h_last) return DR_EINVAL;
    if (!dr_aligned16(xp) || !dr_aligned16(hs) || !dr_aligned16(h0)) return DR_EINVAL;
    GruP p = {};
    p.xp = xp; p.ld_xp = ld_xp; p.U = U; p.h0 = h0; p.lengths = lengths; p.att = att;
    p.hs = hs; p.ld_hs = ld_hs; p.h_last = h_last;
    p.B = B; p.T = T; p.H = H; p.ntiles = (B + 15) / 16;
    return gru_fwd_dispatch(p, stream);
}

extern "C" int64_t dr_gru_seq_bwd_workspace_bytes(int64_t B, int32_t T, int32_t H) {
    const int st = gru_domain(B, T, H);
    if (st != DR_OK) return st;
    if (B == 0) return 0;
    return 4 * B * ((int64_t)T + 1) * 3 * H + gru_dw_ws_bytes(B, T, H);
}

extern "C" int dr_gru_seq_bwd(const float* xp, int64_t ld_xp, const float* U, const float* h0, const int32_t* lengths, const float* att,
                              const float* hs, int64_t ld_hs, int64_t B, int32_t T, int32_t H, const float* d_hs, int64_t ld_dhs,
                              const float* d_h_last, float* d_xp, int64_t ld_dxp, float* dU, float* d_h0, float* d_att, void* ws,
                              int64_t ws_bytes, dr_stream_t stream) {
    const int st = gru_domain(B, T, H);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_xp, 3 * H) || dr_bad_ld(ld_hs, H) || dr_bad_ld(ld_dxp, 3 * H)) return DR_EINVAL;
    if (d_hs != nullptr && dr_bad_ld(ld_dhs, H)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!xp || !U || !hs || !d_xp || !dU || !ws) return DR_EINVAL;
    if (!dr_aligned16(xp) || !dr_aligned16(hs) || !dr_aligned16(d_xp) || !dr_aligned16(ws) || !dr_aligned16(h0) || !dr_aligned16(d_hs))
        return DR_EINVAL;
    if (ws_bytes < dr_gru_seq_bwd_workspace_bytes(B, T, H)) return DR_EINVAL;
    GruP p = {};
    p.xp = xp; p.ld_xp = ld_xp; p.U = U; p.h0 = h0; p.lengths = lengths; p.att = att;
    p.hs_in = hs; p.ld_hs = ld_hs; p.d_hs = d_hs; p.ld_dhs = ld_dhs; p.d_h_last = d_h_last;
    p.d_xp = d_xp; p.ld_dxp = ld_dxp; p.d_h0 = d_h0; p.d_att = d_att;
    p.dg0 = static_cast<float*>(ws);
    p.dgs = p.dg0 + B * 3 * H;
    float* lws = p.dgs + B * (int64_t)T * 3 * H;
    const int64_t lws_bytes = gru_dw_ws_bytes(B, T, H);
    p.B = B; p.T = T; p.H = H; p.ntiles = (B + 15) / 16;
    const int st2 = gru_bwd_dispatch(p, stream);
    if (st2 != DR_OK) return st2;
    // dU = sum_b sum_t h_{t-1}^T dg_t: rows (b, s) of hs against the shifted dg rows, then h0 against the rows t = 0
    if (hipMemsetAsync(dU, 0, sizeof(float) * (size_t)H * 3 * H, dr_s(stream)) != hipSuccess) return DR_ELAUNCH;
    int st3 = dr_linear_bwd_dw(hs, ld_hs, p.dgs, 3 * H, B * T, H, 3 * H, 1.f, dU, 3 * H, nullptr, lws, lws_bytes, stream);
    if (st3 != DR_OK) return st3;
    if (h0 != nullptr) st3 = dr_linear_bwd_dw(h0, H, p.dg0, 3 * H, B, H, 3 * H, 1.f, dU, 3 * H, nullptr, lws, lws_bytes, stream);
    return st3;
}

extern "C" int dr_seq_attn_fwd(const float* hs, int64_t ld_hs, const float* q, const int32_t* lengths, int64_t B, int32_t T, int32_t H,
                               float* a, dr_stream_t stream) {
    const int st = gru_domain(B, T, H);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_hs, H)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!hs || !q || !a || !dr_aligned16(hs) || !dr_aligned16(q)) return DR_EINVAL;
    hipLaunchKernelGGL(seq_attn_fwd_kernel, dim3(dr_grid_for(B, 4)), dim3(256), 0, dr_s(stream), hs, ld_hs, q, lengths, B, T, H, a);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_seq_attn_bwd(const float* hs, int64_t ld_hs, const float* q, const int32_t* lengths, const float* a, const float* d_a,
                               int64_t B, int32_t T, int32_t H, float* d_hs, int64_t ld_dhs, float* d_q, dr_stream_t stream) {
    const int st = gru_domain(B, T, H);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_hs, H) || dr_bad_ld(ld_dhs, H)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!hs || !q || !a || !d_a || !d_hs || !d_q || !dr_aligned16(hs) || !dr_aligned16(q) || !dr_aligned16(d_hs)) return DR_EINVAL;
    hipLaunchKernelGGL(seq_attn_bwd_kernel, dim3(dr_grid_for(B, 4)), dim3(256), 0, dr_s(stream), hs, ld_hs, q, lengths, a, d_a, B, T, H,
                       d_hs, ld_dhs, d_q);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
