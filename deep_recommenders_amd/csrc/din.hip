// DIN (keras/models/ranking/din.py of the reference) on gfx950:
//   * dr_dice_fwd / dr_dice_bwd          the Dice activation (din.py:88-130) over the rows of x [M, N], literally as the reference
//     computes it: the standard deviation s (named "var" there) gets ANOTHER square root, r = 1 / sqrt(s + eps);
//   * dr_din_pool_fwd / dr_din_pool_bwd  the ActivationUnit (din.py:8-86) scored for every key of a behaviour sequence against the
//     example's query, and the sequence summed with those scores; the [B*T, 3D] pair matrix never exists.
//
// Dice: one wave owns a row (lane l owns columns l, l + 64, ...; rows of up to 256 columns stay in registers, wider rows are re-read),
// reductions are dr_wave_sum.  Backward:  dx_i = dpre_i * prelu'(x_i) + r (c_i - mean c) - 0.5 r^3 (sum_j c_j (x_j - m)) (x_i - m) / (N s).
// DEVIATION from TensorFlow: where s == 0 (a constant row; always for N == 1) the last term is taken as ZERO; TF returns NaN there
// (0 / 0 in the gradient of sqrt), and a dead unit row with a zero bias is such a row.  dalpha is summed over rows in a fixed order in
// two stages (1024-row chunks, then the chunks by 16 interleaved lanes and a fixed tree): no float atomics.
//
// Pooling forward, one block per example, one launch: the query's share of the hidden layer hq = q W[0:D] (+ q W[2D:3D]) + b is one
// vector; the per-key share is keys_b [T, D] . Weff_b [D, U] with Weff = W[D:2D] (mode 0), W[D:2D] - W[2D:3D] (mode 1: q - k),
// W[D:2D] + diag(q_b) W[2D:3D] (mode 2: q * k), built once per example in LDS.  A wave owns 16 keys and computes the TRANSPOSED tile
// H^T = Weff^T K^T on the fp32-input MFMA v_mfma_f32_16x16x4_f32 (lane (i16, g): key i16, hidden units 16 ut + 4 g + r), so a key's
// activation, Dice statistics and score are reductions inside a lane plus two cross-lane steps.  The score-weighted sum of the keys is
// T * D multiply-adds per example on the VALU from the registers that already hold the keys as the MFMA operand (1 / U of the product).
// Masked keys are SKIPPED: they are never loaded (select at the load), so whatever they hold reaches no result; tiles without a valid
// key are not computed.  The sum over t runs in a fixed order (per wave: its tiles ascending; 16 keys by a shuffle tree; 4 waves).
//
// Pooling backward, three launches: (1) per example, the hidden layer is recomputed, dH [T, U] is written to the one [B*T, U]
// intermediate G (zero rows at masked keys), d_keys = score * d_out + dH Weff^T and (mode 2) q's share through dH W[2D:3D]^T on the
// MFMA, d_query; d_w_out / d_b_out / dalpha are carried in registers over a block's contiguous range of examples and written as one
// partial per block.  (2) dW and db: row chunks of (keys, G) -> partial K^T G, q^T G, (q * k)^T G on the MFMA, one partial per chunk.
// (3) the partials summed in a fixed order (16 interleaved lanes per element, then a fixed tree).  No float atomics, no inter-block waits: two runs are bit-equal.
#include "dr_common.h"
#include <math.h>
#include <algorithm>

namespace {

// Dice of one element given its row's mean m and r = 1 / sqrt(s + eps): p, the PReLU output and y
__device__ __forceinline__ float dice_elem(float x, float al, float m, float r, float& p, float& pre) {
    p = dr_sigmoidf((x - m) * r);
    pre = fmaxf(x, 0.f) - al * fmaxf(-x, 0.f);
    return pre > 0.f ? p * pre : (1.f - p) * pre;
}

// the two per-element factors of the backward: dpre = dy * dy/dpre, c = dy * dy/dz with z = (x - m) r
__device__ __forceinline__ void dice_elem_bwd(float x, float al, float m, float r, float dy, float& dpre, float& c) {
    float p, pre;
    dice_elem(x, al, m, r, p, pre);
    const bool pos = pre > 0.f;
    dpre = dy * (pos ? p : 1.f - p);
    c = dy * pre * (pos ? 1.f : -1.f) * p * (1.f - p);
}

__device__ __forceinline__ float dice_dx(float x, float al, float m, float s, float r, float n, float dpre, float c, float csum, float cxsum) {
    float dx = dpre * (x > 0.f ? 1.f : x < 0.f ? al : 0.f) + r * (c - csum / n);
    if (s > 0.f) dx -= 0.5f * r * r * r * cxsum * (x - m) / (n * s);     // s == 0: taken as zero (see the head of the file)
    return dx;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Dice over the rows of a matrix
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int DICE_REG = 4;            // columns per lane kept in registers (N <= 256)
constexpr int DICE_CHUNK = 1024;       // rows per first-stage dalpha partial

template <bool REG>
__device__ __forceinline__ void dice_row_stats(const float* __restrict__ row, int N, int lane, float (&xr)[DICE_REG], float eps, float& m,
                                               float& s, float& r) {
    float acc = 0.f;
    if (REG) {
#pragma unroll
        for (int k = 0; k < DICE_REG; ++k) {
            const int j = lane + 64 * k;
            xr[k] = j < N ? row[j] : 0.f;
            acc += xr[k];
        }
    } else {
        for (int j = lane; j < N; j += 64) acc += row[j];
    }
    m = dr_wave_sum(acc) / (float)N;
    acc = 0.f;
    if (REG) {
#pragma unroll
        for (int k = 0; k < DICE_REG; ++k)
            if (lane + 64 * k < N) acc += (xr[k] - m) * (xr[k] - m);
    } else {
        for (int j = lane; j < N; j += 64) acc += (row[j] - m) * (row[j] - m);
    }
    s = sqrtf(dr_wave_sum(acc) / (float)N);
    r = 1.f / sqrtf(s + eps);
}

template <bool REG>
__global__ __launch_bounds__(256) void dice_fwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ alpha, int64_t M,
                                                       int N, float eps, float* __restrict__ y, int64_t ld_y) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const float* xp = x + row * ld_x;
        float* yp = y + row * ld_y;
        float xr[DICE_REG], m, s, r, p, pre;
        dice_row_stats<REG>(xp, N, lane, xr, eps, m, s, r);
        if (REG) {
#pragma unroll
            for (int k = 0; k < DICE_REG; ++k) {
                const int j = lane + 64 * k;
                if (j < N) yp[j] = dice_elem(xr[k], alpha[j], m, r, p, pre);
            }
        } else {
            for (int j = lane; j < N; j += 64) yp[j] = dice_elem(xp[j], alpha[j], m, r, p, pre);
        }
    }
}

// dx and the row statistic (m, r) that the dalpha stage reads back
template <bool REG>
__global__ __launch_bounds__(256) void dice_bwd_dx_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ alpha,
                                                          const float* __restrict__ dy, int64_t ld_dy, int64_t M, int N, float eps,
                                                          float* __restrict__ dx, int64_t ld_dx, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
        const float* xp = x + row * ld_x;
        const float* dyp = dy + row * ld_dy;
        float* dxp = dx + row * ld_dx;
        float xr[DICE_REG], m, s, r;
        dice_row_stats<REG>(xp, N, lane, xr, eps, m, s, r);
        float csum = 0.f, cxsum = 0.f;
        if (REG) {
            float dprer[DICE_REG], cr[DICE_REG];
#pragma unroll
            for (int k = 0; k < DICE_REG; ++k) {
                const int j = lane + 64 * k;
                dprer[k] = cr[k] = 0.f;
                if (j < N) {
                    dice_elem_bwd(xr[k], alpha[j], m, r, dyp[j], dprer[k], cr[k]);
                    csum += cr[k];
                    cxsum += cr[k] * (xr[k] - m);
                }
            }
            csum = dr_wave_sum(csum);
            cxsum = dr_wave_sum(cxsum);
#pragma unroll
            for (int k = 0; k < DICE_REG; ++k) {
                const int j = lane + 64 * k;
                if (j < N) dxp[j] = dice_dx(xr[k], alpha[j], m, s, r, (float)N, dprer[k], cr[k], csum, cxsum);
            }
        } else {
            float dpre, c;
            for (int j = lane; j < N; j += 64) {
                dice_elem_bwd(xp[j], alpha[j], m, r, dyp[j], dpre, c);
                csum += c;
                cxsum += c * (xp[j] - m);
            }
            csum = dr_wave_sum(csum);
            cxsum = dr_wave_sum(cxsum);
            for (int j = lane; j < N; j += 64) {
                dice_elem_bwd(xp[j], alpha[j], m, r, dyp[j], dpre, c);
                dxp[j] = dice_dx(xp[j], alpha[j], m, s, r, (float)N, dpre, c, csum, cxsum);
            }
        }
        if (lane == 0) {
            stats[2 * row] = m;
            stats[2 * row + 1] = r;
        }
    }
}

// stage 1: partial[chunk][j] = sum over the chunk's rows (4 interleaved row lanes, each ascending, then (0 + 1) + (2 + 3))
__global__ __launch_bounds__(256) void dice_dalpha_partial_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ alpha,
                                                                  const float* __restrict__ dy, int64_t ld_dy, int64_t M, int N,
                                                                  const float* __restrict__ stats, float* __restrict__ partial) {
    __shared__ float part[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int j = blockIdx.y * 64 + cl;
    const int64_t r0 = (int64_t)blockIdx.x * DICE_CHUNK, r1 = r0 + DICE_CHUNK < M ? r0 + DICE_CHUNK : M;
    float acc = 0.f;
    if (j < N) {
        const float al = alpha[j];
        for (int64_t row = r0 + rl; row < r1; row += 4) {
            const float xv = x[row * ld_x + j];
            float dpre, c;
            dice_elem_bwd(xv, al, stats[2 * row], stats[2 * row + 1], dy[row * ld_dy + j], dpre, c);
            acc += dpre * fminf(xv, 0.f);
        }
    }
    part[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && j < N) partial[(int64_t)blockIdx.x * N + j] = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
}

// stage 2 (also the pooling's): dst[j] = sum_c partial[c * ld + j] in a fixed order -- 16 row lanes per column, lane l over the chunks
// l, l + 16, ... ascending, then a fixed tree over the lanes
__device__ __forceinline__ float din_tree16(float (*part)[16], int rl, int cl, float acc) {
    part[rl][cl] = acc;
    __syncthreads();
    float v = 0.f;
    if (rl == 0) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = part[2 * i][cl] + part[2 * i + 1][cl];
        v = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    }
    return v;
}

__global__ __launch_bounds__(256) void din_colsum_kernel(const float* __restrict__ partial, int64_t chunks, int64_t ld, int n,
                                                         float* __restrict__ dst) {
    __shared__ float part[16][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + cl;
    float acc = 0.f;
    if (j < n) {
#pragma unroll 4
        for (int64_t c = rl; c < chunks; c += 16) acc += partial[c * ld + j];
    }
    const float v = din_tree16(part, rl, cl, acc);
    if (rl == 0 && j < n) dst[j] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Interest pooling
// ---------------------------------------------------------------------------------------------------------------------------------
struct PoolP {
    const float *q, *keys, *W, *b, *w_out, *b_out, *alpha, *d_out, *d_scores;
    const uint8_t* mask;
    float *out, *scores, *d_q, *d_keys, *G, *part_a, *part_w;
    int64_t ld_q, ld_k, ld_out, ld_do, ld_dq, ld_dk, B, rows_per_chunk;
    int32_t T, D, U, D16, U16, mode, act, nblk;
    float eps;
};

constexpr int POOL_MAX_BLOCKS = 1024;      // blocks of the example-owning backward kernel (one partial of the small gradients each)
constexpr int POOL_MAX_CHUNKS = 512;       // row chunks of the weight-gradient kernel (one [3D + 1, U] partial each)

__device__ __forceinline__ float quad_sum(float v) {       // over the 4 lanes g of one i16
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {      // over the 16 lanes i16 of one g
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

// LDS image of one example: qs [D16], wo / al [U16], Weff (and W[2D:3D] when W2s != nullptr) [D16][U16 + 4], hq [U16]; zero padded.
// hqp [2][U16] is scratch.
__device__ __forceinline__ void pool_setup(const PoolP& p, int64_t b, float* Ws, float* W2s, float* qs, float* hq, float* hqp, float* wo,
                                           float* al) {
    const int D = p.D, U = p.U, LS = p.U16 + 4;
    for (int d = threadIdx.x; d < p.D16; d += 256) qs[d] = d < D ? p.q[b * p.ld_q + d] : 0.f;
    for (int u = threadIdx.x; u < p.U16; u += 256) {
        wo[u] = u < U ? p.w_out[u] : 0.f;
        al[u] = (p.alpha && u < U) ? p.alpha[u] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = threadIdx.x; i < p.D16 * p.U16; i += 256) {
        const int d = i / p.U16, u = i - d * p.U16;
        float v = 0.f, v2 = 0.f;
        if (d < D && u < U) {
            v = p.W[(int64_t)(D + d) * U + u];
            if (p.mode == 1) v -= p.W[(int64_t)(2 * D + d) * U + u];
            if (p.mode == 2) {
                v2 = p.W[(int64_t)(2 * D + d) * U + u];
                v = fmaf(qs[d], v2, v);
            }
        }
        Ws[d * LS + u] = v;
        if (W2s) W2s[d * LS + u] = v2;
    }
    {   // hq: thread (u, half) sums its half of the d range ascending (loads batched by the unroll), then b + (half 0 + half 1)
        const int u = threadIdx.x & 127, half = threadIdx.x >> 7;
        const int d0 = half ? D / 2 : 0, d1 = half ? D : D / 2;
        float acc = 0.f;
        if (u < U) {
#pragma unroll 8
            for (int d = d0; d < d1; ++d) {
                float w = p.W[(int64_t)d * U + u];
                if (p.mode == 1) w += p.W[(int64_t)(2 * D + d) * U + u];
                acc = fmaf(qs[d], w, acc);
            }
        }
        if (u < p.U16) hqp[half * p.U16 + u] = acc;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < p.U16; u += 256) hq[u] = ((p.b && u < U) ? p.b[u] : 0.f) + (hqp[u] + hqp[p.U16 + u]);
    __syncthreads();
}

// the wave's 16 keys as the MFMA operand: kreg[c][e] = key[16c + 4g + e]; zeros for a key that is masked or outside T
template <int NC>
__device__ __forceinline__ void pool_load_keys(dr_f32x4 (&kreg)[NC], const float* kp, bool valid, int D, int g) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int d0 = 16 * c + 4 * g;
        kreg[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid && d0 < D) kreg[c] = *reinterpret_cast<const dr_f32x4*>(kp + d0);
    }
}

// h[ut][r] = hq[u] + sum_d key[d] Weff[d][u] for the lane's key, u = 16 ut + 4 g + r
template <int NC, int NU>
__device__ __forceinline__ void pool_hidden(const float* Ws, const float* hq, const dr_f32x4 (&kreg)[NC], dr_f32x4 (&h)[NU], int D16, int U16, int i16,
                                            int g) {
    const int LS = U16 + 4;
#pragma unroll
    for (int ut = 0; ut < NU; ++ut) {
        dr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (16 * ut < U16) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (16 * c < D16) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ws[(16 * c + 4 * g + e) * LS + 16 * ut + i16], kreg[c][e], acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += hq[16 * ut + 4 * g + r];
        }
        h[ut] = acc;
    }
}

// a = act(h) over the lane's hidden units (0 beyond U); for Dice also the row's (m, s, r).  Returns the key's score without b_out.
template <int NU>
__device__ __forceinline__ float pool_act(const PoolP& p, const dr_f32x4 (&h)[NU], dr_f32x4 (&a)[NU], const float* wo, const float* al, int g, float& m,
                                          float& s, float& r) {
    const int U = p.U;
    m = s = r = 0.f;
    if (p.act == 4) {
        float acc = 0.f;
#pragma unroll
        for (int ut = 0; ut < NU; ++ut)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (16 * ut + 4 * g + q < U) acc += h[ut][q];
        m = quad_sum(acc) / (float)U;
        acc = 0.f;
#pragma unroll
        for (int ut = 0; ut < NU; ++ut)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (16 * ut + 4 * g + q < U) acc += (h[ut][q] - m) * (h[ut][q] - m);
        s = sqrtf(quad_sum(acc) / (float)U);
        r = 1.f / sqrtf(s + p.eps);
    }
    float sc = 0.f;
#pragma unroll
    for (int ut = 0; ut < NU; ++ut)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = 16 * ut + 4 * g + q;
            float v = 0.f;
            if (u < U) {
                const float x = h[ut][q];
                float pp, pre;
                v = p.act == 1 ? fmaxf(x, 0.f) : p.act == 2 ? dr_sigmoidf(x) : p.act == 3 ? tanhf(x) : p.act == 4 ? dice_elem(x, al[u], m, r, pp, pre) : x;
                sc = fmaf(v, wo[u], sc);
            }
            a[ut][q] = v;
        }
    return quad_sum(sc);
}

template <int NC, int NU>
__global__ __launch_bounds__(256) void din_pool_fwd_kernel(const PoolP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = p.D, T = p.T, D16 = p.D16, U16 = p.U16, LS = U16 + 4;
    float* Ws = lds;
    float* qs = Ws + D16 * LS;
    float* hq = qs + D16;
    float* wo = hq + U16;
    float* al = wo + U16;
    float* hqp = al + U16;                                     // [2][U16]
    float* red = hqp + 2 * U16;                                // [4][D16]
    const int64_t b = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    pool_setup(p, b, Ws, nullptr, qs, hq, hqp, wo, al);
    const float b_out = p.b_out ? p.b_out[0] : 0.f;
    dr_f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = wave * 16; t0 < T; t0 += 64) {
        const int t = t0 + i16;
        const bool inr = t < T;
        const bool valid = inr && (!p.mask || p.mask[b * T + t] != 0);
        float score = 0.f;
        if (__ballot(valid) != 0ull) {
            dr_f32x4 kreg[NC], h[NU], a[NU];
            pool_load_keys<NC>(kreg, p.keys + (b * T + t) * p.ld_k, valid, D, g);
            pool_hidden<NC, NU>(Ws, hq, kreg, h, D16, U16, i16, g);
            float m, s, r;
            const float sc = pool_act<NU>(p, h, a, wo, al, g, m, s, r) + b_out;
            if (valid) {                                       // a partially valid tile: the other rows are discarded by select
                score = sc;
#pragma unroll
                for (int c = 0; c < NC; ++c) oacc[c] += sc * kreg[c];
            }
        }
        if (inr && g == 0) p.scores[b * T + t] = score;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (16 * c < D16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = row16_sum(oacc[c][e]);
                if (i16 == 0) red[wave * D16 + 16 * c + 4 * g + e] = v;
            }
        }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) p.out[b * p.ld_out + d] = (red[d] + red[D16 + d]) + (red[2 * D16 + d] + red[3 * D16 + d]);
}

// The example-owning backward: block k owns the examples [k * per, (k + 1) * per).
template <int NC, int NU>
__global__ __launch_bounds__(256) void din_pool_bwd_kernel(const PoolP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = p.D, U = p.U, T = p.T, D16 = p.D16, U16 = p.U16, LS = U16 + 4;
    float* Ws = lds;
    float* W2s = Ws + D16 * LS;                                // only for mode 2
    float* qs = W2s + (p.mode == 2 ? D16 * LS : 0);
    float* hq = qs + D16;
    float* wo = hq + U16;
    float* al = wo + U16;
    float* dhqs = al + U16;                                    // [U16]
    float* redu = dhqs + U16;                                  // [4][U16]
    float* redd = redu + 4 * U16;                              // [4][D16]
    if (p.mode != 2) W2s = nullptr;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const float b_out = p.b_out ? p.b_out[0] : 0.f;
    const int64_t per = (p.B + p.nblk - 1) / p.nblk;
    const int64_t b_begin = blockIdx.x * per, b_end = b_begin + per < p.B ? b_begin + per : p.B;
    dr_f32x4 wacc[NU], aacc[NU];                                     // d_w_out and dalpha of this block's examples
#pragma unroll
    for (int ut = 0; ut < NU; ++ut) wacc[ut] = aacc[ut] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    float boacc = 0.f;
    for (int64_t b = b_begin; b < b_end; ++b) {
        __syncthreads();                                       // the previous example's readers of the LDS image
        pool_setup(p, b, Ws, W2s, qs, hq, redu, wo, al);       // redu doubles as the setup's scratch
        dr_f32x4 doreg[NC], dqacc[NC], dhq[NU];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int d0 = 16 * c + 4 * g;
            doreg[c] = dqacc[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
            if (d0 < D) doreg[c] = *reinterpret_cast<const dr_f32x4*>(p.d_out + b * p.ld_do + d0);
        }
#pragma unroll
        for (int ut = 0; ut < NU; ++ut) dhq[ut] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t0 = wave * 16; t0 < T; t0 += 64) {
            const int t = t0 + i16;
            const bool inr = t < T;
            const bool valid = inr && (!p.mask || p.mask[b * T + t] != 0);
            const int64_t n = b * T + t;
            dr_f32x4 dh[NU], dk[NC];
#pragma unroll
            for (int ut = 0; ut < NU; ++ut) dh[ut] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) dk[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
            if (__ballot(valid) != 0ull) {
                dr_f32x4 kreg[NC], h[NU], a[NU];
                pool_load_keys<NC>(kreg, p.keys + n * p.ld_k, valid, D, g);
                pool_hidden<NC, NU>(Ws, hq, kreg, h, D16, U16, i16, g);
                float m, s, r;
                const float sc = pool_act<NU>(p, h, a, wo, al, g, m, s, r) + b_out;
                float ds = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ds = fmaf(kreg[c][e], doreg[c][e], ds);
                ds = quad_sum(ds);
                if (p.d_scores && valid) ds += p.d_scores[n];
                if (!valid) ds = 0.f;
                if (g == 0) boacc += ds;
                // dH of the lane's key
                float csum = 0.f, cxsum = 0.f;
                dr_f32x4 dpre[NU];
#pragma unroll
                for (int ut = 0; ut < NU; ++ut)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = 16 * ut + 4 * g + q;
                        float v = 0.f;
                        dpre[ut][q] = 0.f;
                        if (u < U && valid) {
                            const float x = h[ut][q], av = a[ut][q], da = ds * wo[u];
                            wacc[ut][q] = fmaf(ds, av, wacc[ut][q]);
                            if (p.act == 4) {
                                float dp;
                                dice_elem_bwd(x, al[u], m, r, da, dp, v);              // v = c for now
                                dpre[ut][q] = dp;
                                csum += v;
                                cxsum += v * (x - m);
                                aacc[ut][q] += dp * fminf(x, 0.f);
                            } else {
                                v = p.act == 1 ? (x > 0.f ? da : 0.f) : p.act == 2 ? da * av * (1.f - av) : p.act == 3 ? da * (1.f - av * av) : da;
                            }
                        }
                        dh[ut][q] = v;
                    }
                if (p.act == 4) {
                    csum = quad_sum(csum);
                    cxsum = quad_sum(cxsum);
#pragma unroll
                    for (int ut = 0; ut < NU; ++ut)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int u = 16 * ut + 4 * g + q;
                            dh[ut][q] = (u < U && valid) ? dice_dx(h[ut][q], al[u], m, s, r, (float)U, dpre[ut][q], dh[ut][q], csum, cxsum) : 0.f;
                        }
                }
#pragma unroll
                for (int ut = 0; ut < NU; ++ut) dhq[ut] += dh[ut];
                // d_keys^T = Weff dH^T (and E^T = W[2D:3D] dH^T for the query's share in mode 2): dk[c][r'] = column 16c + 4g + r'
                dr_f32x4 ek[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    ek[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
                    if (16 * c < D16) {
#pragma unroll
                        for (int ut = 0; ut < NU; ++ut)
                            if (16 * ut < U16) {
                                const dr_f32x4 w = *reinterpret_cast<const dr_f32x4*>(Ws + (16 * c + i16) * LS + 16 * ut + 4 * g);
#pragma unroll
                                for (int q = 0; q < 4; ++q) dk[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[q], dh[ut][q], dk[c], 0, 0, 0);
                                if (W2s) {
                                    const dr_f32x4 w2 = *reinterpret_cast<const dr_f32x4*>(W2s + (16 * c + i16) * LS + 16 * ut + 4 * g);
#pragma unroll
                                    for (int q = 0; q < 4; ++q) ek[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[q], dh[ut][q], ek[c], 0, 0, 0);
                                }
                            }
                    }
                    if (valid) {
                        dk[c] += sc * doreg[c];
                        dqacc[c] += kreg[c] * ek[c];
                    } else {
                        dk[c] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
            if (inr) {
#pragma unroll
                for (int ut = 0; ut < NU; ++ut)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = 16 * ut + 4 * g + q;
                        if (u < U) p.G[n * U + u] = dh[ut][q];
                    }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int d0 = 16 * c + 4 * g;
                    if (d0 < D) *reinterpret_cast<dr_f32x4*>(p.d_keys + n * p.ld_dk + d0) = dk[c];
                }
            }
        }
        // d_query = (sum_t dH) (W[0:D] (+ W[2D:3D]))^T (+ sum_t k * E in mode 2)
#pragma unroll
        for (int ut = 0; ut < NU; ++ut)
            if (16 * ut < U16) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float v = row16_sum(dhq[ut][q]);
                    if (i16 == 0) redu[wave * U16 + 16 * ut + 4 * g + q] = v;
                }
            }
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (16 * c < D16) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = row16_sum(dqacc[c][e]);
                    if (i16 == 0) redd[wave * D16 + 16 * c + 4 * g + e] = v;
                }
            }
        __syncthreads();
        for (int u = threadIdx.x; u < U16; u += 256) dhqs[u] = (redu[u] + redu[U16 + u]) + (redu[2 * U16 + u] + redu[3 * U16 + u]);
        __syncthreads();
        {   // P adjacent lanes per d, each over u = part, part + P, ... ascending, then a shuffle tree over the P lanes
            const int P = D <= 32 ? 8 : D <= 64 ? 4 : 2;
            const int d = threadIdx.x / P, part = threadIdx.x - d * P;
            float v = 0.f;
            if (d < D) {
#pragma unroll 4
                for (int u = part; u < U; u += P) {
                    float w = p.W[(int64_t)d * U + u];
                    if (p.mode == 1) w += p.W[(int64_t)(2 * D + d) * U + u];
                    v = fmaf(dhqs[u], w, v);
                }
            }
            for (int o = 1; o < P; o <<= 1) v += __shfl_xor(v, o, 64);
            if (d < D && part == 0) {
                if (p.mode == 2) v += (redd[d] + redd[D16 + d]) + (redd[2 * D16 + d] + redd[3 * D16 + d]);
                p.d_q[b * p.ld_dq + d] = v;
            }
        }
    }
    // this block's partial of d_w_out [U16], dalpha [U16], d_b_out
    __syncthreads();
    float* part = p.part_a + (int64_t)blockIdx.x * (2 * U16 + 1);
#pragma unroll
    for (int ut = 0; ut < NU; ++ut)
        if (16 * ut < U16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = row16_sum(wacc[ut][q]);
                if (i16 == 0) redu[wave * U16 + 16 * ut + 4 * g + q] = v;
            }
        }
    boacc = dr_wave_sum(boacc);
    if (lane == 0) redd[wave] = boacc;
    __syncthreads();
    for (int u = threadIdx.x; u < U16; u += 256) part[u] = (redu[u] + redu[U16 + u]) + (redu[2 * U16 + u] + redu[3 * U16 + u]);
    if (threadIdx.x == 0) part[2 * U16] = (redd[0] + redd[1]) + (redd[2] + redd[3]);
    __syncthreads();
#pragma unroll
    for (int ut = 0; ut < NU; ++ut)
        if (16 * ut < U16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = row16_sum(aacc[ut][q]);
                if (i16 == 0) redu[wave * U16 + 16 * ut + 4 * g + q] = v;
            }
        }
    __syncthreads();
    for (int u = threadIdx.x; u < U16; u += 256) part[U16 + u] = (redu[u] + redu[U16 + u]) + (redu[2 * U16 + u] + redu[3 * U16 + u]);
}

// Weight gradients: chunk c owns the rows [c * rows_per_chunk, ...) of (keys, G) and writes part_w[c] = [q^T G | K^T G | (q * k)^T G | colsum G]
// ([3][D][U] + [U]).  Wave w owns the 16-row blocks dt = w, w + 4 of the D axis; 4 rows (the MFMA's k) per step, ascending.
template <int NC, int NU>
__global__ __launch_bounds__(256) void din_pool_wgrad_kernel(const PoolP p) {
    constexpr int NDW = (NC + 3) / 4;
    const int D = p.D, U = p.U, T = p.T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int64_t rows = p.B * T;
    const int64_t n_begin = blockIdx.x * p.rows_per_chunk, n_end = n_begin + p.rows_per_chunk < rows ? n_begin + p.rows_per_chunk : rows;
    dr_f32x4 acc0[NDW][NU], acc1[NDW][NU], acc2[NDW][NU];
    float dbacc[NU];
#pragma unroll
    for (int ut = 0; ut < NU; ++ut) {
        dbacc[ut] = 0.f;
#pragma unroll
        for (int i = 0; i < NDW; ++i) acc0[i][ut] = acc1[i][ut] = acc2[i][ut] = dr_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t n0 = n_begin; n0 < n_end; n0 += 4) {
        const int64_t n = n0 + g;
        const bool ok = n < n_end && (!p.mask || p.mask[n] != 0);
        const int64_t bq = n / T;
        float bv[NU];
#pragma unroll
        for (int ut = 0; ut < NU; ++ut) {
            const int u = 16 * ut + i16;
            bv[ut] = (ok && u < U) ? p.G[n * U + u] : 0.f;
            dbacc[ut] += bv[ut];
        }
#pragma unroll
        for (int i = 0; i < NDW; ++i) {
            const int dt = wave + 4 * i;
            if (16 * dt < p.D16) {
                const int d = 16 * dt + i16;
                const bool dok = ok && d < D;
                const float a1 = dok ? p.keys[n * p.ld_k + d] : 0.f;
                const float a0 = dok ? p.q[bq * p.ld_q + d] : 0.f;
                const float a2 = a0 * a1;
#pragma unroll
                for (int ut = 0; ut < NU; ++ut)
                    if (16 * ut < p.U16) {
                        acc0[i][ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[ut], acc0[i][ut], 0, 0, 0);
                        acc1[i][ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv[ut], acc1[i][ut], 0, 0, 0);
                        if (p.mode == 2) acc2[i][ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bv[ut], acc2[i][ut], 0, 0, 0);
                    }
            }
        }
    }
    float* part = p.part_w + (int64_t)blockIdx.x * ((int64_t)3 * D * U + U);
#pragma unroll
    for (int i = 0; i < NDW; ++i)
#pragma unroll
        for (int ut = 0; ut < NU; ++ut)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * (wave + 4 * i) + 4 * g + r, u = 16 * ut + i16;
                if (d < D && u < U) {
                    part[(int64_t)d * U + u] = acc0[i][ut][r];
                    part[(int64_t)(D + d) * U + u] = acc1[i][ut][r];
                    part[(int64_t)(2 * D + d) * U + u] = acc2[i][ut][r];
                }
            }
    if (wave == 0) {
#pragma unroll
        for (int ut = 0; ut < NU; ++ut) {
            const float v = quad_sum(dbacc[ut]);
            const int u = 16 * ut + i16;
            if (g == 0 && u < U) part[(int64_t)3 * D * U + u] = v;
        }
    }
}

// dW [n_in * D, U] and db [U] from the chunk partials (16 row lanes per element as in din_colsum_kernel); mode 1: dW[2D:3D] = q^T G - K^T G
__global__ __launch_bounds__(256) void din_pool_wgrad_final_kernel(const float* __restrict__ part, int64_t chunks, int D, int U, int mode,
                                                                  float* __restrict__ dW, float* __restrict__ db) {
    __shared__ float red[3][16][16];
    const int DU = D * U;
    const int64_t ld = (int64_t)3 * DU + U;
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + cl;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (i < DU) {
#pragma unroll 4
        for (int64_t c = rl; c < chunks; c += 16) {
            s0 += part[c * ld + i];
            s1 += part[c * ld + DU + i];
            if (mode == 2) s2 += part[c * ld + 2 * DU + i];
        }
    } else if (i < DU + U) {
#pragma unroll 4
        for (int64_t c = rl; c < chunks; c += 16) s0 += part[c * ld + 3 * DU + (i - DU)];
    }
    s0 = din_tree16(red[0], rl, cl, s0);
    s1 = din_tree16(red[1], rl, cl, s1);
    s2 = din_tree16(red[2], rl, cl, s2);
    if (rl != 0) return;
    if (i < DU) {
        dW[i] = s0;
        dW[DU + i] = s1;
        if (mode == 1) dW[2 * DU + i] = s0 - s1;
        if (mode == 2) dW[2 * DU + i] = s2;
    } else if (i < DU + U && db) {
        db[i - DU] = s0;
    }
}

// d_w_out [U], dalpha [U], d_b_out [1] from the example-owning kernel's partials [nblk][2 U16 + 1]
__global__ __launch_bounds__(256) void din_pool_small_final_kernel(const float* __restrict__ part, int64_t nblk, int U, int U16,
                                                                  float* __restrict__ d_w_out, float* __restrict__ dalpha,
                                                                  float* __restrict__ d_b_out) {
    __shared__ float red[16][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + cl, ld = 2 * U16 + 1;
    float acc = 0.f;
    if (j < ld) {
#pragma unroll 4
        for (int64_t c = rl; c < nblk; c += 16) acc += part[c * ld + j];
    }
    const float v = din_tree16(red, rl, cl, acc);
    if (rl != 0 || j >= ld) return;
    if (j < U16) {
        if (j < U) d_w_out[j] = v;
    } else if (j < 2 * U16) {
        if (dalpha && j - U16 < U) dalpha[j - U16] = v;
    } else if (d_b_out) {
        d_b_out[0] = v;
    }
}

inline int pool_round16(int v) { return (v + 15) & ~15; }
inline int pool_nblk(int64_t B) { return (int)std::min<int64_t>(std::max<int64_t>(B, 1), POOL_MAX_BLOCKS); }
inline int64_t pool_rows_per_chunk(int64_t rows) {
    int64_t r = (rows + POOL_MAX_CHUNKS - 1) / POOL_MAX_CHUNKS;
    r = (std::max<int64_t>(r, 64) + 3) & ~(int64_t)3;
    return r;
}
inline int64_t pool_chunks(int64_t rows) { return std::max<int64_t>(1, (rows + pool_rows_per_chunk(rows) - 1) / pool_rows_per_chunk(rows)); }

inline bool pool_domain(int32_t T, int32_t D, int32_t U) { return D % 4 == 0 && D >= 4 && D <= 128 && U >= 1 && U <= 128 && T >= 1; }

// instantiations: D <= 32 / 64 / 128 and U <= 32 / 64 / 128 (the loops skip the 16-blocks beyond round16(D), round16(U)); these kernels
// opt in to large dynamic LDS from 48 KiB
#define DIN_DISPATCH(KERNEL, grid, lds_bytes)                                                               \
    do {                                                                                                    \
        const int nc_ = p.D16 <= 32 ? 2 : p.D16 <= 64 ? 4 : 8, nu_ = p.U16 <= 32 ? 2 : p.U16 <= 64 ? 4 : 8; \
        const dim3 g_((unsigned)(grid));                                                                    \
        int st_;                                                                                            \
        if (nc_ == 2 && nu_ == 2) st_ = dr_launch<48>(KERNEL<2, 2>, g_, dim3(256), lds_bytes, s, p);        \
        else if (nc_ == 2 && nu_ == 4) st_ = dr_launch<48>(KERNEL<2, 4>, g_, dim3(256), lds_bytes, s, p);   \
        else if (nc_ == 2) st_ = dr_launch<48>(KERNEL<2, 8>, g_, dim3(256), lds_bytes, s, p);               \
        else if (nc_ == 4 && nu_ == 2) st_ = dr_launch<48>(KERNEL<4, 2>, g_, dim3(256), lds_bytes, s, p);   \
        else if (nc_ == 4 && nu_ == 4) st_ = dr_launch<48>(KERNEL<4, 4>, g_, dim3(256), lds_bytes, s, p);   \
        else if (nc_ == 4) st_ = dr_launch<48>(KERNEL<4, 8>, g_, dim3(256), lds_bytes, s, p);               \
        else if (nu_ == 2) st_ = dr_launch<48>(KERNEL<8, 2>, g_, dim3(256), lds_bytes, s, p);               \
        else if (nu_ == 4) st_ = dr_launch<48>(KERNEL<8, 4>, g_, dim3(256), lds_bytes, s, p);               \
        else st_ = dr_launch<48>(KERNEL<8, 8>, g_, dim3(256), lds_bytes, s, p);                             \
        if (st_ != DR_OK) return st_;                                                                       \
    } while (0)

}  // namespace

extern "C" int dr_dice_fwd(const float* x, int64_t ld_x, const float* alpha, int64_t M, int32_t N, float eps, float* y, int64_t ld_y,
                           dr_stream_t stream) {
    if (M < 0 || N < 1) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    if (!x || !alpha || !y || ld_x < N || ld_y < N) return DR_EINVAL;
    const int grid = dr_grid_for(M, 4);
    if (N <= 64 * DICE_REG) hipLaunchKernelGGL(dice_fwd_kernel<true>, dim3(grid), dim3(256), 0, dr_s(stream), x, ld_x, alpha, M, N, eps, y, ld_y);
    else hipLaunchKernelGGL(dice_fwd_kernel<false>, dim3(grid), dim3(256), 0, dr_s(stream), x, ld_x, alpha, M, N, eps, y, ld_y);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_dice_bwd_workspace_bytes(int64_t M, int32_t N) {
    if (M < 0 || N < 1) return 0;
    const int64_t chunks = (M + DICE_CHUNK - 1) / DICE_CHUNK;
    return (2 * M + chunks * N) * (int64_t)sizeof(float);
}

extern "C" int dr_dice_bwd(const float* x, int64_t ld_x, const float* alpha, const float* dy, int64_t ld_dy, int64_t M, int32_t N, float eps,
                           float* dx, int64_t ld_dx, float* dalpha, void* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    if (M < 0 || N < 1) return DR_ESHAPE;
    if (!dalpha) return DR_EINVAL;
    hipStream_t s = dr_s(stream);
    if (M == 0) {
        if (hipMemsetAsync(dalpha, 0, (size_t)N * sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        return DR_OK;
    }
    if (!x || !alpha || !dy || !dx || !workspace || ld_x < N || ld_dy < N || ld_dx < N) return DR_EINVAL;
    if (workspace_bytes < dr_dice_bwd_workspace_bytes(M, N)) return DR_EINVAL;
    float* stats = static_cast<float*>(workspace);
    float* partial = stats + 2 * M;
    const int64_t chunks = (M + DICE_CHUNK - 1) / DICE_CHUNK;
    const int grid = dr_grid_for(M, 4);
    if (N <= 64 * DICE_REG)
        hipLaunchKernelGGL(dice_bwd_dx_kernel<true>, dim3(grid), dim3(256), 0, s, x, ld_x, alpha, dy, ld_dy, M, N, eps, dx, ld_dx, stats);
    else
        hipLaunchKernelGGL(dice_bwd_dx_kernel<false>, dim3(grid), dim3(256), 0, s, x, ld_x, alpha, dy, ld_dy, M, N, eps, dx, ld_dx, stats);
    DR_CHECK_LAUNCH();
    hipLaunchKernelGGL(dice_dalpha_partial_kernel, dim3((unsigned)chunks, (unsigned)((N + 63) / 64)), dim3(256), 0, s, x, ld_x, alpha, dy, ld_dy, M,
                       N, stats, partial);
    DR_CHECK_LAUNCH();
    hipLaunchKernelGGL(din_colsum_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, s, partial, chunks, (int64_t)N, N, dalpha);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

static int din_pool_params(PoolP& p, const float* query, int64_t ld_q, const float* keys, int64_t ld_k, const uint8_t* mask, const float* W,
                           const float* b, const float* w_out, const float* b_out, const float* alpha, int64_t B, int32_t T, int32_t D,
                           int32_t U, int32_t mode, int32_t act, float eps) {
    if (B < 0 || !pool_domain(T, D, U)) return DR_ESHAPE;
    if (mode < 0 || mode > 2 || act < 0 || act > 4 || (act == 4 && !alpha)) return DR_EINVAL;
    if (B > 0 && (!query || !keys || !W || !w_out || ld_q < D || dr_bad_ld(ld_k, D) || !dr_aligned16(keys))) return DR_EINVAL;
    p = PoolP{};
    p.q = query; p.keys = keys; p.mask = mask; p.W = W; p.b = b; p.w_out = w_out; p.b_out = b_out; p.alpha = act == 4 ? alpha : nullptr;
    p.ld_q = ld_q; p.ld_k = ld_k; p.B = B; p.T = T; p.D = D; p.U = U; p.D16 = pool_round16(D); p.U16 = pool_round16(U);
    p.mode = mode; p.act = act; p.eps = eps;
    return DR_OK;
}

extern "C" int dr_din_pool_fwd(const float* query, int64_t ld_q, const float* keys, int64_t ld_k, const uint8_t* mask, const float* W,
                               const float* b, const float* w_out, const float* b_out, const float* alpha, int64_t B, int32_t T, int32_t D,
                               int32_t U, int32_t mode, int32_t act, float eps, float* out, int64_t ld_out, float* scores,
                               dr_stream_t stream) {
    PoolP p;
    const int st = din_pool_params(p, query, ld_q, keys, ld_k, mask, W, b, w_out, b_out, alpha, B, T, D, U, mode, act, eps);
    if (st != DR_OK) return st;
    if (B == 0) return DR_OK;
    if (!out || !scores || ld_out < D) return DR_EINVAL;
    p.out = out; p.ld_out = ld_out; p.scores = scores;
    hipStream_t s = dr_s(stream);
    const size_t lds_bytes = sizeof(float) * ((size_t)p.D16 * (p.U16 + 4) + p.D16 + 5 * p.U16 + 4 * p.D16);
    DIN_DISPATCH(din_pool_fwd_kernel, B, lds_bytes);
    return DR_OK;
}

extern "C" int64_t dr_din_pool_bwd_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t U) {
    if (B < 0 || !pool_domain(T, D, U)) return 0;
    const int64_t rows = B * T;
    return (rows * U + (int64_t)pool_nblk(B) * (2 * pool_round16(U) + 1) + pool_chunks(rows) * ((int64_t)3 * D * U + U)) * (int64_t)sizeof(float);
}

extern "C" int dr_din_pool_bwd(const float* query, int64_t ld_q, const float* keys, int64_t ld_k, const uint8_t* mask, const float* W,
                               const float* b, const float* w_out, const float* b_out, const float* alpha, const float* d_out, int64_t ld_do,
                               const float* d_scores, int64_t B, int32_t T, int32_t D, int32_t U, int32_t mode, int32_t act, float eps,
                               float* d_query, int64_t ld_dq, float* d_keys, int64_t ld_dk, float* dW, float* db, float* d_w_out,
                               float* d_b_out, float* dalpha, void* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    PoolP p;
    const int st = din_pool_params(p, query, ld_q, keys, ld_k, mask, W, b, w_out, b_out, alpha, B, T, D, U, mode, act, eps);
    if (st != DR_OK) return st;
    if (!dW || !d_w_out || (act == 4 && !dalpha)) return DR_EINVAL;
    hipStream_t s = dr_s(stream);
    if (B == 0) {
        const size_t n_in = mode == 0 ? 2 : 3;
        if (hipMemsetAsync(dW, 0, n_in * D * U * sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        if (hipMemsetAsync(d_w_out, 0, (size_t)U * sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        if (db && hipMemsetAsync(db, 0, (size_t)U * sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        if (d_b_out && hipMemsetAsync(d_b_out, 0, sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        if (dalpha && hipMemsetAsync(dalpha, 0, (size_t)U * sizeof(float), s) != hipSuccess) return DR_ELAUNCH;
        return DR_OK;
    }
    if (!d_out || !d_query || !d_keys || !workspace || dr_bad_ld(ld_do, D) || ld_dq < D || dr_bad_ld(ld_dk, D) || !dr_aligned16(d_out) ||
        !dr_aligned16(d_keys) || !dr_aligned16(workspace))
        return DR_EINVAL;
    if (workspace_bytes < dr_din_pool_bwd_workspace_bytes(B, T, D, U)) return DR_EINVAL;
    const int64_t rows = B * T, chunks = pool_chunks(rows);
    p.d_out = d_out; p.ld_do = ld_do; p.d_scores = d_scores; p.d_q = d_query; p.ld_dq = ld_dq; p.d_keys = d_keys; p.ld_dk = ld_dk;
    p.nblk = pool_nblk(B);
    p.rows_per_chunk = pool_rows_per_chunk(rows);
    p.G = static_cast<float*>(workspace);
    p.part_a = p.G + rows * U;
    p.part_w = p.part_a + (int64_t)p.nblk * (2 * p.U16 + 1);
    const size_t lds_bytes = sizeof(float) * ((size_t)(mode == 2 ? 2 : 1) * p.D16 * (p.U16 + 4) + p.D16 + 4 * p.U16 + 4 * p.U16 + 4 * p.D16);
    DIN_DISPATCH(din_pool_bwd_kernel, p.nblk, lds_bytes);
    DIN_DISPATCH(din_pool_wgrad_kernel, chunks, 0);
    const int DU = D * U;
    hipLaunchKernelGGL(din_pool_wgrad_final_kernel, dim3((unsigned)((DU + U + 15) / 16)), dim3(256), 0, s, p.part_w, chunks, D, U, mode, dW, db);
    DR_CHECK_LAUNCH();
    hipLaunchKernelGGL(din_pool_small_final_kernel, dim3((unsigned)((2 * p.U16 + 1 + 15) / 16)), dim3(256), 0, s, p.part_a, (int64_t)p.nblk, U, p.U16,
                       d_w_out, dalpha, d_b_out);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
