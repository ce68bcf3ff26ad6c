// K7 / K8 — fp32 GEMMs on the gfx950 matrix cores with the layer's elementwise tail fused into the epilogue.  Inputs,
// outputs and accumulators are fp32 (the reference's parity bar is 1e-5 relative on the loss: no reduced-precision
// path).  Two ways of forming the products, same results to fp32 rounding (dr_set_gemm_mode, include/dr_hotpath.h):
//   native   v_mfma_f32_32x32x2_f32
//   bf16x3   every operand value split exactly into three bf16 terms on its way into LDS, six
//            v_mfma_f32_32x32x16_bf16 products per fp32 product (the fp32 MFMA runs at 1/16 of the bf16 rate, so this
//            has a 2.65x higher ceiling); default for the wide-tile tower / cross GEMMs
// Entry points:
//   fwd     y   = act(x @ W + b)                       (Dense: keras deepfm.py:30-34, estimator dnn.py:17-29)
//   cross   out = x0 * (x @ W + b + diag*x) + x        (Cross.call: keras dcn.py:81-88; dense_cross.hip)
//   bwd_dx  dx  = (dy @ W^T) * (relu_src > 0) [+ dx]   (autodiff of the above)
//   bwd_dw  dst += scale * x^T @ dy, dstb += scale*colsum(dy)   (split over the batch, fp32 atomics)
// This file: the tower linears (plain, grouped, split-K, and the skinny Dense(1) kernels) and the process-wide GEMM mode / split.
// The kernel template is gemm_f32_core.h; the fused tower head is dense_head.hip, the two-tower score passes dense_scores.hip.
#include "gemm_f32_core.h"
#include <atomic>
#include <cstdlib>
#include <cstring>

namespace {

// process-wide GEMM mode (dr_set_gemm_mode); the default can be overridden with DR_GEMM_MODE=native|bf16x3
static int gemm_mode_default() {
    const char* e = getenv("DR_GEMM_MODE");
    if (e != nullptr && (e[0] == 'n' || e[0] == 'N' || e[0] == '1')) return DR_GEMM_NATIVE_F32;
    return DR_GEMM_BF16X3;
}
static std::atomic<int> g_gemm_mode{gemm_mode_default()};
// process-wide operand split of the register-split GEMMs (dr_set_gemm_split): THE one parser of DR_GEMM_SPLIT -- f16x2 iff the
// variable is unset or spells exactly "f16x2"; anything else is the six-product bf16x3 split
static int gemm_split_default() {
    const char* e = getenv("DR_GEMM_SPLIT");
    return (e == nullptr || strcmp(e, "f16x2") == 0) ? DR_GEMM_SPLIT_F16X2 : DR_GEMM_SPLIT_BF16X3;
}
static std::atomic<int> g_gemm_split{gemm_split_default()};

// dst[k][n] += scale * sum_s partial[s][k][n]   (deterministic split-K combine with the SGD step fused)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial, int32_t split, int64_t K,
                                                            int32_t N, float scale, float* __restrict__ dst,
                                                            int64_t ld) {
    const int64_t total = K * N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        float acc = 0.f;
        for (int s = 0; s < split; ++s) acc += partial[(int64_t)s * total + i];
        const int64_t k = i / N;
        const int n = (int)(i - k * N);
        dst[k * ld + n] = fmaf(scale, acc, dst[k * ld + n]);
    }
}

// ---- skinny shapes (min(K, N) < 4: the Dense(1) heads) : streaming kernels, no MFMA -------------------------------
// y[m][n] = act(sum_k x[m][k] W[k][n] + b[n]) ; one lane group of 16 per row, k strided over the lanes
__device__ __forceinline__ void skinny_fwd_body(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W, int64_t ldw,
                                                const float* __restrict__ b, int64_t M, int32_t K, int32_t N, int32_t act,
                                                float* __restrict__ y, int64_t ldy) {
    const int lane = threadIdx.x & 15;
    const int64_t groups = (int64_t)gridDim.x * (blockDim.x >> 4);
    for (int64_t m = (int64_t)blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4); m < M; m += groups) {
        for (int n = 0; n < N; ++n) {
            float acc = 0.f;
            for (int k = lane; k < K; k += 16) acc = fmaf(x[m * ldx + k], W[(int64_t)k * ldw + n], acc);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
            if (lane == 0) {
                float v = acc + (b != nullptr ? b[n] : 0.f);
                if (act == 1) v = fmaxf(v, 0.f);
                y[m * ldy + n] = v;
            }
        }
    }
}
__global__ __launch_bounds__(256) void skinny_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                         const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ b, int64_t M, int32_t K, int32_t N,
                                                         int32_t act, float* __restrict__ y, int64_t ldy) {
    skinny_fwd_body(x, ldx, W, ldw, b, M, K, N, act, y, ldy);
}
// grouped: group blockIdx.y reads x / W / b and writes y at its group offsets
__global__ __launch_bounds__(256) void skinny_fwd_grouped_kernel(const float* __restrict__ x, int64_t ldx, int64_t x_gs,
                                                                 const float* __restrict__ W, int64_t ldw, int64_t w_gs,
                                                                 const float* __restrict__ b, int64_t b_gs, int64_t M, int32_t K,
                                                                 int32_t N, int32_t act, float* __restrict__ y, int64_t ldy,
                                                                 int64_t y_gs) {
    const int64_t z = blockIdx.y;
    skinny_fwd_body(x + z * x_gs, ldx, W + z * w_gs, ldw, b != nullptr ? b + z * b_gs : nullptr, M, K, N, act, y + z * y_gs, ldy);
}
// dx[m][k] = (sum_n dy[m][n] W[k][n]) * (relu_src[m][k] > 0) (+ dx)
__device__ __forceinline__ void skinny_dx_body(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ W, int64_t ldw,
                                               int64_t M, int32_t K, int32_t N, const float* __restrict__ rs, int64_t ldrs,
                                               int32_t accumulate, float* __restrict__ dx, int64_t lddx) {
    const int64_t total = M * K;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / K;
        const int k = (int)(i - m * K);
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc = fmaf(dy[m * lddy + n], W[(int64_t)k * ldw + n], acc);
        if (rs != nullptr && !(rs[m * ldrs + k] > 0.f)) acc = 0.f;
        if (accumulate) acc += dx[m * lddx + k];
        dx[m * lddx + k] = acc;
    }
}
__global__ __launch_bounds__(256) void skinny_dx_kernel(const float* __restrict__ dy, int64_t lddy,
                                                        const float* __restrict__ W, int64_t ldw, int64_t M, int32_t K,
                                                        int32_t N, const float* __restrict__ rs, int64_t ldrs,
                                                        int32_t accumulate, float* __restrict__ dx, int64_t lddx) {
    skinny_dx_body(dy, lddy, W, ldw, M, K, N, rs, ldrs, accumulate, dx, lddx);
}
__global__ __launch_bounds__(256) void skinny_dx_grouped_kernel(const float* __restrict__ dy, int64_t lddy, int64_t dy_gs,
                                                                const float* __restrict__ W, int64_t ldw, int64_t w_gs, int64_t M,
                                                                int32_t K, int32_t N, const float* __restrict__ rs, int64_t ldrs,
                                                                int64_t rs_gs, int32_t accumulate, float* __restrict__ dx,
                                                                int64_t lddx, int64_t dx_gs) {
    const int64_t z = blockIdx.y;
    skinny_dx_body(dy + z * dy_gs, lddy, W + z * w_gs, ldw, M, K, N, rs != nullptr ? rs + z * rs_gs : nullptr, ldrs, accumulate,
                   dx + z * dx_gs, lddx);
}
// dst[k][n] += scale * sum_m x[m][k] dy[m][n] ; dstb[n] += scale * sum_m dy[m][n].  A block owns a slab of rows and
// all (k, n) pairs (strided over its threads), accumulates in registers, then one atomic per (k, n) per block.
// (128 rows per block: 512 blocks at M = 65536.  With 1024 the Dense(1) weight gradient of the DCN tower ran on 64 of 256 CUs,
// every thread a 1024-long dependent chain: 258 us for a 67 MB read)
constexpr int SK_ROWS = 128;
__global__ __launch_bounds__(256) void skinny_dw_kernel(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ dy, int64_t lddy, int64_t M, int32_t K,
                                                        int32_t N, float scale, float* __restrict__ dst, int64_t ldw,
                                                        float* __restrict__ dstb) {
    __shared__ float sm[256];
    const int64_t m0 = (int64_t)blockIdx.x * SK_ROWS;
    const int64_t m1 = m0 + SK_ROWS < M ? m0 + SK_ROWS : M;
    const int KN = K * N;
    const int lanes_e = KN < 256 ? KN : 256;     // threads along the (k, n) pairs; the rest split the rows
    const int R = 256 / lanes_e;
    const int e0 = threadIdx.x % lanes_e, rl = threadIdx.x / lanes_e;
    // the same-address atomics of different blocks serialise (~88 per us): combine the row-lanes in LDS first,
    // then ONE atomic per (k, n) per block
    for (int eb = 0; eb < KN; eb += lanes_e) {
        const int e = eb + e0;
        float acc = 0.f;
        if (e < KN && rl < R) {
            const int k = e / N, n = e - k * N;
            for (int64_t m = m0 + rl; m < m1; m += R) acc = fmaf(x[m * ldx + k], dy[m * lddy + n], acc);
        }
        sm[threadIdx.x] = acc;
        __syncthreads();
        if (rl == 0 && e < KN) {
            float t = 0.f;
            for (int r = 0; r < R; ++r) t += sm[e0 + r * lanes_e];
            const int k = e / N, n = e - k * N;
            unsafeAtomicAdd(dst + (int64_t)k * ldw + n, scale * t);
        }
        __syncthreads();
    }
    if (dstb != nullptr) {
        const int ln = N < 256 ? N : 256;
        const int Rb = 256 / ln;
        const int n0 = threadIdx.x % ln, rb = threadIdx.x / ln;
        for (int nb = 0; nb < N; nb += ln) {
            const int n = nb + n0;
            float acc = 0.f;
            if (n < N && rb < Rb)
                for (int64_t m = m0 + rb; m < m1; m += Rb) acc += dy[m * lddy + n];
            sm[threadIdx.x] = acc;
            __syncthreads();
            if (rb == 0 && n < N) {
                float t = 0.f;
                for (int r = 0; r < Rb; ++r) t += sm[n0 + r * ln];
                unsafeAtomicAdd(dstb + n, scale * t);
            }
            __syncthreads();
        }
    }
}

// grouped skinny weight gradient: block (x = row slab, y = group) as skinny_dw_kernel; with `partial` the block's sums are stored
// to partial[group][slab][K*N] (+ [slab][N] for the bias) and summed in slab order by grouped_reduce_kernel (deterministic)
__global__ __launch_bounds__(256) void skinny_dw_grouped_kernel(const float* __restrict__ x, int64_t ldx, int64_t x_gs,
                                                                const float* __restrict__ dy, int64_t lddy, int64_t dy_gs, int64_t M,
                                                                int32_t K, int32_t N, float scale, float* __restrict__ dst,
                                                                int64_t ldw, int64_t w_gs, float* __restrict__ dstb, int64_t b_gs,
                                                                float* __restrict__ partial, int64_t part_gs) {
    __shared__ float sm[256];
    const int64_t z = blockIdx.y;
    x += z * x_gs;
    dy += z * dy_gs;
    dst += z * w_gs;
    if (dstb != nullptr) dstb += z * b_gs;
    const int nslab = gridDim.x;
    const int64_t m0 = (int64_t)blockIdx.x * SK_ROWS;
    const int64_t m1 = m0 + SK_ROWS < M ? m0 + SK_ROWS : M;
    const int KN = K * N;
    float* part = partial != nullptr ? partial + z * part_gs : nullptr;
    const int lanes_e = KN < 256 ? KN : 256;
    const int R = 256 / lanes_e;
    const int e0 = threadIdx.x % lanes_e, rl = threadIdx.x / lanes_e;
    for (int eb = 0; eb < KN; eb += lanes_e) {
        const int e = eb + e0;
        float acc = 0.f;
        if (e < KN && rl < R) {
            const int k = e / N, n = e - k * N;
            for (int64_t m = m0 + rl; m < m1; m += R) acc = fmaf(x[m * ldx + k], dy[m * lddy + n], acc);
        }
        sm[threadIdx.x] = acc;
        __syncthreads();
        if (rl == 0 && e < KN) {
            float t = 0.f;
            for (int r = 0; r < R; ++r) t += sm[e0 + r * lanes_e];
            const int k = e / N, n = e - k * N;
            if (part != nullptr) part[(int64_t)blockIdx.x * KN + e] = t;
            else unsafeAtomicAdd(dst + (int64_t)k * ldw + n, scale * t);
        }
        __syncthreads();
    }
    if (dstb != nullptr) {
        const int ln = N < 256 ? N : 256;
        const int Rb = 256 / ln;
        const int n0 = threadIdx.x % ln, rb = threadIdx.x / ln;
        for (int nb = 0; nb < N; nb += ln) {
            const int n = nb + n0;
            float acc = 0.f;
            if (n < N && rb < Rb)
                for (int64_t m = m0 + rb; m < m1; m += Rb) acc += dy[m * lddy + n];
            sm[threadIdx.x] = acc;
            __syncthreads();
            if (rb == 0 && n < N) {
                float t = 0.f;
                for (int r = 0; r < Rb; ++r) t += sm[n0 + r * ln];
                if (part != nullptr) part[(int64_t)nslab * KN + (int64_t)blockIdx.x * N + n] = t;
                else unsafeAtomicAdd(dstb + n, scale * t);
            }
            __syncthreads();
        }
    }
}

// dst[g][k][n] += scale * sum_s partial[g][s][k][n] ; dstb[g][n] += scale * sum_s partial[g][split][s][n]  (grid.y = group).
// The weight part sums in the order of splitk_reduce_kernel, so a group's dW equals the single-group call's bit for bit.
__global__ __launch_bounds__(256) void grouped_reduce_kernel(const float* __restrict__ partial, int64_t part_gs, int32_t split,
                                                             int64_t K, int32_t N, float scale, float* __restrict__ dst, int64_t ld,
                                                             int64_t w_gs, float* __restrict__ dstb, int64_t b_gs) {
    const int64_t z = blockIdx.y;
    const float* part = partial + z * part_gs;
    dst += z * w_gs;
    const int64_t kn = K * N;
    const int64_t total = kn + (dstb != nullptr ? N : 0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        float acc = 0.f;
        if (i < kn) {
            for (int s = 0; s < split; ++s) acc += part[(int64_t)s * kn + i];
            const int64_t k = i / N;
            const int n = (int)(i - k * N);
            dst[k * ld + n] = fmaf(scale, acc, dst[k * ld + n]);
        } else {
            const int64_t n = i - kn;
            for (int s = 0; s < split; ++s) acc += part[(int64_t)split * kn + (int64_t)s * N + n];
            float* db = dstb + z * b_gs;
            db[n] = fmaf(scale, acc, db[n]);
        }
    }
}

}  // namespace

// the argument blocks of the three operations, shared by the plain and the grouped entry points
static GemmArgs fwd_args(const float* x, int64_t ld_x, const float* W, int64_t ld_w, const float* b, int64_t M, int32_t K, int32_t N,
                         int32_t act, float* y, int64_t ld_y) {
    GemmArgs g = gemm_args(x, ld_x, W, ld_w, M, N, K, y, ld_y);
    g.bias = b; g.act = act;
    return g;
}
// dx[i=m][j=k] = sum_{r=n} dy[m][n] * W[k][n]  -> A = dy (RC), B(r=n, j=k) = W[k*ld_w + n] (RC)
static GemmArgs dx_args(const float* dy, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int32_t K, int32_t N,
                        const float* relu_src, int64_t ld_relu_src, int32_t accumulate, float* dx, int64_t ld_dx) {
    GemmArgs g = gemm_args(dy, ld_dy, W, ld_w, M, K, N, dx, ld_dx);
    g.e0 = relu_src; g.lde0 = ld_relu_src; g.accumulate = accumulate;
    return g;
}

extern "C" int dr_linear_fwd(const float* x, int64_t ld_x, const float* W, int64_t ld_w, const float* b, int64_t M,
                             int32_t K, int32_t N, int32_t act, float* y, int64_t ld_y, dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0 || act < 0 || act > 1) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x || !W || !y || bad_ld(ld_x, K) || bad_ld(ld_w, N) || ld_y < N || misaligned(x) || misaligned(W))
        return DR_EINVAL;
    if (K < 4 || N < 4) {
        hipLaunchKernelGGL(skinny_fwd_kernel, dim3(dr_grid_for(M, 16)), dim3(256), 0, dr_s(stream), x, ld_x, W, ld_w, b, M, K,
                           N, act, y, ld_y);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = fwd_args(x, ld_x, W, ld_w, b, M, K, N, act, y, ld_y);
    return launch<true, false, EPI_BIAS_ACT>(g, dr_s(stream));
}

extern "C" int dr_linear_bwd_dx(const float* dy, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int32_t K,
                                int32_t N, const float* relu_src, int64_t ld_relu_src, int32_t accumulate, float* dx,
                                int64_t ld_dx, dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!dy || !W || !dx || bad_ld(ld_dy, N) || bad_ld(ld_w, N) || ld_dx < K || misaligned(dy) || misaligned(W))
        return DR_EINVAL;
    if (relu_src != nullptr && ld_relu_src < K) return DR_EINVAL;
    if (K < 4 || N < 4) {
        hipLaunchKernelGGL(skinny_dx_kernel, dim3(dr_grid_for(M * K, 256)), dim3(256), 0, dr_s(stream), dy, ld_dy, W, ld_w, M,
                           K, N, relu_src, ld_relu_src, accumulate, dx, ld_dx);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = dx_args(dy, ld_dy, W, ld_w, M, K, N, relu_src, ld_relu_src, accumulate, dx, ld_dx);
    return launch<true, true, EPI_MASK>(g, dr_s(stream));
}

// dgrad of the FIRST tower layer with the FM second-order gradient folded in:
//   d_concat[m, j] = (dy @ W^T)[m, j] + d_fm_logit[m] * (sum_x[m, j % D] - concat[m, j])   for j < F*D
// so the embedding backward needs ONE gradient stream and never re-reads concat (HBM-bound there, free here).
extern "C" int dr_linear_bwd_dx_fm(const float* dy, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int32_t K,
                                   int32_t N, const float* d_fm_logit, const float* sum_x, const float* concat,
                                   int64_t ld_concat, int32_t D, int32_t FD, float* dx, int64_t ld_dx,
                                   dr_stream_t stream) {
    if (M < 0 || K < 4 || N < 4 || D <= 0 || FD < 0 || FD > K) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!dy || !W || !dx || !d_fm_logit || !sum_x || !concat || bad_ld(ld_dy, N) || bad_ld(ld_w, N) || ld_dx < K ||
        ld_concat < FD || misaligned(dy) || misaligned(W))
        return DR_EINVAL;
    GemmArgs g = gemm_args(dy, ld_dy, W, ld_w, M, K, N, dx, ld_dx);
    g.e0 = concat; g.lde0 = ld_concat; g.e1 = sum_x; g.lde1 = D; g.vec = d_fm_logit; g.fm_D = D; g.fm_FD = FD;
    return launch<true, true, EPI_FMGRAD>(g, dr_s(stream));
}

static int dw_split_for(int64_t M, int32_t K, int32_t N, int mode) {
    const int bn = N <= 32 ? 32 : BN;
    const int64_t tiles = ((int64_t)(K + BM - 1) / BM) * ((N + bn - 1) / bn);
    // resident blocks of one wave of the grid: 256 CUs x 3 (native wide tile) or x 2 (bf16x3: 60 KB of LDS per block)
    const int64_t slots = (mode == DR_GEMM_BF16X3 && N > 32) ? 512 : 768;
    int64_t max_split = (M + 8 * BK - 1) / (8 * BK);           // at least 8 k-tiles per block
    if (max_split > 64) max_split = 64;
    if (max_split < 1) max_split = 1;
    // fill whole waves of resident blocks: the smallest split whose last wave is (nearly) as full as the best one
    // (28 tiles: 18 or 27 splits = 98 %; 196 tiles (1677 x 1677 cross wgrad): 5 splits = 96 % instead of 2 = 77 %)
    double best = 0.0;
    for (int64_t sp = 1; sp <= max_split; ++sp) {
        const int64_t blocks = tiles * sp, waves = (blocks + slots - 1) / slots;
        const double eff = (double)blocks / (double)(waves * slots);
        if (eff > best) best = eff;
    }
    for (int64_t sp = 1; sp <= max_split; ++sp) {
        const int64_t blocks = tiles * sp, waves = (blocks + slots - 1) / slots;
        if ((double)blocks / (double)(waves * slots) >= 0.95 * best) return (int)sp;
    }
    return 1;
}
static int dw_split(int64_t M, int32_t K, int32_t N) {
    return dw_split_for(M, K, N, g_gemm_mode.load(std::memory_order_relaxed));
}
// the workspace must be large enough for either mode (the mode may change between the allocation and the call)
static int dw_split_max(int64_t M, int32_t K, int32_t N) {
    const int a = dw_split_for(M, K, N, DR_GEMM_BF16X3), b = dw_split_for(M, K, N, DR_GEMM_NATIVE_F32);
    return a > b ? a : b;
}

// Splits g's reduction over grid.y in about `split` slices.  A slice covers `per` = roundup(ceil(R / split), BK) reduction rows, so
// trailing slices can be EMPTY (R = 8192, split = 31: per = 288, slices 29 and 30 start past R).  An empty block would return
// before storing its partial tile while the reduce still summed that (uninitialised) workspace slice: launch and reduce the
// effective number of slices only.
static void set_split(GemmArgs& g, int split) {
    g.per = ((g.R + split - 1) / split + BK - 1) / BK * BK;
    g.split = (int32_t)((g.R + g.per - 1) / g.per);
}
// dW[i=k][j=n] = sum_{r=m} x[m][k] * dy[m][n] -> A(i=k, r=m) = x[m*ld_x + k] (not RC), B = dy (not RC)
static GemmArgs dw_args(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t M, int32_t K, int32_t N, float scale,
                        float* dstW, int64_t ld_w, float* dstb) {
    GemmArgs g = gemm_args(x, ld_x, dy, ld_dy, K, N, M, dstW, ld_w);
    g.alpha = scale; g.colsum_dst = dstb;
    set_split(g, dw_split(M, K, N));
    return g;
}

extern "C" int64_t dr_linear_bwd_dw_workspace_bytes(int64_t M, int32_t K, int32_t N) {
    if (M <= 0 || K <= 0 || N <= 0) return 0;
    return (int64_t)dw_split_max(M, K, N) * K * N * (int64_t)sizeof(float);
}

extern "C" int dr_linear_bwd_dw(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t M, int32_t K,
                                int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb, float* workspace,
                                int64_t workspace_bytes, dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x || !dy || !dstW || bad_ld(ld_x, K) || bad_ld(ld_dy, N) || ld_w < N || misaligned(x) || misaligned(dy))
        return DR_EINVAL;
    if (K < 4 || N < 4 || M < 4) {
        hipLaunchKernelGGL(skinny_dw_kernel, dim3((unsigned)((M + SK_ROWS - 1) / SK_ROWS)), dim3(256), 0, dr_s(stream), x, ld_x,
                           dy, ld_dy, M, K, N, scale, dstW, ld_w, dstb);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = dw_args(x, ld_x, dy, ld_dy, M, K, N, scale, dstW, ld_w, dstb);
    const bool use_ws = workspace != nullptr && workspace_bytes >= dr_linear_bwd_dw_workspace_bytes(M, K, N) && g.split > 1;
    g.partial = use_ws ? workspace : nullptr;
    int rc = launch<false, false, EPI_ATOMIC>(g, dr_s(stream));
    if (rc != DR_OK) return rc;
    if (use_ws) {
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(dr_grid_for((int64_t)K * N, 256)), dim3(256), 0, dr_s(stream), workspace,
                           g.split, (int64_t)K, N, scale, dstW, ld_w);
        DR_CHECK_LAUNCH();
    }
    return DR_OK;
}

// ---- grouped dense layers: G independent problems of one shape in one launch (gridDim.z = G on the tile kernel, grid.y on the
// skinny kernels).  Group g reads x from x + g*x_gs (pitch ld_x), W from W + g*w_gs, b from b + g*b_gs and writes y + g*y_gs.
// grid.x cap of a memory-bound kernel whose grid.y runs over G groups: dr_grid_for's 2048 blocks in all
static int group_blocks(int32_t G) { return 2048 / G > 0 ? 2048 / G : 1; }
static bool bad_group(int32_t G, int64_t a, int64_t b, int64_t c, int64_t d) {
    return G < 1 || a < 0 || b < 0 || c < 0 || d < 0;
}

extern "C" int dr_linear_fwd_grouped(const float* x, int64_t ld_x, int64_t x_gs, const float* W, int64_t ld_w, int64_t w_gs,
                                     const float* b, int64_t b_gs, int64_t M, int32_t K, int32_t N, int32_t G, int32_t act,
                                     float* y, int64_t ld_y, int64_t y_gs, dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0 || act < 0 || act > 1 || bad_group(G, x_gs, w_gs, b_gs, y_gs)) return DR_EINVAL;
    if (G > 65535) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    if (!x || !W || !y || bad_ld(ld_x, K) || bad_ld(ld_w, N) || ld_y < N || misaligned(x) || misaligned(W)) return DR_EINVAL;
    if (K < 4 || N < 4) {
        hipLaunchKernelGGL(skinny_fwd_grouped_kernel, dim3(dr_grid_for(M, 16, group_blocks(G)), G), dim3(256), 0,
                           dr_s(stream), x, ld_x, x_gs, W, ld_w, w_gs, b, b_gs, M, K, N, act, y, ld_y, y_gs);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = fwd_args(x, ld_x, W, ld_w, b, M, K, N, act, y, ld_y);
    g.groups = G; g.a_gs = x_gs; g.b_gs = w_gs; g.c_gs = y_gs; g.bias_gs = b_gs;
    return launch<true, false, EPI_BIAS_ACT, true>(g, dr_s(stream));
}

extern "C" int dr_linear_bwd_dx_grouped(const float* dy, int64_t ld_dy, int64_t dy_gs, const float* W, int64_t ld_w, int64_t w_gs,
                                        int64_t M, int32_t K, int32_t N, int32_t G, const float* relu_src, int64_t ld_relu_src,
                                        int64_t rs_gs, int32_t accumulate, float* dx, int64_t ld_dx, int64_t dx_gs,
                                        dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0 || bad_group(G, dy_gs, w_gs, rs_gs, dx_gs)) return DR_EINVAL;
    if (G > 65535) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    if (!dy || !W || !dx || bad_ld(ld_dy, N) || bad_ld(ld_w, N) || ld_dx < K || misaligned(dy) || misaligned(W)) return DR_EINVAL;
    if (relu_src != nullptr && ld_relu_src < K) return DR_EINVAL;
    if (K < 4 || N < 4) {
        hipLaunchKernelGGL(skinny_dx_grouped_kernel, dim3(dr_grid_for(M * K, 256, group_blocks(G)), G), dim3(256), 0,
                           dr_s(stream), dy, ld_dy, dy_gs, W, ld_w, w_gs, M, K, N, relu_src, ld_relu_src, rs_gs, accumulate, dx,
                           ld_dx, dx_gs);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = dx_args(dy, ld_dy, W, ld_w, M, K, N, relu_src, ld_relu_src, accumulate, dx, ld_dx);
    g.groups = G; g.a_gs = dy_gs; g.b_gs = w_gs; g.c_gs = dx_gs; g.e0_gs = rs_gs;
    return launch<true, true, EPI_MASK, true>(g, dr_s(stream));
}

static bool dw_skinny(int64_t M, int32_t K, int32_t N) { return K < 4 || N < 4 || M < 4; }
// floats of one group's partials: split slices of [K][N] and of [N]
static int64_t dw_group_floats(int64_t M, int32_t K, int32_t N, int split) { return (int64_t)split * ((int64_t)K * N + N); }

extern "C" int64_t dr_linear_bwd_dw_grouped_workspace_bytes(int64_t M, int32_t K, int32_t N, int32_t G) {
    if (M <= 0 || K <= 0 || N <= 0 || G < 1) return 0;
    const int split = dw_skinny(M, K, N) ? (int)((M + SK_ROWS - 1) / SK_ROWS) : dw_split_max(M, K, N);
    return (int64_t)G * dw_group_floats(M, K, N, split) * (int64_t)sizeof(float);
}

extern "C" int dr_linear_bwd_dw_grouped(const float* x, int64_t ld_x, int64_t x_gs, const float* dy, int64_t ld_dy, int64_t dy_gs,
                                        int64_t M, int32_t K, int32_t N, int32_t G, float scale, float* dstW, int64_t ld_w,
                                        int64_t w_gs, float* dstb, int64_t b_gs, float* workspace, int64_t workspace_bytes,
                                        dr_stream_t stream) {
    if (M < 0 || K <= 0 || N <= 0 || bad_group(G, x_gs, dy_gs, w_gs, b_gs)) return DR_EINVAL;
    if (G > 65535) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    if (!x || !dy || !dstW || bad_ld(ld_x, K) || bad_ld(ld_dy, N) || ld_w < N || misaligned(x) || misaligned(dy)) return DR_EINVAL;
    const bool ws_ok = workspace != nullptr && workspace_bytes >= dr_linear_bwd_dw_grouped_workspace_bytes(M, K, N, G);
    if (dw_skinny(M, K, N)) {
        const int nslab = (int)((M + SK_ROWS - 1) / SK_ROWS);
        const int64_t part_gs = dw_group_floats(M, K, N, nslab);
        hipLaunchKernelGGL(skinny_dw_grouped_kernel, dim3((unsigned)nslab, G), dim3(256), 0, dr_s(stream), x, ld_x, x_gs, dy, ld_dy,
                           dy_gs, M, K, N, scale, dstW, ld_w, w_gs, dstb, b_gs, ws_ok ? workspace : nullptr, part_gs);
        DR_CHECK_LAUNCH();
        if (ws_ok) {
            hipLaunchKernelGGL(grouped_reduce_kernel, dim3(dr_grid_for((int64_t)K * N + N, 256, group_blocks(G)), G),
                               dim3(256), 0, dr_s(stream), workspace, part_gs, nslab, (int64_t)K, N, scale, dstW, ld_w, w_gs, dstb,
                               b_gs);
            DR_CHECK_LAUNCH();
        }
        return DR_OK;
    }
    GemmArgs g = dw_args(x, ld_x, dy, ld_dy, M, K, N, scale, dstW, ld_w, dstb);
    // split == 1: every output element has one writer, the atomic epilogue is already deterministic
    const bool use_ws = ws_ok && g.split > 1;
    const int64_t part_gs = dw_group_floats(M, K, N, g.split);
    g.partial = use_ws ? workspace : nullptr;
    g.groups = G; g.a_gs = x_gs; g.b_gs = dy_gs; g.c_gs = w_gs; g.cs_gs = b_gs; g.part_gs = part_gs;
    int rc = launch<false, false, EPI_ATOMIC, true>(g, dr_s(stream));
    if (rc != DR_OK) return rc;
    if (use_ws) {
        hipLaunchKernelGGL(grouped_reduce_kernel, dim3(dr_grid_for((int64_t)K * N + N, 256, group_blocks(G)), G),
                           dim3(256), 0, dr_s(stream), workspace, part_gs, g.split, (int64_t)K, N, scale, dstW, ld_w, w_gs, dstb,
                           b_gs);
        DR_CHECK_LAUNCH();
    }
    return DR_OK;
}

// y[m][n] += sum_k x[m][k] W[k][n] for SHORT-AND-WIDE problems (few output tiles, long reduction: the two-tower dq = G c with
// G [B, B], c [B, 128] has 64 tiles of 128 x 128 for 256 CUs): the reduction is split over grid.y into a workspace and the
// slices are summed in a fixed order (deterministic), exactly as the weight gradients do.
extern "C" int64_t dr_linear_fwd_splitk_workspace_bytes(int64_t M, int32_t K, int32_t N) {
    if (M <= 0 || K <= 0 || N <= 0 || M > 0x7fffffff) return 0;
    return (int64_t)dw_split_max(K, (int32_t)M, N) * M * N * (int64_t)sizeof(float);
}

extern "C" int dr_linear_fwd_splitk(const float* x, int64_t ld_x, const float* W, int64_t ld_w, int64_t M, int32_t K, int32_t N,
                                    float* y, int64_t ld_y, float* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    if (M < 0 || M > 0x7fffffff || K < 4 || N < 4) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x || !W || !y || !workspace || bad_ld(ld_x, K) || bad_ld(ld_w, N) || ld_y < N || misaligned(x) || misaligned(W))
        return DR_EINVAL;
    if (workspace_bytes < dr_linear_fwd_splitk_workspace_bytes(M, K, N)) return DR_EINVAL;
    // A(i = m, r = k) = x[m ld_x + k] (row-contiguous), B(r = k, j = n) = W[k ld_w + n]
    GemmArgs g = gemm_args(x, ld_x, W, ld_w, M, N, K, y, ld_y);
    g.alpha = 1.f;
    set_split(g, dw_split(K, (int32_t)M, N));
    g.partial = workspace;
    int rc = launch<true, false, EPI_ATOMIC>(g, dr_s(stream));
    if (rc != DR_OK) return rc;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(dr_grid_for(M * N, 256)), dim3(256), 0, dr_s(stream), workspace, g.split, M, N,
                       1.f, y, ld_y);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int32_t dr_set_gemm_mode(int32_t mode) {
    if (mode != DR_GEMM_BF16X3 && mode != DR_GEMM_NATIVE_F32) return DR_EINVAL;
    return g_gemm_mode.exchange(mode);
}

extern "C" int32_t dr_get_gemm_mode(void) { return g_gemm_mode.load(); }

extern "C" int32_t dr_set_gemm_split(int32_t split) {
    if (split != DR_GEMM_SPLIT_BF16X3 && split != DR_GEMM_SPLIT_F16X2) return DR_EINVAL;
    return g_gemm_split.exchange(split);
}

extern "C" int32_t dr_get_gemm_split(void) { return g_gemm_split.load(); }

extern "C" const char* dr_version(void) { return "deep_recommenders_amd hot path / gfx950 / f32"; }
