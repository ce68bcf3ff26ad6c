// Multi-task heads: MMoE's gate softmax + expert mixture, the per-task MSE loss, the ESMM probability head, a strided Adam step
// and the input layer's column assembly (include/dr_hotpath.h, "Multi-task learning").
//   gate-mix   p[b,t,:] = softmax(l[b, t*E : (t+1)*E]) ; out[b, t*U+u] = sum_e p[b,t,e] h[b, e*U+u]
//              (estimator/models/multi_task_learning/mixture_of_experts.py:71-77: softmax(dense(inputs)) @ stack(experts))
//   mse        loss[t] = mean_b (pred[b,t] - y[b,t])^2 , d_pred = 2 (pred - y) / B   (tf.losses.mean_squared_error)
//   esmm       p_cvr = sigmoid(l[b,0]), p_ctr = sigmoid(l[b,1]), p_ctcvr = p_ctr * p_cvr   (esmm.py:33-55)
// Every kernel writes each output element once and sums in a fixed order: two launches on the same inputs agree bit for bit.
#include "dr_common.h"
#include <math.h>

namespace {

constexpr int MT_MAX_T = 16;   // tasks per gate-mix row (registers per lane)
constexpr int MT_MAX_E = 64;   // experts: one lane each

// One 64-lane wave per batch row, 4 rows per block, rows grid-strided.  Lane e < E holds p[t][e] for every task; the mixture is
// computed 64 columns u at a time (lane = u), summing over e in ascending order.
__global__ __launch_bounds__(256) void gate_mix_fwd_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ l,
                                                           int64_t ld_l, int64_t B, int E, int T, int U, float* __restrict__ p,
                                                           int64_t ld_p, float* __restrict__ out, int64_t ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t rows_per_grid = (int64_t)gridDim.x * 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < B; row += rows_per_grid) {
        float pr[MT_MAX_T];
#pragma unroll
        for (int t = 0; t < MT_MAX_T; ++t) {
            pr[t] = 0.f;
            if (t < T) {
                const float v = lane < E ? l[row * ld_l + t * E + lane] : -INFINITY;
                const float mx = dr_wave_max(v);
                const float ex = lane < E ? expf(v - mx) : 0.f;
                const float s = dr_wave_sum(ex);
                pr[t] = ex / s;
                if (lane < E) p[row * ld_p + t * E + lane] = pr[t];
            }
        }
        const float* hr = h + row * ld_h;
        float* orow = out + row * ld_out;
        for (int u0 = 0; u0 < U; u0 += 64) {
            const int u = u0 + lane;
            float acc[MT_MAX_T];
#pragma unroll
            for (int t = 0; t < MT_MAX_T; ++t) acc[t] = 0.f;
            for (int e = 0; e < E; ++e) {
                const float hv = u < U ? hr[(int64_t)e * U + u] : 0.f;
#pragma unroll
                for (int t = 0; t < MT_MAX_T; ++t)
                    if (t < T) acc[t] = fmaf(dr_readlane(pr[t], e), hv, acc[t]);
            }
            if (u < U) {
#pragma unroll
                for (int t = 0; t < MT_MAX_T; ++t)
                    if (t < T) orow[(int64_t)t * U + u] = acc[t];
            }
        }
    }
}

// Backward: d_h[e*U+u] = sum_t p[t,e] d_out[t*U+u] (ascending t); g[t,e] = <d_out_t, h_e> as wave reductions over each 64-column
// chunk, accumulated chunk by chunk in lane e; d_l[t,e] = p[t,e] (g[t,e] - sum_e' p[t,e'] g[t,e']).
__global__ __launch_bounds__(256) void gate_mix_bwd_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ p,
                                                           int64_t ld_p, const float* __restrict__ d_out, int64_t ld_do, int64_t B,
                                                           int E, int T, int U, float* __restrict__ d_h, int64_t ld_dh,
                                                           float* __restrict__ d_l, int64_t ld_dl) {
    const int lane = threadIdx.x & 63;
    const int64_t rows_per_grid = (int64_t)gridDim.x * 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < B; row += rows_per_grid) {
        float pr[MT_MAX_T], g[MT_MAX_T];
#pragma unroll
        for (int t = 0; t < MT_MAX_T; ++t) {
            pr[t] = (t < T && lane < E) ? p[row * ld_p + t * E + lane] : 0.f;
            g[t] = 0.f;
        }
        const float* hr = h + row * ld_h;
        const float* dor = d_out + row * ld_do;
        float* dhr = d_h + row * ld_dh;
        for (int u0 = 0; u0 < U; u0 += 64) {
            const int u = u0 + lane;
            float dv[MT_MAX_T];
#pragma unroll
            for (int t = 0; t < MT_MAX_T; ++t) dv[t] = (t < T && u < U) ? dor[(int64_t)t * U + u] : 0.f;
            for (int e = 0; e < E; ++e) {
                const float hv = u < U ? hr[(int64_t)e * U + u] : 0.f;
                float dh = 0.f;
#pragma unroll
                for (int t = 0; t < MT_MAX_T; ++t)
                    if (t < T) dh = fmaf(dr_readlane(pr[t], e), dv[t], dh);
                if (u < U) dhr[(int64_t)e * U + u] = dh;
#pragma unroll
                for (int t = 0; t < MT_MAX_T; ++t)
                    if (t < T) {
                        const float s = dr_wave_sum(dv[t] * hv);     // identical on every lane (xor butterfly)
                        if (lane == e) g[t] += s;
                    }
            }
        }
#pragma unroll
        for (int t = 0; t < MT_MAX_T; ++t)
            if (t < T) {
                const float s = dr_wave_sum(lane < E ? pr[t] * g[t] : 0.f);
                if (lane < E) d_l[row * ld_dl + t * E + lane] = pr[t] * (g[t] - s);
            }
    }
}

// ---- MSE over T task columns: stage 1 grid (blocks, T) writes d_pred and per-block partial sums, stage 2 one block per task
constexpr int MSE_BLOCKS = 256;

__global__ __launch_bounds__(256) void mse_stage1(const float* __restrict__ pred, int64_t ld_pred, const float* __restrict__ y,
                                                  int64_t ld_y, int64_t B, float* __restrict__ d_pred, int64_t ld_d,
                                                  float* __restrict__ partial) {
    __shared__ float red[4];
    const int t = blockIdx.y;
    const float two_inv_n = 2.f / (float)B;
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
        const float r = pred[i * ld_pred + t] - y[i * ld_y + t];
        acc = fmaf(r, r, acc);
        if (d_pred != nullptr) d_pred[i * ld_d + t] = two_inv_n * r;
    }
    acc = dr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)t * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void mse_stage2(const float* __restrict__ partial, int nparts, int64_t B, float* __restrict__ loss) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc += (double)partial[(int64_t)t * nparts + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[t] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / (double)B);
}

// ---- ESMM head
__device__ __forceinline__ float stable_sigmoid(float x) {
    if (x >= 0.f) return 1.f / (1.f + expf(-x));
    const float e = expf(x);
    return e / (1.f + e);
}

__global__ __launch_bounds__(256) void esmm_fwd_kernel(const float* __restrict__ logits, int64_t ld, int64_t B,
                                                       float* __restrict__ p_cvr, float* __restrict__ p_ctr,
                                                       float* __restrict__ p_ctcvr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
        const float cvr = stable_sigmoid(logits[i * ld]);
        const float ctr = stable_sigmoid(logits[i * ld + 1]);
        p_cvr[i] = cvr;
        p_ctr[i] = ctr;
        p_ctcvr[i] = ctr * cvr;
    }
}

__global__ __launch_bounds__(256) void esmm_bwd_kernel(const float* __restrict__ p_cvr, const float* __restrict__ p_ctr,
                                                       const float* __restrict__ d_cvr, const float* __restrict__ d_ctr,
                                                       const float* __restrict__ d_ctcvr, int64_t B, float* __restrict__ d_logits,
                                                       int64_t ld) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
        const float cvr = p_cvr[i], ctr = p_ctr[i];
        const float dcc = d_ctcvr != nullptr ? d_ctcvr[i] : 0.f;
        const float gcvr = (d_cvr != nullptr ? d_cvr[i] : 0.f) + dcc * ctr;
        const float gctr = (d_ctr != nullptr ? d_ctr[i] : 0.f) + dcc * cvr;
        d_logits[i * ld] = gcvr * cvr * (1.f - cvr);
        d_logits[i * ld + 1] = gctr * ctr * (1.f - ctr);
    }
}

// ---- Adam on a [rows, cols] block with its own pitch per operand (a column slice of a concatenated parameter); the same
// arithmetic as dr_adam_step, element for element
__global__ __launch_bounds__(256) void adam_2d_kernel(float* __restrict__ p, int64_t ld_p, const float* __restrict__ g, int64_t ld_g,
                                                      float* __restrict__ m, float* __restrict__ v, int64_t ld_mv, int64_t rows,
                                                      int32_t cols, float lr_t, float b1, float b2, float eps, float gscale) {
    const int64_t n = rows * cols;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        const float gi = g[r * ld_g + c] * gscale;
        const int64_t j = r * ld_mv + c;
        const float mi = fmaf(b1, m[j], (1.f - b1) * gi);
        const float vi = fmaf(b2, v[j], (1.f - b2) * gi * gi);
        m[j] = mi;
        v[j] = vi;
        p[r * ld_p + c] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

// out[m][j] = map[j] >= 0 ? a[m][map[j]] : b[m][-map[j] - 1]
__global__ __launch_bounds__(256) void gather_cols_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                          int64_t ldb, const int32_t* __restrict__ map, int64_t M, int32_t N,
                                                          float* __restrict__ out, int64_t ldo) {
    const int64_t n = M * N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / N;
        const int j = (int)(i - r * N);
        const int s = map[j];
        out[r * ldo + j] = s >= 0 ? a[r * lda + s] : b[r * ldb + (-s - 1)];
    }
}

int gate_mix_check(int64_t B, int32_t E, int32_t T, int32_t U) {
    if (B < 0) return DR_EINVAL;
    if (E < 1 || E > MT_MAX_E || T < 1 || T > MT_MAX_T || U < 1) return DR_ESHAPE;
    return DR_OK;
}

int rows_grid(int64_t B) { return dr_grid_for(B, 4, 8192); }

}  // namespace

extern "C" int dr_mmoe_gate_mix_fwd(const float* h, int64_t ld_h, const float* logits, int64_t ld_l, int64_t B, int32_t E, int32_t T,
                                    int32_t U, float* p, int64_t ld_p, float* out, int64_t ld_out, dr_stream_t stream) {
    int rc = gate_mix_check(B, E, T, U);
    if (rc != DR_OK) return rc;
    if (B == 0) return DR_OK;
    if (!h || !logits || !p || !out || ld_h < (int64_t)E * U || ld_l < (int64_t)T * E || ld_p < (int64_t)T * E ||
        ld_out < (int64_t)T * U)
        return DR_EINVAL;
    hipLaunchKernelGGL(gate_mix_fwd_kernel, dim3(rows_grid(B)), dim3(256), 0, dr_s(stream), h, ld_h, logits, ld_l, B, E, T, U, p, ld_p,
                       out, ld_out);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_mmoe_gate_mix_bwd(const float* h, int64_t ld_h, const float* p, int64_t ld_p, const float* d_out, int64_t ld_do,
                                    int64_t B, int32_t E, int32_t T, int32_t U, float* d_h, int64_t ld_dh, float* d_l, int64_t ld_dl,
                                    dr_stream_t stream) {
    int rc = gate_mix_check(B, E, T, U);
    if (rc != DR_OK) return rc;
    if (B == 0) return DR_OK;
    if (!h || !p || !d_out || !d_h || !d_l || ld_h < (int64_t)E * U || ld_p < (int64_t)T * E || ld_do < (int64_t)T * U ||
        ld_dh < (int64_t)E * U || ld_dl < (int64_t)T * E)
        return DR_EINVAL;
    hipLaunchKernelGGL(gate_mix_bwd_kernel, dim3(rows_grid(B)), dim3(256), 0, dr_s(stream), h, ld_h, p, ld_p, d_out, ld_do, B, E, T, U,
                       d_h, ld_dh, d_l, ld_dl);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_mse_workspace_bytes(int32_t T) { return T < 1 ? 0 : (int64_t)T * MSE_BLOCKS * (int64_t)sizeof(float); }

extern "C" int dr_mse_fwd_bwd(const float* pred, int64_t ld_pred, const float* labels, int64_t ld_labels, int64_t B, int32_t T,
                              float* loss, float* d_pred, int64_t ld_dpred, float* workspace, int64_t workspace_bytes,
                              dr_stream_t stream) {
    if (B <= 0 || T < 1 || T > 65535) return DR_EINVAL;
    if (!pred || !labels || !loss || !workspace || ld_pred < T || ld_labels < T || (d_pred != nullptr && ld_dpred < T) ||
        workspace_bytes < dr_mse_workspace_bytes(T))
        return DR_EINVAL;
    const int grid = dr_grid_for(B, 256, MSE_BLOCKS);
    hipLaunchKernelGGL(mse_stage1, dim3(grid, T), dim3(256), 0, dr_s(stream), pred, ld_pred, labels, ld_labels, B, d_pred, ld_dpred,
                       workspace);
    hipLaunchKernelGGL(mse_stage2, dim3(T), dim3(256), 0, dr_s(stream), workspace, grid, B, loss);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_esmm_head_fwd(const float* logits, int64_t ld_logits, int64_t B, float* p_cvr, float* p_ctr, float* p_ctcvr,
                                dr_stream_t stream) {
    if (B < 0) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!logits || !p_cvr || !p_ctr || !p_ctcvr || ld_logits < 2) return DR_EINVAL;
    hipLaunchKernelGGL(esmm_fwd_kernel, dim3(dr_grid_for(B, 256)), dim3(256), 0, dr_s(stream), logits, ld_logits, B, p_cvr, p_ctr,
                       p_ctcvr);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_esmm_head_bwd(const float* p_cvr, const float* p_ctr, const float* d_cvr, const float* d_ctr, const float* d_ctcvr,
                                int64_t B, float* d_logits, int64_t ld_dlogits, dr_stream_t stream) {
    if (B < 0) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!p_cvr || !p_ctr || !d_logits || ld_dlogits < 2) return DR_EINVAL;
    hipLaunchKernelGGL(esmm_bwd_kernel, dim3(dr_grid_for(B, 256)), dim3(256), 0, dr_s(stream), p_cvr, p_ctr, d_cvr, d_ctr, d_ctcvr, B,
                       d_logits, ld_dlogits);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_adam_step_2d(float* param, int64_t ld_p, const float* grad, int64_t ld_g, float* m, float* v, int64_t ld_mv,
                               int64_t rows, int32_t cols, float lr_t, float beta1, float beta2, float eps, float grad_scale,
                               dr_stream_t stream) {
    if (rows < 0 || cols < 0) return DR_EINVAL;
    if (rows == 0 || cols == 0) return DR_OK;
    if (!param || !grad || !m || !v || ld_p < cols || ld_g < cols || ld_mv < cols) return DR_EINVAL;
    hipLaunchKernelGGL(adam_2d_kernel, dim3(dr_grid_for(rows * cols, 256 * 4)), dim3(256), 0, dr_s(stream), param, ld_p, grad, ld_g, m,
                       v, ld_mv, rows, cols, lr_t, beta1, beta2, eps, grad_scale);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_gather_cols(const float* a, int64_t lda, const float* b, int64_t ldb, const int32_t* map, int64_t M, int32_t N,
                              float* out, int64_t ldo, dr_stream_t stream) {
    if (M < 0 || N < 0) return DR_EINVAL;
    if (M == 0 || N == 0) return DR_OK;
    if (!map || !out || ldo < N || (a == nullptr && b == nullptr)) return DR_EINVAL;
    hipLaunchKernelGGL(gather_cols_kernel, dim3(dr_grid_for(M * N, 256)), dim3(256), 0, dr_s(stream), a, lda, b, ldb, map, M, N, out,
                       ldo);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
