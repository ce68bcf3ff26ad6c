// The DCN cross layer (Cross.call: keras dcn.py:81-88): out = x0 * (x @ W + b + diag * x) + x as the EPI_CROSS epilogue of the fp32
// GEMM template, and the elementwise combine passes for the forms without a GEMM (W == NULL, tiny widths, the backward).
#include "gemm_f32_core.h"

namespace {

__global__ __launch_bounds__(256) void cross_combine_fwd_kernel(const float* __restrict__ x0,
                                                                const float* __restrict__ x,
                                                                float* __restrict__ prod, const float* __restrict__ b,
                                                                int64_t M, int32_t Dm, int64_t ld, float diag,
                                                                float* __restrict__ out) {
    const int64_t n = M * Dm;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / Dm;
        const int c = (int)(i - r * Dm);
        const int64_t o = r * ld + c;
        const float xv = x[o];
        const float p = prod[o] + (b != nullptr ? b[c] : 0.f) + diag * xv;
        prod[o] = p;
        out[o] = x0[o] * p + xv;
    }
}

__global__ __launch_bounds__(256) void cross_combine_bwd_kernel(const float* __restrict__ x0,
                                                                const float* __restrict__ prod,
                                                                const float* __restrict__ d_out, int64_t M, int32_t Dm,
                                                                int64_t ld, float diag, float* __restrict__ d_prod,
                                                                float* __restrict__ d_x0, float* __restrict__ d_x,
                                                                uint32_t* __restrict__ dp_amax) {
    const int64_t n = M * Dm;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float mx = 0.f;                                           // (dp_amax != NULL: the record of d_prod for the f16x2 GEMMs that read it)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / Dm;
        const int c = (int)(i - r * Dm);
        const int64_t o = r * ld + c;
        const float go = d_out[o];
        const float dp = go * x0[o];
        d_prod[o] = dp;
        mx = fmaxf(mx, fabsf(dp));
        if (d_x0 != nullptr) d_x0[o] += go * prod[o];
        if (d_x != nullptr) d_x[o] += go + diag * dp;
    }
    if (dp_amax != nullptr) {
        uint32_t m = __float_as_uint(mx);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(dp_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dp_amax, m);
    }
}

}  // namespace

extern "C" int dr_cross_fwd(const float* x0, const float* x, int64_t ld, const float* W, int64_t ld_w, const float* b,
                            float diag_scale, int64_t M, int32_t Dm, float* out, float* prod_out,
                            dr_stream_t stream) {
    if (M < 0 || Dm <= 0 || diag_scale < 0.f) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x0 || !x || !out || bad_ld(ld, Dm)) return DR_EINVAL;
    if (W == nullptr) {
        if (prod_out == nullptr) return DR_EINVAL;
        hipLaunchKernelGGL(cross_combine_fwd_kernel, dim3(dr_grid_for(M * Dm, 256)), dim3(256), 0, dr_s(stream), x0, x,
                           prod_out, b, M, Dm, ld, diag_scale, out);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    if (bad_ld(ld_w, Dm) || misaligned(x) || misaligned(W)) return DR_EINVAL;
    if (Dm < 4) {   // tiny feature width: streaming product into prod (or out as scratch), then the combine pass
        float* pbuf = prod_out != nullptr ? prod_out : out;
        const int rc = dr_linear_fwd(x, ld, W, ld_w, nullptr, M, Dm, Dm, 0, pbuf, ld, stream);   // the skinny kernel (dense.hip)
        if (rc != DR_OK) return rc;
        hipLaunchKernelGGL(cross_combine_fwd_kernel, dim3(dr_grid_for(M * Dm, 256)), dim3(256), 0, dr_s(stream), x0, x, pbuf,
                           b, M, Dm, ld, diag_scale, out);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    GemmArgs g = gemm_args(x, ld, W, ld_w, M, Dm, Dm, out, ld);
    g.bias = b; g.e0 = x0; g.lde0 = ld; g.e1 = x; g.lde1 = ld; g.aux = prod_out; g.ldaux = ld;
    g.alpha = diag_scale;
    return launch<true, false, EPI_CROSS>(g, dr_s(stream));
}

// d_prod_amax (may be NULL): also leaves max |d_prod| (float bits) in d_prod_amax[0] (reset first): the amax record of d_prod for the
// f16x2 GEMMs that take it as an operand (dr_h2_linear_nt, dr_h2_wgrad)
extern "C" int dr_cross_combine_bwd(const float* x0, const float* prod, const float* d_out, int64_t M, int32_t Dm,
                                    int64_t ld, float diag_scale, float* d_prod, float* d_x0_accum, float* d_x_accum,
                                    uint32_t* d_prod_amax, dr_stream_t stream) {
    if (M < 0 || Dm <= 0) return DR_EINVAL;
    if (d_prod_amax != nullptr && hipMemsetAsync(d_prod_amax, 0, sizeof(uint32_t), dr_s(stream)) != hipSuccess) return DR_ELAUNCH;
    if (M == 0) return DR_OK;
    if (!x0 || !prod || !d_out || !d_prod || ld < Dm) return DR_EINVAL;
    hipLaunchKernelGGL(cross_combine_bwd_kernel, dim3(dr_grid_for(M * Dm, 256)), dim3(256), 0, dr_s(stream), x0, prod,
                       d_out, M, Dm, ld, diag_scale, d_prod, d_x0_accum, d_x_accum, d_prod_amax);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
