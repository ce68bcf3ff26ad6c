// The fused tower head: the last hidden layer's GEMM with the Dense(1), the loss and their backward in its epilogue (EPI_HEAD of the
// fp32 GEMM template), and the small kernel that sums the per-block partials.
#include "gemm_f32_core.h"

// w2[n] += scale * sum_b partial[b][n] ; b2 += scale * sum_b partial[b][32] ; loss = inv_n * sum_b partial[b][33].
// Fixed summation order.  7 groups of 34 threads stride over the blocks with 8 loads in flight each: a plain
// "acc += partial[b]" loop is a chain of dependent L2 round trips (128 of them cost ~45 us for a 70 KB reduction).
__global__ __launch_bounds__(256) void head_finish_kernel(const float* __restrict__ partial, int32_t nblocks, int32_t N,
                                                          float scale, float inv_n, float* w2, int64_t ldw2,
                                                          float* b2, float* __restrict__ loss_out) {
    constexpr int NG = 7;
    __shared__ float red[NG][HEAD_PART];
    const int grp = threadIdx.x / HEAD_PART, c = threadIdx.x % HEAD_PART;
    if (grp < NG) {
        float acc = 0.f;
        for (int b0 = grp; b0 < nblocks; b0 += NG * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int b = b0 + u * NG;
                v[u] = partial[(int64_t)(b < nblocks ? b : b0) * HEAD_PART + c];
                if (b >= nblocks) v[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        red[grp][c] = acc;
    }
    __syncthreads();
    if (threadIdx.x < HEAD_PART) {
        float sacc = 0.f;
#pragma unroll
        for (int g2 = 0; g2 < NG; ++g2) sacc += red[g2][c];
        if (c < 32) {
            if (c < N && w2 != nullptr && scale != 0.f) w2[(int64_t)c * ldw2] = fmaf(scale, sacc, w2[(int64_t)c * ldw2]);
        } else if (c == 32) {
            if (b2 != nullptr && scale != 0.f) b2[0] = fmaf(scale, sacc, b2[0]);
        } else if (loss_out != nullptr) {
            loss_out[0] = sacc * inv_n;
        }
    }
}

extern "C" int64_t dr_tower_head_workspace_bytes(int64_t M) {
    const int64_t tiles = (M + BM - 1) / BM;
    return (tiles > 0 ? tiles : 1) * HEAD_PART * (int64_t)sizeof(float);
}

// In two halves (parts = 1: the GEMM + head kernel -- prob, d_logit, d_h and the per-block partials; parts = 2: the small finish kernel
// that sums the partials into dst_w2 / dst_b2 / loss_out; 3 = both).  Nothing the rest of the step reads comes out of part 2, so a
// caller may run it on another stream (it must finish before the NEXT call's part 1: w2 / b2 and the workspace).  Round 4: the three
// small reduce kernels of the step off the training stream.
extern "C" int dr_tower_head_fwd_bwd(const float* x, int64_t ld_x, const float* W1, int64_t ld_w1, const float* b1,
                                     int64_t M, int64_t n_total, int32_t K, int32_t H, int32_t act, const float* w2,
                                     int64_t ld_w2, const float* b2, const float* extra_logit, const float* labels,
                                     int32_t loss_mode, float scale, float* dst_w2, int64_t ld_dst_w2, float* dst_b2,
                                     float* h_out, int64_t ld_h, float* prob, float* d_logit, float* d_h, int64_t ld_dh,
                                     float* loss_out, void* workspace, int64_t workspace_bytes, int32_t parts, dr_stream_t stream) {
    if (parts < 1 || parts > 3) return DR_EINVAL;
    if (M <= 0 || K <= 0 || H <= 0) return DR_EINVAL;
    if (H > 32) return DR_ESHAPE;
    if (!x || !W1 || !w2 || !labels || !workspace || loss_mode < 0 || loss_mode > 2) return DR_EINVAL;
    if (ld_x < K || ld_w1 < H || ld_w2 < 1 || (dst_w2 && ld_dst_w2 < 1) || (h_out && ld_h < H) || (d_h && ld_dh < H)) return DR_EINVAL;
    if (workspace_bytes < dr_tower_head_workspace_bytes(M)) return DR_EINVAL;
    GemmArgs g = gemm_args(x, ld_x, W1, ld_w1, M, H, K, h_out, ld_h);
    g.bias = b1; g.act = act;
    g.head_w = w2; g.ld_head_w = ld_w2; g.head_b = b2; g.head_extra = extra_logit; g.labels = labels;
    g.loss_mode = loss_mode; g.inv_n = 1.f / (float)(n_total > 0 ? n_total : M);
    g.prob = prob; g.d_logit = d_logit; g.d_h = d_h; g.ld_dh = ld_dh;
    g.head_partial = static_cast<float*>(workspace);
    if (parts & 1) {
        int rc = launch<true, false, EPI_HEAD>(g, dr_s(stream));
        if (rc != DR_OK) return rc;
    }
    if (parts & 2) {
        const int nblocks = (int)((M + BM - 1) / BM);
        hipLaunchKernelGGL(head_finish_kernel, dim3(1), dim3(256), 0, dr_s(stream), g.head_partial, nblocks, H, scale, g.inv_n,
                           dst_w2, ld_dst_w2, dst_b2, loss_out);
    }
    DR_CHECK_LAUNCH();
    return DR_OK;
}

