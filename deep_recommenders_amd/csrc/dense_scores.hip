// The two-tower score passes on the fp32 GEMM template: the in-batch sampled softmax forward (EPI_LSE) and gradient (EPI_SMGRAD),
// the plain scores a @ b^T, and the top-K filter (EPI_FILTER).
#include "gemm_f32_core.h"

// ---- K9: in-batch sampled softmax (Retrieval.call, keras/models/retrieval/sbcnm.py:120-151 of the reference) ----------
__global__ __launch_bounds__(256) void lse_finalize_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                           int32_t nparts, int64_t B, const float* __restrict__ pos,
                                                           const float* __restrict__ w, float* __restrict__ row_lse,
                                                           float* __restrict__ block_sums) {
    __shared__ float red[4];
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
        float m = -INFINITY;
        for (int p = 0; p < nparts; ++p) m = fmaxf(m, part_m[(int64_t)p * B + i]);
        float l = 0.f;
        for (int p = 0; p < nparts; ++p) l += part_l[(int64_t)p * B + i] * safe_exp(part_m[(int64_t)p * B + i] - m);
        const float lse = m + logf(l);
        row_lse[i] = lse;
        acc += (w != nullptr ? w[i] : 1.f) * (lse - pos[i]);
    }
    acc = dr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sum_blocks_kernel(const float* __restrict__ block_sums, int n, float* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)block_sums[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

// f16x2 path of the two score passes (round 5): bf3_gemm.hip's register-split kernel with the LSE / softmax-gradient epilogues (rs_args.h); the
// candidates' two fp16 planes and both amax records live behind the partials in the workspace.
constexpr int IB_H2_MAX_D = 512;                        // the workspace is sized without knowing D: planes budgeted for D <= 512
static int64_t ib_parts_floats(int64_t B) {
    const int64_t tiles_n = (B + BN - 1) / BN;
    return 2 * tiles_n * 2 * B + 1024;
}
static int64_t ib_h2_offset_bytes(int64_t B) { return (ib_parts_floats(B) * 4 + 255) / 256 * 256; }
static int64_t ib_h2_bytes(int64_t B) { return 256 + 2 * ((B + 31) / 32 * 32) * IB_H2_MAX_D * 2; }

extern "C" int64_t dr_inbatch_softmax_workspace_bytes(int64_t B) {
    return ib_h2_offset_bytes(B) + ib_h2_bytes(B);
}

// records + candidate planes into the workspace; returns false when the f16x2 path does not apply (the caller runs the fp32 kernel)
static bool ib_h2_prepare(const float* q, const float* c, int64_t B, int32_t D, float* workspace, int64_t workspace_bytes, hipStream_t stream,
                          uint32_t** rec, void** planes, int64_t* ps, int64_t* ld, int* rc) {
    *rc = DR_OK;
    if (dr_get_gemm_split() != DR_GEMM_SPLIT_F16X2 || workspace == nullptr || (D % 4) != 0 || D > IB_H2_MAX_D || B < 256) return false;
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return false;
    if (workspace_bytes < ib_h2_offset_bytes(B) + ib_h2_bytes(B)) return false;
    char* base = reinterpret_cast<char*>(workspace) + ib_h2_offset_bytes(B);
    *rec = reinterpret_cast<uint32_t*>(base);
    *planes = base + 256;
    *ld = ((int64_t)D + 31) / 32 * 32;
    *ps = ((B + 31) / 32 * 32) * *ld;
    if ((D % 32) != 0 && hipMemsetAsync(*planes, 0, (size_t)(2 * *ps * 2), stream) != hipSuccess) { *rc = DR_ELAUNCH; return true; }
    *rc = dr_h2_amax(q, D, B, D, *rec, 1, stream);
    if (*rc == DR_OK) *rc = dr_h2_amax(c, D, B, D, *rec + 1, 1, stream);
    if (*rc == DR_OK) *rc = dr_h2_split(c, D, B, D, *planes, *ps, *ld, 0, 0, 0, *rec + 1, stream);
    return true;
}

extern "C" int dr_inbatch_softmax_fwd(const float* q, const float* c, int64_t B, int32_t D, const float* cand_prob,
                                      const int64_t* cand_ids, const float* sample_weight, float inv_temperature,
                                      float* row_lse, float* pos_score, float* loss_out, float* workspace,
                                      int64_t workspace_bytes, dr_stream_t stream) {
    if (B <= 0 || D < 4 || B > 0x7fffffff) return DR_EINVAL;
    if (!q || !c || !row_lse || !pos_score || !loss_out || !workspace) return DR_EINVAL;
    if (workspace_bytes < dr_inbatch_softmax_workspace_bytes(B)) return DR_EINVAL;
    const int tiles_n = (int)((B + BN - 1) / BN);
    GemmArgs g = gemm_args(q, D, c, D, B, (int32_t)B, D, nullptr, 0);
    g.cand_prob = cand_prob; g.cand_ids = cand_ids; g.inv_t = inv_temperature;
    g.part_m = workspace; g.part_l = workspace + (int64_t)2 * tiles_n * B; g.pos = pos_score;
    int nparts = 2 * tiles_n;
    uint32_t* rec = nullptr;
    void* planes = nullptr;
    int64_t ps = 0, ld = 0;
    int rc = DR_OK;
    if (ib_h2_prepare(q, c, B, D, workspace, workspace_bytes, dr_s(stream), &rec, &planes, &ps, &ld, &rc)) {
        // the scores on the f16x2 register-split kernel (three fp16 products per fp32 product; 256-column tiles: one partial per tile)
        if (rc == DR_OK)
            rc = dr_h2_inbatch_lse(q, D, rec, planes, ps, ld, rec + 1, B, D, cand_prob, cand_ids, inv_temperature, g.part_m, g.part_l,
                                   pos_score, stream);
        nparts = (int)((B + 255) / 256);
    } else {
        rc = launch<true, true, EPI_LSE>(g, dr_s(stream));
    }
    if (rc != DR_OK) return rc;
    float* block_sums = workspace + (int64_t)4 * tiles_n * B;
    const int grid = dr_grid_for(B, 256, 512);
    hipLaunchKernelGGL(lse_finalize_kernel, dim3(grid), dim3(256), 0, dr_s(stream), g.part_m, g.part_l, nparts, B,
                       pos_score, sample_weight, row_lse, block_sums);
    hipLaunchKernelGGL(sum_blocks_kernel, dim3(1), dim3(256), 0, dr_s(stream), block_sums, grid, loss_out);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// G[i][j] = d_loss * w_i * (softmax_ij - delta_ij) * inv_t  (the gradient of the loss wrt the raw q.c^T scores);
// the caller finishes with two plain GEMMs: dq = G @ c (dr_linear_fwd), dc = G^T @ q (dr_linear_bwd_dw).
// workspace (may be NULL; dr_inbatch_softmax_workspace_bytes(B) bytes; the forward's may be reused, its contents are not needed): lets
// the pass run on the f16x2 register-split kernel, which wants the candidates as fp16 planes.  workspace NULL / too small, or a split /
// shape the f16x2 path does not take: the fp32 kernel.
extern "C" int dr_inbatch_softmax_grad_scores(const float* q, const float* c, int64_t B, int32_t D, const float* cand_prob,
                                              const int64_t* cand_ids, const float* sample_weight, float inv_temperature,
                                              const float* row_lse, float d_loss, float* G, int64_t ld_g, float* workspace,
                                              int64_t workspace_bytes, dr_stream_t stream) {
    if (B <= 0 || D < 4 || B > 0x7fffffff || ld_g < B) return DR_EINVAL;
    if (!q || !c || !row_lse || !G) return DR_EINVAL;
    uint32_t* rec = nullptr;
    void* planes = nullptr;
    int64_t ps = 0, ld = 0;
    int rc = DR_OK;
    if (ib_h2_prepare(q, c, B, D, workspace, workspace_bytes, dr_s(stream), &rec, &planes, &ps, &ld, &rc)) {
        if (rc != DR_OK) return rc;
        return dr_h2_inbatch_smgrad(q, D, rec, planes, ps, ld, rec + 1, B, D, cand_prob, cand_ids, inv_temperature, row_lse, sample_weight,
                                    d_loss, G, ld_g, stream);
    }
    GemmArgs g = gemm_args(q, D, c, D, B, (int32_t)B, D, G, ld_g);
    g.cand_prob = cand_prob; g.cand_ids = cand_ids; g.inv_t = inv_temperature; g.lse = row_lse; g.vec = sample_weight;
    g.alpha = d_loss;
    return launch<true, true, EPI_SMGRAD>(g, dr_s(stream));
}

// plain scores = a @ b^T for two reduction-contiguous operands (queries x candidates), used by the top-K search
// internal (C++ linkage, used by retrieval.hip): scores = a @ b^T, filtered against tau into per-row candidate lists
int dr_scores_nt_filter(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t M, int32_t N, int32_t D,
                        const float* tau, float* cand_s, int32_t* cand_c, int32_t* cand_cnt, int64_t cand_cap,
                        dr_stream_t stream) {
    if (M < 0 || N <= 0 || D < 4 || lda < D || ldb < D || cand_cap <= 0) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!a || !b || !tau || !cand_s || !cand_c || !cand_cnt) return DR_EINVAL;
    GemmArgs g = gemm_args(a, lda, b, ldb, M, N, D, nullptr, 0);
    g.tau = tau; g.cand_s = cand_s; g.cand_c = cand_c; g.cand_cnt = cand_cnt; g.cand_cap = cand_cap;
    return launch<true, true, EPI_FILTER>(g, dr_s(stream));
}

extern "C" int dr_scores_nt(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t M, int32_t N, int32_t D,
                            float* out, int64_t ld_out, dr_stream_t stream) {
    if (M < 0 || N <= 0 || D < 4 || ld_out < N || lda < D || ldb < D) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!a || !b || !out) return DR_EINVAL;
    GemmArgs g = gemm_args(a, lda, b, ldb, M, N, D, out, ld_out);
    return launch<true, true, EPI_BIAS_ACT>(g, dr_s(stream));
}

