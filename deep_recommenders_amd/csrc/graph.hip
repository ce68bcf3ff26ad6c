// Graph aggregation for the GCN layer (include/dr_hotpath.h, "Graph convolution"):
//   spmm       out[r] = sum_k val[k] X[col[k]] over k in [row_ptr[r], row_ptr[r+1])   (tf.sparse.sparse_dense_matmul, gcn.py:44-52)
//   plan       the long rows of a CSR and their fixed chunks (built once per graph)
//   transpose  the CSR of A^T on the device, sources ascending inside each column (the backward dX = A^T dAgg is the same spmm)
//   softmax    wave-per-row softmax and its Jacobian product (the `activation="softmax"` output layer)
//   cce_prob   Keras' categorical cross-entropy on probabilities (normalise, clip to [eps, 1 - eps]) per row, with its gradient
// No float atomics anywhere: every output element is written once and summed in a fixed order, so two calls agree bit for bit.
#include "dr_common.h"
#include "dr_scan.h"
#include "dr_csr_gather.h"      // load_cols / store_cols / fma4 / gather_seg, shared with intent_conv.hip
#include <math.h>
#include <algorithm>

#ifndef DR_CSR_LONG_ROW
#define DR_CSR_LONG_ROW 512       // rows with more entries are split (measured on the scaled power-law graph)
#endif

namespace {

constexpr int64_t LONG_ROW = DR_CSR_LONG_ROW;
constexpr int64_t CHUNK = 512;     // entries per chunk of a long row

__device__ __forceinline__ float4 epilogue(float4 v, int64_t r, int s, int D, const float* __restrict__ relu_src, int64_t ld_rs,
                                           int accumulate, const float* __restrict__ out, int64_t ld_out) {
    if (relu_src != nullptr) {
        const float4 m = load_cols(relu_src + r * ld_rs, s, D);
        v.x = m.x > 0.f ? v.x : 0.f;
        v.y = m.y > 0.f ? v.y : 0.f;
        v.z = m.z > 0.f ? v.z : 0.f;
        v.w = m.w > 0.f ? v.w : 0.f;
    }
    if (accumulate) {
        const float4 o = load_cols(out + r * ld_out, s, D);
        v.x += o.x;
        v.y += o.y;
        v.z += o.z;
        v.w += o.w;
    }
    return v;
}

// Short rows: one group of G lanes per row (64 / G rows per wave), lane gl owns float4 slots gl, gl + 64, ... (the second and later
// only when G == 64 and D > 256).  Rows longer than LONG_ROW are skipped here: spmm_chunk_kernel + spmm_combine_kernel write them.
template <int G>
__global__ __launch_bounds__(256) void spmm_rows_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ val, int64_t n_rows, const float* __restrict__ X,
                                                        int64_t ld_x, int D, const float* __restrict__ relu_src, int64_t ld_rs,
                                                        int accumulate, float* __restrict__ out, int64_t ld_out) {
    constexpr int RW = 64 / G;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r = wave * RW + lane / G;
    int64_t kb = 0, ke = 0;
    bool mine = false;
    if (r < n_rows) {
        kb = row_ptr[r];
        ke = row_ptr[r + 1];
        mine = ke - kb <= LONG_ROW;
        if (!mine) ke = kb;
    }
    const int D4 = (D + 3) >> 2;
    for (int s0 = 0; s0 < D4; s0 += G) {            // one pass unless G == 64 and D > 256
        const int s = s0 + (lane & (G - 1));
        float4 v = gather_seg<G>(col, val, kb, ke, X, ld_x, s, D);
        if (mine && s < D4) store_cols(out + r * ld_out, s, D, epilogue(v, r, s, D, relu_src, ld_rs, accumulate, out, ld_out));
    }
}

// Plan layout (int64): [0] n_long, [1] n_chunks, long_row[L], long_first[L + 1], chunk_row[C], chunk_kb[C]
struct PlanView {
    int64_t* hdr;
    int64_t* long_row;
    int64_t* long_first;
    int64_t* chunk_row;
    int64_t* chunk_kb;
};
__host__ __device__ inline int64_t plan_max_long(int64_t nnz) { return nnz / (LONG_ROW + 1); }
__host__ __device__ inline int64_t plan_max_chunks(int64_t nnz) { return plan_max_long(nnz) + (nnz + CHUNK - 1) / CHUNK; }
__host__ __device__ inline PlanView plan_view(int64_t* p, int64_t nnz) {
    const int64_t L = plan_max_long(nnz), C = plan_max_chunks(nnz);
    PlanView v;
    v.hdr = p;
    v.long_row = p + 2;
    v.long_first = v.long_row + L;
    v.chunk_row = v.long_first + L + 1;
    v.chunk_kb = v.chunk_row + C;
    return v;
}

// One chunk of a long row per group: its partial sum goes to ws[chunk] (row pitch ld_ws).  Chunks are grid-strided over the plan's
// device-side count.
template <int G>
__global__ __launch_bounds__(256) void spmm_chunk_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, const int64_t* __restrict__ plan, int64_t nnz,
                                                         const float* __restrict__ X, int64_t ld_x, int D, float* __restrict__ ws,
                                                         int64_t ld_ws) {
    constexpr int RW = 64 / G;
    const PlanView pv = plan_view(const_cast<int64_t*>(plan), nnz);
    const int64_t n_chunks = pv.hdr[1];
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    const int D4 = (D + 3) >> 2;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW; base < n_chunks; base += n_waves * RW) {
        const int64_t q = base + lane / G;
        int64_t kb = 0, ke = 0;
        if (q < n_chunks) {
            kb = pv.chunk_kb[q];
            ke = min(kb + CHUNK, row_ptr[pv.chunk_row[q] + 1]);
        }
        for (int s0 = 0; s0 < D4; s0 += G) {
            const int s = s0 + (lane & (G - 1));
            float4 v = gather_seg<G>(col, val, kb, ke, X, ld_x, s, D);
            if (q < n_chunks && s < D4) *reinterpret_cast<float4*>(ws + q * ld_ws + 4 * s) = v;
        }
    }
}

// A long row's chunks added in chunk order (one lane per float4 slot, 64 slots per pass), then the epilogue.
__global__ __launch_bounds__(256) void spmm_combine_kernel(const int64_t* __restrict__ plan, int64_t nnz, int D,
                                                           const float* __restrict__ ws, int64_t ld_ws,
                                                           const float* __restrict__ relu_src, int64_t ld_rs, int accumulate,
                                                           float* __restrict__ out, int64_t ld_out) {
    const PlanView pv = plan_view(const_cast<int64_t*>(plan), nnz);
    const int64_t n_long = pv.hdr[0];
    const int lane = threadIdx.x & 63;
    const int D4 = (D + 3) >> 2;
    for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n_long; j += (int64_t)gridDim.x * 4) {
        const int64_t r = pv.long_row[j], q0 = pv.long_first[j], q1 = pv.long_first[j + 1];
        for (int s = lane; s < D4; s += 64) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int64_t q = q0; q < q1; ++q) {
                const float4 p = *reinterpret_cast<const float4*>(ws + q * ld_ws + 4 * s);
                acc.x += p.x;
                acc.y += p.y;
                acc.z += p.z;
                acc.w += p.w;
            }
            store_cols(out + r * ld_out, s, D, epilogue(acc, r, s, D, relu_src, ld_rs, accumulate, out, ld_out));
        }
    }
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plan_count_kernel(const int64_t* __restrict__ row_ptr, int64_t n_rows,
                                                         int64_t* __restrict__ is_long, int64_t* __restrict__ n_ch) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        const int64_t len = row_ptr[r + 1] - row_ptr[r];
        const bool lg = len > LONG_ROW;
        is_long[r] = lg ? 1 : 0;
        n_ch[r] = lg ? (len + CHUNK - 1) / CHUNK : 0;
    }
}

// is_long / n_ch still hold the counts, long_ix / ch_ix their exclusive scans
__global__ __launch_bounds__(256) void plan_fill_kernel(const int64_t* __restrict__ row_ptr, int64_t n_rows, int64_t nnz,
                                                        const int64_t* __restrict__ is_long, const int64_t* __restrict__ n_ch,
                                                        const int64_t* __restrict__ long_ix, const int64_t* __restrict__ ch_ix,
                                                        int64_t* __restrict__ plan) {
    const PlanView pv = plan_view(plan, nnz);
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        if (is_long[r]) {
            const int64_t j = long_ix[r], q0 = ch_ix[r];
            pv.long_row[j] = r;
            pv.long_first[j] = q0;
            for (int64_t q = 0; q < n_ch[r]; ++q) {
                pv.chunk_row[q0 + q] = r;
                pv.chunk_kb[q0 + q] = row_ptr[r] + q * CHUNK;
            }
        }
        if (r == n_rows - 1) {
            const int64_t L = long_ix[r] + is_long[r], C = ch_ix[r] + n_ch[r];
            pv.hdr[0] = L;
            pv.hdr[1] = C;
            pv.long_first[L] = C;
        }
    }
}

__global__ void plan_empty_kernel(int64_t* __restrict__ plan) {
    if (threadIdx.x == 0) {
        plan[0] = 0;
        plan[1] = 0;
    }
}

// ---- transpose: stable LSD radix sort of the entries by column, 8 bits per pass ----------------------------------------------
constexpr int RADIX_TILE = 256 * 8;

__global__ __launch_bounds__(256) void expand_rows_kernel(const int64_t* __restrict__ row_ptr, int64_t n_rows, int32_t* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += (int64_t)gridDim.x * 4)
        for (int64_t k = row_ptr[r] + lane; k < row_ptr[r + 1]; k += 64) rows[k] = (int32_t)r;
}

// hist[d * n_tiles + tile] = number of keys of the tile whose digit is d
__global__ __launch_bounds__(256) void radix_hist_kernel(const int32_t* __restrict__ keys, int64_t n, int shift, int64_t n_tiles,
                                                         int64_t* __restrict__ hist) {
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RADIX_TILE;
    for (int i = threadIdx.x; i < RADIX_TILE; i += 256)
        if (base + i < n) atomicAdd(&cnt[((uint32_t)keys[base + i] >> shift) & 255], 1);     // integer count: exact
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// Stable scatter: the tile's keys in 8 rounds of 256 in index order; a key's place among equal digits of its round comes from a
// 64-lane match (8 ballots) plus the counts of the waves before it and of the rounds before.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ pay_i,
                                                            const float* __restrict__ pay_f, int64_t n, int shift, int64_t n_tiles,
                                                            const int64_t* __restrict__ offs, int32_t* __restrict__ keys_out,
                                                            int32_t* __restrict__ pay_i_out, float* __restrict__ pay_f_out) {
    __shared__ int64_t base_d[256];
    __shared__ int run[256];
    __shared__ int wcnt[4][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    base_d[t] = offs[(int64_t)t * n_tiles + blockIdx.x];
    run[t] = 0;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int round = 0; round < RADIX_TILE / 256; ++round) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wcnt[i][t] = 0;
        __syncthreads();
        const int64_t e = (int64_t)blockIdx.x * RADIX_TILE + round * 256 + t;
        const bool ok = e < n;
        const int32_t key = ok ? keys[e] : 0;
        const int d = ((uint32_t)key >> shift) & 255;
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bl = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? bl : ~bl;
        }
        const int rank = __popcll(peers & lt_mask);
        if (ok && rank == 0) wcnt[w][d] = __popcll(peers);
        __syncthreads();
        if (ok) {
            int off = run[d];
            for (int i = 0; i < w; ++i) off += wcnt[i][d];
            const int64_t pos = base_d[d] + off + rank;
            keys_out[pos] = key;
            pay_i_out[pos] = pay_i[e];
            pay_f_out[pos] = pay_f[e];
        }
        __syncthreads();
        run[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
    }
}

// t_row_ptr[c] = first position of a key >= c in the sorted keys (c = 0 .. n_cols)
__global__ __launch_bounds__(256) void lower_bound_kernel(const int32_t* __restrict__ keys, int64_t n, int64_t n_cols,
                                                          int64_t* __restrict__ t_row_ptr) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= n_cols; c += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        t_row_ptr[c] = lo;
    }
}

int radix_passes(int64_t n_cols) {
    int bits = 0;
    while (bits < 31 && ((n_cols - 1) >> bits) > 0) ++bits;
    return bits == 0 ? 1 : (bits + 7) / 8;
}

// ---- softmax over rows ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* __restrict__ x, int64_t ld_x, int64_t B, int C,
                                                          float* __restrict__ y, int64_t ld_y) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < B; r += (int64_t)gridDim.x * 4) {
        const float* xr = x + r * ld_x;
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
        m = dr_wave_max(m);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(xr[c] - m);
        s = dr_wave_sum(s);
        const float inv = 1.f / s;
        for (int c = lane; c < C; c += 64) y[r * ld_y + c] = expf(xr[c] - m) * inv;
    }
}

// dx = y * (dy - sum_c y dy)
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ y, int64_t ld_y, const float* __restrict__ dy,
                                                          int64_t ld_dy, int64_t B, int C, float* __restrict__ dx, int64_t ld_dx) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < B; r += (int64_t)gridDim.x * 4) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(y[r * ld_y + c], dy[r * ld_dy + c], s);
        s = dr_wave_sum(s);
        for (int c = lane; c < C; c += 64) dx[r * ld_dx + c] = y[r * ld_y + c] * (dy[r * ld_dy + c] - s);
    }
}

// Keras categorical_crossentropy on probabilities: q = clip(p / sum p, eps, 1 - eps), row_loss = w_r * -sum_c y log q;
// d row_loss / d p_c = w_r / S * (sum_{c' unclipped} y_c' - [c unclipped] y_c / q_c)
__global__ __launch_bounds__(256) void cce_prob_kernel(const float* __restrict__ p, int64_t ld_p, const float* __restrict__ y,
                                                       int64_t ld_y, int64_t B, int C, const float* __restrict__ w,
                                                       float* __restrict__ row_loss, float* __restrict__ grad, int64_t ld_g) {
    const float eps = 1e-7f;
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < B; r += (int64_t)gridDim.x * 4) {
        float S = 0.f;
        for (int c = lane; c < C; c += 64) S += p[r * ld_p + c];
        S = dr_wave_sum(S);
        const float wr = w != nullptr ? w[r] : 1.f;
        float l = 0.f, yu = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float q = p[r * ld_p + c] / S;
            const float qc = fminf(fmaxf(q, eps), 1.f - eps);
            const float yc = y[r * ld_y + c];
            l -= yc * logf(qc);
            if (q >= eps && q <= 1.f - eps) yu += yc;
        }
        l = dr_wave_sum(l);
        yu = dr_wave_sum(yu);
        if (lane == 0) row_loss[r] = wr * l;
        if (grad != nullptr)
            for (int c = lane; c < C; c += 64) {
                const float q = p[r * ld_p + c] / S;
                const bool u = q >= eps && q <= 1.f - eps;
                grad[r * ld_g + c] = wr / S * (yu - (u ? y[r * ld_y + c] / q : 0.f));
            }
    }
}

inline int rows_grid(int64_t B) { return dr_grid_for(B, 4, 65535); }

template <int G>
void launch_spmm(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz, const float* X,
                 int64_t ld_x, int D, const float* relu_src, int64_t ld_rs, int accumulate, float* out, int64_t ld_out,
                 const int64_t* plan, float* ws, hipStream_t st) {
    constexpr int RW = 64 / G;
    const int64_t waves = (n_rows + RW - 1) / RW;
    hipLaunchKernelGGL(spmm_rows_kernel<G>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, row_ptr, col, val, n_rows, X, ld_x,
                       D, relu_src, ld_rs, accumulate, out, ld_out);
    if (plan_max_long(nnz) == 0) return;
    const int64_t ld_ws = 4 * (int64_t)((D + 3) >> 2);
    const int64_t cw = (plan_max_chunks(nnz) + RW - 1) / RW;
    hipLaunchKernelGGL(spmm_chunk_kernel<G>, dim3((unsigned)std::min<int64_t>((cw + 3) / 4, 4096)), dim3(256), 0, st, row_ptr, col, val,
                       plan, nnz, X, ld_x, D, ws, ld_ws);
    hipLaunchKernelGGL(spmm_combine_kernel, dim3((unsigned)std::min<int64_t>((plan_max_long(nnz) + 3) / 4, 4096)), dim3(256), 0, st, plan,
                       nnz, D, ws, ld_ws, relu_src, ld_rs, accumulate, out, ld_out);
}

}  // namespace

extern "C" int64_t dr_csr_plan_bytes(int64_t nnz) {
    if (nnz < 0) return 0;
    return (int64_t)sizeof(int64_t) * (2 + 2 * plan_max_long(nnz) + 1 + 2 * plan_max_chunks(nnz));
}

extern "C" int64_t dr_csr_plan_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0) return 0;
    return (int64_t)sizeof(int64_t) * (4 * n_rows + scan_blocks(n_rows) + 1);
}

extern "C" int dr_csr_plan(const int64_t* row_ptr, int64_t n_rows, int64_t nnz, int64_t* plan, int64_t plan_bytes, void* workspace,
                           int64_t workspace_bytes, dr_stream_t stream) {
    if (n_rows < 0 || nnz < 0 || !row_ptr || !plan || plan_bytes < dr_csr_plan_bytes(nnz)) return DR_EINVAL;
    hipStream_t st = dr_s(stream);
    if (n_rows == 0 || plan_max_long(nnz) == 0) {
        hipLaunchKernelGGL(plan_empty_kernel, dim3(1), dim3(64), 0, st, plan);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    if (!workspace || workspace_bytes < dr_csr_plan_workspace_bytes(n_rows)) return DR_EINVAL;
    int64_t* is_long = static_cast<int64_t*>(workspace);
    int64_t* n_ch = is_long + n_rows;
    int64_t* long_ix = n_ch + n_rows;
    int64_t* ch_ix = long_ix + n_rows;
    int64_t* tmp = ch_ix + n_rows;
    const int grid = dr_grid_for(n_rows, 256);
    hipLaunchKernelGGL(plan_count_kernel, dim3(grid), dim3(256), 0, st, row_ptr, n_rows, is_long, n_ch);
    excl_scan(is_long, n_rows, long_ix, tmp, st);
    excl_scan(n_ch, n_rows, ch_ix, tmp, st);
    hipLaunchKernelGGL(plan_fill_kernel, dim3(grid), dim3(256), 0, st, row_ptr, n_rows, nnz, is_long, n_ch, long_ix, ch_ix, plan);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_csr_spmm_workspace_bytes(int64_t nnz, int32_t D) {
    if (nnz < 0 || D < 1) return 0;
    return (int64_t)sizeof(float) * plan_max_chunks(nnz) * 4 * (int64_t)((D + 3) / 4) * (plan_max_long(nnz) > 0 ? 1 : 0);
}

extern "C" int dr_csr_spmm(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz, const float* X,
                           int64_t ld_x, int32_t D, const float* relu_src, int64_t ld_relu_src, int32_t accumulate, float* out,
                           int64_t ld_out, const int64_t* plan, float* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    if (n_rows < 0 || nnz < 0 || D < 1) return DR_EINVAL;
    if (n_rows == 0) return DR_OK;
    if (!row_ptr || !out || dr_bad_ld(ld_out, D) || !dr_aligned16(out)) return DR_EINVAL;
    if (nnz > 0 && (!col || !val || !X || dr_bad_ld(ld_x, D) || !dr_aligned16(X))) return DR_EINVAL;
    if (relu_src != nullptr && (dr_bad_ld(ld_relu_src, D) || !dr_aligned16(relu_src))) return DR_EINVAL;
    if (plan_max_long(nnz) > 0 && (!plan || !workspace || !dr_aligned16(workspace) || workspace_bytes < dr_csr_spmm_workspace_bytes(nnz, D)))
        return DR_EINVAL;
    const int D4 = (D + 3) / 4;
    hipStream_t st = dr_s(stream);
#define DR_SPMM_CASE(GG)                                                                                                           \
    launch_spmm<GG>(row_ptr, col, val, n_rows, nnz, X, ld_x, D, relu_src, ld_relu_src, accumulate, out, ld_out, plan, workspace, st)
    if (D4 <= 1) DR_SPMM_CASE(1);
    else if (D4 <= 2) DR_SPMM_CASE(2);
    else if (D4 <= 4) DR_SPMM_CASE(4);
    else if (D4 <= 8) DR_SPMM_CASE(8);
    else if (D4 <= 16) DR_SPMM_CASE(16);
    else if (D4 <= 32) DR_SPMM_CASE(32);
    else DR_SPMM_CASE(64);
#undef DR_SPMM_CASE
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_csr_transpose_workspace_bytes(int64_t nnz, int64_t n_cols) {
    if (nnz < 0 || n_cols < 0) return 0;
    const int64_t tiles = (nnz + RADIX_TILE - 1) / RADIX_TILE;
    const int64_t nh = 256 * tiles;
    // keys x2, rows x1, vals x1 (the other halves of the ping-pong are the outputs), histogram + its scan tmp
    return 4 * (4 * nnz) + 8 * (nh + scan_blocks(nh) + 1) + 64;
}

extern "C" int dr_csr_transpose(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows, int64_t n_cols,
                                int64_t nnz, int64_t* t_row_ptr, int32_t* t_col, float* t_val, void* workspace,
                                int64_t workspace_bytes, dr_stream_t stream) {
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || n_rows >= (1ll << 31) || n_cols >= (1ll << 31)) return DR_EINVAL;
    if (!t_row_ptr || (nnz > 0 && (!row_ptr || !col || !val || !t_col || !t_val || !workspace)) ||
        workspace_bytes < dr_csr_transpose_workspace_bytes(nnz, n_cols))
        return DR_EINVAL;
    hipStream_t st = dr_s(stream);
    if (nnz == 0) {
        (void)hipMemsetAsync(t_row_ptr, 0, sizeof(int64_t) * (n_cols + 1), st);
        DR_CHECK_LAUNCH();
        return DR_OK;
    }
    const int64_t tiles = (nnz + RADIX_TILE - 1) / RADIX_TILE;
    const int64_t nh = 256 * tiles;
    int64_t* hist = static_cast<int64_t*>(workspace);
    int64_t* tmp = hist + nh;
    int32_t* keys_a = reinterpret_cast<int32_t*>(tmp + scan_blocks(nh) + 1);
    int32_t* keys_b = keys_a + nnz;
    int32_t* rows_w = keys_b + nnz;
    float* vals_w = reinterpret_cast<float*>(rows_w + nnz);
    const int passes = radix_passes(n_cols);
    // the payload ping-pongs between (rows_w, vals_w) and the outputs (t_col, t_val) and must end in the outputs: with an even number
    // of passes the expanded source rows start in t_col
    int32_t* rows_init = (passes & 1) ? rows_w : t_col;
    hipLaunchKernelGGL(expand_rows_kernel, dim3(dr_grid_for(n_rows, 4)), dim3(256), 0, st, row_ptr, n_rows, rows_init);
    const int32_t* k_src = col;
    const int32_t* r_src = rows_init;
    const float* v_src = val;
    for (int p = 0; p < passes; ++p) {
        const bool to_out = ((passes - 1 - p) & 1) == 0;
        int32_t* k_dst = (p & 1) ? keys_b : keys_a;
        int32_t* r_dst = to_out ? t_col : rows_w;
        float* v_dst = to_out ? t_val : vals_w;
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)tiles), dim3(256), 0, st, k_src, nnz, 8 * p, tiles, hist);
        excl_scan(hist, nh, hist, tmp, st);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, st, k_src, r_src, v_src, nnz, 8 * p, tiles,
                           hist, k_dst, r_dst, v_dst);
        k_src = k_dst;
        r_src = r_dst;
        v_src = v_dst;
    }
    hipLaunchKernelGGL(lower_bound_kernel, dim3(dr_grid_for(n_cols + 1, 256)), dim3(256), 0, st, k_src, nnz, n_cols, t_row_ptr);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_softmax_rows_fwd(const float* x, int64_t ld_x, int64_t B, int32_t C, float* y, int64_t ld_y, dr_stream_t stream) {
    if (B < 0 || C < 1) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!x || !y || ld_x < C || ld_y < C) return DR_EINVAL;
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3(rows_grid(B)), dim3(256), 0, dr_s(stream), x, ld_x, B, C, y, ld_y);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_softmax_rows_bwd(const float* y, int64_t ld_y, const float* dy, int64_t ld_dy, int64_t B, int32_t C, float* dx,
                                   int64_t ld_dx, dr_stream_t stream) {
    if (B < 0 || C < 1) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!y || !dy || !dx || ld_y < C || ld_dy < C || ld_dx < C) return DR_EINVAL;
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(rows_grid(B)), dim3(256), 0, dr_s(stream), y, ld_y, dy, ld_dy, B, C, dx, ld_dx);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_cce_prob_rows(const float* p, int64_t ld_p, const float* labels, int64_t ld_labels, int64_t B, int32_t C,
                                const float* sample_weight, float* row_loss, float* grad, int64_t ld_grad, dr_stream_t stream) {
    if (B < 0 || C < 1) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!p || !labels || !row_loss || ld_p < C || ld_labels < C || (grad != nullptr && ld_grad < C)) return DR_EINVAL;
    hipLaunchKernelGGL(cce_prob_kernel, dim3(rows_grid(B)), dim3(256), 0, dr_s(stream), p, ld_p, labels, ld_labels, B, C,
                       sample_weight, row_loss, grad, ld_grad);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
