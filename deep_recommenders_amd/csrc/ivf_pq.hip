// IVF-PQ (inverted file + product quantisation, inner product, residual encoding) -- the index EBR serves its embeddings from
// (Huang et al., KDD 2020, section 4; Jegou et al., "Product quantization for nearest neighbor search", TPAMI 2011).  The coarse
// quantiser, the list build and the packing are IVF-Flat's (ivf.hip); this file adds what the codes need:
//   dr_pq_encode    nearest codeword (squared L2, direct form, ascending d, ties to the lower code) of every residual sub-vector
//   dr_ivfpq_scan   asymmetric distance computation: score = probe_score + sum_j LUT[j][code_j], LUT[j][c] = q_j . cb_j[c]
//   dr_rerank_topk  exact fp32 inner products of a query with the rows a scan named, top k
// ksub = 256 codewords per sub-quantiser (one byte), m sub-quantisers, dsub = D / m.
//
// Layout of the codes: a vector's m bytes are m / 4 words (code j in bits 8 * (j % 4) of word j / 4); a list is stored the way
// IVF-Flat stores its floats -- blocks of 64 vectors, one lane per vector, word-plane-major: packed_codes[(blk * (m/4) + w) * 64 + lane]
// -- so dr_ivf_pack builds it from the codes viewed as [N, m/4] dwords and a wave reads 256 contiguous bytes per load.
//
// The scan runs ONE BLOCK (4 waves) PER QUERY: the m KB lookup table is built once in LDS from q and the codebooks and shared by the
// four waves, which take the 64-vector blocks of the probed lists round-robin, each into its own drtk::List; waves 1..3 then hand
// their lists to wave 0 through LDS, which folds them in in wave order.  The list's order is total (score descending, then the lower
// row), so the result does not depend on which wave saw a vector; a score depends on nothing but the query, the probe's coarse score
// and the vector's codes, so it does not depend on the batch either.
#include "dr_common.h"
#include "topk_list.h"
#include <math.h>

namespace {

constexpr int PQ_KSUB = 256;
#ifndef PQ_SCAN_WAVES
#define PQ_SCAN_WAVES 4              // waves that share one query's lookup table (1 .. 4)
#endif

static inline bool pq_domain(int32_t D, int32_t m) {
    return m >= 4 && m <= 64 && (m & 3) == 0 && D >= m && D <= 1024 && D % m == 0 && D / m <= 64;
}

// One block = 256 vectors x ONE subspace j (blockIdx.y); the subspace's codebook slice [256][dsub] sits in LDS and every codeword is
// a broadcast read; a lane owns a vector and keeps its residual sub-vector in registers (DS = the register array's size >= dsub).
// The arithmetic is written so that a NumPy fp32 restatement is unambiguous: r = x - c (one rounding), then dist += (r - cb)^2 as a
// rounded subtract, a rounded multiply and a rounded add per dimension -- no fused multiply-add (contraction is off in this kernel).
template <int DS>
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* __restrict__ x, const int64_t* __restrict__ assign,
                                                        const float* __restrict__ centroids, int32_t nlist,
                                                        const float* __restrict__ codebooks, int64_t N, int32_t D, int32_t m,
                                                        uint8_t* __restrict__ codes) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float pq_cb[];          // [256][dsub]
    const int dsub = D / m, j = blockIdx.y;
    const float* src = codebooks + (int64_t)j * PQ_KSUB * dsub;
    for (int t = threadIdx.x; t < PQ_KSUB * dsub; t += 256) pq_cb[t] = src[t];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        bool ok = true;
        const float* cen = nullptr;
        if (assign != nullptr) {
            const int64_t a = assign[i];
            ok = a >= 0 && a < nlist;
            if (ok) cen = centroids + a * D + j * dsub;
        }
        const float* xr = x + i * D + j * dsub;
        float r[DS];
#pragma unroll
        for (int d = 0; d < DS; ++d) {
            r[d] = 0.f;
            if (d < dsub && ok) r[d] = cen != nullptr ? xr[d] - cen[d] : xr[d];
        }
        int best = 0;
        if (ok) {
            float bd = INFINITY;
            for (int c = 0; c < PQ_KSUB; ++c) {
                const float* cw = pq_cb + c * dsub;
                float dist = 0.f;
#pragma unroll
                for (int d = 0; d < DS; ++d) {
                    if (d < dsub) {
                        const float diff = r[d] - cw[d];
                        dist = dist + diff * diff;
                    }
                }
                if (dist < bd) { bd = dist; best = c; }              // strict: a tie keeps the lower code
            }
        }
        codes[i * m + j] = (uint8_t)best;                           // byte j of the row == bits 8 * (j % 4) of word j / 4
    }
}

__global__ __launch_bounds__(256) void ivfpq_scan_kernel(const float* __restrict__ q, const int64_t* __restrict__ probes,
                                                         const float* __restrict__ probe_scores,
                                                         const int64_t* __restrict__ blk_off,
                                                         const uint32_t* __restrict__ packed_codes,
                                                         const int64_t* __restrict__ packed_rows,
                                                         const float* __restrict__ codebooks, int32_t D, int32_t m, int32_t nprobe,
                                                         int32_t k, float* __restrict__ out_s, int64_t* __restrict__ out_i) {
    // dynamic LDS: lut [m][256] | q [D]; after the scan the first (waves - 1) * 128 * 12 bytes are reused for the merge
    extern __shared__ __attribute__((aligned(16))) float pq_lds[];
    float* lut = pq_lds;
    float* qs = pq_lds + m * PQ_KSUB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t b = blockIdx.x;
    const int dsub = D / m, mw = m >> 2;
    for (int d = threadIdx.x; d < D; d += blockDim.x) qs[d] = q[b * D + d];
    __syncthreads();
    for (int c = threadIdx.x; c < PQ_KSUB; c += blockDim.x) {       // a thread owns codeword c of every subspace
        for (int j = 0; j < m; ++j) {
            const float* cw = codebooks + ((int64_t)j * PQ_KSUB + c) * dsub;
            const float* qj = qs + j * dsub;
            float a = 0.f;
            for (int d = 0; d < dsub; ++d) a = fmaf(qj[d], cw[d], a);
            lut[j * PQ_KSUB + c] = a;
        }
    }
    __syncthreads();
    drtk::List L;
    L.init(k, lane);
    for (int p = 0; p < nprobe; ++p) {
        const int64_t l = probes[b * nprobe + p];
        if (l < 0) continue;
        const float base = probe_scores[b * nprobe + p];
        const int64_t b0 = blk_off[l], b1 = blk_off[l + 1];
        for (int64_t blk = b0 + wave; blk < b1; blk += nw) {
            const uint32_t* cp = packed_codes + blk * (int64_t)mw * 64 + lane;
            float acc = base;
#pragma unroll 4
            for (int w = 0; w < mw; ++w) {
                const uint32_t word = cp[(int64_t)w * 64];
                const float* t = lut + w * 4 * PQ_KSUB;
                acc += t[word & 255u];
                acc += t[PQ_KSUB + ((word >> 8) & 255u)];
                acc += t[2 * PQ_KSUB + ((word >> 16) & 255u)];
                acc += t[3 * PQ_KSUB + (word >> 24)];
            }
            const int64_t id = packed_rows[blk * 64 + lane];
            L.offer(acc, id, id >= 0);
        }
    }
    if (nw > 1) {
        __syncthreads();                                            // every wave is done with the lookup table
        int64_t* mi = reinterpret_cast<int64_t*>(pq_lds);           // [nw - 1][k]
        float* ms = pq_lds + 3 * drtk::KMAX * 2;                    // [nw - 1][k], behind the largest mi
        if (wave > 0) L.store(ms + (wave - 1) * k, mi + (wave - 1) * k);
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < nw - 1; ++w) {
                for (int base = 0; base < k; base += 64) {
                    const int t = base + lane;
                    const bool in = t < k;
                    const float s = in ? ms[w * k + t] : -INFINITY;
                    const int64_t id = in ? mi[w * k + t] : -1;
                    L.offer(s, id, in && id >= 0);
                }
            }
        }
    }
    if (wave == 0) L.store(out_s + b * k, out_i + b * k);
}

__device__ __forceinline__ int64_t pq_uniform_i64(int64_t v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

// One wave per query.  Each named row is read by the whole wave (coalesced); a score is the lanes' fmaf chains over d = lane,
// lane + 64, ... summed by the xor butterfly 32, 16, ..., 1 -- a fixed order, the same on every lane.  Entry t is then held by lane
// t % 64 (slot t / 64) and the two slots are offered to the list.
__global__ __launch_bounds__(256) void rerank_topk_kernel(const float* __restrict__ q, const float* __restrict__ cand,
                                                          const int64_t* __restrict__ rows, int64_t Bq, int64_t N, int32_t D,
                                                          int32_t kin, int32_t k, float* __restrict__ out_s,
                                                          int64_t* __restrict__ out_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    const int64_t rowc = row < Bq ? row : Bq - 1;                   // surplus waves mirror the last query (no stores)
    const float* qr = q + rowc * D;
    const int64_t* rr = rows + rowc * kin;
    float s0 = -INFINITY, s1 = -INFINITY;
    int64_t r0 = -1, r1 = -1;
    for (int t = 0; t < kin; ++t) {
        const int64_t r = pq_uniform_i64(rr[t]);
        if (r < 0 || r >= N) continue;
        const float* cr = cand + r * D;
        float a = 0.f;
        for (int d = lane; d < D; d += 64) a = fmaf(qr[d], cr[d], a);
        a = dr_wave_sum(a);
        if ((t & 63) == lane) {
            if (t < 64) { s0 = a; r0 = r; } else { s1 = a; r1 = r; }
        }
    }
    drtk::List L;
    L.init(k, lane);
    L.offer(s0, r0, r0 >= 0);
    L.offer(s1, r1, r1 >= 0);
    if (row < Bq) L.store(out_s + row * k, out_i + row * k);
}

}  // namespace

extern "C" int dr_pq_encode(const float* x, const int64_t* assign, const float* centroids, int32_t nlist, const float* codebooks,
                            int64_t N, int32_t D, int32_t m, uint32_t* codes_out, dr_stream_t stream) {
    if (N < 0 || !pq_domain(D, m)) return DR_EINVAL;
    if ((assign == nullptr) != (centroids == nullptr) || (assign != nullptr && nlist <= 0)) return DR_EINVAL;
    if (N == 0) return DR_OK;
    if (!x || !codebooks || !codes_out) return DR_EINVAL;
    const int dsub = D / m;
    const int per_subspace = 4096 / m;                               // ~4096 blocks in all
    const dim3 grid(dr_grid_for(N, 256, per_subspace), m);
    const size_t lds = (size_t)PQ_KSUB * dsub * sizeof(float);      // <= 64 KiB
    uint8_t* codes = reinterpret_cast<uint8_t*>(codes_out);
#define CALL(DS) dr_launch(pq_encode_kernel<DS>, grid, dim3(256), lds, dr_s(stream), x, assign, centroids, nlist, codebooks, N, D, m, codes)
    if (dsub <= 4) return CALL(4);
    if (dsub <= 16) return CALL(16);
    return CALL(64);
#undef CALL
}

extern "C" int dr_ivfpq_scan(const float* q, const int64_t* probes, const float* probe_scores, const int64_t* blk_off,
                             const uint32_t* packed_codes, const int64_t* packed_rows, const float* codebooks, int64_t Bq,
                             int32_t D, int32_t m, int32_t nprobe, int32_t k, float* out_scores, int64_t* out_rows,
                             dr_stream_t stream) {
    if (Bq < 0 || Bq > 0x7fffffff || !pq_domain(D, m) || nprobe <= 0 || k <= 0 || k > drtk::KMAX) return DR_EINVAL;
    if (Bq == 0) return DR_OK;
    if (!q || !probes || !probe_scores || !blk_off || !packed_codes || !packed_rows || !codebooks || !out_scores || !out_rows)
        return DR_EINVAL;
    size_t lds = ((size_t)m * PQ_KSUB + D) * sizeof(float);
    const size_t merge = (size_t)3 * drtk::KMAX * (sizeof(int64_t) + sizeof(float));
    if (lds < merge) lds = merge;
    return dr_launch(ivfpq_scan_kernel, dim3((unsigned)Bq), dim3(64 * PQ_SCAN_WAVES), lds, dr_s(stream), q, probes, probe_scores, blk_off,
                     packed_codes, packed_rows, codebooks, D, m, nprobe, k, out_scores, out_rows);
}

extern "C" int dr_rerank_topk(const float* q, const float* cand, const int64_t* rows, int64_t Bq, int64_t N, int32_t D, int32_t kin,
                              int32_t k, float* out_scores, int64_t* out_rows, dr_stream_t stream) {
    if (Bq < 0 || N < 0 || D <= 0 || D > 1024 || kin <= 0 || kin > drtk::KMAX || k <= 0 || k > drtk::KMAX) return DR_EINVAL;
    if (Bq == 0) return DR_OK;
    if (!q || !rows || !out_scores || !out_rows || (N > 0 && !cand)) return DR_EINVAL;
    const int64_t grid = (Bq + 3) / 4;
    if (grid > 0x7fffffff) return DR_EINVAL;
    hipLaunchKernelGGL(rerank_topk_kernel, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), q, cand, rows, Bq, N, D, kin, k,
                       out_scores, out_rows);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
