// The scatter of per-position gradient rows back into an embedding table with one owner block per table row, shared by
// dr_token_embedding_bwd and dr_bert_embed_bwd.  One block per position p of the id-sorted order; only the block at the first position
// of a run of equal ids works.  It owns the run's table row: lane (rl, col) sums the run's positions p0 + rl, p0 + rl + RL, ... (the
// stable sort keeps them ascending), the RL partial sums are added in rl order, and d_table[id] += scale * sum -- a fixed order, no
// atomics.
#pragma once
#include "dr_common.h"

// Call from every thread of a 256-thread block.  CW (a power of two, 8 <= CW <= 64) columns at a time, RL = 256 / CW positions
// side by side.  term(n, c, acc) adds the contribution of position n to column c into acc (or leaves acc alone).
template <typename Term>
__device__ __forceinline__ void dr_owner_row_scatter(const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ order, int64_t N,
                                                     int64_t V, int32_t D, int32_t CW, float scale, float* __restrict__ d_table, Term term) {
    __shared__ float part[256];
    const int64_t p0 = blockIdx.x;
    const int64_t id = sorted_ids[p0];
    if ((p0 > 0 && sorted_ids[p0 - 1] == id) || id < 0 || id >= V) return;
    int64_t lo = p0, hi = N;             // first position whose id is larger
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted_ids[mid] <= id) lo = mid + 1; else hi = mid;
    }
    const int64_t p1 = lo;
    const int RL = 256 / CW, col = threadIdx.x % CW, rl = threadIdx.x / CW;
    for (int c0 = 0; c0 < D; c0 += CW) {
        const int c = c0 + col;
        float acc = 0.f;
        if (c < D)
            for (int64_t q = p0 + rl; q < p1; q += RL) term(order[q], c, acc);
        __syncthreads();
        part[threadIdx.x] = acc;
        __syncthreads();
        if (rl == 0 && c < D) {
            float sum = 0.f;
            for (int k = 0; k < RL; ++k) sum += part[k * CW + col];
            d_table[id * D + c] = fmaf(scale, sum, d_table[id * D + c]);
        }
    }
}

// the column width the launchers hand to dr_owner_row_scatter
static inline int dr_owner_row_cw(int32_t D) {
    int CW = 8;
    while (CW < 64 && CW < D) CW <<= 1;
    return CW;
}
