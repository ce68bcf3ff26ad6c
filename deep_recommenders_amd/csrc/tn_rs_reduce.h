// The fixed-order reduce of the TN register-split wgrad (bf3_wgrad.hip), as device code with two homes: the stand-alone
// bf3_tn_rs_reduce_kernel (bf3_wgrad.hip) and the rider blocks of K4's duplicate-pass launch (emb_sorted.hip), which apply the first
// layer's wgrad behind the fused dgrad + K4 without a launch of their own.  One text, so a column's bits do not depend on the home.
// Below it the second thing that rides there: the f16x2 plane refresh of the weight the reduce has just stepped (H2RefreshRide).
//
// Workspace of one product (dr_bf3_wgrad_workspace_bytes): partial [split][Fp][Np] | colsum [split][Np] | header [TN_RS_HDR_WORDS].
// The header is written by the f16x2 main kernel: word 0 = max(x_amax, x2_amax), word 1 = y_amax AS THAT KERNEL READ THEM.  The
// reduce divides by the scales of those words and never looks at the live records: a record raised between the two halves (K4 raises
// the table's) cannot put a power of two between what the partials carry and what the reduce divides out.
#pragma once
#include "rs_args.h"

namespace drrs {

constexpr int TN_RS_HDR_WORDS = 4;             // two words used; 16 bytes keep whatever follows 16-byte aligned
constexpr int TN_RS_RED_THREADS = 256;         // threads of a LOGICAL reduce block

// "Deferred dense apply": everything a later launch needs to apply a finished split-K product, dst += scale * sum_s partial[s].
struct TnRsApply {
    const float* partial; const float* colsum;   // colsum may be null (no bias)
    const uint32_t* hdr;                         // the saved amax words; null = the partials carry no scales (bf16x3 mode)
    int32_t split, F, N, Fp, Np;
    float scale;
    float* dst; int64_t ld; float* dstb;
    int32_t vec;                                 // 16-byte accesses allowed (pointers and ld aligned)
};

__host__ __device__ inline int tn_rs_reduce_blocks(int F, int N, int vec) {
    const int w = vec ? (N + 3) / 4 : N;         // threads per row
    return (int)(((int64_t)F * w + TN_RS_RED_THREADS - 1) / TN_RS_RED_THREADS);
}

// Logical block `lb` of tn_rs_reduce_blocks(F, N, V == 4), thread `tid` < 256: V consecutive columns of one row f.  The additions of an
// element run in slice order, one after the other from 0.f, eight slices' loads in flight, and fmaf(wscale, sum, dst) comes last: any
// unrolling or block shape gives the same bits.  The threads of row 0 also apply the column sums, each column in slice order.
// Returns max |value this thread stored into dst| as float bits (0 for a thread past the last row; the bias is not part of it): the
// riders' share of the weight's amax record.  A caller that ignores it compiles to the same code as before.
template <int V>
__device__ __forceinline__ uint32_t tn_rs_reduce_block(const TnRsApply& a, int lb, int tid) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int w = (a.N + V - 1) / V;
    const int64_t t = (int64_t)lb * TN_RS_RED_THREADS + tid;
    const int f = (int)(t / w);
    const int n = (int)(t - (int64_t)f * w) * V;                        // < Np: the padded workspace holds all V columns
    if (f >= a.F) return 0u;
    const int split = a.split, N = a.N, Np = a.Np;
    const int64_t ps = (int64_t)a.Fp * Np;
    float wscale = a.scale;                                             // f16x2 partials carry s_x s_y (powers of two: exact)
    if (a.hdr != nullptr) {
        float sx, ix, sy, iy;
        h2_scale_of(a.hdr[0], sx, ix);
        h2_scale_of(a.hdr[1], sy, iy);
        wscale = a.scale * (ix * iy);
    }
    auto sum_slices = [&](const float* p, int64_t stride) -> vec_t {   // sum_s p[s * stride], V columns each, in slice order
        vec_t acc = 0.f;
        int s = 0;
        for (; s + 8 <= split; s += 8) {
            vec_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const vec_t*>(p + (s + u) * stride);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; s < split; ++s) acc += *reinterpret_cast<const vec_t*>(p + s * stride);
        return acc;
    };
    const vec_t acc = sum_slices(a.partial + (int64_t)f * Np + n, ps);
    float* d = a.dst + (int64_t)f * a.ld + n;
    uint32_t wmax = 0u;
    if (V == 1 || n + V <= N) {
        vec_t o = *reinterpret_cast<vec_t*>(d);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            o[c] = fmaf(wscale, acc[c], o[c]);
            wmax = max(wmax, __float_as_uint(fabsf(o[c])));
        }
        *reinterpret_cast<vec_t*>(d) = o;
    } else {                                                            // the row's last, partial group of columns
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (n + c < N) {
                d[c] = fmaf(wscale, acc[c], d[c]);
                wmax = max(wmax, __float_as_uint(fabsf(d[c])));
            }
    }
    if (f == 0 && a.colsum != nullptr && a.dstb != nullptr) {
        const vec_t cacc = sum_slices(a.colsum + n, Np);
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (n + c < N) a.dstb[n + c] = fmaf(a.scale, cacc[c], a.dstb[n + c]);
    }
    return wmax;
}

// Rider form: block `rider` of `nriders` walks the logical blocks rider, rider + nriders, ...  Returns the thread's maximum over them.
__device__ __forceinline__ uint32_t tn_rs_reduce_ride(const TnRsApply& a, int rider, int nriders, int tid) {
    const int nlb = tn_rs_reduce_blocks(a.F, a.N, a.vec);
    uint32_t wmax = 0u;
    for (int lb = rider; lb < nlb; lb += nriders)
        wmax = max(wmax, a.vec ? tn_rs_reduce_block<4>(a, lb, tid) : tn_rs_reduce_block<1>(a, lb, tid));
    return wmax;
}

// max over the 256 threads of a block, in every thread (wm: 4 words of LDS; ends with the values read, not with a barrier)
__device__ __forceinline__ uint32_t block_max_256(uint32_t m, uint32_t* wm, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((tid & 63) == 0) wm[tid >> 6] = m;
    __syncthreads();
    return max(max(wm[0], wm[1]), max(wm[2], wm[3]));
}

// "Deferred plane refresh": the f16x2 plane images of a weight src [R, C] (row stride ld) and of its transpose, scaled by the maximum of
// the first `nparts` words of `parts` -- per-block maxima of |src| left by an EARLIER launch on the stream (h2_amax_parts_kernel, or the
// riders above, one word each).  Two homes, one text: h2_split_both_kernel (bf3_planes.hip) and the rider blocks behind K4's hot-row
// launch (emb_sorted.hip).  Every block reduces the parts itself; block 0 stores the record.  src == nullptr: nothing deferred.
struct H2RefreshRide {
    const float* src; int64_t ld; int64_t R; int32_t C;
    _Float16* w; int64_t w_ps, w_ld;             // planes [2][R][w_ld]
    _Float16* wt; int64_t wt_ps, wt_ld;          // planes of the transpose [2][C][wt_ld]
    const uint32_t* parts; int32_t nparts;       // nparts <= H2_REFRESH_MAX_PARTS
    uint32_t* amax;                              // the record the GEMMs read
};
constexpr int H2_REFRESH_MAX_PARTS = 1024;

// Block `blk` of `nblk`, 256 threads: elementwise, so any nblk gives the same planes.
__device__ __forceinline__ void h2_split_both_block(const H2RefreshRide& r, int blk, int nblk, int tid) {
    uint32_t m = 0u;
    for (int p = tid; p < r.nparts; p += 256) m = max(m, r.parts[p]);
    __shared__ uint32_t wm[4];
    m = block_max_256(m, wm, tid);
    if (blk == 0 && tid == 0) r.amax[0] = m;                            // the record the GEMMs read (they run behind this launch)
    float sc, inv;
    h2_scale_of(m, sc, inv);
    h2_mode_on();
    const int64_t R = r.R;
    const int32_t C = r.C;
    const int64_t total = R * (int64_t)C, stride = (int64_t)nblk * 256;
    for (int64_t i = (int64_t)blk * 256 + tid; i < 2 * total; i += stride) {
        // consecutive threads: consecutive DESTINATION elements, first of the plain image, then of the transposed one
        int64_t rr, c, off;
        _Float16* dst;
        int64_t ps;
        if (i < total) { rr = i / C; c = i - rr * C; off = rr * r.w_ld + c; dst = r.w; ps = r.w_ps; }
        else { const int64_t j = i - total; c = j / R; rr = j - c * R; off = c * r.wt_ld + rr; dst = r.wt; ps = r.wt_ps; }
        const float v = r.src[rr * r.ld + c] * sc;
        const _Float16 h = (_Float16)v;
        dst[off] = h;
        dst[ps + off] = (_Float16)(v - (float)h);
    }
}

// Splits a workspace (checked by the caller against dr_bf3_wgrad_workspace_bytes) into the descriptor's three regions.
inline TnRsApply tn_rs_apply_of(void* workspace, int split, int32_t F, int32_t N, int Fp, int Np, bool h2, float scale, float* dst,
                                int64_t ld, float* dstb) {
    float* partial = static_cast<float*>(workspace);
    float* colsum = partial + (int64_t)split * Fp * Np;
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(colsum + (int64_t)split * Np);
    const bool vec = ((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && (ld & 3) == 0;
    return TnRsApply{partial, dstb != nullptr ? colsum : nullptr, h2 ? hdr : nullptr, split, F, N, Fp, Np, scale, dst, ld, dstb, vec ? 1 : 0};
}

// bf3_wgrad.hip: the plan of a product's workspace, for a later launch that applies it (emb_sorted.hip's riders)
void tn_rs_plan(int64_t R, int32_t F, int32_t N, int& split, int64_t& per, int& Fp, int& Np);

}  // namespace drrs
