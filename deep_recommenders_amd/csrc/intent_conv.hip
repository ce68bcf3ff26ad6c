// IntentGC's vector-wise convolution (Zhao et al., KDD 2019, IntentNet) over R neighbour types and L local filters
// (include/dr_hotpath.h, "IntentGC"):
//   a_0 = h_v,  a_r = sum_k val[k] h[col[k]] over virtual row v R + r - 1 of the typed block's CSR   (r = 1 .. R; the row's mean)
//   p_i = sum_{r = 0 .. R} W[i, r] a_r,  g_i = relu(p_i),  s = sum_{i < L} theta_i g_i,  out_v = act(s)
// W [L, R + 1] and theta [L] are SCALARS per (filter, type): there is no matrix product, the layer is memory traffic.
//
// A GROUP OF G = pow2ceil(D / 4) LANES OWNS ONE DESTINATION, lane s its columns 4 s .. 4 s + 3.  The forward keeps a_0 .. a_R in
// registers (a_r from gather_seg, the row gather of dr_csr_spmm: ascending k, any row length, no split), applies the filters there
// and writes out[v] once; `agg` [n_dst, R, D] is stored only when the backward will want it.  dr_intent_mix_fwd is the same device
// body with a_r read from memory.  No LDS and no atomics in the forward.
// EVERY SUM IS AN EXPLICIT fmaf CHAIN FROM +0 IN A FIXED ORDER: p_i over ascending r, s over ascending i, the backward's d_a_r over
// ascending i.  Nothing is left for the compiler to contract one way in one kernel and another way in the next, so the gathered and the
// pre-aggregated form give the same bits from the same a_r, and a destination's bits depend neither on its block nor on its place.
// The backward recomputes p_i (and s, unless the forward's out is given) from the saved a_r, writes d_a_0 / d_a_r and per-block partials
// of dW / dtheta: each lane accumulates over its destinations in ascending order, a wave adds its lanes by the xor butterfly, the block
// its four waves in order, and dr_sum_partials adds the blocks in order.  The grid is a function of (n_dst, D) alone.
#include "dr_common.h"
#include "dr_csr_gather.h"
#include "dr_sum_partials.h"

namespace {

constexpr int IC_MAX_R = 7;
constexpr int IC_MAX_L = 16;
constexpr int IC_MAX_D = 256;
constexpr int IC_MAX_PARTS = 512;     // blocks of the backward (= partials of dW / dtheta) at most, while a block has <= 16 passes ...
                                      // ... beyond that the passes per block grow instead

struct IcF {                          // the filter bank; wave-uniform, read through scalar loads
    const float* __restrict__ W;      // [L, R + 1]
    const float* __restrict__ theta;  // [L]
    int R, L, act;
};

// relu that lets a NaN through (a stray read must show in the output)
__device__ __forceinline__ float ic_relu(float x) { return x < 0.f ? 0.f : x; }
__device__ __forceinline__ float4 ic_relu4(float4 v) { return make_float4(ic_relu(v.x), ic_relu(v.y), ic_relu(v.z), ic_relu(v.w)); }

// p_i = ((0 + W[i,0] a_0) + W[i,1] a_1) + ... ; a[] is indexed by constants only (the loop is unrolled under a uniform predicate)
template <int RMAX>
__device__ __forceinline__ float4 ic_filter(const IcF& f, int i, const float4 (&a)[RMAX + 1]) {
    const float* __restrict__ Wi = f.W + i * (f.R + 1);
    float4 p = dr_zero4();
#pragma unroll
    for (int r = 0; r <= RMAX; ++r)
        if (r <= f.R) fma4(Wi[r], a[r], p);
    return p;
}

// s = ((0 + theta_0 g_0) + theta_1 g_1) + ...  before the outer activation
template <int RMAX>
__device__ __forceinline__ float4 ic_mix(const IcF& f, const float4 (&a)[RMAX + 1]) {
    float4 s = dr_zero4();
    for (int i = 0; i < f.L; ++i) fma4(f.theta[i], ic_relu4(ic_filter<RMAX>(f, i, a)), s);
    return s;
}

template <int RMAX>
__device__ __forceinline__ float4 ic_out(const IcF& f, const float4 (&a)[RMAX + 1]) {
    const float4 s = ic_mix<RMAX>(f, a);
    return f.act == 1 ? ic_relu4(s) : s;
}

__device__ __forceinline__ float4 ic_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void ic_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// One group of G lanes per destination, 64 / G destinations per wave.  Every lane of a wave runs every gather (its loop runs to the
// wave's longest row); lanes past n_dst or past column D gather an empty segment and store nothing.
template <int G>
__global__ __launch_bounds__(256) void intent_conv_fwd_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, int64_t n_dst,
                                                              const float* __restrict__ h, int64_t ld_h, int D, const IcF f,
                                                              float* __restrict__ out, int64_t ld_out, float* __restrict__ agg) {
    constexpr int RW = 64 / G;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t v = wave * RW + lane / G;
    const int s = lane & (G - 1);
    const bool live = v < n_dst;
    const bool mine = live && 4 * s < D;
    float4 a[IC_MAX_R + 1];
    a[0] = mine ? ic_ld4(h + v * ld_h + 4 * s) : dr_zero4();
#pragma unroll
    for (int r = 1; r <= IC_MAX_R; ++r) {
        a[r] = dr_zero4();
        if (r <= f.R) {                                        // uniform: the whole wave gathers or none of it
            int64_t kb = 0, ke = 0;
            if (live) {
                kb = row_ptr[v * f.R + (r - 1)];
                ke = row_ptr[v * f.R + r];
            }
            a[r] = gather_seg<G>(col, val, kb, ke, h, ld_h, s, D);
        }
    }
    if (!mine) return;                                         // after the last shuffle
    if (agg != nullptr) {
        float* dst = agg + (v * f.R) * D + 4 * s;
#pragma unroll
        for (int r = 1; r <= IC_MAX_R; ++r)
            if (r <= f.R) ic_st4(dst + (int64_t)(r - 1) * D, a[r]);
    }
    ic_st4(out + v * ld_out + 4 * s, ic_out<IC_MAX_R>(f, a));
}

// a_r from memory; g = the group size of the gathered form (a power of two), so a destination has the same lanes here as there
__global__ __launch_bounds__(256) void intent_mix_fwd_kernel(const float* __restrict__ h_self, int64_t ld_h,
                                                             const float* __restrict__ agg, int64_t n_dst, int D, const IcF f,
                                                             float* __restrict__ out, int64_t ld_out, int g) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t v = wave * (64 / g) + lane / g;
    const int s = lane & (g - 1);
    if (v >= n_dst || 4 * s >= D) return;
    float4 a[IC_MAX_R + 1];
    a[0] = ic_ld4(h_self + v * ld_h + 4 * s);
    const float* src = agg + (v * f.R) * D + 4 * s;
#pragma unroll
    for (int r = 1; r <= IC_MAX_R; ++r) {
        a[r] = dr_zero4();
        if (r <= f.R) a[r] = ic_ld4(src + (int64_t)(r - 1) * D);
    }
    ic_st4(out + v * ld_out + 4 * s, ic_out<IC_MAX_R>(f, a));
}

// ((x.x y.x + x.y y.y) + x.z y.z) + x.w y.w as one fmaf chain
__device__ __forceinline__ float ic_dot4(float4 x, float4 y) {
    float t = x.x * y.x;
    t = fmaf(x.y, y.y, t);
    t = fmaf(x.z, y.z, t);
    return fmaf(x.w, y.w, t);
}

struct IcB {
    const float* __restrict__ h_self; int64_t ld_h;
    const float* __restrict__ agg;
    const float* __restrict__ d_out; int64_t ld_do;
    const float* __restrict__ out; int64_t ld_out;        // NULL: s is recomputed
    float* __restrict__ d_self; int64_t ld_ds;
    float* __restrict__ d_agg;
    float* __restrict__ partials;                         // [gridDim.x, L (R + 2)]: dW [L, R + 1] then dtheta [L]
    int64_t n_dst;
    int D, g, iters;                                      // g: lanes per destination; iters: passes of 256 / g destinations per block
};

// LMAX x (RMAX + 2) accumulators per lane, indexed by constants only: columns 0 .. RMAX are dW[i, r], column RMAX + 1 is dtheta_i.
// Block b owns destinations [b iters dpp, (b + 1) iters dpp), dpp = 256 / g, in ascending order.
template <int LMAX, int RMAX>
__global__ __launch_bounds__(256) void intent_conv_bwd_kernel(const IcB b, const IcF f) {
    constexpr int NA = RMAX + 2;
    __shared__ float red[4][LMAX * NA];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int dpp = 256 / b.g;
    const int s = threadIdx.x & (b.g - 1);
    const bool col_ok = 4 * s < b.D;
    float acc[LMAX][NA];
#pragma unroll
    for (int i = 0; i < LMAX; ++i)
#pragma unroll
        for (int r = 0; r < NA; ++r) acc[i][r] = 0.f;
    const int64_t v0 = (int64_t)blockIdx.x * b.iters * dpp + threadIdx.x / b.g;
    for (int it = 0; it < b.iters; ++it) {
        const int64_t v = v0 + (int64_t)it * dpp;
        if (v >= b.n_dst || !col_ok) continue;
        float4 a[RMAX + 1], da[RMAX + 1];
        a[0] = ic_ld4(b.h_self + v * b.ld_h + 4 * s);
        da[0] = dr_zero4();
        const float* src = b.agg + (v * f.R) * b.D + 4 * s;
#pragma unroll
        for (int r = 1; r <= RMAX; ++r) {
            a[r] = dr_zero4();
            da[r] = dr_zero4();
            if (r <= f.R) a[r] = ic_ld4(src + (int64_t)(r - 1) * b.D);
        }
        float4 ds = ic_ld4(b.d_out + v * b.ld_do + 4 * s);
        if (f.act == 1) {                                  // relu': where the forward's s was > 0
            const float4 o = b.out != nullptr ? ic_ld4(b.out + v * b.ld_out + 4 * s) : ic_mix<RMAX>(f, a);
            ds.x = o.x > 0.f ? ds.x : 0.f;
            ds.y = o.y > 0.f ? ds.y : 0.f;
            ds.z = o.z > 0.f ? ds.z : 0.f;
            ds.w = o.w > 0.f ? ds.w : 0.f;
        }
#pragma unroll
        for (int i = 0; i < LMAX; ++i) {
            if (i < f.L) {
                const float4 p = ic_filter<RMAX>(f, i, a);
                acc[i][RMAX + 1] += ic_dot4(ds, ic_relu4(p));
                const float th = f.theta[i];
                float4 dp;
                dp.x = p.x > 0.f ? th * ds.x : 0.f;
                dp.y = p.y > 0.f ? th * ds.y : 0.f;
                dp.z = p.z > 0.f ? th * ds.z : 0.f;
                dp.w = p.w > 0.f ? th * ds.w : 0.f;
                const float* __restrict__ Wi = f.W + i * (f.R + 1);
#pragma unroll
                for (int r = 0; r <= RMAX; ++r) {
                    if (r <= f.R) {
                        acc[i][r] += ic_dot4(dp, a[r]);
                        fma4(Wi[r], dp, da[r]);
                    }
                }
            }
        }
        ic_st4(b.d_self + v * b.ld_ds + 4 * s, da[0]);
        float* dst = b.d_agg + (v * f.R) * b.D + 4 * s;
#pragma unroll
        for (int r = 1; r <= RMAX; ++r)
            if (r <= f.R) ic_st4(dst + (int64_t)(r - 1) * b.D, da[r]);
    }
    // the block's partial: lanes by the butterfly, then the four waves in order
#pragma unroll
    for (int i = 0; i < LMAX; ++i) {
        if (i < f.L) {
#pragma unroll
            for (int r = 0; r < NA; ++r) {
                if (r <= f.R || r == RMAX + 1) {
                    const float t = dr_wave_sum(acc[i][r]);
                    if (lane == 0) red[w][i * NA + r] = t;
                }
            }
        }
    }
    __syncthreads();
    const int n0 = f.L * (f.R + 1), total = n0 + f.L;
    for (int t = threadIdx.x; t < total; t += 256) {
        const int k = t < n0 ? (t / (f.R + 1)) * NA + t % (f.R + 1) : (t - n0) * NA + RMAX + 1;
        b.partials[(int64_t)blockIdx.x * total + t] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

int ic_domain(int64_t n_dst, int32_t R, int32_t D, int32_t L, int32_t act) {
    if (n_dst < 0 || (act != 0 && act != 1)) return DR_EINVAL;
    if (D < 4 || D > IC_MAX_D || (D & 3) || R < 1 || R > IC_MAX_R || L < 1 || L > IC_MAX_L) return DR_ESHAPE;
    return DR_OK;
}

// (passes per block, blocks) of the backward: a function of (n_dst, D) alone
void ic_bwd_grid(int64_t n_dst, int32_t D, int64_t& iters, int64_t& blocks) {
    const int g = dr_pow2_ceil(D / 4);
    const int64_t dpp = 256 / g, passes = (n_dst + dpp - 1) / dpp;
    iters = (passes + IC_MAX_PARTS - 1) / IC_MAX_PARTS;
    if (iters < 1) iters = 1;
    blocks = (passes + iters - 1) / iters;
}

template <int LMAX, int RMAX>
int ic_bwd_launch(const IcB& b, const IcF& f, int64_t blocks, hipStream_t st) {
    return dr_launch(intent_conv_bwd_kernel<LMAX, RMAX>, dim3((unsigned)blocks), dim3(256), 0, st, b, f);
}

}  // namespace

extern "C" int dr_intent_conv_fwd(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_dst, int32_t R, const float* h,
                                  int64_t ld_h, int32_t D, const float* W, const float* theta, int32_t L, int32_t act, float* out,
                                  int64_t ld_out, float* agg, dr_stream_t stream) {
    const int st = ic_domain(n_dst, R, D, L, act);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_h, D) || dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (n_dst == 0) return DR_OK;
    if (!row_ptr || !h || !W || !theta || !out || !dr_aligned16(h) || !dr_aligned16(out) || !dr_aligned16(agg)) return DR_EINVAL;
    const int g = dr_pow2_ceil(D / 4);
    const int64_t waves = (n_dst + 64 / g - 1) / (64 / g), grid = (waves + 3) / 4;
    if (grid > 0x7fffffff) return DR_EINVAL;
    const IcF f = {W, theta, R, L, act};
    const dim3 gr((unsigned)grid), bl(256);
    hipStream_t s = dr_s(stream);
#define DR_IC_CASE(GG) return dr_launch(intent_conv_fwd_kernel<GG>, gr, bl, 0, s, row_ptr, col, val, n_dst, h, ld_h, (int)D, f, out, ld_out, agg)
    switch (g) {
        case 1: DR_IC_CASE(1);
        case 2: DR_IC_CASE(2);
        case 4: DR_IC_CASE(4);
        case 8: DR_IC_CASE(8);
        case 16: DR_IC_CASE(16);
        case 32: DR_IC_CASE(32);
        default: DR_IC_CASE(64);
    }
#undef DR_IC_CASE
}

extern "C" int dr_intent_mix_fwd(const float* h_self, int64_t ld_h, const float* agg, int64_t n_dst, int32_t R, int32_t D, const float* W,
                                 const float* theta, int32_t L, int32_t act, float* out, int64_t ld_out, dr_stream_t stream) {
    const int st = ic_domain(n_dst, R, D, L, act);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_h, D) || dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (n_dst == 0) return DR_OK;
    if (!h_self || !agg || !W || !theta || !out || !dr_aligned16(h_self) || !dr_aligned16(agg) || !dr_aligned16(out)) return DR_EINVAL;
    const int g = dr_pow2_ceil(D / 4);
    const int64_t waves = (n_dst + 64 / g - 1) / (64 / g), grid = (waves + 3) / 4;
    if (grid > 0x7fffffff) return DR_EINVAL;
    const IcF f = {W, theta, R, L, act};
    return dr_launch(intent_mix_fwd_kernel, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), h_self, ld_h, agg, n_dst, (int)D, f, out,
                     ld_out, g);
}

extern "C" int64_t dr_intent_conv_bwd_workspace_bytes(int64_t n_dst, int32_t D, int32_t R, int32_t L) {
    if (ic_domain(n_dst, R, D, L, 0) != DR_OK) return -1;
    int64_t iters, blocks;
    ic_bwd_grid(n_dst, D, iters, blocks);
    return blocks * L * (R + 2) * (int64_t)sizeof(float);
}

extern "C" int dr_intent_conv_bwd(const float* h_self, int64_t ld_h, const float* agg, const float* d_out, int64_t ld_do, const float* out,
                                  int64_t ld_out, const float* W, const float* theta, int64_t n_dst, int32_t R, int32_t D, int32_t L,
                                  int32_t act, float* d_self, int64_t ld_ds, float* d_agg, float* d_W, float* d_theta, void* workspace,
                                  int64_t workspace_bytes, dr_stream_t stream) {
    const int st = ic_domain(n_dst, R, D, L, act);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_h, D) || dr_bad_ld(ld_do, D) || dr_bad_ld(ld_ds, D) || (out != nullptr && dr_bad_ld(ld_out, D))) return DR_EINVAL;
    if (n_dst == 0) return DR_OK;
    if (!h_self || !agg || !d_out || !W || !theta || !d_self || !d_agg || !d_W || !d_theta || !workspace) return DR_EINVAL;
    if (!dr_aligned16(h_self) || !dr_aligned16(agg) || !dr_aligned16(d_out) || !dr_aligned16(out) || !dr_aligned16(d_self) ||
        !dr_aligned16(d_agg))
        return DR_EINVAL;
    if (workspace_bytes < dr_intent_conv_bwd_workspace_bytes(n_dst, D, R, L)) return DR_EINVAL;
    int64_t iters, blocks;
    ic_bwd_grid(n_dst, D, iters, blocks);
    if (blocks > 0x7fffffff || iters > 0x7fffffff) return DR_EINVAL;
    IcB b = {};
    b.h_self = h_self; b.ld_h = ld_h; b.agg = agg; b.d_out = d_out; b.ld_do = ld_do; b.out = out; b.ld_out = ld_out;
    b.d_self = d_self; b.ld_ds = ld_ds; b.d_agg = d_agg; b.partials = static_cast<float*>(workspace);
    b.n_dst = n_dst; b.D = D; b.g = dr_pow2_ceil(D / 4); b.iters = (int)iters;
    const IcF f = {W, theta, R, L, act};
    hipStream_t s = dr_s(stream);
    int st1;
    if (R <= 3) st1 = L <= 4 ? ic_bwd_launch<4, 3>(b, f, blocks, s) : L <= 8 ? ic_bwd_launch<8, 3>(b, f, blocks, s) : ic_bwd_launch<16, 3>(b, f, blocks, s);
    else st1 = L <= 4 ? ic_bwd_launch<4, 7>(b, f, blocks, s) : L <= 8 ? ic_bwd_launch<8, 7>(b, f, blocks, s) : ic_bwd_launch<16, 7>(b, f, blocks, s);
    if (st1 != DR_OK) return st1;
    return dr_sum_partials(b.partials, blocks, d_W, (int64_t)L * (R + 1), d_theta, L, nullptr, 0, 1, s);
}
