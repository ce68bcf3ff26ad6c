// AFM's attention pooling over field pairs (Xiao et al., IJCAI 2017), forward and backward.
//
//   pairs  q = i (i - 1) / 2 + j, 0 <= j < i < F (DotInteraction's order without the diagonal), P = F (F - 1) / 2
//   p_q = e_i * e_j [D];  z_q = p_q W + b [A];  s_q = sum_a max(z_qa, 0) h_a;  a = softmax_q(s);  out = sum_q a_q p_q;  lse = log sum_q exp(s_q)
//   backward from g = d_out:  ds_q = a_q (<g, p_q> - <g, out>);  dz_q = ds_q h * [z_q > 0];  dh = sum ds_q max(z_q, 0);  db = sum dz_q;
//                             dW = sum p_q^T dz_q;  dp_q = a_q g + dz_q W^T;  de_i = sum_{j != i} dp_(ij) * e_j
//
// ONE WAVE OWNS ONE EXAMPLE AT A TIME; a block of 1, 2 or 4 waves (as many as the LDS holds) shares W, b, h and the pair table in LDS and
// walks the batch with a fixed stride.  The example's F rows sit in LDS (pitch 16 ceil(D / 16) + 4, zero beyond D); the pairs go by in
// tiles of 16.  Every matrix product runs on v_mfma_f32_16x16x4_f32, TRANSPOSED so that the pair sits on the lane:
//   z^T [A, 16] = W^T p^T    A operand W[k][16 at + c] (LDS), B operand p[pair c][k] = e_i[k] e_j[k], formed from two float4 LDS reads per 16 k
//                            (k = 16 s + 4 (lane >> 4) + e in step e of chunk s, for both operands alike).  Lane (c = pair, q4) ends up with
//                            z[pair][a = 16 at + 4 q4 + reg], so s_q is a lane-local sum and two cross-lane adds (xor 16, 32).
//   dp^T [D, 16] = W dz^T    sums over a, the ROW index of the z^T tile: dz goes in from the registers it is made in, W as float4 from LDS.
//   dW [D, A] = p^T dz       sums over the pairs, the LANE index: dz passes through a [16][A + 4] LDS tile once; the A operand
//                            p[pair][d] is formed again from the rows.  Accumulated in registers over all of a wave's examples.
// FORWARD   online softmax over the tiles: running max m, sum l and the pooled vector (the lane owns columns d = lane + 64 n and adds the
//           16 pairs of a tile in pair order, weights and (i, j) read from lane `pair`).  s goes to attn only when attn != NULL and is
//           turned into exp(s - lse) by the lane that wrote it once lse is known.
// BACKWARD  recomputes z per tile.  <g, p_q> is summed next to the z product in the same lane layout and the same fmaf order as <g, out>,
//           so at P = 1 (out == p_0 bit for bit) ds is exactly 0.  dp^T goes to a [16][D + 4] LDS tile; then the lane that owns column d
//           adds the 16 pairs in pair order into the d_emb rows in LDS (one owner per sum, fixed order).  dW, db, dh: the block's waves add
//           their registers in wave order into LDS, the block writes one partial to the workspace, and a second launch adds the partials
//           in block order.  The number of blocks depends on (B, F, D, A) only.
#include "dr_common.h"
#include "dr_sum_partials.h"

namespace {

constexpr int AFM_MAX_F = 64;
constexpr int AFM_MAX_D = 256;
constexpr int AFM_MAX_A = 128;
constexpr int AFM_MAX_TILES = 32;         // DT * AT: the dW accumulators are 4 DT AT registers per lane
constexpr int AFM_LDS_FLOATS = 40000;     // of the 40960 a workgroup can have
constexpr int AFM_FWD_BLOCKS = 2048;
constexpr int AFM_BWD_BLOCKS = 512;

struct AfmP {
    const float* emb; int64_t ld_emb;
    const float* W; const float* b; const float* h;
    const float* out_in; int64_t ld_out; const float* lse_in;      // backward
    const float* g; int64_t ld_g;
    float* out; float* lse; float* attn; int64_t ld_attn;           // forward (ld_out shared)
    float* d_emb; int64_t ld_demb; float* ws;
    int64_t B;
    int32_t F, D, A, P, P16, D16, KC;
};

struct AfmGeo { int DT, AT, nw, D16, A16, P, P16; size_t lds_fwd, lds_bwd; };

// W [D16][PW] (zero beyond D and A), b [A16], h [A16], the pair table [P16] ((i << 8) | j; the pad entries name pair (1, 0))
template <int AT>
__device__ __forceinline__ void afm_stage_shared(const AfmP& p, float* Wl, float* bl, float* hl, int* tab) {
    constexpr int A16 = 16 * AT, PW = A16 + 4;
    for (int idx = threadIdx.x; idx < p.D16 * A16; idx += blockDim.x) {
        const int d = idx / A16, a = idx - d * A16;
        Wl[d * PW + a] = (d < p.D && a < p.A) ? p.W[(int64_t)d * p.A + a] : 0.f;
    }
    for (int a = threadIdx.x; a < A16; a += blockDim.x) {
        bl[a] = a < p.A ? p.b[a] : 0.f;
        hl[a] = a < p.A ? p.h[a] : 0.f;
    }
    for (int q = threadIdx.x; q < p.P16; q += blockDim.x) {
        int i = (int)((1.f + sqrtf(1.f + 8.f * (float)q)) * 0.5f);
        while (i * (i - 1) / 2 > q) --i;
        while ((i + 1) * i / 2 <= q) ++i;
        tab[q] = q < p.P ? ((i << 8) | (q - i * (i - 1) / 2)) : (1 << 8);
    }
}

// the wave's example: F rows of D16 floats at pitch PE, zero beyond D (all zero for a wave without an example)
__device__ __forceinline__ void afm_stage_rows(const AfmP& p, float* el, int64_t b, bool valid, int lane) {
    const int PE = p.D16 + 4, n4 = p.D16 >> 2;
    const float* src = p.emb + b * p.ld_emb;
    for (int idx = lane; idx < p.F * n4; idx += 64) {
        const int f = idx / n4, k = (idx - f * n4) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid && k < p.D) v = *reinterpret_cast<const float4*>(src + (int64_t)f * p.D + k);
        *reinterpret_cast<float4*>(el + f * PE + k) = v;
    }
}

// z^T of the tile's 16 pairs: acc[at][reg] = sum_k W[k][16 at + 4 q4 + reg] p[pair c][k] on lane (c, q4).  With gl != nullptr also
// this lane's part of <g, p> (chunks s, elements e in order; summed over q4 by the caller).
template <int AT>
__device__ __forceinline__ float afm_z_tile(const float* Wl, const float* ei, const float* ej, const float* gl, int KC, int c, int q4,
                                            dr_f32x4* acc) {
    constexpr int PW = 16 * AT + 4;
#pragma unroll
    for (int at = 0; at < AT; ++at) acc[at] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
    float gp = 0.f;
    for (int s = 0; s < KC; ++s) {
        const float4 x = *reinterpret_cast<const float4*>(ei + 16 * s + 4 * q4);
        const float4 y = *reinterpret_cast<const float4*>(ej + 16 * s + 4 * q4);
        const float pv[4] = {x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w};
        if (gl != nullptr) {
            const float4 gv = *reinterpret_cast<const float4*>(gl + 16 * s + 4 * q4);
            gp = fmaf(pv[0], gv.x, gp); gp = fmaf(pv[1], gv.y, gp); gp = fmaf(pv[2], gv.z, gp); gp = fmaf(pv[3], gv.w, gp);
        }
        const float* wk = Wl + (16 * s + 4 * q4) * PW + c;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int at = 0; at < AT; ++at)
                acc[at] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[e * PW + 16 * at], pv[e], acc[at], 0, 0, 0);
    }
    return gp;
}

template <int AT>
__global__ __launch_bounds__(256) void afm_fwd_kernel(const AfmP p) {
    extern __shared__ float afm_lds[];
    constexpr int A16 = 16 * AT, PW = A16 + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    const int PE = p.D16 + 4;
    float* Wl = afm_lds;
    float* bl = Wl + p.D16 * PW;
    float* hl = bl + A16;
    int* tab = reinterpret_cast<int*>(hl + A16);
    float* el = reinterpret_cast<float*>(tab + p.P16) + (size_t)wave * p.F * PE;
    afm_stage_shared<AT>(p, Wl, bl, hl, tab);
    const int64_t stride = (int64_t)gridDim.x * nw;
    const int64_t iters = (p.B + stride - 1) / stride;         // the same for every wave: the barriers match
    const int ntiles = p.P16 >> 4;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t b = it * stride + (int64_t)blockIdx.x * nw + wave;
        const bool valid = b < p.B;
        __syncthreads();                                       // the previous example's rows are read
        afm_stage_rows(p, el, b, valid, lane);
        __syncthreads();
        float m = -INFINITY, l = 0.f;
        float oacc[4] = {0.f, 0.f, 0.f, 0.f};
        float* attn = (p.attn != nullptr && valid) ? p.attn + b * p.ld_attn : nullptr;
        for (int t = 0; t < ntiles; ++t) {
            const int ij = tab[16 * t + c];
            dr_f32x4 acc[AT];
            afm_z_tile<AT>(Wl, el + (ij >> 8) * PE, el + (ij & 255) * PE, nullptr, p.KC, c, q4, acc);
            float sp = 0.f;
#pragma unroll
            for (int at = 0; at < AT; ++at) {
                const float4 bv = *reinterpret_cast<const float4*>(bl + 16 * at + 4 * q4);
                const float4 hv = *reinterpret_cast<const float4*>(hl + 16 * at + 4 * q4);
                sp = fmaf(fmaxf(acc[at][0] + bv.x, 0.f), hv.x, sp);
                sp = fmaf(fmaxf(acc[at][1] + bv.y, 0.f), hv.y, sp);
                sp = fmaf(fmaxf(acc[at][2] + bv.z, 0.f), hv.z, sp);
                sp = fmaf(fmaxf(acc[at][3] + bv.w, 0.f), hv.w, sp);
            }
            sp += __shfl_xor(sp, 16, 64);
            sp += __shfl_xor(sp, 32, 64);
            const bool qv = 16 * t + c < p.P;
            const float s = qv ? sp : -INFINITY;
            if (attn != nullptr && qv && q4 == 0) attn[16 * t + c] = s;
            float mt = s;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mt = fmaxf(mt, __shfl_xor(mt, o, 64));
            const float mn = fmaxf(m, mt);                     // every tile holds a valid pair: mn is finite
            const float scale = expf(m - mn);
            const float w = qv ? expf(s - mn) : 0.f;
            float wsum = w;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) wsum += __shfl_xor(wsum, o, 64);
            l = fmaf(l, scale, wsum);
            m = mn;
#pragma unroll
            for (int n = 0; n < 4; ++n) oacc[n] *= scale;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float wk = dr_readlane(w, kk);
                const int ijk = __builtin_amdgcn_readlane(ij, kk);
                const float* ri = el + (ijk >> 8) * PE;
                const float* rj = el + (ijk & 255) * PE;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int d = lane + 64 * n;
                    if (d < p.D16) oacc[n] = fmaf(wk, ri[d] * rj[d], oacc[n]);
                }
            }
        }
        if (!valid) continue;
        float* o = p.out + b * p.ld_out;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int d = lane + 64 * n;
            if (d < p.D) o[d] = oacc[n] / l;
        }
        const float lse = m + logf(l);
        if (lane == 0) p.lse[b] = lse;
        if (attn != nullptr && q4 == 0)
            for (int q = c; q < p.P; q += 16) attn[q] = expf(attn[q] - lse);
    }
}

// LDS: W, b, h, the pair table, then per wave: rows e [F][PE], d_emb rows [F][PE], g [D16], dz [16][PW], dp [16][PE]
template <int DT, int AT>
__global__ __launch_bounds__(256) void afm_bwd_kernel(const AfmP p) {
    extern __shared__ float afm_lds[];
    constexpr int D16 = 16 * DT, PE = D16 + 4, A16 = 16 * AT, PW = A16 + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c = lane & 15, q4 = lane >> 4;
    float* Wl = afm_lds;
    float* bl = Wl + D16 * PW;
    float* hl = bl + A16;
    int* tab = reinterpret_cast<int*>(hl + A16);
    const int per_wave = 2 * p.F * PE + D16 + 16 * PW + 16 * PE;
    float* el = reinterpret_cast<float*>(tab + p.P16) + (size_t)wave * per_wave;
    float* del = el + p.F * PE;
    float* gl = del + p.F * PE;
    float* dzl = gl + D16;
    float* dpl = dzl + 16 * PW;
    afm_stage_shared<AT>(p, Wl, bl, hl, tab);
    dr_f32x4 dWacc[DT][AT];
    dr_f32x4 dbacc[AT], dhacc[AT];
#pragma unroll
    for (int at = 0; at < AT; ++at) {
        dbacc[at] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
        dhacc[at] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dWacc[dt][at] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int64_t stride = (int64_t)gridDim.x * nw;
    const int64_t iters = (p.B + stride - 1) / stride;
    const int ntiles = p.P16 >> 4;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t b = it * stride + (int64_t)blockIdx.x * nw + wave;
        const bool valid = b < p.B;
        __syncthreads();
        afm_stage_rows(p, el, b, valid, lane);
        for (int idx = lane; idx < p.F * PE; idx += 64) del[idx] = 0.f;
        for (int d = lane; d < D16; d += 64) gl[d] = (valid && d < p.D) ? p.g[b * p.ld_g + d] : 0.f;
        __syncthreads();
        const float lse = valid ? p.lse_in[b] : 0.f;
        float go = 0.f;                                        // <g, out> in the order <g, p_q> is summed in
        {
            const float* ob = p.out_in + b * p.ld_out;
            for (int s = 0; s < p.KC; ++s) {
                const int k = 16 * s + 4 * q4;
                float4 ov = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid && k < p.D) ov = *reinterpret_cast<const float4*>(ob + k);
                const float4 gv = *reinterpret_cast<const float4*>(gl + k);
                go = fmaf(ov.x, gv.x, go); go = fmaf(ov.y, gv.y, go); go = fmaf(ov.z, gv.z, go); go = fmaf(ov.w, gv.w, go);
            }
            go += __shfl_xor(go, 16, 64);
            go += __shfl_xor(go, 32, 64);
        }
        for (int t = 0; t < ntiles; ++t) {
            const int ij = tab[16 * t + c];
            dr_f32x4 acc[AT];
            float gp = afm_z_tile<AT>(Wl, el + (ij >> 8) * PE, el + (ij & 255) * PE, gl, p.KC, c, q4, acc);
            gp += __shfl_xor(gp, 16, 64);
            gp += __shfl_xor(gp, 32, 64);
            float sp = 0.f;
            float4 hreg[AT];
#pragma unroll
            for (int at = 0; at < AT; ++at) {
                const float4 bv = *reinterpret_cast<const float4*>(bl + 16 * at + 4 * q4);
                hreg[at] = *reinterpret_cast<const float4*>(hl + 16 * at + 4 * q4);
                acc[at][0] += bv.x; acc[at][1] += bv.y; acc[at][2] += bv.z; acc[at][3] += bv.w;      // z
                sp = fmaf(fmaxf(acc[at][0], 0.f), hreg[at].x, sp);
                sp = fmaf(fmaxf(acc[at][1], 0.f), hreg[at].y, sp);
                sp = fmaf(fmaxf(acc[at][2], 0.f), hreg[at].z, sp);
                sp = fmaf(fmaxf(acc[at][3], 0.f), hreg[at].w, sp);
            }
            sp += __shfl_xor(sp, 16, 64);
            sp += __shfl_xor(sp, 32, 64);
            const bool qv = valid && 16 * t + c < p.P;
            const float aq = qv ? expf(sp - lse) : 0.f;
            const float ds = qv ? aq * (gp - go) : 0.f;
            dr_f32x4 dz[AT];
#pragma unroll
            for (int at = 0; at < AT; ++at) {
                const float hv[4] = {hreg[at].x, hreg[at].y, hreg[at].z, hreg[at].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = acc[at][r];
                    dz[at][r] = z > 0.f ? ds * hv[r] : 0.f;
                    dhacc[at][r] = fmaf(ds, fmaxf(z, 0.f), dhacc[at][r]);
                    dbacc[at][r] += dz[at][r];
                }
                *reinterpret_cast<float4*>(dzl + c * PW + 16 * at + 4 * q4) = make_float4(dz[at][0], dz[at][1], dz[at][2], dz[at][3]);
            }
            // dp^T = W dz^T, then + a_q g; to dpl[pair][d]
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                dr_f32x4 dp = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int at = 0; at < AT; ++at) {
                    const float4 wv = *reinterpret_cast<const float4*>(Wl + (16 * dt + c) * PW + 16 * at + 4 * q4);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, dz[at][0], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, dz[at][1], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, dz[at][2], dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, dz[at][3], dp, 0, 0, 0);
                }
                const float4 gv = *reinterpret_cast<const float4*>(gl + 16 * dt + 4 * q4);
                *reinterpret_cast<float4*>(dpl + c * PE + 16 * dt + 4 * q4) =
                    make_float4(fmaf(aq, gv.x, dp[0]), fmaf(aq, gv.y, dp[1]), fmaf(aq, gv.z, dp[2]), fmaf(aq, gv.w, dp[3]));
            }
            __syncthreads();                                   // dzl and dpl are written
            // dW += p^T dz: k = the pair 4 ks + q4 of the tile
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int ijk = tab[16 * t + 4 * ks + q4];
                const float* ri = el + (ijk >> 8) * PE + c;
                const float* rj = el + (ijk & 255) * PE + c;
                float dzv[AT];
#pragma unroll
                for (int at = 0; at < AT; ++at) dzv[at] = dzl[(4 * ks + q4) * PW + 16 * at + c];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const float pv = ri[16 * dt] * rj[16 * dt];
#pragma unroll
                    for (int at = 0; at < AT; ++at)
                        dWacc[dt][at] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, dzv[at], dWacc[dt][at], 0, 0, 0);
                }
            }
            // d_emb rows: the lane owns columns d = lane + 64 n and adds the tile's pairs in order
            const int npair = min(16, p.P - 16 * t);
            for (int kk = 0; kk < npair; ++kk) {
                const int ijk = tab[16 * t + kk];
                const int ri = (ijk >> 8) * PE, rj = (ijk & 255) * PE;
#pragma unroll
                for (int n = 0; n < (D16 + 63) / 64; ++n) {
                    const int d = lane + 64 * n;
                    if (d < D16) {
                        const float v = dpl[kk * PE + d];
                        del[ri + d] = fmaf(v, el[rj + d], del[ri + d]);
                        del[rj + d] = fmaf(v, el[ri + d], del[rj + d]);
                    }
                }
            }
            __syncthreads();                                   // dzl and dpl are read
        }
        if (valid) {
            float* dst = p.d_emb + b * p.ld_demb;
            const int n4 = p.D >> 2;
            for (int idx = lane; idx < p.F * n4; idx += 64) {
                const int f = idx / n4, k = (idx - f * n4) << 2;
                *reinterpret_cast<float4*>(dst + (int64_t)f * p.D + k) = *reinterpret_cast<const float4*>(del + f * PE + k);
            }
        }
    }
    // the block's partial: waves add their registers into LDS in wave order (dW over W's image, db and dh over b's and h's)
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                dbacc[at][r] += __shfl_xor(dbacc[at][r], o, 64);
                dhacc[at][r] += __shfl_xor(dhacc[at][r], o, 64);
            }
    for (int w = 0; w < nw; ++w) {
        __syncthreads();
        if (wave != w) continue;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int at = 0; at < AT; ++at)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* dst = Wl + (16 * dt + 4 * q4 + r) * PW + 16 * at + c;
                    *dst = w == 0 ? dWacc[dt][at][r] : *dst + dWacc[dt][at][r];
                }
        if (c == 0) {
#pragma unroll
            for (int at = 0; at < AT; ++at)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int a = 16 * at + 4 * q4 + r;
                    bl[a] = w == 0 ? dbacc[at][r] : bl[a] + dbacc[at][r];
                    hl[a] = w == 0 ? dhacc[at][r] : hl[a] + dhacc[at][r];
                }
        }
    }
    __syncthreads();
    float* part = p.ws + (size_t)blockIdx.x * ((size_t)p.D * p.A + 2 * p.A);
    for (int idx = threadIdx.x; idx < p.D * p.A; idx += blockDim.x) {
        const int d = idx / p.A, a = idx - d * p.A;
        part[idx] = Wl[d * PW + a];
    }
    for (int a = threadIdx.x; a < p.A; a += blockDim.x) {
        part[p.D * p.A + a] = bl[a];
        part[p.D * p.A + p.A + a] = hl[a];
    }
}

// DR_OK and the launch geometry, DR_EINVAL outside the domain, DR_ESHAPE where the registers or the LDS do not hold the problem
int afm_geometry(AfmGeo& g, int64_t B, int32_t F, int32_t D, int32_t A) {
    if (B < 0 || F < 2 || F > AFM_MAX_F || D < 4 || D > AFM_MAX_D || (D & 3) || A < 1 || A > AFM_MAX_A) return DR_EINVAL;
    g.DT = dr_pow2_ceil((D + 15) / 16);
    g.AT = dr_pow2_ceil((A + 15) / 16);
    if (g.DT * g.AT > AFM_MAX_TILES) return DR_ESHAPE;
    g.D16 = 16 * g.DT;
    g.A16 = 16 * g.AT;
    g.P = F * (F - 1) / 2;
    g.P16 = (g.P + 15) / 16 * 16;
    const int PE = g.D16 + 4, PW = g.A16 + 4;
    const int shared = g.D16 * PW + 2 * g.A16 + g.P16;
    const int per_wave = 2 * F * PE + g.D16 + 16 * PW + 16 * PE;
    g.nw = 4;
    while (g.nw > 1 && shared + g.nw * per_wave > AFM_LDS_FLOATS) g.nw >>= 1;
    if (shared + g.nw * per_wave > AFM_LDS_FLOATS) return DR_ESHAPE;
    g.lds_bwd = (size_t)(shared + g.nw * per_wave) * sizeof(float);
    // the forward keeps the same waves per block; its rows have the pitch of 16 ceil(D / 16) + 4, never more than PE
    g.lds_fwd = (size_t)(shared + g.nw * F * PE) * sizeof(float);
    return DR_OK;
}

int64_t afm_bwd_blocks(const AfmGeo& g, int64_t B) {
    const int64_t n = (B + g.nw - 1) / g.nw;
    return n < AFM_BWD_BLOCKS ? n : AFM_BWD_BLOCKS;
}

void afm_fill(AfmP& p, const AfmGeo& g, const float* emb, int64_t ld_emb, const float* W, const float* b, const float* h, int64_t B,
              int32_t F, int32_t D, int32_t A) {
    p.emb = emb; p.ld_emb = ld_emb; p.W = W; p.b = b; p.h = h;
    p.B = B; p.F = F; p.D = D; p.A = A; p.P = g.P; p.P16 = g.P16; p.D16 = g.D16; p.KC = (D + 15) / 16;
}

}  // namespace

#define AFM_BWD_CASE(dt, at) \
    case (dt) * 16 + (at): return dr_launch(afm_bwd_kernel<dt, at>, dim3((unsigned)grid), dim3(64 * g.nw), g.lds_bwd, dr_s(stream), p)

static int afm_bwd_dispatch(const AfmGeo& g, int64_t grid, const AfmP& p, dr_stream_t stream) {
    switch (g.DT * 16 + g.AT) {
        AFM_BWD_CASE(1, 1); AFM_BWD_CASE(1, 2); AFM_BWD_CASE(1, 4); AFM_BWD_CASE(1, 8);
        AFM_BWD_CASE(2, 1); AFM_BWD_CASE(2, 2); AFM_BWD_CASE(2, 4); AFM_BWD_CASE(2, 8);
        AFM_BWD_CASE(4, 1); AFM_BWD_CASE(4, 2); AFM_BWD_CASE(4, 4); AFM_BWD_CASE(4, 8);
        AFM_BWD_CASE(8, 1); AFM_BWD_CASE(8, 2); AFM_BWD_CASE(8, 4);
        AFM_BWD_CASE(16, 1); AFM_BWD_CASE(16, 2);
    }
    return DR_ESHAPE;
}

extern "C" int dr_afm_pool_fwd(const float* emb, int64_t ld_emb, const float* W, const float* b, const float* h, int64_t B, int32_t F,
                               int32_t D, int32_t A, float* out, int64_t ld_out, float* lse, float* attn, int64_t ld_attn,
                               dr_stream_t stream) {
    AfmGeo g = {};
    const int st = afm_geometry(g, B, F, D, A);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_emb, (int64_t)F * D) || dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (attn != nullptr && ld_attn < g.P) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!emb || !W || !b || !h || !out || !lse || !dr_aligned16(emb) || !dr_aligned16(out)) return DR_EINVAL;
    AfmP p = {};
    afm_fill(p, g, emb, ld_emb, W, b, h, B, F, D, A);
    p.D16 = 16 * p.KC;                                         // the forward has no D tiles: rows as wide as the k chunks
    p.out = out; p.ld_out = ld_out; p.lse = lse; p.attn = attn; p.ld_attn = ld_attn;
    int64_t grid = (B + g.nw - 1) / g.nw;
    if (grid > AFM_FWD_BLOCKS) grid = AFM_FWD_BLOCKS;
    const dim3 blocks((unsigned)grid), threads(64 * g.nw);
    switch (g.AT) {
        case 1: return dr_launch(afm_fwd_kernel<1>, blocks, threads, g.lds_fwd, dr_s(stream), p);
        case 2: return dr_launch(afm_fwd_kernel<2>, blocks, threads, g.lds_fwd, dr_s(stream), p);
        case 4: return dr_launch(afm_fwd_kernel<4>, blocks, threads, g.lds_fwd, dr_s(stream), p);
        default: return dr_launch(afm_fwd_kernel<8>, blocks, threads, g.lds_fwd, dr_s(stream), p);
    }
}

extern "C" int64_t dr_afm_pool_bwd_workspace_bytes(int64_t B, int32_t F, int32_t D, int32_t A) {
    AfmGeo g = {};
    const int st = afm_geometry(g, B, F, D, A);
    if (st != DR_OK) return st;
    return afm_bwd_blocks(g, B) * ((int64_t)D * A + 2 * A) * (int64_t)sizeof(float);
}

extern "C" int dr_afm_pool_bwd(const float* emb, int64_t ld_emb, const float* W, const float* b, const float* h, const float* out,
                               int64_t ld_out, const float* lse, const float* d_out, int64_t ld_dout, int64_t B, int32_t F, int32_t D,
                               int32_t A, float* d_emb, int64_t ld_demb, float* dW, float* db, float* dh, void* ws, int64_t ws_bytes,
                               dr_stream_t stream) {
    AfmGeo g = {};
    const int st = afm_geometry(g, B, F, D, A);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_emb, (int64_t)F * D) || dr_bad_ld(ld_demb, (int64_t)F * D)) return DR_EINVAL;
    if (dr_bad_ld(ld_out, D) || dr_bad_ld(ld_dout, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!emb || !W || !b || !h || !out || !lse || !d_out || !d_emb || !dW || !db || !dh || !ws) return DR_EINVAL;
    if (!dr_aligned16(emb) || !dr_aligned16(out) || !dr_aligned16(d_out) || !dr_aligned16(d_emb) || !dr_aligned16(ws)) return DR_EINVAL;
    const int64_t grid = afm_bwd_blocks(g, B);
    if (ws_bytes < grid * ((int64_t)D * A + 2 * A) * (int64_t)sizeof(float)) return DR_EINVAL;
    AfmP p = {};
    afm_fill(p, g, emb, ld_emb, W, b, h, B, F, D, A);
    p.out_in = out; p.ld_out = ld_out; p.lse_in = lse; p.g = d_out; p.ld_g = ld_dout;
    p.d_emb = d_emb; p.ld_demb = ld_demb; p.ws = static_cast<float*>(ws);
    const int st2 = afm_bwd_dispatch(g, grid, p, stream);
    if (st2 != DR_OK) return st2;
    // dW | db | dh = the blocks' partials added in block order
    return dr_sum_partials(p.ws, grid, dW, D * A, db, A, dh, A, (unsigned)((D * A + 2 * A + 255) / 256), dr_s(stream));
}
