// xDeepFM's CIN layer with its sum pooling fused, and a backward on the matrix pipe (notation and formulas: cin.hip, rows r = (b, d)):
//
//   out[b, f, d]  = act(sum_ij W[i Hk + j, f] x0[b, i, d] x[b, j, d] + bias[f]) ;   pooled[b, f] = sum_d out[b, f, d]
//   g[b, f, d]    = (d_out[b, f, d] + d_pooled[b, f]) act'(out[b, f, d])
//   T[r, i, j]    = sum_f g[r, f] W[i, j, f]         d_x[r, j] = sum_i x0[r, i] T[r, i, j]      d_x0[r, i] = sum_j x[r, j] T[r, i, j]
//   dW[i, j, f]   = sum_r x0[r, i] x[r, j] g[r, f]   dbias[f]  = sum_r g[r, f]
//
// Every product runs on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: bitwise an fmaf chain in k order); neither z = x0 (x) x nor T is
// ever written to memory; every sum has a fixed order (no float atomics).
//
// FORWARD   cin.hip's kernel with the 64 columns of a block laid out so that a block owns WHOLE examples: floor(64 / D) examples per
//           block for D <= 64 (the rest of the 64 columns is padding), one example per block looping over 64-column tiles of d for
//           D > 64.  The activated tile goes through LDS once more and one thread per (example, feature map) sums its d in order.
// DX        64 rows per block, 4 waves = (32-row half) x (parity of the j-tile).  g (with act' and the d_pooled broadcast applied), x0
//           and x of the 64 rows are staged in LDS.  For a j-tile of 32 and a fixed i the MFMA runs A = W[(i, j-tile), f], B = g[f, r]:
//           the accumulator is T[r, i, j] with r on the lane and 16 j per lane.  d_x[r, j] += x0[r, i] T stays in 16 registers across
//           the i loop; d_x0[r, i] += sum_j x[r, j] T is a per-lane sum, one exchange with lane ^ 32 and one LDS read-modify-write in a
//           buffer that this wave alone owns (one per j-tile parity; the two are added at the end).  W is read from a packed copy
//           (one launch; [i][j-tile][f / 8][lane] float4, zero padded) so that the A operand of four MFMAs is one coalesced 16-byte load.
// DW        grid = row chunks x H0 x (128 x 128 super-tiles of [j, f]).  A block stages 64 rows of g, x and x0[., i] at a time; wave w owns
//           f-tile w of the super-tile and up to four j-tiles (64 accumulator registers): A = x0[r, i] x[r, j] (one multiply), B = g[f, r].
//           Each chunk writes its partial [H0 Hk Fm + Fm] (the tail is dbias, from the blocks of i = 0) to the workspace; a second launch
//           adds the partials in chunk order.
#include "dr_common.h"
#include "dr_cin_act.h"
#include "dr_sum_partials.h"

namespace {

constexpr int CP_COLS = 64;          // (b, d) rows per block tile
constexpr int CP_PITCH = 65;         // LDS pitch of one field's / feature map's row values (conflict-free per 32-lane half)
constexpr int CP_SUPER = 128;        // dW: j and f extent of a block's super-tile (4 tiles of 32 each)
constexpr int64_t CP_LDS_MAX = 160 * 1024;

__host__ __device__ inline int cp_ceil(int a, int b) { return (a + b - 1) / b; }
// row of the 32x32 C/D tile held in register `reg` of a lane in half `hi`
__device__ __forceinline__ int cp_crow(int reg, int hi) { return (reg & 3) + 8 * (reg >> 2) + 4 * hi; }

// ---- forward ------------------------------------------------------------------------------------------------------------------
// grid.x: groups of E examples (D <= 64) or one example (D > 64); grid.y: groups of 64 feature maps.  4 waves = (column half, f half).
__global__ __launch_bounds__(256) void cin_pool_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ x, int64_t B,
                                                           int32_t H0, int32_t Hk, int32_t D, const float* __restrict__ W, int32_t Fm,
                                                           const float* __restrict__ bias, int32_t act, float* __restrict__ out,
                                                           float* __restrict__ pooled, int32_t E) {
    extern __shared__ float cp_lds[];                    // [H0 + Hk][CP_PITCH] operands, then [64][CP_PITCH] activated tile
    float* xs0 = cp_lds;
    float* xs = cp_lds + (size_t)H0 * CP_PITCH;
    float* ot = cp_lds + (size_t)(H0 + Hk) * CP_PITCH;
    const bool wide = D > CP_COLS;
    const int ntile = wide ? cp_ceil(D, CP_COLS) : 1;
    const int64_t b0 = (int64_t)blockIdx.x * E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int c = (wave & 1) * 32 + l31;                 // this lane's column of the tile (operand B column)
    const int f0 = blockIdx.y * 64;
    const int f = f0 + (wave >> 1) * 32 + l31;           // this lane's feature map (operand A row)
    const bool fv = f < Fm;
    const int fc = fv ? f : Fm - 1;
    float psum = 0.f;                                    // D > 64: pooled[b0, f0 + threadIdx.x] across the tiles (threads 0..63)
    for (int t = 0; t < ntile; ++t) {
        if (t > 0) __syncthreads();
        for (int idx = threadIdx.x; idx < (H0 + Hk) * CP_COLS; idx += blockDim.x) {
            const int fld = idx / CP_COLS, cc = idx % CP_COLS;
            const int e = wide ? 0 : cc / D;
            const int d = wide ? t * CP_COLS + cc : cc - e * D;
            const int64_t b = b0 + e;
            float v = 0.f;
            if (e < E && d < D && b < B) v = fld < H0 ? x0[(b * H0 + fld) * D + d] : x[(b * Hk + (fld - H0)) * D + d];
            cp_lds[(size_t)fld * CP_PITCH + cc] = v;
        }
        __syncthreads();
        dr_f32x16 acc;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        for (int i = 0; i < H0; ++i) {
            const float a0 = xs0[(size_t)i * CP_PITCH + c];
            const float* wrow = W + (int64_t)i * Hk * Fm + fc;
            for (int j = 0; j < Hk; j += 2) {            // reduction pair (j, j + 1): lane half `hi` supplies element j + hi
                const int jj = j + hi;
                const bool jv = jj < Hk;
                const int jc = jv ? jj : Hk - 1;
                const float wv = (jv && fv) ? wrow[(int64_t)jc * Fm] : 0.f;
                const float zv = jv ? a0 * xs[(size_t)jc * CP_PITCH + c] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, zv, acc, 0, 0, 0);
            }
        }
        const int e = wide ? 0 : c / D;
        const int d = wide ? t * CP_COLS + c : c - e * D;
        const int64_t b = b0 + e;
        const bool cv = e < E && d < D && b < B;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int fl = (wave >> 1) * 32 + cp_crow(reg, hi);
            const int fo = f0 + fl;
            float v = 0.f;
            if (cv && fo < Fm) {
                v = cin_act(acc[reg] + (bias != nullptr ? bias[fo] : 0.f), act);
                if (out != nullptr) out[(b * Fm + fo) * D + d] = v;
            }
            ot[(size_t)fl * CP_PITCH + c] = v;
        }
        if (pooled == nullptr) continue;                 // uniform
        __syncthreads();
        if (wide) {
            if (threadIdx.x < 64) {
                const int nc = min(CP_COLS, D - t * CP_COLS);
                for (int cc = 0; cc < nc; ++cc) psum += ot[(size_t)threadIdx.x * CP_PITCH + cc];
            }
        } else {
            for (int p = threadIdx.x; p < 64 * E; p += blockDim.x) {
                const int fl = p & 63, ee = p >> 6;
                const int64_t bb = b0 + ee;
                if (bb >= B || f0 + fl >= Fm) continue;
                float s = 0.f;
                for (int dd = 0; dd < D; ++dd) s += ot[(size_t)fl * CP_PITCH + ee * D + dd];
                pooled[bb * Fm + f0 + fl] = s;
            }
        }
    }
    if (pooled != nullptr && wide && threadIdx.x < 64 && f0 + (int)threadIdx.x < Fm) pooled[b0 * Fm + f0 + threadIdx.x] = psum;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// g of row m = (b, d) and feature map f
__device__ __forceinline__ float cp_g(const float* __restrict__ out, const float* __restrict__ d_out, const float* __restrict__ d_pooled,
                                      int64_t b, int f, int d, int32_t Fm, int32_t D, int32_t act) {
    const int64_t o = (b * Fm + f) * D + d;
    float v = d_out != nullptr ? d_out[o] : 0.f;
    if (d_pooled != nullptr) v += d_pooled[b * Fm + f];
    return act == 0 ? v : v * cin_act_grad(out[o], act);
}

// Wp[i][jt][q][lane] (float4): element s = W[(i Hk + 32 jt + (lane & 31)) Fm + 8 q + 4 (lane >> 5) + s], zero outside W
__global__ __launch_bounds__(256) void cin_pool_pack_w_kernel(const float* __restrict__ W, int32_t H0, int32_t Hk, int32_t Fm, int32_t njt,
                                                              int32_t fq, float4* __restrict__ Wp) {
    const int64_t total = (int64_t)H0 * njt * fq * 64, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int lane = (int)(t & 63);
        const int64_t u = t >> 6;
        const int q = (int)(u % fq);
        const int jt = (int)((u / fq) % njt);
        const int i = (int)(u / ((int64_t)fq * njt));
        const int j = jt * 32 + (lane & 31);
        const int fb = 8 * q + 4 * (lane >> 5);
        float w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) w[s] = (j < Hk && fb + s < Fm) ? W[((int64_t)i * Hk + j) * Fm + fb + s] : 0.f;
        Wp[t] = make_float4(w[0], w[1], w[2], w[3]);
    }
}

// grid.x: tiles of 64 rows.  LDS: g [8 fq][P], x0 [H0][P], x [32 njt][P] (zero padded), d_x0 partials [2][H0][P]
__global__ __launch_bounds__(256) void cin_pool_bwd_dx_kernel(const float* __restrict__ x0, const float* __restrict__ x, int64_t rows,
                                                              int32_t H0, int32_t Hk, int32_t D, const float4* __restrict__ Wp, int32_t Fm,
                                                              int32_t njt, int32_t fq, int32_t act, const float* __restrict__ out,
                                                              const float* __restrict__ d_out, const float* __restrict__ d_pooled,
                                                              float* __restrict__ d_x0, int32_t accumulate_x0, float* __restrict__ d_x) {
    extern __shared__ float cp_lds[];
    const int fpad = 8 * fq, jpad = 32 * njt;
    float* gs = cp_lds;
    float* xs0 = gs + (size_t)fpad * CP_PITCH;
    float* xs = xs0 + (size_t)H0 * CP_PITCH;
    float* px0 = xs + (size_t)jpad * CP_PITCH;
    const int64_t m0 = (int64_t)blockIdx.x * CP_COLS;
    const int nrow = fpad + H0 + jpad + 2 * H0;
    for (int idx = threadIdx.x; idx < nrow * CP_COLS; idx += blockDim.x) {
        const int row = idx / CP_COLS, cc = idx % CP_COLS;
        const int64_t m = m0 + cc;
        float v = 0.f;
        if (m < rows && row < fpad + H0 + jpad) {
            const int64_t b = m / D;
            const int d = (int)(m - b * D);
            if (row < fpad) {
                if (row < Fm) v = cp_g(out, d_out, d_pooled, b, row, d, Fm, D, act);
            } else if (row < fpad + H0) {
                v = x0[(b * H0 + (row - fpad)) * D + d];
            } else if (row - fpad - H0 < Hk) {
                v = x[(b * Hk + (row - fpad - H0)) * D + d];
            }
        }
        cp_lds[(size_t)row * CP_PITCH + cc] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int r = (wave & 1) * 32 + l31;                 // this lane's row of the tile (operand B column)
    const int jh = wave >> 1;                            // this wave's j-tile parity
    const int64_t m = m0 + r;
    const int64_t bm = m / D;
    const int dm = (int)(m - bm * D);
    float* mypx0 = px0 + (size_t)jh * H0 * CP_PITCH;
    for (int jt = jh; jt < njt; jt += 2) {
        dr_f32x16 ax;
#pragma unroll
        for (int k = 0; k < 16; ++k) ax[k] = 0.f;
        for (int i = 0; i < H0; ++i) {
            dr_f32x16 T;
#pragma unroll
            for (int k = 0; k < 16; ++k) T[k] = 0.f;
            const float4* wp = Wp + ((int64_t)i * njt + jt) * fq * 64 + lane;
            for (int q = 0; q < fq; ++q) {               // k order within 8 f: lane half hi supplies f = 8 q + 4 hi + s at step s
                const float4 w = wp[(int64_t)q * 64];
                const float* gp = gs + (size_t)(8 * q + 4 * hi) * CP_PITCH + r;
                T = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, gp[0], T, 0, 0, 0);
                T = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, gp[CP_PITCH], T, 0, 0, 0);
                T = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, gp[2 * CP_PITCH], T, 0, 0, 0);
                T = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, gp[3 * CP_PITCH], T, 0, 0, 0);
            }
            const float x0v = xs0[(size_t)i * CP_PITCH + r];
            float s = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int j = jt * 32 + cp_crow(reg, hi);
                ax[reg] = fmaf(x0v, T[reg], ax[reg]);
                s = fmaf(xs[(size_t)j * CP_PITCH + r], T[reg], s);
            }
            s += __shfl_xor(s, 32, 64);
            if (hi == 0) mypx0[(size_t)i * CP_PITCH + r] += s;
        }
        if (m < rows) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int j = jt * 32 + cp_crow(reg, hi);
                if (j < Hk) d_x[(bm * Hk + j) * D + dm] = ax[reg];
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < H0 * CP_COLS; idx += blockDim.x) {
        const int i = idx / CP_COLS, cc = idx % CP_COLS;
        const int64_t mm = m0 + cc;
        if (mm >= rows) continue;
        const int64_t b = mm / D;
        const int d = (int)(mm - b * D);
        const float v = px0[(size_t)i * CP_PITCH + cc] + px0[(size_t)(H0 + i) * CP_PITCH + cc];
        float* dst = d_x0 + (b * H0 + i) * D + d;
        *dst = accumulate_x0 ? *dst + v : v;
    }
}

// grid.x: row chunks of `chunk_rows` (a multiple of 64); grid.y: i; grid.z: super-tiles (js + nsj * fs).
// LDS: g [nf][P], x [nj][P], x0[., i] [P] with nf / nj = the super-tile's f / j extent rounded up to 32
__global__ __launch_bounds__(256) void cin_pool_bwd_dw_kernel(const float* __restrict__ x0, const float* __restrict__ x, int64_t rows,
                                                              int64_t chunk_rows, int32_t H0, int32_t Hk, int32_t D, int32_t Fm,
                                                              int32_t nsj, int32_t nf, int32_t nj, int32_t act,
                                                              const float* __restrict__ out, const float* __restrict__ d_out,
                                                              const float* __restrict__ d_pooled, float* __restrict__ part) {
    extern __shared__ float cp_lds[];
    float* gs = cp_lds;
    float* xs = gs + (size_t)nf * CP_PITCH;
    float* xi = xs + (size_t)nj * CP_PITCH;
    const int i = blockIdx.y;
    const int js = blockIdx.z % nsj, fs = blockIdx.z / nsj;
    const int j0 = js * CP_SUPER, fb0 = fs * CP_SUPER;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int njt = min(4, cp_ceil(Hk - j0, 32));        // j-tiles of this super-tile (uniform)
    const bool wact = wave * 32 < nf && fb0 + wave * 32 < Fm;   // this wave's f-tile exists (uniform per wave)
    const bool do_bias = i == 0 && js == 0;
    dr_f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;
    float bsum = 0.f;                                    // dbias partial of f = fb0 + threadIdx.x (threads < nf)
    const int64_t mbeg = (int64_t)blockIdx.x * chunk_rows;
    const int64_t mend = min(rows, mbeg + chunk_rows);
    for (int64_t m0 = mbeg; m0 < mend; m0 += CP_COLS) {
        if (m0 > mbeg) __syncthreads();
        for (int idx = threadIdx.x; idx < (nf + nj + 1) * CP_COLS; idx += blockDim.x) {
            const int row = idx / CP_COLS, cc = idx % CP_COLS;
            const int64_t m = m0 + cc;
            float v = 0.f;
            if (m < mend) {
                const int64_t b = m / D;
                const int d = (int)(m - b * D);
                if (row < nf) {
                    if (fb0 + row < Fm) v = cp_g(out, d_out, d_pooled, b, fb0 + row, d, Fm, D, act);
                } else if (row < nf + nj) {
                    if (j0 + row - nf < Hk) v = x[(b * Hk + (j0 + row - nf)) * D + d];
                } else {
                    v = x0[(b * H0 + i) * D + d];
                }
            }
            cp_lds[(size_t)row * CP_PITCH + cc] = v;
        }
        __syncthreads();
        if (do_bias && (int)threadIdx.x < nf)
            for (int cc = 0; cc < CP_COLS; ++cc) bsum += gs[(size_t)threadIdx.x * CP_PITCH + cc];
        if (!wact) continue;
        const float* gp = gs + (size_t)(wave * 32 + l31) * CP_PITCH + hi;
        const float* xp = xs + (size_t)l31 * CP_PITCH + hi;
        for (int p = 0; p < CP_COLS; p += 2) {           // reduction pair (r, r + 1): lane half `hi` supplies row p + hi
            const float gv = gp[p];
            const float xv = xi[p + hi];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < njt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv * xp[(size_t)t * 32 * CP_PITCH + p], gv, acc[t], 0, 0, 0);
        }
    }
    float* mine = part + (int64_t)blockIdx.x * ((int64_t)H0 * Hk * Fm + Fm);
    if (do_bias && (int)threadIdx.x < nf && fb0 + (int)threadIdx.x < Fm) mine[(int64_t)H0 * Hk * Fm + fb0 + threadIdx.x] = bsum;
    if (!wact) return;
    const int f = fb0 + wave * 32 + l31;                 // C/D column
    if (f >= Fm) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t >= njt) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int j = j0 + t * 32 + cp_crow(reg, hi);
            if (j < Hk) mine[((int64_t)i * Hk + j) * Fm + f] = acc[t][reg];
        }
    }
}

struct CpPlan {
    int32_t njt, fq;          // dx: j-tiles of 32, f groups of 8
    int32_t nsj, nsf, nj, nf; // dw: super-tiles along j / f and a block's staged j / f rows
    int64_t chunk_rows;
    int32_t chunks;
    int64_t wp_floats, part_floats;
    int64_t lds_dx, lds_dw;
};

CpPlan cp_plan(int64_t B, int32_t H0, int32_t Hk, int32_t D, int32_t Fm) {
    CpPlan p;
    p.njt = cp_ceil(Hk, 32);
    p.fq = cp_ceil(Fm, 8);
    p.nsj = cp_ceil(Hk, CP_SUPER);
    p.nsf = cp_ceil(Fm, CP_SUPER);
    p.nj = Hk >= CP_SUPER ? CP_SUPER : cp_ceil(Hk, 32) * 32;
    p.nf = Fm >= CP_SUPER ? CP_SUPER : cp_ceil(Fm, 32) * 32;
    const int64_t rows = B * D;
    const int64_t tiles = (rows + CP_COLS - 1) / CP_COLS;
    // enough blocks for 4 per CU of 256, at most 64 chunks (the workspace grows with them), at least one 64-row tile each
    int64_t want = (1024 + (int64_t)H0 * p.nsj * p.nsf - 1) / ((int64_t)H0 * p.nsj * p.nsf);
    if (want > 64) want = 64;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const int64_t tiles_per = (tiles + want - 1) / want;
    p.chunk_rows = tiles_per > 0 ? tiles_per * CP_COLS : CP_COLS;
    p.chunks = tiles > 0 ? (int32_t)((tiles + tiles_per - 1) / tiles_per) : 1;
    p.wp_floats = (int64_t)H0 * p.njt * p.fq * 256;
    p.part_floats = (int64_t)p.chunks * ((int64_t)H0 * Hk * Fm + Fm);
    p.lds_dx = ((int64_t)8 * p.fq + 3 * (int64_t)H0 + 32 * (int64_t)p.njt) * CP_PITCH * 4;
    p.lds_dw = ((int64_t)p.nf + p.nj + 1) * CP_PITCH * 4;
    return p;
}

bool cp_sizes_ok(int64_t B, int32_t H0, int32_t Hk, int32_t D, int32_t Fm) {
    return B >= 0 && H0 > 0 && Hk > 0 && D > 0 && Fm > 0 && (int64_t)H0 * Hk <= 0x7fffffff / Fm && B <= ((int64_t)1 << 40) / D;
}

}  // namespace

extern "C" int dr_cin_pool_fwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W, int32_t Fm,
                               const float* bias, int32_t act, float* out, float* pooled, dr_stream_t stream) {
    if (!cp_sizes_ok(B, H0, Hk, D, Fm) || act < 0 || act > 3) return DR_EINVAL;
    if (B == 0) return DR_OK;                            // nothing to read or write: empty tensors have no address
    if (!x0 || !x || !W || (!out && !pooled)) return DR_EINVAL;
    const int64_t lds = ((int64_t)H0 + Hk + 64) * CP_PITCH * (int64_t)sizeof(float);
    if (lds > CP_LDS_MAX) return DR_ESHAPE;
    const int32_t E = D <= CP_COLS ? CP_COLS / D : 1;
    const int64_t gx = (B + E - 1) / E;
    if (gx > 0x7fffffff) return DR_EINVAL;
    return dr_launch(cin_pool_fwd_kernel, dim3((unsigned)gx, (unsigned)((Fm + 63) / 64)), dim3(256), (size_t)lds, dr_s(stream), x0, x, B, H0,
                     Hk, D, W, Fm, bias, act, out, pooled, E);
}

extern "C" int64_t dr_cin_pool_bwd_workspace_bytes(int64_t B, int32_t H0, int32_t Hk, int32_t D, int32_t Fm) {
    if (!cp_sizes_ok(B, H0, Hk, D, Fm)) return 0;
    const CpPlan p = cp_plan(B, H0, Hk, D, Fm);
    return (p.wp_floats + p.part_floats) * (int64_t)sizeof(float);
}

extern "C" int dr_cin_pool_bwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W, int32_t Fm,
                               int32_t act, const float* out, const float* d_out, const float* d_pooled, float* d_x0,
                               int32_t accumulate_x0, float* d_x, float* dW, float* dbias, void* ws, int64_t ws_bytes,
                               dr_stream_t stream) {
    if (!cp_sizes_ok(B, H0, Hk, D, Fm) || act < 0 || act > 3) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!x0 || !x || !W || !d_x0 || !d_x || !dW || (!d_out && !d_pooled) || (act != 0 && !out)) return DR_EINVAL;
    const CpPlan p = cp_plan(B, H0, Hk, D, Fm);
    if (p.lds_dx > CP_LDS_MAX || p.lds_dw > CP_LDS_MAX) return DR_ESHAPE;
    if (!ws || !dr_aligned16(ws) || ws_bytes < (p.wp_floats + p.part_floats) * (int64_t)sizeof(float)) return DR_EINVAL;
    const int64_t rows = B * D;
    const int64_t gx = (rows + CP_COLS - 1) / CP_COLS;
    if (gx > 0x7fffffff || H0 > 65535 || (int64_t)p.nsj * p.nsf > 65535) return DR_EINVAL;
    float4* Wp = static_cast<float4*>(ws);
    float* part = static_cast<float*>(ws) + p.wp_floats;
    hipLaunchKernelGGL(cin_pool_pack_w_kernel, dim3(dr_grid_for(p.wp_floats / 4, 256)), dim3(256), 0, dr_s(stream), W, H0, Hk, Fm, p.njt,
                       p.fq, Wp);
    int st = dr_launch(cin_pool_bwd_dx_kernel, dim3((unsigned)gx), dim3(256), (size_t)p.lds_dx, dr_s(stream), x0, x, rows, H0, Hk, D, Wp, Fm,
                       p.njt, p.fq, act, out, d_out, d_pooled, d_x0, accumulate_x0, d_x);
    if (st != DR_OK) return st;
    st = dr_launch(cin_pool_bwd_dw_kernel, dim3((unsigned)p.chunks, (unsigned)H0, (unsigned)(p.nsj * p.nsf)), dim3(256), (size_t)p.lds_dw,
                   dr_s(stream), x0, x, rows, p.chunk_rows, H0, Hk, D, Fm, p.nsj, p.nf, p.nj, act, out, d_out, d_pooled, part);
    if (st != DR_OK) return st;
    // dW / dbias = the chunks' partials added in chunk order
    const int64_t nw = (int64_t)H0 * Hk * Fm;
    return dr_sum_partials(part, p.chunks, dW, nw, dbias, Fm, nullptr, 0, dr_grid_for(nw + Fm, 256), dr_s(stream));
}
