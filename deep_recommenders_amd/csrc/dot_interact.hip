// DLRM's pairwise dot interaction (Naumov et al. 2019), forward and backward, one launch each.
//
//   T [N, D]   = rows t_0 = dense[b] (when given) followed by the F embeddings of example b;  N = F + (dense != NULL)
//   out[b, 0:D] = t_0 (c0 = D; without a dense vector c0 = 0)
//   out[b, c0 + i (i - 1) / 2 + j] = <t_i, t_j>,  0 <= j <  i < N          (self_interaction = 0, P = N (N - 1) / 2)
//   out[b, c0 + i (i + 1) / 2 + j] = <t_i, t_j>,  0 <= j <= i < N          (self_interaction = 1, P = N (N + 1) / 2)
//   backward:  S = G + G^T with G the lower-triangular matrix of d_out's triangle;  dT = S T;  dT_0 += d_out[b, 0:D]
//
// Every product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bitwise an fmaf chain in k order).  ONE WAVE OWNS ONE
// EXAMPLE (4 examples per block of 256), so there is no sum across waves, no atomic, and an example's bits do not depend on the batch
// around it.  Z = T T^T [B, N, N] never exists in memory.
//
// FORWARD   T goes through registers once, no LDS: for a chunk of 16 k, lane (r = lane & 15, q = lane >> 4) loads the float4
//           T[16 ti + r][16 s + 4 q ..] of every 16-row tile ti (64 contiguous bytes per row and 16-lane group).  Element e of that
//           fragment is the MFMA operand of step e -- as A (rows i of tile ti) and as B (rows j of tile tj) alike, so both operands walk k
//           in the same order 16 s + 4 q + e.  Only the tiles tj <= ti, the ones that meet the lower triangle, are computed: 3 of 4 at
//           N = 27, 10 of 16 at N = 64.  The accumulator has j on the lane, so 16 lanes store 16 consecutive floats of the triangle's row.
// BACKWARD  S of the wave's example is built in LDS ([16 NT][4 ceil(N / 4) + 1] floats, zero outside N x N, the diagonal doubled) straight
//           from d_out.  A = S[i, k] from LDS, B = T[k, d] from memory: lane (c = lane & 15, q) loads the float4 T[4 ks + q][64 blk + 4 c ..],
//           whose element e is the B operand of "column tile e", so that lane ends up with dT[i][64 blk + 4 c .. + 3] in element order and
//           stores float4s.  T is read once, dT written once, both as 256-byte runs per row.  K = N padded with zeros to a multiple of 4.
#include "dr_common.h"

namespace {

constexpr int DI_WAVES = 4;          // examples per block
constexpr int DI_MAX_N = 64;
constexpr int DI_MAX_D = 256;

struct DiP {
    const float* dense; int64_t ld_dense;      // NULL: no dense row
    const float* emb;   int64_t ld_emb;
    const float* d_out; int64_t ld_dout;       // backward
    float* out;         int64_t ld_out;        // forward
    float* d_dense;     int64_t ld_ddense;     // backward
    float* d_emb;       int64_t ld_demb;
    int64_t B;
    int32_t F, D, N, self, c0, P;
};

// row n of example b's T (n < N)
__device__ __forceinline__ const float* di_row(const DiP& p, int64_t b, int n) {
    const int hd = p.dense != nullptr;
    return (hd && n == 0) ? p.dense + b * p.ld_dense : p.emb + b * p.ld_emb + (int64_t)(n - hd) * p.D;
}

// first column of row i of the triangle within its P columns
__device__ __forceinline__ int di_tri(int i, int self) { return self ? i * (i + 1) / 2 : i * (i - 1) / 2; }

template <int NT>
__global__ __launch_bounds__(256) void dot_interact_fwd_kernel(const DiP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * DI_WAVES + wave;
    if (b >= p.B) return;                                      // wave-uniform; the kernel has no barrier
    constexpr int NACC = NT * (NT + 1) / 2;
    dr_f32x4 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
    const float* row[NT];
    bool rv[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        const int n = 16 * ti + r;
        rv[ti] = n < p.N;
        row[ti] = di_row(p, b, rv[ti] ? n : 0);
    }
    const int nch = (p.D + 15) >> 4;
    float4 a[NT], an[NT];                                      // this chunk's fragments and the next one's, loaded a chunk ahead
    auto load = [&](int s, float4* dst) {
        const int k = 16 * s + 4 * q;
        const bool kv = s < nch && k < p.D;                    // D % 4 == 0: a fragment is whole or absent
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
            dst[ti] = (kv && rv[ti]) ? *reinterpret_cast<const float4*>(row[ti] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    load(0, a);
    for (int s = 0; s < nch; ++s) {
        load(s + 1, an);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int t = 0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                const float av = e == 0 ? a[ti].x : e == 1 ? a[ti].y : e == 2 ? a[ti].z : a[ti].w;
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj, ++t) {
                    const float bv = e == 0 ? a[tj].x : e == 1 ? a[tj].y : e == 2 ? a[tj].z : a[tj].w;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) a[ti] = an[ti];
    }
    float* o = p.out + b * p.ld_out;
    if (p.dense != nullptr) {
        const float* t0 = p.dense + b * p.ld_dense;
        for (int d = lane; d < p.D; d += 64) o[d] = t0[d];
    }
    for (int64_t c = p.c0 + p.P + lane; c < p.ld_out; c += 64) o[c] = 0.f;
    o += p.c0;
    int t = 0;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj, ++t) {
            const int j = 16 * tj + r;                         // C/D: column on the lane, row 4 q + reg
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = 16 * ti + 4 * q + reg;
                if (i < p.N && (j < i || (p.self && j == i))) o[di_tri(i, p.self) + j] = acc[t][reg];
            }
        }
    }
}

// LDS: DI_WAVES images of S, [16 NT][pitch] each, pitch = 4 ceil(N / 4) + 1
template <int NT>
__global__ __launch_bounds__(256) void dot_interact_bwd_kernel(const DiP p) {
    extern __shared__ float di_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * DI_WAVES + wave;
    const bool bv = b < p.B;                                   // wave-uniform; every wave reaches the barrier
    const int ksteps = (p.N + 3) >> 2;
    const int pitch = 4 * ksteps + 1;
    float* S = di_lds + (size_t)wave * (16 * NT) * pitch;
    const float* g = p.d_out + (bv ? b : 0) * p.ld_dout + p.c0;
    for (int idx = lane; idx < 16 * NT * 4 * ksteps; idx += 64) {
        const int i = idx / (4 * ksteps), j = idx - i * (4 * ksteps);
        float v = 0.f;
        if (bv && i < p.N && j < p.N) {
            if (i != j) {
                const int hi = i > j ? i : j, lo = i > j ? j : i;
                v = g[di_tri(hi, p.self) + lo];
            } else if (p.self) {
                v = 2.f * g[di_tri(i, 1) + i];
            }
        }
        S[i * pitch + j] = v;
    }
    __syncthreads();
    if (!bv) return;
    const int hd = p.dense != nullptr;
    const int nblk = (p.D + 63) >> 6;
    for (int blk = 0; blk < nblk; ++blk) {
        const int d = 64 * blk + 4 * c;
        const bool dv = d < p.D;                               // D % 4 == 0: a float4 of columns is whole or absent
        dr_f32x4 acc[NT][4];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[ti][e] = (dr_f32x4){0.f, 0.f, 0.f, 0.f};
        auto load = [&](int ks) {                                // row 4 ks + q of T, columns d .. d + 3; zero beyond N and D
            const int k = 4 * ks + q;
            return (dv && k < p.N) ? *reinterpret_cast<const float4*>(di_row(p, b, k) + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        float4 t = load(0);
        for (int ks = 0; ks < ksteps; ++ks) {
            const float4 tn = load(ks + 1);                      // a k-step ahead (k >= N past the end: no access)
            const int k = 4 * ks + q;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                const float sv = S[(16 * ti + c) * pitch + k];  // A[i = lane & 15][k = q]
                acc[ti][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, t.x, acc[ti][0], 0, 0, 0);
                acc[ti][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, t.y, acc[ti][1], 0, 0, 0);
                acc[ti][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, t.z, acc[ti][2], 0, 0, 0);
                acc[ti][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, t.w, acc[ti][3], 0, 0, 0);
            }
            t = tn;
        }
        if (!dv) continue;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = 16 * ti + 4 * q + reg;           // C/D row; column tile e holds column d + e
                if (i >= p.N) continue;
                float4 v = make_float4(acc[ti][0][reg], acc[ti][1][reg], acc[ti][2][reg], acc[ti][3][reg]);
                if (hd && i == 0) {
                    const float* g0 = p.d_out + b * p.ld_dout + d;
                    v.x += g0[0]; v.y += g0[1]; v.z += g0[2]; v.w += g0[3];
                    *reinterpret_cast<float4*>(p.d_dense + b * p.ld_ddense + d) = v;
                } else {
                    *reinterpret_cast<float4*>(p.d_emb + b * p.ld_demb + (int64_t)(i - hd) * p.D + d) = v;
                }
            }
        }
    }
}

// fills the sizes; DR_OK, or DR_EINVAL outside the domain
int di_sizes(DiP& p, const float* dense, int64_t ld_dense, const float* emb, int64_t ld_emb, int64_t B, int32_t F, int32_t D,
             int32_t self) {
    if (B < 0 || F < 1 || D < 4 || D > DI_MAX_D || (D & 3) || (self != 0 && self != 1)) return DR_EINVAL;
    const int32_t N = F + (dense != nullptr ? 1 : 0);
    if (N < 2 || N > DI_MAX_N) return DR_EINVAL;
    if (dr_bad_ld(ld_emb, (int64_t)F * D)) return DR_EINVAL;
    if (dense != nullptr && dr_bad_ld(ld_dense, D)) return DR_EINVAL;
    p.dense = dense; p.ld_dense = ld_dense; p.emb = emb; p.ld_emb = ld_emb;
    p.B = B; p.F = F; p.D = D; p.N = N; p.self = self;
    p.c0 = dense != nullptr ? D : 0;
    p.P = self ? N * (N + 1) / 2 : N * (N - 1) / 2;
    return DR_OK;
}

}  // namespace

#define DI_DISPATCH(kernel, nt, grid, lds)                                                               \
    switch (nt) {                                                                                         \
        case 1: return dr_launch(kernel<1>, dim3((unsigned)(grid)), dim3(256), (lds), dr_s(stream), p);   \
        case 2: return dr_launch(kernel<2>, dim3((unsigned)(grid)), dim3(256), (lds), dr_s(stream), p);   \
        case 3: return dr_launch(kernel<3>, dim3((unsigned)(grid)), dim3(256), (lds), dr_s(stream), p);   \
        default: return dr_launch(kernel<4>, dim3((unsigned)(grid)), dim3(256), (lds), dr_s(stream), p);  \
    }

extern "C" int dr_dot_interact_fwd(const float* dense, int64_t ld_dense, const float* emb, int64_t ld_emb, int64_t B, int32_t F, int32_t D,
                                   int32_t self_interaction, float* out, int64_t ld_out, dr_stream_t stream) {
    DiP p = {};
    const int st = di_sizes(p, dense, ld_dense, emb, ld_emb, B, F, D, self_interaction);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_out, (int64_t)p.c0 + p.P)) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!emb || !out || !dr_aligned16(emb) || !dr_aligned16(dense)) return DR_EINVAL;
    const int64_t grid = (B + DI_WAVES - 1) / DI_WAVES;
    if (grid > 0x7fffffff) return DR_EINVAL;
    p.out = out; p.ld_out = ld_out;
    const int nt = (p.N + 15) / 16;
    DI_DISPATCH(dot_interact_fwd_kernel, nt, grid, 0);
}

extern "C" int dr_dot_interact_bwd(const float* dense, int64_t ld_dense, const float* emb, int64_t ld_emb, const float* d_out,
                                   int64_t ld_dout, int64_t B, int32_t F, int32_t D, int32_t self_interaction, float* d_dense,
                                   int64_t ld_ddense, float* d_emb, int64_t ld_demb, dr_stream_t stream) {
    DiP p = {};
    const int st = di_sizes(p, dense, ld_dense, emb, ld_emb, B, F, D, self_interaction);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_dout, (int64_t)p.c0 + p.P) || dr_bad_ld(ld_demb, (int64_t)F * D)) return DR_EINVAL;
    if (dense != nullptr && dr_bad_ld(ld_ddense, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!emb || !d_out || !d_emb || (dense != nullptr && !d_dense)) return DR_EINVAL;
    if (!dr_aligned16(emb) || !dr_aligned16(dense) || !dr_aligned16(d_emb) || (dense != nullptr && !dr_aligned16(d_dense))) return DR_EINVAL;
    const int64_t grid = (B + DI_WAVES - 1) / DI_WAVES;
    if (grid > 0x7fffffff) return DR_EINVAL;
    p.d_out = d_out; p.ld_dout = ld_dout; p.d_dense = d_dense; p.ld_ddense = ld_ddense; p.d_emb = d_emb; p.ld_demb = ld_demb;
    const int nt = (p.N + 15) / 16;
    // at most 4 x 64 x 65 floats = 65 KB: above the 64 KiB that need the opt-in for N >= 61 only, so NT = 4
    const size_t lds = (size_t)DI_WAVES * 16 * nt * (4 * ((p.N + 3) / 4) + 1) * sizeof(float);
    DI_DISPATCH(dot_interact_bwd_kernel, nt, grid, lds);
}
