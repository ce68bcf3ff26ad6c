// FFM's field-aware pairwise interaction (Juan et al., RecSys 2016), forward and backward, over gathered rows and straight from the table.
//
//   A [F, F, k] = the F rows of example b, row i = the feature of field i, block j of it (k floats) = its factor towards field j
//   inter[b]       = sum_{i = 1 .. F-1} sum_{j < i} sum_c A[i, j, c] A[j, i, c]
//   d_rows[i, j, :] = d_inter[b] A[j, i, :]  (j != i),  d_rows[i, i, :] = +0.0;  the diagonal blocks A[i, i, :] are never read
//
// Every off-diagonal element is used exactly once, so there is nothing to reuse and nothing to stage: the kernels are gather bandwidth.
// A GROUP OF G LANES OWNS ONE EXAMPLE (G = 64, a whole wave, from F = 12 up; 8, 16 or 32 for the small shapes, so that a block of 256
// holds 4 .. 32 examples): no sum crosses groups, there is no atomic, no LDS, no barrier, and an example's bits depend neither on the
// batch around it nor on its place in it.
//
// FORWARD   the example's work is T = P k / 4 items, item t = (pair p = t / (k / 4), chunk c = t % (k / 4)), pairs in the row-major order
//           of the lower triangle (p = i (i - 1) / 2 + j).  Lane l of the group takes the items l, l + G, l + 2 G ... : for each it loads
//           the float4 A[i, j, 4 c ..] (for consecutive t these run along row i: coalesced) and its partner A[j, i, 4 c ..] (one 16-byte
//           piece per row at stride F k floats: the other lanes' pieces of the same 128-byte lines are fetched by this very group a few
//           instructions apart, so the line is served by the cache the second time), and chains 4 fmaf per item into one accumulator.
//           Four items per lane are in flight before the first is consumed.  The G partial sums meet in an xor butterfly (G / 2 .. 1).
//           The order is a function of (F, k) alone, and the rows kernel and the gather kernel share this one body: given the same
//           operand bits they return the same bits.
// BACKWARD  item t of F F k / 4 is the float4 d_rows[t]: written in order (coalesced 16-byte stores), read from the partner block (the
//           strided side).  One correctly rounded multiply per element.
// GATHER    row i = table + (row_base[i] + ids[b, i]) F k; lane f < F of the group holds row f's index, the items fetch it by shuffle.  A
//           missing id (< 0) is a row of zeros: nothing is loaded for it and 0.0f takes the value's place in the same arithmetic, which is
//           what the rows path computes on K3's concat.  first_order = lin_bias + sum_f lin_w[row f], added in field order by one lane.
#include "dr_common.h"
#include <algorithm>

namespace {

constexpr int FFM_MAX_F = 64;
constexpr int FFM_MAX_K = 128;
constexpr int FFM_MAX_D = 256;        // F * k: the slab's row width
constexpr int FFM_U = 4;              // items a lane keeps in flight

struct FfmP {
    const float* rows; int64_t ld_rows;          // rows path: [B, F F k] at pitch ld_rows
    const int64_t* ids; const int64_t* row_base; // gather path: ids [B, F], row_base [F], table [R, F k]
    const float* table;
    const float* lin_w; const float* lin_bias;   // gather forward, all three may be NULL
    float* first_order;
    const float* d_inter;                        // backward
    float* inter;                                // forward
    float* d_rows; int64_t ld_d;                 // backward
    int64_t B;
    int32_t F, k, k4, D;                         // k4 = k / 4, D = F k
};

// the example's rows as the items address them: load(i, j * k + 4 c) is the float4 A[i, j, 4 c ..]
template <int G, bool GATHER>
struct FfmRows {
    const float* base;      // rows path
    const float* table;     // gather path
    int64_t my_row;         // gather path: lane f of the group holds row_base[f] + id (or -1)
    int32_t D;
    __device__ __forceinline__ float4 load(int i, int off_in_row) const {
        if constexpr (GATHER) {
            const int64_t r = __shfl(my_row, i, G);
            const float4 v = *reinterpret_cast<const float4*>(table + (r >= 0 ? r : 0) * D + off_in_row);   // row 0 stands in, unused
            return r >= 0 ? v : dr_zero4();
        } else {
            return *reinterpret_cast<const float4*>(base + (int64_t)i * D + off_in_row);
        }
    }
};

template <int G, bool GATHER>
__device__ __forceinline__ FfmRows<G, GATHER> ffm_rows(const FfmP& p, int64_t b, int gl, float* lw) {
    FfmRows<G, GATHER> r;
    r.D = p.D;
    r.base = nullptr; r.table = nullptr; r.my_row = -1;
    *lw = 0.f;
    if constexpr (GATHER) {
        r.table = p.table;
        if (gl < p.F) {                                        // G >= F: one lane per field
            const int64_t id = p.ids[b * p.F + gl];
            if (id >= 0) {
                r.my_row = p.row_base[gl] + id;
                if (p.lin_w != nullptr) *lw = p.lin_w[r.my_row];
            }
        }
    } else {
        r.base = p.rows + b * p.ld_rows;
    }
    return r;
}

// pair p -> (i, j), j < i, p = i (i - 1) / 2 + j; p <= 2015, where the float square root is off by at most one step
__device__ __forceinline__ void ffm_pair(int p, int& i, int& j) {
    i = (int)((1.f + sqrtf(1.f + 8.f * (float)p)) * 0.5f);
    if (i * (i - 1) / 2 > p) --i;
    if ((i + 1) * i / 2 <= p) ++i;
    j = p - i * (i - 1) / 2;
}

template <int G, bool GATHER>
__global__ __launch_bounds__(256) void ffm_fwd_kernel(const FfmP p) {
    constexpr int EPB = 256 / G;                               // examples per block
    const int gl = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * EPB + threadIdx.x / G;
    const bool bv = b0 < p.B;
    const int64_t b = bv ? b0 : p.B - 1;                       // a group past the end repeats the last example and stores nothing
    float lw;
    const FfmRows<G, GATHER> A = ffm_rows<G, GATHER>(p, b, gl, &lw);
    const int T = p.F * (p.F - 1) / 2 * p.k4;
    float acc = 0.f;
    for (int t0 = 0; t0 < T; t0 += G * FFM_U) {                // uniform over the block: T depends on (F, k) only
        float4 x[FFM_U], y[FFM_U];
#pragma unroll
        for (int u = 0; u < FFM_U; ++u) {
            const int t = t0 + u * G + gl;
            const bool tv = t < T;
            const int tc = tv ? t : T - 1;                     // clamped, not masked: every lane takes part in the shuffles
            const int pr = tc / p.k4, c = tc - pr * p.k4;
            int i, j;
            ffm_pair(pr, i, j);
            x[u] = A.load(i, j * p.k + 4 * c);
            y[u] = A.load(j, i * p.k + 4 * c);
            if (!tv) { x[u] = dr_zero4(); y[u] = dr_zero4(); }
        }
#pragma unroll
        for (int u = 0; u < FFM_U; ++u) {
            acc = fmaf(x[u].x, y[u].x, acc);
            acc = fmaf(x[u].y, y[u].y, acc);
            acc = fmaf(x[u].z, y[u].z, acc);
            acc = fmaf(x[u].w, y[u].w, acc);
        }
    }
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) acc += __shfl_xor(acc, m, G);
    float fo = 0.f;
    const bool want_fo = GATHER && p.first_order != nullptr && p.lin_w != nullptr;
    if (want_fo) {
        fo = p.lin_bias != nullptr ? p.lin_bias[0] : 0.f;
        for (int f = 0; f < p.F; ++f) fo += __shfl(lw, f, G);  // field order
    }
    if (bv && gl == 0) {
        p.inter[b] = acc;
        if (want_fo) p.first_order[b] = fo;
    }
}

template <int G, bool GATHER>
__global__ __launch_bounds__(256) void ffm_bwd_kernel(const FfmP p) {
    constexpr int EPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int64_t b0 = (int64_t)blockIdx.x * EPB + threadIdx.x / G;
    const bool bv = b0 < p.B;
    const int64_t b = bv ? b0 : p.B - 1;
    float lw;
    const FfmRows<G, GATHER> A = ffm_rows<G, GATHER>(p, b, gl, &lw);
    const float d = p.d_inter[b];
    float* out = p.d_rows + b * p.ld_d;
    const int Dk4 = p.F * p.k4;                                // float4s per row
    const int T = p.F * Dk4;
    for (int t0 = 0; t0 < T; t0 += G * FFM_U) {
        float4 y[FFM_U];
        bool diag[FFM_U];
#pragma unroll
        for (int u = 0; u < FFM_U; ++u) {
            const int t = t0 + u * G + gl;
            const int tc = t < T ? t : T - 1;
            const int i = tc / Dk4, rem = tc - i * Dk4;
            const int j = rem / p.k4, c = rem - j * p.k4;
            diag[u] = i == j;
            const int jr = diag[u] ? (i + 1 < p.F ? i + 1 : i - 1) : j;   // the diagonal block is not read: a neighbour's stands in, unused
            y[u] = A.load(jr, i * p.k + 4 * c);
        }
#pragma unroll
        for (int u = 0; u < FFM_U; ++u) {
            const int t = t0 + u * G + gl;
            const float4 g = diag[u] ? dr_zero4() : make_float4(d * y[u].x, d * y[u].y, d * y[u].z, d * y[u].w);
            if (bv && t < T) *reinterpret_cast<float4*>(out + 4 * t) = g;
        }
    }
}

// fills the sizes; DR_OK, or DR_EINVAL outside the domain
int ffm_sizes(FfmP& p, int64_t B, int32_t F, int32_t k) {
    if (B < 0 || F < 2 || F > FFM_MAX_F || k < 4 || k > FFM_MAX_K || (k & 3) || (int64_t)F * k > FFM_MAX_D) return DR_EINVAL;
    p.B = B; p.F = F; p.k = k; p.k4 = k >> 2; p.D = F * k;
    return DR_OK;
}

// lanes per example: a power of two that covers the fields (the gather keeps one row index per lane) and, up to a wave, the forward's items
int ffm_group(int32_t F, int32_t k) {
    const int need = std::max(F, F * (F - 1) / 2 * (k >> 2));
    return std::min(64, std::max(8, dr_pow2_ceil(need)));
}

}  // namespace

#define FFM_LAUNCH(kernel, gather)                                                                                     \
    {                                                                                                                  \
        const int g = ffm_group(p.F, p.k);                                                                             \
        const int64_t grid = (p.B + 256 / g - 1) / (256 / g);                                                          \
        if (grid > 0x7fffffff) return DR_EINVAL;                                                                       \
        switch (g) {                                                                                                   \
            case 8: return dr_launch(kernel<8, gather>, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), p);          \
            case 16: return dr_launch(kernel<16, gather>, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), p);        \
            case 32: return dr_launch(kernel<32, gather>, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), p);        \
            default: return dr_launch(kernel<64, gather>, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), p);        \
        }                                                                                                              \
    }

extern "C" int dr_ffm_fwd(const float* rows, int64_t ld_rows, int64_t B, int32_t F, int32_t k, float* inter, dr_stream_t stream) {
    FfmP p = {};
    const int st = ffm_sizes(p, B, F, k);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_rows, (int64_t)F * F * k)) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!rows || !inter || !dr_aligned16(rows)) return DR_EINVAL;
    p.rows = rows; p.ld_rows = ld_rows; p.inter = inter;
    FFM_LAUNCH(ffm_fwd_kernel, false)
}

extern "C" int dr_ffm_bwd(const float* rows, int64_t ld_rows, const float* d_inter, int64_t B, int32_t F, int32_t k, float* d_rows,
                          int64_t ld_d, dr_stream_t stream) {
    FfmP p = {};
    const int st = ffm_sizes(p, B, F, k);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_rows, (int64_t)F * F * k) || dr_bad_ld(ld_d, (int64_t)F * F * k)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!rows || !d_inter || !d_rows || !dr_aligned16(rows) || !dr_aligned16(d_rows)) return DR_EINVAL;
    p.rows = rows; p.ld_rows = ld_rows; p.d_inter = d_inter; p.d_rows = d_rows; p.ld_d = ld_d;
    FFM_LAUNCH(ffm_bwd_kernel, false)
}

extern "C" int dr_ffm_gather_fwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t k,
                                 const float* lin_w, const float* lin_bias, float* inter, float* first_order, dr_stream_t stream) {
    FfmP p = {};
    const int st = ffm_sizes(p, B, F, k);
    if (st != DR_OK) return st;
    if (B == 0) return DR_OK;
    if (!ids || !row_base || !table || !inter || !dr_aligned16(table)) return DR_EINVAL;
    p.ids = ids; p.row_base = row_base; p.table = table; p.lin_w = lin_w; p.lin_bias = lin_bias; p.inter = inter;
    p.first_order = first_order;
    FFM_LAUNCH(ffm_fwd_kernel, true)
}

extern "C" int dr_ffm_gather_bwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t k,
                                 const float* d_inter, float* d_rows, int64_t ld_d, dr_stream_t stream) {
    FfmP p = {};
    const int st = ffm_sizes(p, B, F, k);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_d, (int64_t)F * F * k)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!ids || !row_base || !table || !d_inter || !d_rows || !dr_aligned16(table) || !dr_aligned16(d_rows)) return DR_EINVAL;
    p.ids = ids; p.row_base = row_base; p.table = table; p.d_inter = d_inter; p.d_rows = d_rows; p.ld_d = ld_d;
    FFM_LAUNCH(ffm_bwd_kernel, true)
}
