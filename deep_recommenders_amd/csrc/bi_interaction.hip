// NFM's Bi-Interaction pooling (He & Chua, SIGIR 2017), forward and backward, over gathered rows and straight from the table.
//
//   e_f = field f's row (D floats),  s = sum_f e_f,  q = sum_f e_f * e_f
//   out[b, :]       = 0.5 (s * s - q)                       the pairwise sum sum_{i < j} e_i * e_j, a VECTOR: K3 only keeps its sum over d
//   d_rows[b, f, :] = d_out[b, :] * (s - e_f)               s is recomputed in the backward, nothing is saved
//
// Every row is read once (twice in the backward) and every column is independent, so the kernels are gather bandwidth.  A GROUP OF
// D / 4 LANES OWNS ONE EXAMPLE: lane l keeps the float4 at column 4 l of s and q in registers and walks the fields in ascending
// order, BI_U rows in flight before the first is consumed.  No LDS, no atomics, no workspace, no cross-lane arithmetic: the order is a
// function of (F, D) alone, results are bit-identical from run to run and an example's bits depend neither on its batch nor on its
// place in it.  The rows kernels and the gather kernels share one body: given the same operand bits they return the same bits.
//
// s * s and q are each rounded before they are subtracted (no contraction across the difference): with F = 1 both are the same
// rounded square and out is exactly +0.0.
// GATHER  row f = table + (row_base[f] + ids[b, f]) D.  A missing id (< 0) is a row of zeros: nothing is loaded for it and 0.0f takes
//         the value's place in the same arithmetic, which is what the rows path computes on K3's concat.  first_order = lin_bias +
//         sum_f lin_w[row f], added in field order by the group's first lane.
#include "dr_common.h"

namespace {

constexpr int BI_MAX_F = 1024;
constexpr int BI_MAX_D = 256;
constexpr int BI_U = 8;               // rows a lane keeps in flight

struct BiP {
    const float* rows; int64_t ld_rows;          // rows path: [B, F D] at pitch ld_rows
    const int64_t* ids; const int64_t* row_base; // gather path: ids [B, F], row_base [F], table [R, D]
    const float* table;
    const float* lin_w; const float* lin_bias;   // gather forward, all three may be NULL
    float* first_order;
    const float* d_out; int64_t ld_do;           // backward
    float* out; int64_t ld_out;                  // forward
    float* d_rows; int64_t ld_d;                 // backward
    int64_t B;
    int32_t F, D, L, epb;                        // L = D / 4 lanes per example, epb = 256 / L examples per block
};

// the float4 at column 4 l of the example's rows f0 .. f0 + BI_U - 1 (those below F), all loads issued before any is used
template <bool GATHER>
struct BiRows {
    const float* base;      // rows path: the example's first row + 4 l;  gather path: table + 4 l
    const int64_t* ids;     // gather path: the example's ids
    const int64_t* row_base;
    int32_t D, F;
    __device__ __forceinline__ void load(int f0, float4 (&e)[BI_U], int64_t (&r)[BI_U]) const {
        if constexpr (GATHER) {
#pragma unroll
            for (int u = 0; u < BI_U; ++u) {
                r[u] = -1;
                if (f0 + u < F) {
                    const int64_t id = ids[f0 + u];
                    r[u] = id >= 0 ? row_base[f0 + u] + id : -1;
                }
            }
#pragma unroll
            for (int u = 0; u < BI_U; ++u)
                e[u] = r[u] >= 0 ? *reinterpret_cast<const float4*>(base + r[u] * D) : dr_zero4();
        } else {
#pragma unroll
            for (int u = 0; u < BI_U; ++u) {
                r[u] = f0 + u;
                e[u] = f0 + u < F ? *reinterpret_cast<const float4*>(base + (int64_t)(f0 + u) * D) : dr_zero4();
            }
        }
    }
};

template <bool GATHER>
__device__ __forceinline__ BiRows<GATHER> bi_rows(const BiP& p, int64_t b, int l) {
    BiRows<GATHER> A;
    A.D = p.D; A.F = p.F; A.ids = nullptr; A.row_base = nullptr;
    if constexpr (GATHER) {
        A.base = p.table + 4 * l;
        A.ids = p.ids + b * p.F;
        A.row_base = p.row_base;
    } else {
        A.base = p.rows + b * p.ld_rows + 4 * l;
    }
    return A;
}

// s = sum_f e_f in ascending field order (and q = sum_f e_f e_f when WANT_Q)
template <bool GATHER, bool WANT_Q>
__device__ __forceinline__ void bi_sums(const BiRows<GATHER>& A, float4& s, float4& q, const float* lin_w, float& fo) {
    s = dr_zero4(); q = dr_zero4();
    for (int f0 = 0; f0 < A.F; f0 += BI_U) {                   // uniform over the block
        float4 e[BI_U];
        int64_t r[BI_U];
        A.load(f0, e, r);
        if constexpr (GATHER && WANT_Q) {
            if (lin_w != nullptr) {
#pragma unroll
                for (int u = 0; u < BI_U; ++u)
                    if (f0 + u < A.F && r[u] >= 0) fo += lin_w[r[u]];      // field order, missing ids skipped
            }
        }
#pragma unroll
        for (int u = 0; u < BI_U; ++u) {
            if (f0 + u < A.F) {
                s.x += e[u].x; s.y += e[u].y; s.z += e[u].z; s.w += e[u].w;
                if constexpr (WANT_Q) {
                    q.x = fmaf(e[u].x, e[u].x, q.x); q.y = fmaf(e[u].y, e[u].y, q.y);
                    q.z = fmaf(e[u].z, e[u].z, q.z); q.w = fmaf(e[u].w, e[u].w, q.w);
                }
            }
        }
    }
}

template <bool GATHER>
__global__ __launch_bounds__(256) void bi_fwd_kernel(const BiP p) {
#pragma clang fp contract(off)
    const int g = threadIdx.x / p.L, l = threadIdx.x - g * p.L;
    const int64_t b = (int64_t)blockIdx.x * p.epb + g;
    if (g >= p.epb || b >= p.B) return;                        // no lane of another group is waited for
    const BiRows<GATHER> A = bi_rows<GATHER>(p, b, l);
    const bool want_fo = GATHER && p.first_order != nullptr && p.lin_w != nullptr && l == 0;
    float4 s, q;
    float fo = want_fo && p.lin_bias != nullptr ? p.lin_bias[0] : 0.f;
    bi_sums<GATHER, true>(A, s, q, want_fo ? p.lin_w : nullptr, fo);
    float4 o;
    const float sx = s.x * s.x, sy = s.y * s.y, sz = s.z * s.z, sw = s.w * s.w;      // rounded, then subtracted
    o.x = 0.5f * (sx - q.x); o.y = 0.5f * (sy - q.y); o.z = 0.5f * (sz - q.z); o.w = 0.5f * (sw - q.w);
    *reinterpret_cast<float4*>(p.out + b * p.ld_out + 4 * l) = o;
    if (want_fo) p.first_order[b] = fo;
}

template <bool GATHER>
__global__ __launch_bounds__(256) void bi_bwd_kernel(const BiP p) {
#pragma clang fp contract(off)
    const int g = threadIdx.x / p.L, l = threadIdx.x - g * p.L;
    const int64_t b = (int64_t)blockIdx.x * p.epb + g;
    if (g >= p.epb || b >= p.B) return;
    const BiRows<GATHER> A = bi_rows<GATHER>(p, b, l);
    const float4 d = *reinterpret_cast<const float4*>(p.d_out + b * p.ld_do + 4 * l);
    float4 s, q;
    float fo = 0.f;
    bi_sums<GATHER, false>(A, s, q, nullptr, fo);
    float* dst = p.d_rows + b * p.ld_d + 4 * l;
    for (int f0 = 0; f0 < p.F; f0 += BI_U) {
        float4 e[BI_U];
        int64_t r[BI_U];
        A.load(f0, e, r);                                      // the second read of the rows: this group's own lines, a few microseconds old
#pragma unroll
        for (int u = 0; u < BI_U; ++u) {
            if (f0 + u < p.F) {
                const float4 gr = make_float4(d.x * (s.x - e[u].x), d.y * (s.y - e[u].y), d.z * (s.z - e[u].z), d.w * (s.w - e[u].w));
                *reinterpret_cast<float4*>(dst + (int64_t)(f0 + u) * p.D) = gr;
            }
        }
    }
}

// fills the sizes; DR_OK, or DR_EINVAL / DR_ESHAPE outside the domain
int bi_sizes(BiP& p, int64_t B, int32_t F, int32_t D) {
    if (B < 0 || F < 1 || F > BI_MAX_F) return DR_EINVAL;
    if (D < 4 || D > BI_MAX_D || (D & 3)) return DR_ESHAPE;
    p.B = B; p.F = F; p.D = D; p.L = D >> 2; p.epb = 256 / p.L;
    return DR_OK;
}

template <typename K>
int bi_launch(K kernel, const BiP& p, dr_stream_t stream) {
    const int64_t grid = (p.B + p.epb - 1) / p.epb;
    if (grid > 0x7fffffff) return DR_EINVAL;
    return dr_launch(kernel, dim3((unsigned)grid), dim3(256), 0, dr_s(stream), p);
}

}  // namespace

extern "C" int dr_bi_interact_fwd(const float* rows, int64_t ld_rows, int64_t B, int32_t F, int32_t D, float* out, int64_t ld_out,
                                  dr_stream_t stream) {
    BiP p = {};
    const int st = bi_sizes(p, B, F, D);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_rows, (int64_t)F * D) || dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;                                  // nothing to read or write: empty tensors have no address
    if (!rows || !out || !dr_aligned16(rows) || !dr_aligned16(out)) return DR_EINVAL;
    p.rows = rows; p.ld_rows = ld_rows; p.out = out; p.ld_out = ld_out;
    return bi_launch(bi_fwd_kernel<false>, p, stream);
}

extern "C" int dr_bi_interact_bwd(const float* rows, int64_t ld_rows, const float* d_out, int64_t ld_do, int64_t B, int32_t F,
                                  int32_t D, float* d_rows, int64_t ld_d, dr_stream_t stream) {
    BiP p = {};
    const int st = bi_sizes(p, B, F, D);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_rows, (int64_t)F * D) || dr_bad_ld(ld_do, D) || dr_bad_ld(ld_d, (int64_t)F * D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!rows || !d_out || !d_rows || !dr_aligned16(rows) || !dr_aligned16(d_out) || !dr_aligned16(d_rows)) return DR_EINVAL;
    p.rows = rows; p.ld_rows = ld_rows; p.d_out = d_out; p.ld_do = ld_do; p.d_rows = d_rows; p.ld_d = ld_d;
    return bi_launch(bi_bwd_kernel<false>, p, stream);
}

extern "C" int dr_bi_interact_gather_fwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table,
                                         int32_t D, const float* lin_w, const float* lin_bias, float* out, int64_t ld_out,
                                         float* first_order, dr_stream_t stream) {
    BiP p = {};
    const int st = bi_sizes(p, B, F, D);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_out, D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!ids || !row_base || !table || !out || !dr_aligned16(table) || !dr_aligned16(out)) return DR_EINVAL;
    p.ids = ids; p.row_base = row_base; p.table = table; p.lin_w = lin_w; p.lin_bias = lin_bias; p.out = out; p.ld_out = ld_out;
    p.first_order = first_order;
    return bi_launch(bi_fwd_kernel<true>, p, stream);
}

extern "C" int dr_bi_interact_gather_bwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table,
                                         int32_t D, const float* d_out, int64_t ld_do, float* d_rows, int64_t ld_d,
                                         dr_stream_t stream) {
    BiP p = {};
    const int st = bi_sizes(p, B, F, D);
    if (st != DR_OK) return st;
    if (dr_bad_ld(ld_do, D) || dr_bad_ld(ld_d, (int64_t)F * D)) return DR_EINVAL;
    if (B == 0) return DR_OK;
    if (!ids || !row_base || !table || !d_out || !d_rows || !dr_aligned16(table) || !dr_aligned16(d_out) || !dr_aligned16(d_rows))
        return DR_EINVAL;
    p.ids = ids; p.row_base = row_base; p.table = table; p.d_out = d_out; p.ld_do = ld_do; p.d_rows = d_rows; p.ld_d = ld_d;
    return bi_launch(bi_bwd_kernel<true>, p, stream);
}
