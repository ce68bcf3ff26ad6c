// =====================================================================================================================
// Fused first layer of the DeepFM / DCN tower:  hash ids -> [gather + stack/concat + first-order + FM second-order] -> Dense.
// The register-split GEMM (bf3_gemm.hip's bf3_gemm_rs_kernel and its tile: 256 x 256 x 32, 8 waves x 32 rows, weights pre-split in an LDS ring) whose
// activation operand is GATHERED: k-tile kt of example b is dims 32 (kt & 1) .. + 31 of table row row_base[f] + ids[b][f],
// f = kt >> 1 (D == 64) -- the same 128-byte lines K3 (dr_emb_pool_fwd) reads -- so the kernel that multiplies the concatenated
// embeddings by the first Dense kernel is also the one that fetches them.  On their way through the CU the values are (1) stored
// to `concat` (the backward kernels read it) and (2) summed into the FM terms K3 produced (sum_x, sum of squares, first-order
// weights): keras/models/ranking/fm.py:23-37 and deepfm.py:36-47 of the reference in ONE launch with deepfm.py:30-34's first
// Dense.  K3's 0.9 GB of HBM traffic moves in the shadow of an MFMA-bound kernel instead of in a 220 us kernel of its own.
//
// How the rows travel (what the first two versions of this kernel taught):
//   * A load in which every lane addresses its own row costs the CU's address path one request per LANE: 256 per wave and
//     k-tile for the row loads, as many again for the concat stores.  With ids and first-order weights on top the REQUEST rate
//     -- not HBM, not the matrix pipe -- set the pace: 437 us (273 for the plain GEMM + 218 for K3 = 491), and 488 us with an
//     L2 prefetch added (+128 requests per wave and k-tile => +0.9 us per k-tile).
//   * So the rows are fetched by LDS-DMA, 8 lanes x 16 bytes per 128-byte line (8 requests per instruction, 32 per wave and
//     k-tile), two k-tiles ahead, into a wave-private 2 x 4 KB LDS image -- no destination VGPRs, which is what allows the
//     two-step lead.  Each field is addressed as a STRUCTURED buffer (base = its first row, index = bucket id, stride 256 B;
//     buffer offsets are 32 bits wide, so a field may have 2^24 rows).  The image is XOR-swizzled by the choice of which (row, chunk) each DMA lane fetches
//     (chunk c of row r at position c ^ (r & 7) ^ ((r >> 4) & 1), emb_a_swizzle in bf3_rs_core.h), so that both readers are
//     conflict-free: the MFMA-operand read (lane = row, 4 x ds_read_b128, served in the lane groups {0-3, 12-15, 20-27} and
//     {4-11, 16-19, 28-31} of each half wave: the eight rows of one parity in a group need eight distinct swizzle values, which
//     r & 7 alone does not give -- rows 12 and 20 share it; bf3_rs_core.h proves the image at compile time) and the position-wise
//     read that feeds the COALESCED concat stores (8 lanes per 128-byte line again; lane-linear).
//   * LDS: 2 x 48 KB weight stages + 2 x 32 KB activation stages = all 160 KB.  The weight pieces of k-tile s + 1 are issued first
//     in step s, the gather of s + 2 and the id / weight loads after them, so the one counted wait per step (vmcnt(10) in front
//     of the barrier) covers exactly the pieces and leaves the younger gather in flight.
// Single-valued fields, D == 64, at most 32 dense features (one more k-tile, read from `dense_pad` [M, 32], zero-padded; the
// caller also places them in concat[:, 64 F : K) for the backward).  Any N works: only the first column tile of a row panel
// stores the side outputs.
// =====================================================================================================================
// Cache-policy experiment (round 4): a stream that is read / written ONCE marked nontemporal so that it does not wash the weight
// planes (and, in K4, the first-order lines) out of the L2 / Infinity Cache.  0 = default policy, 1 = nontemporal.
#ifndef DR_NT_FWD_GATHER
#define DR_NT_FWD_GATHER 1
#endif
#include "bf3_rs_core.h"
#include "tower_tail_core.h"

namespace {

using namespace drrs;

struct EmbArgs {
    const int64_t* ids; int32_t F;               // [M, F] bucket ids (-1 = missing -> zero embedding, no first-order term)
    const int64_t* row_base;                     // [F] first row of each field in the slab
    const float* table;                          // [R, 64]
    const float* lin_w; const float* lin_bias;   // first-order weights [R] / bias [1] (may be null)
    const float* dense_pad;                      // [M, 32] dense features, zero-padded (null when K == 64 F)
    float* concat; int64_t ld_concat;            // out: [M, ld], columns [0, 64 F)
    float* sum_x; float* fm_logit;               // out: [M, 64], [M]
    float* lin_vals;                             // out (may be null): [F, M] field-major, the first-order weight every slot read -- K4
                                                 // then only WRITES lin_w[row] (one line operation per slot instead of two; round 4)
    const uint32_t* dense_amax;                  // f16x2 mode: amax record of dense_pad (null: none); the table's is RsArgs::a_amax
};

// The tower tail as the epilogue of this kernel (TAIL instantiation; N == 256 == one column tile, so a wave ends the main loop with
// complete rows of h0 in its accumulators): Dense(H <= 32, relu) + Dense(1) + fm_logit, the loss, and the backward of both layers
// down to d h0 -- the steps of tower_tail_fused_kernel (tower_tail.hip) on registers, h0 itself never written unless RsArgs::C is set.
struct FwdTailArgs {
    const float* W1; int64_t ldw1; const float* b1; int32_t H;   // [256, H]
    const float* w2; int64_t ld_w2; const float* b2;
    const float* labels; int32_t loss_mode; float inv_n;
    float* prob; float* d_logit; float* d_h; int64_t ld_dh;      // d_h may be null
    float* dx; int64_t lddx;                                     // d h0 [M, 256]
    float* partial;                                              // [grid][(256 + 1) * 32]   (tower_tail_reduce_kernel's layouts)
    float* head_partial;                                         // [grid][34]
    uint32_t* amax_part;                                         // [grid]: every block's max |dx| as float bits
    uint32_t* dx_amax;                                           // (may be null) the record, raised with atomicMax: part 1 without the reduce
};

// the tail kernel's kernarg segment (explicit arguments in order, each at its natural alignment): its epilogue reads `t` from there
struct FwdTailKernargs { RsArgs g; EmbArgs e; FwdTailArgs t; };

__device__ __forceinline__ int sload_i32(const void* base, int byte_off) {      // scalar load of a wave-uniform word, on the spot
    int v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "s"(byte_off) : "memory");
    return v;
}

// H2: the f16x2 operand mode (h2_split8): two fp16 weight planes (32 KB stages, 4 pieces per wave and k-tile), three MFMAs per
// fragment pair; the activation scale comes from the larger of the table's and the dense features' amax records.
//
// TAIL: the tower-tail epilogue (FwdTailArgs).  That kernel is launched with ONE tile per block (grid = row panels, not capped at the CU
// count): nothing of a next tile is in flight while the epilogue uses the LDS, and a block's partials are its tile's.  Past 256 row
// panels that costs one pipeline refill per tile; the bench shape (one tile per CU) nothing.
template <int H2>
__global__ __launch_bounds__(512, 2) void bf3_emb_linear_kernel(RsArgs g, EmbArgs e) {
    constexpr int TAIL = 0;
    [[maybe_unused]] const FwdTailArgs tk{};                            // (the shared body names it; only the tail kernel has one)
#include "bf3_emb_linear_body.h"
}

template <int H2>
__global__ __launch_bounds__(512, 2) void bf3_emb_linear_tail_kernel(RsArgs g, EmbArgs e, FwdTailArgs tk) {
    constexpr int TAIL = 1;
#include "bf3_emb_linear_body.h"
}

}  // namespace

// Fused K3 + first Dense layer (see bf3_emb_linear_kernel): h[m][n] = act(sum_k x[m][k] W[k][n] + bias[n]) with
// x = concat(field embeddings of ids[m], dense features = dense_pad[m, : K - 64 F]); also writes concat[:, : 64 F],
// sum_x [M, 64] and fm_logit [M] = lin_bias + sum_f lin_w[row] + 0.5 sum_d ((sum_f x_fd)^2 - sum_f x_fd^2).
static int emb_linear_fwd_impl(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                               const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad, float* concat,
                               int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride, int64_t ld_planes, int32_t N,
                               const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                               float* lin_vals_t, dr_stream_t stream, const uint32_t* table_amax = nullptr,
                               const uint32_t* dense_amax = nullptr, const uint32_t* w_amax = nullptr, const FwdTailArgs* tail = nullptr) {
    if (M < 0 || M > 0x7fffff00 || F <= 0 || N <= 0 || K < 64 * F || act < 0 || act > 1) return DR_EINVAL;
    // the k-tile <-> (field, half row) map is built for 64-wide rows; the dense features are one k-tile; a field is one 4 GB buffer
    if (D != 64 || K > 64 * F + 32 || field_rows_max <= 0 || field_rows_max > (1 << 24)) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    // concat may be NULL: nothing then stores the gathered embeddings (the wgrad gathers them itself, dr_bf3_wgrad_emb)
    if (!ids || !row_base || !table || !sum_x || !fm_logit || (!out && !tail) || !planes_ok(wt_planes, plane_stride, ld_planes))
        return DR_EINVAL;
    if (K > 64 * F && (!dense_pad || (reinterpret_cast<uintptr_t>(dense_pad) & 15) != 0)) return DR_EINVAL;
    if ((concat != nullptr && ((reinterpret_cast<uintptr_t>(concat) & 15) != 0 || (ld_concat & 3) != 0 || ld_concat < K)) ||
        (reinterpret_cast<uintptr_t>(table) & 15) != 0 || (reinterpret_cast<uintptr_t>(sum_x) & 15) != 0)
        return DR_EINVAL;
    if (ld_planes < (K + BK - 1) / BK * BK || (out != nullptr && ld_out < N)) return DR_EINVAL;
    RsArgs g{nullptr, 0, static_cast<const __bf16*>(wt_planes), plane_stride, ld_planes, M, N, K, out, ld_out, bias, act, nullptr, 0, 0,
             nullptr, nullptr, 0, 0.f, nullptr};
    EmbArgs e{ids, F, row_base, table, lin_w, lin_bias, K > 64 * F ? dense_pad : nullptr, concat, ld_concat, sum_x, fm_logit,
              lin_w != nullptr ? lin_vals_t : nullptr, K > 64 * F ? dense_amax : nullptr};
    const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
    if (tiles > 0x7fffffff) return DR_EINVAL;
    const int grid = tail != nullptr ? (int)tiles : (int)(tiles < 256 ? tiles : 256);
    if (table_amax != nullptr) {                                        // f16x2 operand mode
        if (!w_amax || (K > 64 * F && !dense_amax)) return DR_EINVAL;
        g.a_amax = table_amax;
        g.b_amax = w_amax;
        if (tail != nullptr) {
            if (tail->dx_amax != nullptr && hipMemsetAsync(tail->dx_amax, 0, sizeof(uint32_t), dr_s(stream)) != hipSuccess) return DR_ELAUNCH;
            hipLaunchKernelGGL(bf3_emb_linear_tail_kernel<1>, dim3(grid), dim3(512), 0, dr_s(stream), g, e, *tail);
        } else hipLaunchKernelGGL(bf3_emb_linear_kernel<1>, dim3(grid), dim3(512), 0, dr_s(stream), g, e);
    } else {
        hipLaunchKernelGGL(bf3_emb_linear_kernel<0>, dim3(grid), dim3(512), 0, dr_s(stream), g, e);
    }
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// lin_vals_t [F, M] field-major (may be NULL): also saves the first-order weight of every slot as it was read (lin_vals_t[f * M + m] =
// lin_w[row_base[f] + ids[m, f]]; undefined for a missing id).  dr_emb_pool_bwd_sorted takes it as `lin_old_t`: the backward then
// updates a unique row's first-order weight with ONE write instead of a read-modify-write of a line it would have to fetch again.
extern "C" int dr_bf3_emb_linear_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                                     const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad,
                                     float* concat, int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride,
                                     int64_t ld_planes, int32_t N, const float* bias, int32_t act, float* sum_x, float* fm_logit,
                                     float* out, int64_t ld_out, float* lin_vals_t, dr_stream_t stream) {
    return emb_linear_fwd_impl(ids, M, F, row_base, field_rows_max, table, D, lin_w, lin_bias, dense_pad, concat, ld_concat, K, wt_planes,
                               plane_stride, ld_planes, N, bias, act, sum_x, fm_logit, out, ld_out, lin_vals_t, stream);
}

// dr_bf3_emb_linear_fwd in the f16x2 operand mode: wt_planes = two fp16 planes (dr_h2_split with w_amax); table_amax >= the largest
// magnitude in `table` (the engine keeps it as a running maximum: dr_h2_amax over the table once, K4 afterwards); dense_amax = the
// record of dense_pad (required iff K > 64 F).  lin_vals_t may be NULL.
extern "C" int dr_h2_emb_linear_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                                    const float* table, int32_t D, const uint32_t* table_amax, const float* lin_w, const float* lin_bias,
                                    const float* dense_pad, const uint32_t* dense_amax, float* concat, int64_t ld_concat, int32_t K,
                                    const void* wt_planes, int64_t plane_stride, int64_t ld_planes, const uint32_t* w_amax, int32_t N,
                                    const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                                    float* lin_vals_t, dr_stream_t stream) {
    if (!table_amax || !w_amax) return DR_EINVAL;
    return emb_linear_fwd_impl(ids, M, F, row_base, field_rows_max, table, D, lin_w, lin_bias, dense_pad, concat, ld_concat, K, wt_planes,
                               plane_stride, ld_planes, N, bias, act, sum_x, fm_logit, out, ld_out, lin_vals_t, stream, table_amax,
                               dense_amax, w_amax);
}

// ---- dr_h2_emb_linear_fwd with the tower tail as its epilogue (bf3_emb_linear_tail_kernel) ---------------------------------------
static int fwd_tail_grid(int64_t M) { return (int)((M + 255) / 256); }     // one tile per block

extern "C" int64_t dr_h2_emb_linear_tail_fwd_workspace_bytes(int64_t M) {
    if (M <= 0) return 512;
    return (int64_t)fwd_tail_grid(M) * ((int64_t)(256 + 1) * 32 + drtail::TAIL_HEAD_PART + 1) * (int64_t)sizeof(float);
}

// dr_h2_emb_linear_fwd followed by dr_tower_tail_fused (extra_logit = fm_logit, n_total = M) on its output, in ONE kernel plus the
// tail's reduce: h0 = act(x W0 + bias) stays in the accumulators (`out` may be NULL: it is then never written), and the kernel leaves
// prob, d_logit, d_h (may be NULL), dx = d h0 and per-block partials; parts & 2 launches the reduce that applies
// dst_* += scale * gradient and writes loss_out.  dx_amax (may be NULL) receives max |dx| as float bits: with parts == 3 the reduce stores
// it from the blocks' maxima; with parts == 1 it is reset in front of the kernel and raised by it (as dr_tower_tail_fused does).
// Row-wise outputs are the bits the two calls give; the four weight steps and the loss are the same fixed-order fp32 sums grouped by
// this kernel's blocks.  Domain: N == 256 (one column tile), H <= 32, M a positive multiple of 32, and dr_h2_emb_linear_fwd's own
// (D == 64, K <= 64 F + 32, field_rows_max <= 2^24); DR_ESHAPE outside it, nothing launched.
extern "C" int dr_h2_emb_linear_tail_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                                         const float* table, int32_t D, const uint32_t* table_amax, const float* lin_w,
                                         const float* lin_bias, const float* dense_pad, const uint32_t* dense_amax, float* concat,
                                         int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride, int64_t ld_planes,
                                         const uint32_t* w_amax, int32_t N, const float* bias, int32_t act, float* sum_x, float* fm_logit,
                                         float* out, int64_t ld_out, float* lin_vals_t, const float* W1, int64_t ld_w1, const float* b1,
                                         int32_t H, const float* w2, int64_t ld_w2, const float* b2, const float* labels, int32_t loss_mode,
                                         float scale, float* dst_w1, int64_t ld_dst_w1, float* dst_b1, float* dst_w2, int64_t ld_dst_w2,
                                         float* dst_b2, float* prob, float* d_logit, float* d_h, int64_t ld_dh, float* dx, int64_t ld_dx,
                                         float* loss_out, void* workspace, int64_t workspace_bytes, int32_t parts, uint32_t* dx_amax,
                                         dr_stream_t stream) {
    if (M <= 0 || H <= 0 || parts < 1 || parts > 3 || loss_mode < 0 || loss_mode > 2) return DR_EINVAL;
    if (!table_amax || !w_amax || !W1 || !w2 || !labels || !dst_w1 || !prob || !d_logit || !dx || !workspace) return DR_EINVAL;
    if (N != 256 || H > 32 || (M % 32) != 0) return DR_ESHAPE;
    if (ld_w1 < H || ld_dst_w1 < H || ld_w2 < 1 || (dst_w2 && ld_dst_w2 < 1) || (d_h && ld_dh < H) || ld_dx < N) return DR_EINVAL;
    if (workspace_bytes < dr_h2_emb_linear_tail_fwd_workspace_bytes(M)) return DR_EINVAL;
    const int grid = fwd_tail_grid(M);
    float* partial = static_cast<float*>(workspace);
    float* head_partial = partial + (int64_t)grid * (N + 1) * 32;
    uint32_t* amax_part = reinterpret_cast<uint32_t*>(head_partial + (int64_t)grid * drtail::TAIL_HEAD_PART);
    const float inv_n = 1.f / (float)M;
    if (parts & 1) {
        uint32_t* const rec = parts == 1 ? dx_amax : nullptr;
        const FwdTailArgs t{W1, ld_w1, b1, H, w2, ld_w2, b2, labels, loss_mode, inv_n, prob, d_logit, d_h, ld_dh, dx, ld_dx,
                            partial, head_partial, amax_part, rec};
        const int rc = emb_linear_fwd_impl(ids, M, F, row_base, field_rows_max, table, D, lin_w, lin_bias, dense_pad, concat, ld_concat, K,
                                           wt_planes, plane_stride, ld_planes, N, bias, act, sum_x, fm_logit, out, ld_out, lin_vals_t, stream,
                                           table_amax, dense_amax, w_amax, &t);
        if (rc != DR_OK) return rc;
    }
    if (parts & 2)
        return drtail::launch_reduce(partial, head_partial, grid, N, H, scale, inv_n, dst_w1, ld_dst_w1, dst_b1, dst_w2, ld_dst_w2, dst_b2,
                                     loss_out, (dx_amax != nullptr && parts == 3) ? amax_part : nullptr, dx_amax, stream);
    return DR_OK;
}
