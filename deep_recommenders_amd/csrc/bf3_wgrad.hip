// =====================================================================================================================
// TN, "register split" wgrad:  dst[f][n] += scale * sum_r X[r][f] Y[r][n],  dstb[n] += scale * sum_r Y[r][n]
// Both operands are fp32 ACTIVATIONS, reduction-major (x [R, F] and dy [R, N] as their producers write them); nothing is
// pre-split.  A block owns a 256 (f) x 256 (n) tile of one reduction slice; each of its 8 waves owns 32 f x all 256 n.
//   A (x):  every lane loads the 16 reduction elements of ITS column f for a k-tile with 16 dword loads (the 32 lanes of a half
//           wave cover 128 contiguous bytes of one row) and splits them in registers -- the transposition MFMA's A operand
//           needs ("8 consecutive k per lane") is free because the lane index runs along f.
//   B (dy): the same loads with the lane index along n give every lane 8 consecutive r of its column, i.e. exactly one
//           16-byte fragment chunk per plane: wave w splits the 32 columns 32 w .. 32 w + 31 of the tile once and writes the
//           three planes as ds_write_b128 into the [n][32 r] image the fragment reads of the NT kernels use (with a swizzle of
//           its own, tn_img_swizzle: the 8 consecutive rows of a store's lane group must be spread too); the 8 waves' pieces
//           make the tile that all of them read.  Two LDS stages: step g's MFMAs read stage g while stage g + 1 is
//           written from registers loaded during step g - 1.
// The in-kernel-split wgrad of dense.hip (the kernel template of gemm_f32_core.h) re-stages BOTH operands through the LDS per 128 x 128 tile; here x never touches
// it and each dy element is split once per 256 rows of x.
// Partials go to a padded workspace [split][tiles_f * 256][tiles_n * 256] (+ [split][tiles_n * 256] column sums): every store of
// the epilogue is unconditional; a fixed-order reduce applies them (deterministic).
// =====================================================================================================================
// Cache-policy experiment (round 4): a stream that is read / written ONCE marked nontemporal so that it does not wash the weight
// planes (and, in K4, the first-order lines) out of the L2 / Infinity Cache.  0 = default policy, 1 = nontemporal.
#ifndef DR_NT_WGRAD_GATHER
#define DR_NT_WGRAD_GATHER 0
#endif
#include "bf3_rs_core.h"
#include "tn_rs_reduce.h"

namespace {

using namespace drrs;

struct TnRsArgs {
    const float* X; int64_t ldx;
    const float* Y; int64_t ldy;
    int64_t R; int32_t F; int32_t N;
    int64_t per; int32_t split;                  // reduction rows per slice (multiple of 32), number of slices
    float* partial; float* colsum;               // [split][Fp][Np], [split][Np] (colsum may be null)
    // GATHER form (the first layer of the DeepFM / DCN tower): X is never materialised -- column c < 64 nf of reduction row r is
    // element (c & 63) of table row row_base[c >> 6] + ids_t[c >> 6][r] (zero for a missing id), columns [64 nf, F) come from
    // dense_pad[r][c - 64 nf]
    const int32_t* ids_t; const int64_t* row_base; const float* table; int32_t nf; const float* dense_pad;
    // f16x2 mode: amax records of x (GATHER: the table's; x2 = the dense features', may be null) and of dy
    const uint32_t* x_amax; const uint32_t* x2_amax; const uint32_t* y_amax;
    uint32_t* hdr;                               // f16x2 mode: the workspace's header, where the amax words this launch used are saved
};

// H2: the f16x2 operand mode (h2_split8): both operands split into two fp16 terms with their tensors' scales; the partials carry
// s_x s_y and the reduce kernel divides it out.
template <int GATHER, int H2 = 0>
__global__ __launch_bounds__(512, 2) void bf3_gemm_tn_rs_kernel(TnRsArgs g) {
    constexpr int NW = 8, BMF = 32 * NW, BN = 256, NT = BN / 32;
    constexpr int NPL = RS_NPL<H2>, B_PLANE = RS_B_PLANE, STAGE = RS_STAGE<H2>;    // the dy image's two stages (bf3_rs_core.h)
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int tiles_n = (g.N + BN - 1) / BN, tiles_f = (g.F + BMF - 1) / BMF;
    const int per_slice = tiles_f * tiles_n;
    const int Fp = tiles_f * BMF, Np = tiles_n * BN;
    const int lid = xcd_remap(blockIdx.x, per_slice * g.split);         // consecutive logical ids share a reduction slice
    const int slice = lid / per_slice, t = lid % per_slice;
    const int f0 = (t / tiles_n) * BMF, n0 = (t % tiles_n) * BN;
    const int64_t r_begin = (int64_t)slice * g.per;
    int64_t r_end = r_begin + g.per;
    if (r_end > g.R) r_end = g.R;
    const int nk = (int)((r_end - r_begin + BK - 1) / BK);              // >= 1 by construction of split
    const bool want_cs = g.colsum != nullptr && f0 == 0;
    float h2_sx = 1.f, h2_sy = 1.f;
    if constexpr (H2) {
        float inv;
        h2_prologue(g.x_amax, g.x2_amax, g.y_amax, h2_sx, h2_sy, inv);
        if (lid == 0 && tid == 0) {                                     // the words these scales came from, for the reduce
            g.hdr[0] = max(g.x_amax[0], g.x2_amax != nullptr ? g.x2_amax[0] : 0u);
            g.hdr[1] = g.y_amax[0];
        }
    }

    // this lane's columns (clamped: columns past the edge only feed outputs nobody reads)
    const int fcol = min(f0 + wave * 32 + l31, g.F - 1);
    const int ncol = min(n0 + wave * 32 + l31, g.N - 1);
    // fragment read addresses as in bf3_gemm_rs_kernel (bf3_gemm.hip): B row = 32 nt + l31, chunk (2 hi + s) ^ tn_img_swizzle(row)
    // (rows 32 nt + l31 and 32 wave + l31 have the swizzle of l31)
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
    const int sw = tn_img_swizzle(l31);
    unsigned b_addr[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) b_addr[s] = rs_frag_addr(lds0, l31, hi, sw, s);
    // where this lane writes its own column's chunks: row 32 wave + l31 of the image, same swizzle
    unsigned char* const wrow = smem + (wave * 32 + l31) * 64;

    // raw operand values of one k-tile: element e = 8 s + j  <->  reduction row r0 + 16 hi + 8 s + j   (the k permutation of
    // the RS kernels: lane half hi holds k = 16 hi .. 16 hi + 15, k-step s uses 16 hi + 8 s .. + 7 = chunk 2 hi + s)
    float xa[16], yb[16];
    // per-lane byte offset inside a k-tile's rows (32-bit) + a wave-uniform row pointer per load: one address register, the
    // row stepping stays on the scalar unit
    const unsigned xoff = (unsigned)((16 * hi * g.ldx + fcol) * 4), yoff = (unsigned)((16 * hi * g.ldy + ncol) * 4);
    // (elements [e0, e1): all 16, or one k-step's 8 where the main loop re-issues an operand in pieces; known_full: the caller
    // knows that the k-tile is a full one, and the other arm is not even compiled in)
    auto load_raw = [&](float (&dst)[16], const float* base, int64_t ld, unsigned voff, int64_t r0, int e0 = 0, int e1 = 16, bool known_full = false) {
        if (known_full || r0 + BK <= r_end) {                           // (wave-uniform) a full k-tile: no checks
            const char* rowp = reinterpret_cast<const char*>(base + r0 * ld);
#pragma unroll
            for (int e = e0; e < e1; ++e) dst[e] = *reinterpret_cast<const float*>(rowp + (int64_t)e * ld * 4 + voff);
        } else {                                                        // the slice's last, partial k-tile (or past its end)
#pragma unroll
            for (int e = e0; e < e1; ++e) {
                const int64_t r = r0 + 16 * hi + e;
                const bool ok = r < r_end;
                const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base + (ok ? r : r_end - 1) * ld) +
                                                                (voff - (unsigned)(16 * hi * ld * 4)));
                dst[e] = ok ? v : 0.f;
            }
        }
    };
    // GATHER: where this wave's 32 columns live.  A wave covers half a field's row (32 of its 64 dims: one 128-byte line per
    // reduction row and lane half, exactly the lines the forward's gather fetched), or the dense features, or nothing (columns
    // past F: an empty buffer, every load returns 0; the outputs are never read).  Every load stays unconditional.
    const int c0w = f0 + wave * 32;
    const bool w_field = GATHER && c0w < 64 * g.nf;
    const bool w_dense = GATHER && !w_field && g.dense_pad != nullptr && c0w < 64 * g.nf + 32;
    // One raw buffer resource per wave (its field's rows / the dense features / a dummy): the address of a load is then ONE 32-bit
    // VALU operation, id * 256 + column (a field is below 2^24 rows = 4 GB, as in the fused forward), instead of 64-bit pointer
    // arithmetic per lane and load.  The resource's range check does ALL the masking: a missing id (-1) becomes offset 0xFFFFFF00 +
    // column >= num_records and the hardware returns 0 -- no clamp, no select; a row past the slice's end (its last, partial k-tile
    // only) is given that offset, and a wave without columns has num_records = 0.  So xa needs no validity mask and the main loop
    // no selects; the partial k-tile's offset fix-up is VALU only, under a wave-uniform branch.  The 32 ids of a k-tile sit in the
    // lanes so that DPP row_share:e hands every lane the id of ITS row e (lanes 0-31: rows 0-15 twice, lanes 32-63: rows 16-31
    // twice) -- one VALU move per load, no LDS shuffle.  (First cut: 64-bit pointers + ds_bpermute + clamp + select: +53 us on
    // the kernel.)
    const float* gptr = g.table;
    unsigned gpitch = 0;                                                // bytes per source row
    const int32_t* idrow = nullptr;
    if (GATHER) {
        if (w_field) {
            const int fld = c0w >> 6;
            // (readfirstlane: the load through the argument struct's generic pointer counts as divergent, and a resource that may
            // differ from lane to lane puts every buffer load of the main loop into a loop over the distinct resources)
            const int64_t rbv = g.row_base[fld];
            const int64_t rb = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rbv >> 32)) << 32) |
                                         (uint32_t)__builtin_amdgcn_readfirstlane((int)rbv));
            gptr = g.table + rb * 64 + (c0w & 32);
            gpitch = 256;
            idrow = g.ids_t + (int64_t)fld * g.R;
        } else if (w_dense) {
            gptr = g.dense_pad;
            gpitch = 128;
        }
    }
    const __amdgpu_buffer_rsrc_t grsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gptr), 0, (w_field || w_dense) ? (int)0xFFFFFF00u : 0, 0x00020000);
    const unsigned gcol = (unsigned)l31 * 4u;
    const int id_lane = (lane & 15) + 16 * hi;                          // the row of the k-tile whose id this lane keeps
    int idv = 0;                                                        // ids of the k-tile whose rows are fetched next
    auto gather_id = [&](int ids_of_tile, int e) -> int {              // DPP row_share:e (the control word must be a literal)
        switch (e) {
#define GATHER_ID(E) case E: return __builtin_amdgcn_update_dpp(0, ids_of_tile, 0x150 + E, 0xf, 0xf, false);
            GATHER_ID(0) GATHER_ID(1) GATHER_ID(2) GATHER_ID(3) GATHER_ID(4) GATHER_ID(5) GATHER_ID(6) GATHER_ID(7)
            GATHER_ID(8) GATHER_ID(9) GATHER_ID(10) GATHER_ID(11) GATHER_ID(12) GATHER_ID(13) GATHER_ID(14)
#undef GATHER_ID
            default: return __builtin_amdgcn_update_dpp(0, ids_of_tile, 0x15f, 0xf, 0xf, false);
        }
    };
    auto load_ids = [&](int64_t r0) -> int {
        if (!w_field) return 0;                                         // (wave-uniform)
        const int64_t r = r0 + id_lane < g.R ? r0 + id_lane : g.R - 1;
        return idrow[r];
    };
    // the byte offsets of elements [e0, e1) of the k-tile at r0 (whose ids are ids_of_tile), then the loads themselves: two steps, so
    // that the main loop can put the next id load between them
    auto gather_offsets = [&](unsigned (&off)[16], int ids_of_tile, int64_t r0, int e0, int e1, bool known_full = false) {
        const bool full = known_full || r0 + BK <= r_end;               // (wave-uniform) all but a slice's last k-tile
        if (w_field) {                                                  // (wave-uniform; ONE branch, not one per load)
#pragma unroll
            for (int e = e0; e < e1; ++e) off[e] = (unsigned)gather_id(ids_of_tile, e) * gpitch;
        } else {                                                        // dense_pad: R rows of 128 bytes, below 4 GB; no columns: 0
            const unsigned o0 = (unsigned)(r0 + 16 * hi) * gpitch;
#pragma unroll
            for (int e = e0; e < e1; ++e) off[e] = o0 + (unsigned)e * gpitch;
        }
        if (!full) {
            const int nv = (int)(r_end - r0 < BK ? r_end - r0 : BK) - 16 * hi;     // this lane half's rows inside the slice (<= 0: none)
#pragma unroll
            for (int e = e0; e < e1; ++e) off[e] = e < nv ? off[e] : 0xFFFFFF00u;
        }
    };
    auto gather_issue = [&](float (&dst)[16], const unsigned (&off)[16], int e0, int e1) {
#pragma unroll
        for (int e = e0; e < e1; ++e)
            dst[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grsrc, (int)(off[e] + gcol), 0, DR_NT_WGRAD_GATHER ? 2 : 0));
    };
    auto load_gather = [&](float (&dst)[16], int ids_of_tile, int64_t r0) {
        unsigned off[16];
        gather_offsets(off, ids_of_tile, r0, 0, 16);
        gather_issue(dst, off, 0, 16);
    };
    bf16x8 fa[2][3];
    bf16x8 fb[4][3];                                                    // group q uses buffer q & 3, read two groups ahead
    float cs = 0.f;
    auto stage_b = [&](int stage) {                                     // yb -> three planes of this lane's column
        if (want_cs) {                                                  // (block-uniform) only the f0 == 0 blocks store the column sum
#pragma unroll
            for (int e = 0; e < 16; ++e) cs += yb[e];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 p0, p1, p2;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = yb[8 * s + j];
            if constexpr (H2) h2_split8v(v, h2_sy, p0, p1);
            else rs_split8v(v, p0, p1, p2);
            unsigned char* w = wrow + stage * STAGE + rs_chunk_off(hi, sw, s);
            *reinterpret_cast<bf16x8*>(w) = p0;
            *reinterpret_cast<bf16x8*>(w + B_PLANE) = p1;
            if constexpr (!H2) *reinterpret_cast<bf16x8*>(w + 2 * B_PLANE) = p2;
        }
    };
    auto read_b = [&](int buf, int stage, int q) {
        const unsigned bb = b_addr[q >> 3] + stage * STAGE;
        rs_read_frag<NPL>(fb[buf], bb, q & 7);
    };
    f32x16 acc[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[tt][k] = 0.f;

    auto split_a = [&](int s) {                                         // k-step s of xa -> its terms
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xa[8 * s + j];
        if constexpr (H2) h2_split8v(v, h2_sx, fa[s][0], fa[s][1]);
        else rs_split8v(v, fa[s][0], fa[s][1], fa[s][2]);
    };
    // The 16 MFMA groups of the k-tile in `stage` (groups 0 and 1 are in fb already); more: another k-tile follows in the other stage.
    // before_group(q) is the place of whatever a caller interleaves with the groups.
    auto mma_groups = [&](int stage, bool more, auto&& before_group) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            before_group(q);
            if (q < 14) {
                rs_wait_frag<NPL, NPL>(fb[q & 3]);                     // the next group's NPL reads may fly
                read_b((q + 2) & 3, stage, q + 2);
            } else if (q == 14) {
                // groups 14 and 15 are in registers, this wave is done reading this stage and its ds_writes of the next one
                // have retired (lgkmcnt(0) covers both): publish
                rs_wait_frag<NPL, 0>(fb[2]);
                asm volatile("s_barrier" ::: "memory");
                if (more) read_b(0, stage ^ 1, 0);
            } else {
                if (more) read_b(1, stage ^ 1, 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int term = 0; term < RS_TERMS<H2>; ++term) acc[q & 7] = rs_mma_term<H2>(term, fa[q >> 3], fb[q & 3], acc[q & 7]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if constexpr (!H2) {
        // ---- prologue: B(0) into stage 0, A(0) and B(1) into registers ---------------------------------------------------------
        load_raw(yb, g.Y, g.ldy, yoff, r_begin);
        stage_b(0);
        if (GATHER) {
            idv = load_ids(r_begin);
            load_gather(xa, idv, r_begin);
            idv = load_ids(r_begin + BK);
        } else {
            load_raw(xa, g.X, g.ldx, xoff, r_begin);
        }
        load_raw(yb, g.Y, g.ldy, yoff, r_begin + BK);                   // (all zeros when nk == 1)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        read_b(0, 0, 0);
        read_b(1, 0, 1);
        for (int kt = 0; kt < nk; ++kt) {
            const int stage = kt & 1;
            // A of this k-tile -> bf16 terms; B of the next k-tile -> the other stage (its readers passed the barrier at the end of
            // the previous step); the loads of the k-tile after that go into flight
            split_a(0);
            split_a(1);
            if (kt + 1 < nk) stage_b(stage ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            if (GATHER) {
                // (the loads stay between these two scheduling barriers, in front of the MFMA loop's fragment reads)
                load_gather(xa, idv, r_begin + (int64_t)(kt + 1) * BK);
                idv = load_ids(r_begin + (int64_t)(kt + 2) * BK);
            } else {
                load_raw(xa, g.X, g.ldx, xoff, r_begin + (int64_t)(kt + 1) * BK);
            }
            load_raw(yb, g.Y, g.ldy, yoff, r_begin + (int64_t)(kt + 2) * BK);
            __builtin_amdgcn_sched_barrier(0);
            mma_groups(stage, kt + 1 < nk, [](int) {});
        }
    } else {
        // f16x2 mode (the registers of the third plane are free).  Every operand register set is consumed where its first reader
        // needs it and re-issued at once, at THREE points of a step, so that a block never has all of its loads retired at the same
        // time -- its eight waves run in one phase, and with one consume-all / issue-all point per step the CU had nothing in flight
        // once per k-tile.  k-step 0 of x at the top, k-step 1 in front of MFMA group Q_A1 (its first reader is group 8), dy in front
        // of group Q_B (its image is published by the barrier of group 14).  Issue order: x k-step 0, ids, x k-step 1, dy; at the
        // three waits 24 / 24 / 16 younger loads stay in flight (+ the id load).
        // The waits are the compiler's, and they come out exact only while NO load result is consumed under a branch on any path
        // into the loop: the select of load_raw's partial arm drains everything there, and every wait behind the join inherits the
        // drained path (measured in the ISA: vmcnt(8) where 24 were possible).  So the pipelined loop runs over the slice's FULL
        // k-tiles only, its loads are all of the unchecked kind (a prefetch past the last full k-tile reads that one again and is
        // never consumed), and a partial last k-tile gets a step of its own behind the loop.  Same products in the same order.
        constexpr int Q_A1 = 5, Q_B = 10;                               // (3 - 6 and 10 - 12 measured: within 3 us of one another)
        const int nfull = (int)((r_end - r_begin) / BK);                // nk == nfull, or nfull + 1 with a partial last k-tile
        if (nfull > 0) {
            const int64_t r_last = r_begin + (int64_t)(nfull - 1) * BK;
            int64_t r1 = nfull > 1 ? r_begin + BK : r_last;             // the k-tile after this step's, and the one after that
            int64_t r2 = nfull > 2 ? r_begin + 2 * BK : r_last;
            // ---- prologue: B(0) into stage 0, A(0) and B(1) into registers, in the loop's issue order --------------------------
            load_raw(yb, g.Y, g.ldy, yoff, r_begin, 0, 16, true);
            stage_b(0);
            if (GATHER) {
                idv = load_ids(r_begin);
                unsigned off[16];
                gather_offsets(off, idv, r_begin, 0, 16, true);
                gather_issue(xa, off, 0, 8);
                __builtin_amdgcn_sched_barrier(0);
                idv = load_ids(r1);
                __builtin_amdgcn_sched_barrier(0);
                gather_issue(xa, off, 8, 16);
            } else {
                load_raw(xa, g.X, g.ldx, xoff, r_begin, 0, 16, true);
            }
            __builtin_amdgcn_sched_barrier(0);
            load_raw(yb, g.Y, g.ldy, yoff, r1, 0, 16, true);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            read_b(0, 0, 0);
            read_b(1, 0, 1);
            for (int kt = 0; kt < nfull; ++kt) {
                const int stage = kt & 1;
                const bool more = kt + 1 < nfull;
                split_a(0);
                __builtin_amdgcn_sched_barrier(0);
                if (GATHER) {
                    unsigned off[16];
                    gather_offsets(off, idv, r1, 0, 8, true);
                    gather_issue(xa, off, 0, 8);
                } else {
                    load_raw(xa, g.X, g.ldx, xoff, r1, 0, 8, true);
                }
                __builtin_amdgcn_sched_barrier(0);
                mma_groups(stage, more, [&](int q) {
                    if (q == Q_A1) {
                        split_a(1);
                        __builtin_amdgcn_sched_barrier(0);
                        if (GATHER) {
                            unsigned off[16];
                            gather_offsets(off, idv, r1, 8, 16, true);  // (the last readers of this id register)
                            idv = load_ids(r2);
                            gather_issue(xa, off, 8, 16);
                        } else {
                            load_raw(xa, g.X, g.ldx, xoff, r1, 8, 16, true);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (q == Q_B) {
                        if (more) stage_b(stage ^ 1);                   // (its readers passed the barrier of the previous step)
                        __builtin_amdgcn_sched_barrier(0);
                        load_raw(yb, g.Y, g.ldy, yoff, r2, 0, 16, true);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
                r1 = r2;
                r2 = r2 < r_last ? r2 + BK : r_last;
            }
        }
        if (nk > nfull) {
            // ---- the slice's last, partial k-tile: rows past the end are zeros (load_raw's checks, the gather's range check) ------
            const int stage = nfull & 1;                                // (last read two barriers ago)
            const int64_t r0 = r_begin + (int64_t)nfull * BK;
            load_raw(yb, g.Y, g.ldy, yoff, r0);
            if (GATHER) {
                idv = load_ids(r0);
                load_gather(xa, idv, r0);
            } else {
                load_raw(xa, g.X, g.ldx, xoff, r0);
            }
            stage_b(stage);
            split_a(0);
            split_a(1);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            read_b(0, stage, 0);
            read_b(1, stage, 1);
            mma_groups(stage, false, [](int) {});
        }
    }
    // ---- epilogue: partial tile (padded workspace: unconditional stores); C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 hi
    float* out = g.partial + ((int64_t)slice * Fp + f0 + wave * 32 + 4 * hi) * Np + n0 + l31;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) out[(int64_t)((reg & 3) + 8 * (reg >> 2)) * Np + nt * 32] = acc[nt][reg];
    if (want_cs) {
        cs += __shfl_xor(cs, 32, 64);
        if (hi == 0) g.colsum[(int64_t)slice * Np + n0 + wave * 32 + l31] = cs;
    }
}

// dst[f][n] += scale * sum_s partial[s][f][n]  (fixed order);  dstb[n] += scale * sum_s colsum[s][n]
// A streaming kernel over tn_rs_reduce_block (tn_rs_reduce.h), one logical block per block.
template <int V>
__global__ __launch_bounds__(TN_RS_RED_THREADS) void bf3_tn_rs_reduce_kernel(TnRsApply a) {
    tn_rs_reduce_block<V>(a, blockIdx.x, threadIdx.x);
}

void launch_tn_rs_reduce(const TnRsApply& a, dr_stream_t stream) {
    const int nlb = tn_rs_reduce_blocks(a.F, a.N, a.vec);
    if (a.vec) hipLaunchKernelGGL(bf3_tn_rs_reduce_kernel<4>, dim3(nlb), dim3(TN_RS_RED_THREADS), 0, dr_s(stream), a);
    else hipLaunchKernelGGL(bf3_tn_rs_reduce_kernel<1>, dim3(nlb), dim3(TN_RS_RED_THREADS), 0, dr_s(stream), a);
}
}  // namespace

void drrs::tn_rs_plan(int64_t R, int32_t F, int32_t N, int& split, int64_t& per, int& Fp, int& Np) {
    const int tf = (F + 255) / 256, tn = (N + 255) / 256;
    Fp = tf * 256;
    Np = tn * 256;
    int64_t sp = 256 / ((int64_t)tf * tn);                              // about one block per CU
    const int64_t max_split = (R + 16 * BK - 1) / (16 * BK);            // at least 16 k-tiles per slice
    if (sp > max_split) sp = max_split;
    if (sp < 1) sp = 1;
    per = ((R + sp - 1) / sp + BK - 1) / BK * BK;
    split = (int)((R + per - 1) / per);                                 // every slice non-empty
}

extern "C" int64_t dr_bf3_wgrad_workspace_bytes(int64_t R, int32_t F, int32_t N) {
    if (R <= 0 || F <= 0 || N <= 0) return 0;
    int split, Fp, Np;
    int64_t per;
    tn_rs_plan(R, F, N, split, per, Fp, Np);
    return ((int64_t)split * Fp * Np + (int64_t)split * Np + TN_RS_HDR_WORDS) * (int64_t)sizeof(float);
}

// dstW[f][n] += scale * sum_r x[r][f] dy[r][n];  dstb[n] += scale * sum_r dy[r][n] (dstb may be NULL).  x [R, F], dy [R, N] fp32
// row-major; the bf16x3 product mode, deterministic (fixed-order reduce over the reduction slices).
static int wgrad_impl(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t R, int32_t F, int32_t N,
                      float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes,
                      dr_stream_t stream, const uint32_t* x_amax = nullptr, const uint32_t* dy_amax = nullptr) {
    if (R <= 0 || F <= 0 || N <= 0) return DR_EINVAL;
    if (!x || !dy || !dstW || !workspace || ld_x < F || ld_dy < N || ld_w < N) return DR_EINVAL;
    if (workspace_bytes < dr_bf3_wgrad_workspace_bytes(R, F, N)) return DR_EINVAL;
    int split, Fp, Np;
    int64_t per;
    tn_rs_plan(R, F, N, split, per, Fp, Np);
    const bool h2 = x_amax != nullptr;
    const TnRsApply ap = tn_rs_apply_of(workspace, split, F, N, Fp, Np, h2, scale, dstW, ld_w, dstb);
    TnRsArgs g{x, ld_x, dy, ld_dy, R, F, N, per, split, const_cast<float*>(ap.partial), const_cast<float*>(ap.colsum), nullptr, nullptr, nullptr, 0,
               nullptr, x_amax, nullptr, dy_amax, const_cast<uint32_t*>(ap.hdr)};
    const int grid = (Fp / 256) * (Np / 256) * split;
    if (h2) hipLaunchKernelGGL((bf3_gemm_tn_rs_kernel<0, 1>), dim3(grid), dim3(512), 0, dr_s(stream), g);
    else hipLaunchKernelGGL((bf3_gemm_tn_rs_kernel<0, 0>), dim3(grid), dim3(512), 0, dr_s(stream), g);
    launch_tn_rs_reduce(ap, stream);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_bf3_wgrad(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t R, int32_t F, int32_t N,
                            float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes,
                            dr_stream_t stream) {
    return wgrad_impl(x, ld_x, dy, ld_dy, R, F, N, scale, dstW, ld_w, dstb, workspace, workspace_bytes, stream);
}

// dr_bf3_wgrad in the f16x2 operand mode (h2_split8): x_amax / dy_amax are the operands' amax records (dr_h2_amax, or a producer's).
// Same workspace, same fixed-order reduce.
extern "C" int dr_h2_wgrad(const float* x, int64_t ld_x, const uint32_t* x_amax, const float* dy, int64_t ld_dy, const uint32_t* dy_amax,
                           int64_t R, int32_t F, int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace,
                           int64_t workspace_bytes, dr_stream_t stream) {
    if (!x_amax || !dy_amax) return DR_EINVAL;
    return wgrad_impl(x, ld_x, dy, ld_dy, R, F, N, scale, dstW, ld_w, dstb, workspace, workspace_bytes, stream, x_amax, dy_amax);
}

// The same wgrad for the FIRST tower layer, whose x = concat(field embeddings, dense features) is never read from a buffer: the
// kernel gathers it from the tables (GATHER form of TnRsArgs; D = 64).  ids_t [nf][R] int32: the batch's bucket ids, field-major
// (dr_ids_transpose_i32), -1 = missing; dense_pad [R, 32] zero-padded dense features (NULL iff F == 64 nf).  With this the forward
// need not store `concat` at all (keras/models/ranking/deepfm.py:44-45: stack / concat become pure fiction).
static int wgrad_emb_impl(const int32_t* ids_t, int64_t R, int32_t nf, const int64_t* row_base, const float* table, int32_t D,
                          const float* dense_pad, const float* dy, int64_t ld_dy, int32_t F, int32_t N, float scale, float* dstW,
                          int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes, int32_t parts, dr_stream_t stream,
                          const uint32_t* table_amax = nullptr, const uint32_t* dense_amax = nullptr, const uint32_t* dy_amax = nullptr) {
    if (R <= 0 || F <= 0 || N <= 0 || nf <= 0) return DR_EINVAL;
    if (table_amax != nullptr && (!dy_amax || (F > 64 * nf && !dense_amax))) return DR_EINVAL;
    if (D != 64 || F < 64 * nf || F > 64 * nf + 32) return DR_ESHAPE;
    if (!ids_t || !row_base || !table || !dy || !dstW || !workspace || ld_dy < N || ld_w < N) return DR_EINVAL;
    if (F > 64 * nf && !dense_pad) return DR_EINVAL;
    if (workspace_bytes < dr_bf3_wgrad_workspace_bytes(R, F, N)) return DR_EINVAL;
    int split, Fp, Np;
    int64_t per;
    tn_rs_plan(R, F, N, split, per, Fp, Np);
    const bool h2 = table_amax != nullptr;
    const TnRsApply ap = tn_rs_apply_of(workspace, split, F, N, Fp, Np, h2, scale, dstW, ld_w, dstb);
    TnRsArgs g{nullptr, 0, dy, ld_dy, R, F, N, per, split, const_cast<float*>(ap.partial), const_cast<float*>(ap.colsum), ids_t, row_base, table,
               nf, F > 64 * nf ? dense_pad : nullptr, table_amax, F > 64 * nf ? dense_amax : nullptr, dy_amax, const_cast<uint32_t*>(ap.hdr)};
    const int grid = (Fp / 256) * (Np / 256) * split;
    if (parts & 1) {
        if (h2) hipLaunchKernelGGL((bf3_gemm_tn_rs_kernel<1, 1>), dim3(grid), dim3(512), 0, dr_s(stream), g);
        else hipLaunchKernelGGL((bf3_gemm_tn_rs_kernel<1, 0>), dim3(grid), dim3(512), 0, dr_s(stream), g);
    }
    if (parts & 2) launch_tn_rs_reduce(ap, stream);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// In two halves: parts = 1 the split-K GEMM into the workspace, parts = 2 the fixed-order reduce that applies it (dstW += scale * sum,
// dstb likewise), 3 = both.  Part 2 may run on another stream (the engine puts it in front of the weight-plane refresh, which lives
// there already); it must finish before anything reads dstW / dstb and before the next part 1 over the same workspace.
extern "C" int dr_bf3_wgrad_emb(const int32_t* ids_t, int64_t R, int32_t nf, const int64_t* row_base, const float* table, int32_t D,
                                const float* dense_pad, const float* dy, int64_t ld_dy, int32_t F, int32_t N, float scale, float* dstW,
                                int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes, int32_t parts, dr_stream_t stream) {
    if (parts < 1 || parts > 3) return DR_EINVAL;
    return wgrad_emb_impl(ids_t, R, nf, row_base, table, D, dense_pad, dy, ld_dy, F, N, scale, dstW, ld_w, dstb, workspace, workspace_bytes,
                          parts, stream);
}

// dr_bf3_wgrad_emb in the f16x2 operand mode: table_amax as in dr_h2_emb_linear_fwd, dense_amax the record of dense_pad (required
// iff F > 64 nf), dy_amax the record of dy.  The records must be the same for part 1 and part 2 of one product.
extern "C" int dr_h2_wgrad_emb(const int32_t* ids_t, int64_t R, int32_t nf, const int64_t* row_base, const float* table, int32_t D,
                               const uint32_t* table_amax, const float* dense_pad, const uint32_t* dense_amax, const float* dy, int64_t ld_dy,
                               const uint32_t* dy_amax, int32_t F, int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb,
                               void* workspace, int64_t workspace_bytes, int32_t parts, dr_stream_t stream) {
    if (parts < 1 || parts > 3 || !table_amax || !dy_amax) return DR_EINVAL;
    return wgrad_emb_impl(ids_t, R, nf, row_base, table, D, dense_pad, dy, ld_dy, F, N, scale, dstW, ld_w, dstb, workspace, workspace_bytes,
                          parts, stream, table_amax, dense_amax, dy_amax);
}
