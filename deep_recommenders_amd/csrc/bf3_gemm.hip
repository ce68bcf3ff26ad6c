// =====================================================================================================================
// NT, "register split" (RS):  C[m][n] = epilogue( sum_k A[m][k] B[n][k] ),  A fp32 row-major (an ACTIVATION: x, dy),
// B pre-split planes (a WEIGHT: W^T for the forward, W for the dgrad).
//
// Why: every LDS-staged variant above lands at 150 - 165 TFLOP/s whatever its schedule, because a CU cannot INGEST operand
// tiles faster than ~14 - 21 bytes per clock through LDS-DMA (tools/exp/bf3_ablate.hip: the DMA stream alone takes 300 us of
// the 340, the MFMAs alone 250) -- and 128 x 128 / 128 x 256 tiles of six-byte elements need 31 / 23 bytes per clock at the
// matrix pipe's rate.  A 256 x 256 tile needs 16, but its two operands do not fit the LDS three stages deep.  So only B (shared
// by the block's 8 waves) goes through the LDS; each wave owns 32 rows x all 256 columns of the tile and loads ITS rows of A
// straight from HBM into registers as fp32 -- 16 contiguous floats per lane and k-tile, lanes l and l + 32 together one
// 128-byte line per row -- and splits them into the three bf16 terms in registers (VALU work in the shadow of the other
// wave's MFMAs; no LDS write, no fragment read for A).  Activations therefore stay fp32 in HBM (4 bytes per element instead
// of 6, nothing for their producers to do); only the weights are kept as planes (dr_bf3_split after each update).
// The k index inside a k-tile is permuted consistently on both operands: lane half `hi` holds k = 16 hi .. 16 hi + 15, k-step s
// uses 16 hi + 8 s .. + 7, i.e. B's 16-byte chunk 2 hi + s.
//
// Per step (k-tile of 32), B ring of three 48 KB stages, all counts per wave:
//   start:     split A(g) in registers (6 fragments), issue the 4 global loads of A(g + 1)
//   q = 0..15  (k-step q >> 3, column tile q & 7): fragment reads for group q + 1, 6 MFMAs on acc[q & 7];
//              LDS-DMA pieces of step g + 2 after q = 1, 3, .., 11 (into the stage step g - 1 used)
//   q = 15:    before reading group 0 of step g + 1: lgkmcnt(0) (done with stage g), vmcnt(10) (step g + 1 landed; A(g + 1) and
//              step g + 2 may be in flight), s_barrier
// =====================================================================================================================

// Cache-policy experiment (round 4): a stream that is read / written ONCE marked nontemporal so that it does not wash the weight
// planes (and, in K4, the first-order lines) out of the L2 / Infinity Cache.  0 = default policy, 1 = nontemporal.
#ifndef DR_NT_DGRAD_STORE
#define DR_NT_DGRAD_STORE 0
#endif
#include "bf3_rs_core.h"
#include <cstdlib>

namespace {

using namespace drrs;

// EPI: 0 = bias / ReLU, 1 = + ReLU' mask, 3 = accumulate (C +=), 2 = DCN cross combine, 4 = top-K filter, 5 = scatter into the
// embedding-gradient send layout (one epilogue per
// instantiation: all of them unrolled over the 8 column tiles in one kernel cost 50 spilled registers)
// MS: 32-row sets per wave.  1 = 8 waves x 32 rows (two waves per SIMD, 128 accumulator registers each); 2 = 4 waves x 64 rows (ONE
// wave per SIMD with all 512 registers, 256 of them accumulators): every weight fragment read from the LDS feeds 12 MFMAs instead
// of 6 and the ring's DMA pieces per MFMA stay the same, at the price of a single in-order instruction stream per SIMD.
// CS: column split of the tile between waves.  CS = 2 (with MS = 2): 8 waves again, wave w owns rows 64 (w & 3) .. + 63 and column tiles
// 4 (w >> 2) .. + 3 -- the same 128 accumulator registers as the default and two waves per SIMD, but half the fragment reads per
// MFMA; the price is that each activation row is loaded and split by two waves (w and w + 4: one SIMD, one L1).
// H2: the f16x2 operand mode (see h2_split8 above): B holds TWO fp16 planes (32 KB stages, 4 pieces per wave and k-tile), three MFMAs
// per fragment pair.
// AR (round 5; H2 only): RESIDENT activation operand for short reductions, K == 32 AR (AR = 4: the top-K scan's K = 128).  A block
// keeps ONE row tile for all of its output tiles (block b: row tile b % tiles_m, column tiles b / tiles_m + j * (grid / tiles_m); the
// launcher makes grid a multiple of tiles_m), loads and splits its 32 K floats per lane ONCE into 16 AR registers and the step
// loop carries no activation loads, no split and no wait for them: only the weight ring, the fragment reads and the MFMAs.  The
// products and their order are those of the streaming kernel -- bit-identical results (the scan's dense first chunk, which runs
// the streaming kernel, must tie exactly with the filtered chunks).
template <int EPI, int DBG = 0, int MS = 1, int CS = 1, int H2 = 0, int AR = 0>
__global__ __launch_bounds__(512 * CS / MS, MS == CS ? 2 : 1) void bf3_gemm_rs_kernel(RsArgs g) {
    constexpr int NW = 8 * CS / MS, RGW = NW / CS, BM = 32 * MS * RGW, BN = 256, NT = BN / 32, NTW = NT / CS, NS = 3;
    static_assert(CS == 1 || (CS == 2 && MS == 2), "column split only with 64-row waves");
    static_assert(!H2 || CS == 1, "f16x2: no column split");
    static_assert(AR == 0 || (H2 && MS == 1 && CS == 1 && DBG == 0), "resident activations: f16x2, 8 waves x 32 rows");
    constexpr int NPL = RS_NPL<H2>, STAGE = RS_STAGE<H2>;               // the weight ring's stages (bf3_rs_core.h)
    constexpr int PW = STAGE / 1024 / NW;                               // 6 MS (4) LDS-DMA pieces per wave and k-tile
    static_assert(PW * NW == 16 * NPL && (MS == 1 || MS == 2), "piece schedule below assumes 16 NPL / NW pieces per wave and k-tile");
    constexpr int KT_UNROLL = AR ? AR : 1;                              // (AR: the k-tile loop is unrolled, see there)
    constexpr int VM_STEP = (AR ? 0 : 4 * MS) + PW;                     // VMEM operations of one step (A loads + pieces)
    constexpr int VM_WAIT_STEP = 0x0F70 | (VM_STEP & 15) | ((VM_STEP >> 4) << 14);   // s_waitcnt vmcnt(VM_STEP) (6-bit field, split)
    // EPI 5 in the f16x2 mode stages each wave's 32 x 32 accumulator block through the LDS (row-major, pitch 36 floats) behind the ring
    // (+ the wave's 32 x 4 destinations and 32 d_fm_logit values of the tile: registers are what this epilogue is short of)
    constexpr int PK_PITCH = 36, PK_STG = 32 * PK_PITCH * 4, PK_WAVE = PK_STG + 32 * 4 * 4 + 32 * 4;    // 4608 + 512 + 128 bytes per wave
    constexpr int PK_BYTES = (EPI == 5 && H2) ? NW * PK_WAVE : 0;       // 41 KB: 96 + 41 of the 160 KB
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE + PK_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int rgi = CS == 1 ? wave : (wave & (RGW - 1));               // row group / column half of this wave
    const int chi = CS == 1 ? 0 : (wave / RGW);

    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_m = (int)((g.M + BM - 1) / BM);
    const int ntiles = tiles_m * tiles_n;
    const int nk = (g.K + BK - 1) / BK;
    const bool ktail = (g.K % BK) != 0;
    // the block's tiles: `tile` = blockIdx.x + j gridDim.x, j < my_tiles; lid_of(tile) = its logical id (row tile * tiles_n + column tile)
    const int ar_npg = AR ? (int)gridDim.x / tiles_m : 1;               // AR: column tiles are dealt round-robin to the grid / tiles_m blocks of a row tile
    const int ar_n0 = AR ? (int)blockIdx.x / tiles_m : 0;
    const int my_tiles = AR ? (ar_n0 < tiles_n ? (tiles_n - ar_n0 + ar_npg - 1) / ar_npg : 0)
                            : ((int)blockIdx.x < ntiles ? (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0);
    if (my_tiles <= 0) return;
    const int tile_end = (int)blockIdx.x + my_tiles * (int)gridDim.x;
    auto lid_of = [&](int tile) {
        if constexpr (AR != 0) return ((int)blockIdx.x % tiles_m) * tiles_n + ar_n0 + ((tile - (int)blockIdx.x) / (int)gridDim.x) * ar_npg;
        else return xcd_remap(tile, ntiles);
    };
    const int total = my_tiles * nk;                                    // steps of this block

    // B fragment read addresses (stage 0, plane 0, column tile 0), one per k-step: row = 32 nt + l31, chunk 2 hi + s swizzled
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
    const int sw = rs_swizzle(l31);
    unsigned b_addr[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) b_addr[s] = rs_frag_addr(lds0, l31, hi, sw, s) + chi * (NTW * 2048);

    // ---- producer state: the block's stream of steps (tile, k-tile), shared by the B pieces and the A loads -----------------
    // B: piece j = wave + 8 i of a stage: plane j / 16, rows 16 (j % 16) .. + 15, lane -> (row, 16-byte chunk).
    // Issued as MUBUF `buffer_load_dwordx4 ... offen lds` (raw buffer builtin), not as global_load_lds: hipcc's wait-count pass
    // treats the FLAT-encoded form as "may touch LDS through flat" and from then on waits vmcnt(0) for every VMEM result,
    // the buffer form is counted exactly (a register load followed by 6 pieces gets vmcnt(6)).
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16*>(g.B), 0, (int)min((int64_t)0x7fffffff, NPL * g.b_ps * 2), 0x00020000);
    float h2_sa = 1.f, h2_out = 1.f;                                    // H2: A's scale, 1 / (s_a s_b)
    float cmax = 0.f;                                                   // H2: largest |value| this lane stored into C
    if constexpr (H2) {
        float sb;
        h2_prologue(g.a_amax, nullptr, g.b_amax, h2_sa, sb, h2_out);
    }
    int bvoff[12];                                                      // per-lane byte offset of piece i < PW at k = 0 (arrays the
                                                                        // lambdas capture have FIXED sizes: with a template-dependent size
                                                                        // hipcc silently drops the kernel's host stub)
    int pb_tile = blockIdx.x, pb_kt = 0, pb_stage = 0, pb_koff = 0;     // pb_koff: byte offset along k of the next real step
    auto setup_b = [&](int tile) {
        const int n0 = (lid_of(tile) % tiles_n) * BN;
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int j = wave + NW * i;
            const int plane = j >> 4, rb = j & 15;
            const int row = rb * 16 + (lane >> 2);
            const int c = (lane & 3) ^ ((row >> 2) & 3);
            int64_t grow = (int64_t)n0 + row;
            grow = grow < g.N ? grow : g.N - 1;                         // columns past the edge only feed unstored outputs
            bvoff[i] = (int)((plane * g.b_ps + grow * g.b_ld + c * 8) * 2);
        }
    };
    // EVERY step issues exactly 4 A loads and 6 pieces, also the last ones of the block (whose successors do not exist): with a
    // fixed number of VMEM operations per step the counted waits are constants, and hipcc's own wait for the A registers comes
    // out as vmcnt(6).  A step that does not exist re-fetches the last k-tile into a stage nobody will read again.
    auto issue_b = [&](int i) {
        unsigned char* dst = smem + pb_stage * STAGE + (wave + NW * i) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(brsrc, (lds_ptr_t)dst, 16, bvoff[i], (DBG & 4) ? 0 : pb_koff, 0, 0);
    };
    auto advance_b = [&]() {                                            // after the 6 pieces of a REAL step
        pb_stage = pb_stage == NS - 1 ? 0 : pb_stage + 1;
        pb_koff += BK * 2;
        if (++pb_kt == nk) {
            pb_kt = 0;
            pb_tile += gridDim.x;
            if (pb_tile < tile_end) {
                setup_b(pb_tile);
                pb_koff = 0;
            } else {
                pb_koff -= BK * 2;                                      // end of the stream: dummies re-fetch the last k-tile
            }
        }
    };
    // A: this lane's 16 floats of a k-tile
    const float* asrc[2];
    int pa_tile = blockIdx.x, pa_kt = 0;
    auto setup_a = [&](int tile) {
        const int64_t m0 = (int64_t)(lid_of(tile) / tiles_n) * BM;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
            int64_t row = m0 + rgi * (32 * MS) + 32 * ms + l31;
            row = row < g.M ? row : g.M - 1;                            // rows past the edge only feed unstored outputs
            asrc[ms] = g.A + row * g.lda + 16 * hi;
        }
    };
    float4 an[2][4];                                                    // A of the NEXT step, in flight
    const int kv4 = (g.K + 3) / 4 * 4;                                  // rows are readable up to here (lda % 4 == 0, lda >= K)
    int an_k0 = 0;                                                      // k index of an[0].x
    auto mask_a = [&]() {
        if (!ktail) return;                                             // kernel-uniform: K % 32 == 0 has nothing to zero
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = an_k0 + 4 * q;
                an[ms][q].x = k < g.K ? an[ms][q].x : 0.f;
                an[ms][q].y = k + 1 < g.K ? an[ms][q].y : 0.f;
                an[ms][q].z = k + 2 < g.K ? an[ms][q].z : 0.f;
                an[ms][q].w = k + 3 < g.K ? an[ms][q].w : 0.f;
            }
    };
    auto load_a = [&](bool real) {
        // Every load unconditional (a load under a divergent branch makes hipcc's wait-count pass fall back to vmcnt(0), which
        // would also drain the LDS-DMA pieces in flight): in the last k-tile of a row a 16-byte load that would start past the
        // row's readable end is pulled back inside it, and everything at k >= K is zeroed in registers -- B's planes are zero
        // there, but 0 * NaN is not.
        // The zeroing happens when the values are CONSUMED (mask_a, at the start of the step that uses them): touching them
        // here would wait for the loads on the spot.
        an_k0 = pa_kt * BK + 16 * hi;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int over = max(0, an_k0 + 4 * q - (kv4 - 4));
                an[ms][q] = *reinterpret_cast<const float4*>(asrc[ms] + 4 * q - over);
            }
        if (!real) return;                                              // (uniform; no VMEM below)
        if constexpr (!(DBG & 8)) {
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) asrc[ms] += BK;
        }
        if (++pa_kt == nk) {
            pa_kt = 0;
            pa_tile += gridDim.x;
            if (pa_tile < tile_end) setup_a(pa_tile);
            else if constexpr (!(DBG & 8)) {                            // end of the stream: the dummy loads re-read k-tile 0 of the
#pragma unroll                                                          // last rows (pa_kt == 0, so `over` keeps them inside the row)
                for (int ms = 0; ms < MS; ++ms) asrc[ms] -= (int64_t)nk * BK;
            }
        }
    };

    bf16x8 fa[MS][2][3];                                                // [row set][k-step][plane] of the CURRENT step
    bf16x8 fb[4][3];                                                    // [buffer][plane]: group q uses buffer q & 3; the
                                                                        // reads run TWO groups (12 MFMAs) ahead of their use
                                                                        // (CS == 2: buffers 0 / 1, ONE group = 12 MFMAs ahead)
    auto read_b = [&](int buf, int stage, int q) {                      // group q = (k-step q / NTW, column tile q % NTW)
        if constexpr (DBG & 32) return;                                 // ablation: no fragment reads (stale registers)
        const unsigned bb = b_addr[q / NTW] + stage * STAGE;
        rs_read_frag<((DBG & 256) || H2) ? 2 : 3>(fb[buf], bb, q % NTW);     // (DBG & 256, ablation: two planes)
    };
    auto wait_b = [&](int buf, bool all) {   // group's fragments landed; `all`: every LDS read of this wave retired
        if constexpr (DBG & 32) return;
        if (all) rs_wait_frag<NPL, 0>(fb[buf]);
        else rs_wait_frag<NPL, (DBG & 256) ? 2 : NPL>(fb[buf]);         // the next group's NPL reads may fly
    };
    f32x16 acc[MS][NTW];

    // ---- prologue: B steps 0 and 1, A step 0 ---------------------------------------------------------------------------------
    setup_b(pb_tile);
    setup_a(pa_tile);
    bf16x8 fa_res[AR ? AR : 1][2][2];                                   // AR: [k-tile][k-step][plane] of the block's row tile
    if constexpr (AR != 0) {                                            // ... loaded and split here, before any weight piece is in flight
#pragma unroll
        for (int t = 0; t < (AR ? AR : 1); ++t) {
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4*>(asrc[0] + t * BK + 4 * q);
            h2_split8(v[0], v[1], h2_sa, fa_res[t][0][0], fa_res[t][0][1]);
            h2_split8(v[2], v[3], h2_sa, fa_res[t][1][0], fa_res[t][1][1]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < PW; ++i) issue_b(i);
    advance_b();
    if constexpr (AR == 0) load_a(true);                                // BEFORE step 1's pieces: 6 VMEM operations follow the A
#pragma unroll                                                          // loads on every path into the loop, as inside it
    for (int i = 0; i < PW; ++i) issue_b(i);
    if (total > 1) advance_b();
    __builtin_amdgcn_s_waitcnt(VM_WAIT_STEP);                           // vmcnt(4 MS + PW): step 0's pieces landed
    asm volatile("s_barrier" ::: "memory");
    read_b(0, 0, 0);
    if constexpr (CS == 1) read_b(1, 0, 1);

    int tile = blockIdx.x, kt = 0, stage = 0;
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[ms][t][k] = 0.f;
    int step = 0;
    for (; tile < tile_end; tile += gridDim.x) {
    // (AR: the k-tiles unrolled, so that each step names its resident registers directly -- fa is an alias then, not a copy)
#pragma unroll KT_UNROLL
    for (kt = 0; kt < (AR ? AR : nk); ++kt, ++step) {
        // ---- step start: A of this step -> bf16 terms (the compiler waits for the loads here), next step's A into flight ----
        if constexpr (AR != 0) {                                        // resident: this k-tile's terms out of the block's registers
#define RS_AR_PICK(KT)                                                                                     \
            if constexpr (KT < (AR ? AR : 1)) {                                                            \
                if (kt == KT) {                                                                            \
                    fa[0][0][0] = fa_res[KT][0][0]; fa[0][0][1] = fa_res[KT][0][1];                        \
                    fa[0][1][0] = fa_res[KT][1][0]; fa[0][1][1] = fa_res[KT][1][1];                        \
                }                                                                                          \
            }
            RS_AR_PICK(0) RS_AR_PICK(1) RS_AR_PICK(2) RS_AR_PICK(3)
#undef RS_AR_PICK
        } else {
        mask_a();
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
            if constexpr (DBG & 64) {                                   // ablation: no split (the loaded bits as operands)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        fa[ms][s2][pl] = __builtin_bit_cast(bf16x8, an[ms][2 * s2 + (pl & 1)]);
            } else if constexpr (H2 != 0) {
                h2_split8(an[ms][0], an[ms][1], h2_sa, fa[ms][0][0], fa[ms][0][1]);
                h2_split8(an[ms][2], an[ms][3], h2_sa, fa[ms][1][0], fa[ms][1][1]);
            } else {
                rs_split8(an[ms][0], an[ms][1], fa[ms][0][0], fa[ms][0][1], fa[ms][0][2]);
                rs_split8(an[ms][2], an[ms][3], fa[ms][1][0], fa[ms][1][1], fa[ms][1][2]);
            }
        }
        }   // !AR
        __builtin_amdgcn_sched_barrier(0);
        const bool has_a = step + 1 < total, has_b = step + 2 < total;
        if constexpr (AR == 0) load_a(has_a);
        __builtin_amdgcn_sched_barrier(0);
        const int nstage = stage == NS - 1 ? 0 : stage + 1;
        if constexpr (CS == 2) {
#pragma unroll
            for (int q = 0; q < 2 * NTW; ++q) {
                // this group's three fragments were issued a whole group (12 MFMAs) ago
                rs_wait_frag<3, 0>(fb[q & 1]);
                if (q + 1 < 2 * NTW) {
                    read_b((q + 1) & 1, stage, q + 1);
                } else {
                    // this wave is done reading stage `stage`; publish step + 1
                    __builtin_amdgcn_s_waitcnt(VM_WAIT_STEP);
                    asm volatile("s_barrier" ::: "memory");
                    if (has_a) read_b(0, nstage, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int term = 0; term < 6; ++term)
#pragma unroll
                    for (int ms = 0; ms < MS; ++ms) acc[ms][q % NTW] = rs_mma_term<0>(term, fa[ms][q / NTW], fb[q & 1], acc[ms][q % NTW]);
                __builtin_amdgcn_sched_barrier(0);
                if (q < PW) {
                    if constexpr (!(DBG & 1)) issue_b(q);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (q < 14) {
                wait_b(q & 3, false);
                read_b((q + 2) & 3, stage, q + 2);
            } else if (q == 14) {
                // groups 14 and 15 are in registers and this wave is done reading stage `stage`; publish step + 1
                wait_b(2, true);
                __builtin_amdgcn_s_waitcnt(VM_WAIT_STEP);              // all but this step's 4 MS A loads + PW pieces
                if constexpr (!(DBG & 512)) asm volatile("s_barrier" ::: "memory");   // (DBG 512, ablation: what the step's rendezvous costs -- racy garbage)
                if (has_a) read_b(0, nstage, 0);
            } else {
                if (has_a) read_b(1, nstage, 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!(DBG & 2)) {
                // (MS == 2: the two row sets' chains interleaved or one after the other -- fenced, or the machine scheduler re-interleaves
                // them -- measure the same)
                // (DBG & 128, ablation only: THREE products per fragment pair -- what a two-plane fp16 split would issue)
#pragma unroll
                for (int term = (!H2 && (DBG & 128)) ? 3 : 0; term < RS_TERMS<H2>; ++term)
#pragma unroll
                    for (int ms = 0; ms < MS; ++ms) acc[ms][q & 7] = rs_mma_term<H2>(term, fa[ms][q >> 3], fb[q & 3], acc[ms][q & 7]);
            } else {
                acc[0][q & 7][0] += (float)fa[0][q >> 3][0][0] + (float)fb[q & 3][0][0] + (float)fb[q & 3][1][0] + (H2 ? 0.f : (float)fb[q & 3][2][0]);
            }
            __builtin_amdgcn_sched_barrier(0);    // keeps the next group's lgkmcnt wait from being hoisted between these MFMAs
            if (MS == 2 ? q < PW : ((q & 1) == 1 && q < 2 * PW)) {
                if constexpr (!(DBG & 1)) issue_b(MS == 2 ? q : q >> 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        }   // CS == 1
        if (has_b) advance_b();
        stage = nstage;
    }
        // ---- epilogue of an output tile: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        {
            const int lid = lid_of(tile);
            const int64_t tm0 = (int64_t)(lid / tiles_n) * BM;
            const int tn0 = (lid % tiles_n) * BN;
            const bool relu = g.act == 1;
#pragma unroll
          for (int ms = 0; ms < MS; ++ms) {
            const int64_t r0 = tm0 + rgi * (32 * MS) + 32 * ms + 4 * hi;
            const int cb0 = tn0 + chi * (NTW * 32);                     // first column of this wave's column tiles
            // interior tiles: every load / store of the epilogue unconditional (a memory operation under a divergent branch makes
            // hipcc wait vmcnt(0) in front of each one); edge tiles take the guarded loop
            const bool interior = tm0 + BM <= g.M && tn0 + BN <= g.N;
            constexpr bool cross = EPI == 2;
            if constexpr (EPI == 4) {
                // top-K filter: nothing is stored unless a score beats its row's threshold -- rare once tau has warmed up (expected
                // k / items_seen of a chunk), plentiful in the first filtered chunks (~400 per row right behind the dense chunk).
                // Written in round 2 as "per (register, column tile): ballot, one atomic by the first survivor, wait for its result,
                // store" -- up to 128 dependent atomic round trips per wave and tile, each behind the previous one's stores (the first
                // filtered chunk took 858 us against 316 us in steady state).  Now: (0) the 16 thresholds of the lane's rows loaded
                // together; (1) a counting pass -- the survivors of each row of this half-wave, summed over the 8 column tiles with
                // scalar popcounts; (2) ONE atomic instruction for the tile: lane r < 16 of each half reserves row r's slots;
                // (3) a storing pass that recomputes the masks (compares are cheap, keeping 128 masks is not).  Stores are
                // unconditional inside a wave-uniform branch: lanes without a survivor repeat the first survivor's store (same address,
                // same data) -- a memory operation under a divergent branch would make hipcc drain vmcnt in front of each one.
                // Which slot of its row's list a candidate lands in is arbitrary, as before (the list's order is total: topk_list.h).
                // lane r < 16 of a half stands for row r of that half: its threshold here, its survivor count and its list slots below
                const int64_t lrow = r0 + (l31 & 3) + 8 * ((l31 >> 2) & 3);
                float tlane = g.tau[lrow < g.M ? lrow : g.M - 1];
                // compared with the RAW accumulators (f16x2: the threshold in accumulator units -- a power-of-two factor, exact): the
                // scaled scores are formed only where one is stored
                if constexpr (H2) tlane = tlane / h2_out;
                if (!(lrow < g.M)) tlane = INFINITY;                    // rows past the edge: nothing passes
                int mycnt = 0;                                          // lane r < 16 of a half: survivors of row r of that half
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    int c_lo = 0, c_hi = 0;                             // (scalar)
                    const float tq = __shfl(tlane, 32 * hi + reg, 64);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        const unsigned long long b = __ballot(cb0 + nt * 32 + l31 < g.N && acc[ms][nt][reg] > tq);
                        c_lo += __popc((unsigned)b);
                        c_hi += __popc((unsigned)(b >> 32));
                    }
                    if (l31 == reg) mycnt = hi ? c_hi : c_lo;
                    __builtin_amdgcn_sched_barrier(0);                  // one register at a time (hoisted, the 128 scaled scores spill)
                }
                if (__ballot(mycnt > 0) != 0ull) {                      // (wave-uniform)
                    int mybase = 0;
                    if (mycnt > 0) mybase = atomicAdd(g.cand_cnt + lrow, mycnt);     // (only lanes l31 < 16 count)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int64_t row = r0 + (reg & 3) + 8 * (reg >> 2);
                        int run = __shfl(mybase, 32 * hi + reg, 64);    // next free slot of this half's row
                        const float tq = __shfl(tlane, 32 * hi + reg, 64);
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt) {
                            const int col = cb0 + nt * 32 + l31;
                            float raw = acc[ms][nt][reg];
                            asm volatile("" : "+v"(raw));               // opaque: else the counting pass's 128 compare results are kept (spilled) for reuse
                            acc[ms][nt][reg] = 0.f;
                            const bool pass = col < g.N && raw > tq;
                            const unsigned long long b = __ballot(pass);
                            if (b == 0ull) continue;                    // (wave-uniform)
                            const float v = H2 ? raw * h2_out : raw;
                            const unsigned half = (unsigned)(b >> (32 * hi));
                            const int pos = run + __popc(half & ((1u << l31) - 1u));
                            run += __popc(half);
                            const bool ok = pass && pos < g.cand_cap;
                            const unsigned long long okb = __ballot(ok);
                            if (okb == 0ull) continue;
                            const int first = __ffsll((long long)okb) - 1;   // (wave-uniform) the survivor the idle lanes repeat
                            int64_t dst = row * g.cand_cap + pos;
                            const int d_lo = __builtin_amdgcn_readlane((int)(dst & 0xffffffffll), first);
                            const int d_hi = __builtin_amdgcn_readlane((int)(dst >> 32), first);
                            const float v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), first));
                            const int c1 = __builtin_amdgcn_readlane(col, first);
                            if (!ok) dst = ((int64_t)d_hi << 32) | (uint32_t)d_lo;
                            g.cand_s[dst] = ok ? v : v1;
                            g.cand_c[dst] = ok ? col : c1;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt) acc[ms][nt][reg] = 0.f;
                }
            } else if constexpr (EPI == 6 || EPI == 7) {
                // in-batch softmax on the scores of this tile (see RsArgs).  Lane r < 16 of a half stands for row r of that half (its
                // candidate id, lse, weight: one load each per tile, handed out by shuffles); a lane's 8 columns keep their
                // correction and id in registers.  Exponentials by v_exp_f32 (__expf: 2 ulp): the arguments carry the products' 1e-6
                // already, and libm's expf was a third of this epilogue (128 per lane and tile).
                constexpr float MIN_FLOAT = -3.4028234663852886e36f;    // np.finfo(np.float32).min / 100 (sbcnm.py:10)
                const bool ids_on = g.sm_cand_ids != nullptr;
                const int64_t lrow = r0 + (l31 & 3) + 8 * ((l31 >> 2) & 3);
                const int64_t lrc = lrow < g.M ? lrow : g.M - 1;
                const int64_t rid_l = ids_on ? g.sm_cand_ids[lrc] : 0;
                float lse_l = 0.f, w_l = 1.f;
                if constexpr (EPI == 7) {
                    lse_l = g.sm_lse[lrc];
                    w_l = g.sm_w != nullptr ? g.sm_w[lrc] : 1.f;
                }
                float colcorr[NTW];
                int64_t colid[NTW];
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    const int col = cb0 + nt * 32 + l31;
                    const int cc = col < g.N ? col : g.N - 1;
                    colcorr[nt] = g.sm_cand_prob != nullptr ? -logf(g.sm_cand_prob[cc]) : 0.f;
                    colid[nt] = ids_on ? g.sm_cand_ids[cc] : 0;
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t row = r0 + (reg & 3) + 8 * (reg >> 2);
                    const bool rv = row < g.M;
                    const int src = 32 * hi + reg;
                    const int rlo = __shfl((int)(rid_l & 0xffffffffll), src, 64), rhi = __shfl((int)(rid_l >> 32), src, 64);
                    const int64_t rid = ((int64_t)rhi << 32) | (uint32_t)rlo;
                    float sv[NTW];
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        float v = fmaf(acc[ms][nt][reg], h2_out, colcorr[nt]);
                        acc[ms][nt][reg] = 0.f;
                        if (ids_on && rid == colid[nt] && row != cb0 + nt * 32 + l31) v += MIN_FLOAT;
                        sv[nt] = v * g.sm_inv_t;
                    }
                    if constexpr (EPI == 6) {
                        float m = -INFINITY;
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt)
                            if (cb0 + nt * 32 + l31 < g.N) m = fmaxf(m, sv[nt]);
#pragma unroll
                        for (int o = 1; o < 32; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                        float l = 0.f;
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt)
                            if (cb0 + nt * 32 + l31 < g.N) l += (sv[nt] - m < -87.f ? 0.f : __expf(sv[nt] - m));
#pragma unroll
                        for (int o = 1; o < 32; o <<= 1) l += __shfl_xor(l, o, 64);
                        if (rv && l31 == 0) {
                            const int64_t pc = tn0 / BN;
                            g.sm_part_m[pc * g.M + row] = m;
                            g.sm_part_l[pc * g.M + row] = l;
                        }
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt)
                            if (rv && row == cb0 + nt * 32 + l31) g.sm_pos[row] = sv[nt];
                    } else {
                        const float lse = __shfl(lse_l, src, 64), w = __shfl(w_l, src, 64);
                        const float scale = w * g.sm_inv_t * g.sm_alpha;
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt) {
                            const int col = cb0 + nt * 32 + l31;
                            const float d = sv[nt] - lse;
                            const float pr = (d < -87.f ? 0.f : __expf(d)) - (row == col ? 1.f : 0.f);
                            if (interior) g.C[row * g.ldc + col] = pr * scale;
                            else if (rv && col < g.N) g.C[row * g.ldc + col] = pr * scale;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);                  // one row at a time (hoisted, the exponentials' temporaries spill)
                }
            } else if constexpr (EPI == 5 && H2 != 0) {
                // The pack epilogue, second construction (round 5; the bf16x3 one below moves 4 bytes per lane and instruction and lost to
                // dgrad + pack by 27 %).  Each 32 x 32 accumulator block goes through a per-wave LDS buffer, row-major, and comes back
                // as float4s with 8 lanes on one row: a row's 32 columns of a field are ONE 128-byte line of its destination row and of
                // the x row it reads -- 16-byte loads and stores, 4 passes of 8 rows per block.  Loads unconditional (rows clamped);
                // stores unconditional on interior row tiles (a memory operation under a per-lane condition makes hipcc drain vmcnt
                // in front of each one); the first-order copy is written by all 8 lanes of a row (one address, one value).
                // (the launcher admits this epilogue for interior tiles only -- M a multiple of 256 -- with the FM term present and
                // destinations that fit 32 bits: no per-lane guards, no optional loads)
                const int kemb = min(64 * g.pack_F, g.N);
                float* stg = reinterpret_cast<float*>(smem + NS * STAGE + wave * PK_WAVE);
                const int64_t rw0 = r0 - 4 * hi;                                        // the wave's first row
                const int prow = lane >> 3, pd4 = (lane & 7) * 4;                       // storing pass: row within the 8-row group, column
                const int f0 = cb0 >> 6;                                                // the tile's first field (4 fields per 256 columns)
                // per tile: the wave's 32 x 4 destinations (x 64: float offsets) and its rows' d_fm_logit, through the LDS (lane -> row lane / 2,
                // fields 2 (lane & 1) + {0, 1}; lanes < 32 -> d_fm_logit of row lane)
                int* pk_pos = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(stg) + PK_STG);
                float* pk_dl = reinterpret_cast<float*>(pk_pos + 128);
                {
                    const int64_t prw = rw0 + (lane >> 1);
                    const int fa0 = min(f0 + 2 * (lane & 1), g.pack_F - 1), fa1 = min(f0 + 2 * (lane & 1) + 1, g.pack_F - 1);
                    const int64_t q0 = g.pack_pos[prw * g.pack_F + fa0], q1 = g.pack_pos[prw * g.pack_F + fa1];
                    const float dlr = g.pack_dl[rw0 + l31];
                    pk_pos[(lane >> 1) * 4 + 2 * (lane & 1)] = (int)q0 * 64;
                    pk_pos[(lane >> 1) * 4 + 2 * (lane & 1) + 1] = (int)q1 * 64;
                    if (hi == 0) pk_dl[l31] = dlr;
                }
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    const int cg = cb0 + nt * 32;                                       // (uniform) first column of the block
                    if (cg >= kemb) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) acc[ms][nt][reg] = 0.f;
                        continue;
                    }
                    const int fi = nt >> 1, hb = nt & 1, dbase = 32 * hb;
                    float4 xv[4], sxv[4];
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int64_t row = rw0 + 8 * it + prow;
                        xv[it] = *reinterpret_cast<const float4*>(g.xin + row * g.ldx + cg + pd4);
                        sxv[it] = *reinterpret_cast<const float4*>(g.pack_sumx + row * 64 + dbase + pd4);
                    }
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        stg[((reg & 3) + 8 * (reg >> 2) + 4 * hi) * PK_PITCH + l31] = acc[ms][nt][reg] * h2_out;
                        acc[ms][nt][reg] = 0.f;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // (one wave, in-order LDS: written before it is read)
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        float4 v = *reinterpret_cast<const float4*>(stg + (8 * it + prow) * PK_PITCH + pd4);
                        const int pp = pk_pos[(8 * it + prow) * 4 + fi];
                        const float dl = pk_dl[8 * it + prow];
                        v.x += dl * (sxv[it].x - xv[it].x); v.y += dl * (sxv[it].y - xv[it].y);
                        v.z += dl * (sxv[it].z - xv[it].z); v.w += dl * (sxv[it].w - xv[it].w);
                        *reinterpret_cast<float4*>(g.C + pp + dbase + pd4) = v;
                        if (hb == 0 && g.pack_lin != nullptr) g.pack_lin[pp >> 6] = dl;            // (uniform condition; 8 lanes, one address, one value)
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // the block's reads retired before the next block's writes
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if constexpr (EPI == 5) {
                // Every load unconditional (clamped).  The stores are under WAVE-UNIFORM conditions only: a 32-column group lies inside
                // one field or entirely behind the embeddings (64 F and the group width are multiples of 32), and all rows of an
                // interior row tile exist -- a store under a per-lane condition makes hipcc drain vmcnt in front of each one (the
                // first version, with per-lane guards: 627 us for the half batch instead of 175 + 150).  A group's 32 lanes write
                // one contiguous 128-byte piece of the destination row.
                const bool fmterm = g.pack_sumx != nullptr;
                const float* sxp = fmterm ? g.pack_sumx : g.pack_dl;
                const float* xp = fmterm ? g.xin : g.pack_dl;
                const int64_t xld = fmterm ? g.ldx : 0, sxld = fmterm ? 64 : 0;
                const int kemb = min(64 * g.pack_F, g.N);
                const bool rows_in = tm0 + BM <= g.M;
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    const int cg = cb0 + nt * 32;                                       // (uniform) first column of the group
                    if (cg >= kemb) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) acc[ms][nt][reg] = 0.f;
                        continue;
                    }
                    const int col = cg + l31;
                    const int f = cg >> 6, d = col & 63;
                    const bool lin_here = (cg & 63) == 0 && g.pack_lin != nullptr;      // (uniform) the group that holds d == 0
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        int64_t pp[4];
                        float dlv[4], sxv[4], xv[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int64_t row = r0 + e + 8 * c4;
                            const int64_t rc = row < g.M ? row : g.M - 1;
                            pp[e] = g.pack_pos[rc * g.pack_F + f];
                            dlv[e] = g.pack_dl[rc];
                            sxv[e] = sxp[rc * sxld + (fmterm ? d : 0)];
                            xv[e] = xp[rc * xld + (fmterm ? col : 0)];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int reg = 4 * c4 + e;
                            float v = acc[ms][nt][reg];
                            acc[ms][nt][reg] = 0.f;
                            if (fmterm) v += dlv[e] * (sxv[e] - xv[e]);
                            if (rows_in) {
                                g.C[pp[e] * 64 + d] = v;
                                if (lin_here) g.pack_lin[pp[e]] = dlv[e];               // 32 lanes, one address, one value
                            } else if (r0 + e + 8 * c4 < g.M) {
                                g.C[pp[e] * 64 + d] = v;
                                if (lin_here) g.pack_lin[pp[e]] = dlv[e];
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);     // (four rows at a time: hoisted across groups, the loads spill 93 registers)
                    }
                }
            } else {
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int col = cb0 + nt * 32 + l31;
                const bool cv = col < g.N;
                float bj = g.bias != nullptr ? g.bias[cv ? col : g.N - 1] : 0.f;
                asm volatile("" : "+v"(bj));      // consume the load on every path (see bf3_gemm_nt_pipe_kernel, bf3_planes.hip)
                if (interior) {
                    float* crow = g.C + r0 * g.ldc + col;
                    if constexpr (cross) {
                        const int64_t xo = r0 * g.ldx + col;
#pragma unroll
                        for (int c4 = 0; c4 < 4; ++c4) {             // four rows at a time: short-lived temporaries (the 128
                            float x0v[4], xv[4];                      // accumulators are all live here)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                x0v[e] = g.x0[xo + (int64_t)(e + 8 * c4) * g.ldx];
                                xv[e] = g.xin[xo + (int64_t)(e + 8 * c4) * g.ldx];
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int reg = 4 * c4 + e;
                                const float pr = (H2 ? fmaf(acc[ms][nt][reg], h2_out, bj) : acc[ms][nt][reg] + bj) + g.diag * xv[e];
                                acc[ms][nt][reg] = 0.f;
                                if (g.prod_out != nullptr) g.prod_out[xo + (int64_t)(e + 8 * c4) * g.ldx] = pr;
                                const float o = fmaf(x0v[e], pr, xv[e]);
                                if constexpr (H2) cmax = fmaxf(cmax, fabsf(o));
                                crow[(int64_t)(e + 8 * c4) * g.ldc] = o;
                            }
                        }
                    } else if constexpr (EPI == 1 || EPI == 3) {
#pragma unroll
                        for (int c4 = 0; c4 < 4; ++c4) {
                            float aux[4];                              // EPI 1: the mask values, EPI 3: the old outputs
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                aux[e] = EPI == 1 ? g.mask[(r0 + e + 8 * c4) * g.ld_mask + col] : crow[(int64_t)(e + 8 * c4) * g.ldc];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int reg = 4 * c4 + e;
                                float v = H2 ? fmaf(acc[ms][nt][reg], h2_out, bj) : acc[ms][nt][reg] + bj;
                                acc[ms][nt][reg] = 0.f;
                                v = relu ? fmaxf(v, 0.f) : v;
                                const float o = EPI == 1 ? (aux[e] > 0.f ? v : 0.f) : aux[e] + v;
                                if constexpr (H2) cmax = fmaxf(cmax, fabsf(o));
                                crow[(int64_t)(e + 8 * c4) * g.ldc] = o;
                            }
                        }
                    } else {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            float v = H2 ? fmaf(acc[ms][nt][reg], h2_out, bj) : acc[ms][nt][reg] + bj;
                            acc[ms][nt][reg] = 0.f;
                            if constexpr (H2) cmax = fmaxf(cmax, relu ? fmaxf(v, 0.f) : fabsf(v));
                            if (DR_NT_DGRAD_STORE && EPI == 0) __builtin_nontemporal_store(relu ? fmaxf(v, 0.f) : v, &crow[(int64_t)((reg & 3) + 8 * (reg >> 2)) * g.ldc]);
                            else crow[(int64_t)((reg & 3) + 8 * (reg >> 2)) * g.ldc] = relu ? fmaxf(v, 0.f) : v;
                        }
                    }
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int64_t row = r0 + (reg & 3) + 8 * (reg >> 2);
                        float v = H2 ? fmaf(acc[ms][nt][reg], h2_out, bj) : acc[ms][nt][reg] + bj;
                        acc[ms][nt][reg] = 0.f;
                        if (!cv || row >= g.M) continue;
                        float* dst = g.C + row * g.ldc + col;
                        if constexpr (cross) {
                            const float xv = g.xin[row * g.ldx + col];
                            const float pr = v + g.diag * xv;
                            if (g.prod_out != nullptr) g.prod_out[row * g.ldx + col] = pr;
                            const float o = fmaf(g.x0[row * g.ldx + col], pr, xv);
                            if constexpr (H2) cmax = fmaxf(cmax, fabsf(o));
                            *dst = o;
                            continue;
                        }
                        v = relu ? fmaxf(v, 0.f) : v;
                        if constexpr (EPI == 1) {
                            if (!(g.mask[row * g.ld_mask + col] > 0.f)) v = 0.f;
                        } else if constexpr (EPI == 3) {
                            v = *dst + v;
                        }
                        if constexpr (H2) cmax = fmaxf(cmax, fabsf(v));
                        *dst = v;
                    }
                }
                // MS == 2: all 256 accumulators live in AGPRs; without a fence per column tile the scheduler copies them out
                // ahead of the stores and spills 265 registers
                if constexpr (MS == 2) __builtin_amdgcn_sched_barrier(0);
            }
            }   // EPI != 4
          }     // ms
            // Stores and loads share vmcnt on gfx9 and hipcc treats a mix of the two as unordered: left pending into the next
            // k-tile, the stores turn its wait for the A registers into vmcnt(0) on EVERY k-tile.  Draining here costs the
            // pipeline one refill per output tile instead.
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
    }
    if constexpr (H2 && EPI != 4) {
        if (g.c_amax != nullptr) {                                      // (kernel-uniform) one load per wave, an atomic only if it raises the record
            uint32_t m = __float_as_uint(cmax);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
            if (lane == 0 && m > __hip_atomic_load(g.c_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(g.c_amax, m);
        }
    }
}

// one launch of the register-split kernel
template <int EPI, int DBG = 0, int MS = 1, int CS = 1, int H2 = 0, int AR = 0>
int rs_run(const RsArgs& g, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((bf3_gemm_rs_kernel<EPI, DBG, MS, CS, H2, AR>), dim3(grid), dim3(512 * CS / MS), 0, stream, g);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
// the plain epilogues, chosen by the arguments: ReLU' mask (1), accumulate (3), bias / ReLU (0)
template <int MS, int CS, int H2>
int rs_run_plain(const RsArgs& g, int grid, hipStream_t stream) {
    if (g.mask != nullptr) return rs_run<1, 0, MS, CS, H2>(g, grid, stream);
    if (g.accumulate) return rs_run<3, 0, MS, CS, H2>(g, grid, stream);
    return rs_run<0, 0, MS, CS, H2>(g, grid, stream);
}

int rs_launch(const RsArgs& g, hipStream_t stream) {
    const int64_t tiles = ((g.M + 255) / 256) * ((g.N + 255) / 256);
    if (tiles > 0x7fffffff) return DR_EINVAL;
    const int grid = (int)(tiles < 256 ? tiles : 256);                  // persistent: one block per CU
    if (g.mask != nullptr && g.accumulate) return DR_EINVAL;            // (no caller needs both)
    // the kernels address B's planes through ONE buffer resource with 32-bit offsets: planes further apart than that would be clamped
    // away and read as zeros without any error -- refuse instead
    if ((int64_t)(g.a_amax != nullptr ? 2 : 3) * g.b_ps * 2 > (int64_t)0x7fffffff) return DR_EINVAL;
    // (read at the first launch of any kind, the ablation variable below too; before the launcher was folded, at the first launch
    // that reached the path concerned: the variables are meant to be set before the process starts)
    // bf16x3 wave shapes: DR_BF3_RS64=1 one 64-row wave per SIMD (MS = 2, see the kernel), =2 8 waves x (64 rows x 128 columns) (MS = CS = 2)
    static const char rs64 = [] { const char* e = getenv("DR_BF3_RS64"); return e != nullptr ? e[0] : '\0'; }();
#ifdef DR_BF3_ABLATE
    // ablations of the bias / ReLU epilogue (tools/exp/h2_ablate.py, rs64_bench.py): DR_BF3_RS_DBG = the kernel's DBG bits -- 32 no
    // fragment reads, 64 no split, 2 no MFMA, 1 no weight DMA, 8 A from cache, 4 B always k-tile 0, 512 no per-step barrier, and their
    // sums; with DR_BF3_RS64=1 on 4 waves x 64 rows
    static const int dbg = [] { const char* e = getenv("DR_BF3_RS_DBG"); return e ? atoi(e) : 0; }();
#define RS_ABL(D, H2) \
    if (dbg == D) return rs64 == '1' ? rs_run<0, D, 2, 1, H2>(g, grid, stream) : rs_run<0, D, 1, 1, H2>(g, grid, stream);
#endif
    if (g.a_amax != nullptr) {                                          // f16x2 operand mode
        if (g.b_amax == nullptr) return DR_EINVAL;
        if (g.c_amax != nullptr && hipMemsetAsync(g.c_amax, 0, sizeof(uint32_t), stream) != hipSuccess) return DR_ELAUNCH;
        if (g.pack_pos != nullptr) return rs_run<5, 0, 1, 1, 1>(g, grid, stream);
        // in-batch softmax.  The streaming kernel: with the resident activations of AR = 4 the epilogue's per-column corrections and
        // ids (24 registers) do not fit beside 64 resident operand registers (30 - 54 spilled, reloaded inside the step loop)
        if (g.sm_part_m != nullptr) return rs_run<6, 0, 1, 1, 1>(g, grid, stream);
        if (g.sm_lse != nullptr) return rs_run<7, 0, 1, 1, 1>(g, grid, stream);
        if (g.tau != nullptr) {
            // the scan's reduction is short (K = the embedding width): resident activations (AR, see the kernel) when K is 128 or 64
            // and the row tiles divide into the grid; the streaming kernel otherwise
            const int tiles_m = (int)((g.M + 255) / 256);
            if ((g.K == 128 || g.K == 64) && tiles_m <= 256) {
                const int ar_grid = 256 / tiles_m * tiles_m;
                return g.K == 128 ? rs_run<4, 0, 1, 1, 1, 4>(g, ar_grid, stream) : rs_run<4, 0, 1, 1, 1, 2>(g, ar_grid, stream);
            }
            return rs_run<4, 0, 1, 1, 1>(g, grid, stream);
        }
        if (g.x0 != nullptr) return rs_run<2, 0, 1, 1, 1>(g, grid, stream);
        {   // round 6: the 16-wave form (h2_occ.hip) for the plain epilogues; the 8-wave kernel below takes what it declines
#ifdef DR_OCC_ABLATE
            // tools/exp/occ_bench.py, occ_ablate.py, fused_k4_bench.py: DR_H2_OCC=0 keeps the 8-wave kernel (A/B)
            static const bool occ = [] { const char* e = getenv("DR_H2_OCC"); return e == nullptr || e[0] != '0'; }();
#else
            constexpr bool occ = true;
#endif
            if (occ) {
                const int rc = occ_nt_launch(g, stream);
                if (rc != 1) return rc;
            }
        }
#ifdef DR_BF3_ABLATE
        if (g.mask == nullptr && !g.accumulate) {
            RS_ABL(0, 1) RS_ABL(32, 1) RS_ABL(64, 1) RS_ABL(96, 1) RS_ABL(2, 1) RS_ABL(1, 1)
            // what the no-MFMA time (131 us of the plain forward's 223) is made of: 34 = no MFMA + no fragment reads, 3 = + no weight DMA,
            // 10 = + A from cache, 98 = + no reads + no split, 35 = + no reads + no DMA, 43 = that + A from cache (what is left: the loop,
            // the barrier, the epilogue stores)
            RS_ABL(34, 1) RS_ABL(3, 1) RS_ABL(10, 1) RS_ABL(98, 1) RS_ABL(35, 1) RS_ABL(43, 1)
            // round 5, WITH the MFMAs: 8 = A from cache, 4 = B always k-tile 0, 12 = both, 9 = no weight DMA + A from cache
            RS_ABL(8, 1) RS_ABL(4, 1) RS_ABL(12, 1) RS_ABL(9, 1)
            // 512 = no per-step barrier; 544 = that + no fragment reads; 521 = that + A from cache + no weight DMA
            RS_ABL(512, 1) RS_ABL(544, 1) RS_ABL(521, 1)
        }
#endif
        return rs_run_plain<1, 1, 1>(g, grid, stream);
    }
    if (g.tau != nullptr) return rs_run<4>(g, grid, stream);
    if (g.pack_pos != nullptr) return rs_run<5>(g, grid, stream);
#ifdef DR_BF3_ABLATE
    if (dbg != 0 && g.x0 == nullptr && g.mask == nullptr && !g.accumulate) {
        RS_ABL(32, 0) RS_ABL(64, 0) RS_ABL(96, 0) RS_ABL(2, 0) RS_ABL(1, 0) RS_ABL(128, 0) RS_ABL(384, 0) RS_ABL(448, 0)
    }
#undef RS_ABL
#endif
    if (g.x0 != nullptr) return rs_run<2>(g, grid, stream);
    if (rs64 == '2') return rs_run_plain<2, 2, 0>(g, grid, stream);
    if (rs64 == '1') return rs_run_plain<2, 1, 0>(g, grid, stream);
    return rs_run_plain<1, 1, 0>(g, grid, stream);
}

}  // namespace

// C[m][n] (+)= act(sum_k A[m][k] B[n][k] + bias[n]) (zeroed where mask[m][n] <= 0).  A: fp32 [M, K] row-major (ld multiple of 4,
// 16-byte aligned base); B: planes [3][N][b_ld], b_ld >= roundup(K, 32), columns [K, roundup(K, 32)) zero.
extern "C" int dr_bf3_linear_nt(const float* A, int64_t lda, const void* b_planes, int64_t b_plane_stride, int64_t b_ld, int64_t M,
                                int32_t N, int32_t K, const float* bias, int32_t act, const float* mask, int64_t ld_mask,
                                int32_t accumulate, float* C, int64_t ldc, dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || act < 0 || act > 1) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!A || !C || !planes_ok(b_planes, b_plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(A) & 15) != 0 || (lda & 3) != 0 || lda < K) return DR_EINVAL;
    if (b_ld < (K + BK - 1) / BK * BK || ldc < N || (mask != nullptr && ld_mask < N)) return DR_EINVAL;
    RsArgs g{A, lda, static_cast<const __bf16*>(b_planes), b_plane_stride, b_ld, M, N, K, C, ldc, bias, act, mask, ld_mask, accumulate,
             nullptr, nullptr, 0, 0.f, nullptr};
    return rs_launch(g, dr_s(stream));
}

// dr_bf3_linear_nt in the f16x2 mode: b_planes = two fp16 planes (dr_h2_split with b_amax), A fp32 with the record a_amax.
// c_amax (may be NULL): reset, then raised to max |value stored into C| -- the record the next GEMM wants for C as ITS operand.
extern "C" int dr_h2_linear_nt(const float* A, int64_t lda, const uint32_t* a_amax, const void* b_planes, int64_t b_plane_stride,
                               int64_t b_ld, const uint32_t* b_amax, int64_t M, int32_t N, int32_t K, const float* bias, int32_t act,
                               const float* mask, int64_t ld_mask, int32_t accumulate, float* C, int64_t ldc, uint32_t* c_amax,
                               dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || act < 0 || act > 1 || !a_amax || !b_amax) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!A || !C || !planes_ok(b_planes, b_plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(A) & 15) != 0 || (lda & 3) != 0 || lda < K) return DR_EINVAL;
    if (b_ld < (K + BK - 1) / BK * BK || ldc < N || (mask != nullptr && ld_mask < N)) return DR_EINVAL;
    RsArgs g{A, lda, static_cast<const __bf16*>(b_planes), b_plane_stride, b_ld, M, N, K, C, ldc, bias, act, mask, ld_mask, accumulate,
             nullptr, nullptr, 0, 0.f, nullptr};
    g.a_amax = a_amax;
    g.b_amax = b_amax;
    g.c_amax = c_amax;
    return rs_launch(g, dr_s(stream));
}

// dr_bf3_cross_fwd in the f16x2 mode (DCN cross layer, keras/models/ranking/dcn.py:81-88): x_amax the record of x (the GEMM's
// activation operand), wt_planes two fp16 planes of W^T with w_amax; out_amax (may be NULL) receives the record of `out`, which is
// the next cross layer's x.
extern "C" int dr_h2_cross_fwd(const float* x0, const float* x, int64_t ld, const uint32_t* x_amax, const void* wt_planes,
                               int64_t plane_stride, int64_t ld_planes, const uint32_t* w_amax, const float* b, float diag_scale,
                               int64_t M, int32_t Dm, float* out, float* prod_out, uint32_t* out_amax, dr_stream_t stream) {
    if (M < 0 || Dm <= 0 || diag_scale < 0.f || !x_amax || !w_amax) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x0 || !x || !out || !planes_ok(wt_planes, plane_stride, ld_planes)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || (ld & 3) != 0 || ld < Dm || ld_planes < (Dm + BK - 1) / BK * BK) return DR_EINVAL;
    RsArgs g{x, ld, static_cast<const __bf16*>(wt_planes), plane_stride, ld_planes, M, Dm, Dm, out, ld, b, 0, nullptr, 0, 0,
             x0, x, ld, diag_scale, prod_out};
    g.a_amax = x_amax;
    g.b_amax = w_amax;
    g.c_amax = out_amax;
    return rs_launch(g, dr_s(stream));
}

// dr_bf3_scores_filter in the f16x2 mode (retrieval.hip's top-K scan)
int dr_h2_scores_filter(const float* a, int64_t lda, const uint32_t* a_amax, const void* b_planes, int64_t b_plane_stride, int64_t b_ld,
                        const uint32_t* b_amax, int64_t M, int32_t N, int32_t K, const float* tau, float* cand_s, int32_t* cand_c,
                        int32_t* cand_cnt, int64_t cand_cap, dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || cand_cap <= 0 || !a_amax || !b_amax) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!a || !tau || !cand_s || !cand_c || !cand_cnt || !planes_ok(b_planes, b_plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a) & 15) != 0 || (lda & 3) != 0 || lda < K || b_ld < (K + BK - 1) / BK * BK) return DR_EINVAL;
    RsArgs g{a, lda, static_cast<const __bf16*>(b_planes), b_plane_stride, b_ld, M, N, K, nullptr, 0, nullptr, 0, nullptr, 0, 0,
             nullptr, nullptr, 0, 0.f, nullptr, tau, cand_s, cand_c, cand_cnt, cand_cap};
    g.a_amax = a_amax;
    g.b_amax = b_amax;
    return rs_launch(g, dr_s(stream));
}

namespace {
__global__ __launch_bounds__(256) void bf3_pack_bias_kernel(const float* dl, int64_t n, float* bias_sum) {
    dr_block_sum_axpy(dl, n, 1.f, bias_sum);
}
}  // namespace

// First-layer dgrad of a tower whose input is the concatenation of F 64-wide embeddings (+ dense features) fused with
// dr_emb_pack_grads: the gradient of slot (m, f) -- sum_k dy[m][k] W[64 f + d][k] + d_fm_logit[m] (sum_x[m][d] - x[m][64 f + d]) --
// goes straight to out_rows[pos[m, f], d], the all-to-all send layout; d_concat is never written (0.44 GB less written and 0.66 GB
// less read per 65 536 examples than dgrad + pack).  w_planes: W as planes [3][K_in rows][b_ld] (rows = input features, as for
// dr_bf3_linear_nt's dgrad use); N = number of input features (>= 64 F; the columns behind the embeddings are dropped).
// out_lin (may be NULL): out_lin[pos[m, f]] = d_fm_logit[m].  bias_sum (may be NULL): += sum_m d_fm_logit[m], fixed order.
// sum_x == NULL: no FM term (x / ld_x unused).  pos must be a permutation of the slots, as for dr_emb_pack_grads.
extern "C" int dr_bf3_linear_nt_pack(const float* dy, int64_t ld_dy, const void* w_planes, int64_t plane_stride, int64_t b_ld, int64_t M,
                                     int32_t N, int32_t K, const int64_t* pos, int32_t F, const float* d_fm_logit, const float* sum_x,
                                     const float* x, int64_t ld_x, float* out_rows, float* out_lin, float* bias_sum,
                                     dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || F <= 0 || (int64_t)F * 64 > N) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!dy || !pos || !d_fm_logit || !out_rows || !planes_ok(w_planes, plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(dy) & 15) != 0 || (ld_dy & 3) != 0 || ld_dy < K || b_ld < (K + BK - 1) / BK * BK) return DR_EINVAL;
    if (sum_x != nullptr && (x == nullptr || ld_x < (int64_t)F * 64)) return DR_EINVAL;
    RsArgs g{dy, ld_dy, static_cast<const __bf16*>(w_planes), plane_stride, b_ld, M, N, K, out_rows, 0, nullptr, 0, nullptr, 0, 0,
             nullptr, x, ld_x, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, pos, F, d_fm_logit, sum_x, out_lin};
    const int rc = rs_launch(g, dr_s(stream));
    if (rc != DR_OK) return rc;
    if (bias_sum != nullptr) {
        hipLaunchKernelGGL(bf3_pack_bias_kernel, dim3(1), dim3(256), 0, dr_s(stream), d_fm_logit, M, bias_sum);
        DR_CHECK_LAUNCH();
    }
    return DR_OK;
}

// dr_bf3_linear_nt_pack in the f16x2 operand mode: dy with its amax record, the weights as two fp16 planes with theirs (dr_h2_split).
// x / ld_x: the concatenated embeddings of the forward, rows 16-byte aligned (ld_x % 4 == 0); sum_x rows are 64 floats.
extern "C" int dr_h2_linear_nt_pack(const float* dy, int64_t ld_dy, const uint32_t* dy_amax, const void* w_planes, int64_t plane_stride,
                                    int64_t b_ld, const uint32_t* w_amax, int64_t M, int32_t N, int32_t K, const int64_t* pos, int32_t F,
                                    const float* d_fm_logit, const float* sum_x, const float* x, int64_t ld_x, float* out_rows,
                                    float* out_lin, float* bias_sum, dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || F <= 0 || (int64_t)F * 64 > N) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!dy || !dy_amax || !w_amax || !pos || !d_fm_logit || !out_rows || !planes_ok(w_planes, plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(dy) & 15) != 0 || (ld_dy & 3) != 0 || ld_dy < K || b_ld < (K + BK - 1) / BK * BK) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out_rows) & 15) != 0) return DR_EINVAL;
    if (!sum_x || !x || ld_x < (int64_t)F * 64 || (ld_x & 3) != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(sum_x) & 15) != 0)
        return DR_EINVAL;
    // the epilogue's domain (see there): interior row tiles only, destinations in 32 bits.  Outside it the caller runs
    // dr_h2_linear_nt + dr_emb_pack_grads.
    if ((M % 256) != 0 || M * (int64_t)F >= ((int64_t)1 << 25)) return DR_ESHAPE;
    RsArgs g{dy, ld_dy, static_cast<const __bf16*>(w_planes), plane_stride, b_ld, M, N, K, out_rows, 0, nullptr, 0, nullptr, 0, 0,
             nullptr, x, ld_x, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, pos, F, d_fm_logit, sum_x, out_lin, dy_amax, w_amax,
             nullptr};
    const int rc = rs_launch(g, dr_s(stream));
    if (rc != DR_OK) return rc;
    if (bias_sum != nullptr) {
        hipLaunchKernelGGL(bf3_pack_bias_kernel, dim3(1), dim3(256), 0, dr_s(stream), d_fm_logit, M, bias_sum);
        DR_CHECK_LAUNCH();
    }
    return DR_OK;
}

// internal (C++ linkage, used by retrieval.hip): the top-K scan's scores = a @ B^T on the register-split kernel -- a [M, K] fp32
// queries, B = a corpus chunk as planes [3][N rows][b_ld] -- filtered against tau into per-row candidate lists (the epilogue of
// dense_scores.hip's dr_scores_nt_filter on this file's tile: 256 x 256, weights through the LDS ring, activations split in registers)
int dr_bf3_scores_filter(const float* a, int64_t lda, const void* b_planes, int64_t b_plane_stride, int64_t b_ld, int64_t M, int32_t N,
                         int32_t K, const float* tau, float* cand_s, int32_t* cand_c, int32_t* cand_cnt, int64_t cand_cap,
                         dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || cand_cap <= 0) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!a || !tau || !cand_s || !cand_c || !cand_cnt || !planes_ok(b_planes, b_plane_stride, b_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a) & 15) != 0 || (lda & 3) != 0 || lda < K || b_ld < (K + BK - 1) / BK * BK) return DR_EINVAL;
    RsArgs g{a, lda, static_cast<const __bf16*>(b_planes), b_plane_stride, b_ld, M, N, K, nullptr, 0, nullptr, 0, nullptr, 0, 0,
             nullptr, nullptr, 0, 0.f, nullptr, tau, cand_s, cand_c, cand_cnt, cand_cap};
    return rs_launch(g, dr_s(stream));
}

// internal (C++ linkage, used by dense_scores.hip's dr_inbatch_softmax_*): the in-batch softmax's two score passes on the register-split
// f16x2 kernel.  q [B, D] fp32 with its record, c as two fp16 planes [2][B][c_ld] with its record.
int dr_h2_inbatch_lse(const float* q, int64_t ldq, const uint32_t* q_amax, const void* c_planes, int64_t c_ps, int64_t c_ld,
                      const uint32_t* c_amax, int64_t B, int32_t D, const float* cand_prob, const int64_t* cand_ids, float inv_t,
                      float* part_m, float* part_l, float* pos, dr_stream_t stream) {
    if (B <= 0 || B > 0x7fffffff || !q || !q_amax || !c_amax || !part_m || !part_l || !pos || !planes_ok(c_planes, c_ps, c_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0 || (ldq & 3) != 0 || ldq < D) return DR_EINVAL;
    RsArgs g{};
    g.A = q; g.lda = ldq; g.B = static_cast<const __bf16*>(c_planes); g.b_ps = c_ps; g.b_ld = c_ld; g.M = B; g.N = (int32_t)B; g.K = D;
    g.a_amax = q_amax; g.b_amax = c_amax;
    g.sm_cand_prob = cand_prob; g.sm_cand_ids = cand_ids; g.sm_inv_t = inv_t; g.sm_part_m = part_m; g.sm_part_l = part_l; g.sm_pos = pos;
    return rs_launch(g, dr_s(stream));
}
int dr_h2_inbatch_smgrad(const float* q, int64_t ldq, const uint32_t* q_amax, const void* c_planes, int64_t c_ps, int64_t c_ld,
                         const uint32_t* c_amax, int64_t B, int32_t D, const float* cand_prob, const int64_t* cand_ids, float inv_t,
                         const float* row_lse, const float* sample_weight, float d_loss, float* G, int64_t ld_g, dr_stream_t stream) {
    if (B <= 0 || B > 0x7fffffff || !q || !q_amax || !c_amax || !row_lse || !G || ld_g < B || !planes_ok(c_planes, c_ps, c_ld)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0 || (ldq & 3) != 0 || ldq < D) return DR_EINVAL;
    RsArgs g{};
    g.A = q; g.lda = ldq; g.B = static_cast<const __bf16*>(c_planes); g.b_ps = c_ps; g.b_ld = c_ld; g.M = B; g.N = (int32_t)B; g.K = D;
    g.C = G; g.ldc = ld_g; g.a_amax = q_amax; g.b_amax = c_amax;
    g.sm_cand_prob = cand_prob; g.sm_cand_ids = cand_ids; g.sm_inv_t = inv_t; g.sm_lse = row_lse; g.sm_w = sample_weight; g.sm_alpha = d_loss;
    return rs_launch(g, dr_s(stream));
}

// DCN cross layer forward on pre-split weights (same math as dr_cross_fwd, keras/models/ranking/dcn.py:81-88):
//   prod = x @ W + b + diag_scale * x ;  out = x0 * prod + x ;  prod_out (may be NULL) saves prod for the backward.
// wt_planes: W^T as planes [3][Dm][ld_planes] (dr_bf3_split(..., transpose = 1)).  x0, x, out, prod_out share `ld`.
extern "C" int dr_bf3_cross_fwd(const float* x0, const float* x, int64_t ld, const void* wt_planes, int64_t plane_stride,
                                int64_t ld_planes, const float* b, float diag_scale, int64_t M, int32_t Dm, float* out,
                                float* prod_out, dr_stream_t stream) {
    if (M < 0 || Dm <= 0 || diag_scale < 0.f) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!x0 || !x || !out || !planes_ok(wt_planes, plane_stride, ld_planes)) return DR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || (ld & 3) != 0 || ld < Dm || ld_planes < (Dm + BK - 1) / BK * BK) return DR_EINVAL;
    RsArgs g{x, ld, static_cast<const __bf16*>(wt_planes), plane_stride, ld_planes, M, Dm, Dm, out, ld, b, 0, nullptr, 0, 0,
             x0, x, ld, diag_scale, prod_out};
    return rs_launch(g, dr_s(stream));
}
