// PLANES family: fp32 GEMMs on operands that are pre-split on BOTH sides, and the kernels that make and read planes (split, join,
// amax records, the f16x2 weight split).  Operand format and LDS images: bf3_rs_core.h.
#include "bf3_rs_core.h"
#include "tn_rs_reduce.h"

namespace {

using namespace drrs;

constexpr int NWAVES = 8;
constexpr int NTHREADS = 64 * NWAVES;

// =====================================================================================================================
// NT:  C[m][n] = epilogue( sum_k A[m][k] B[n][k] )
// =====================================================================================================================
struct NtArgs {
    const __bf16* A; int64_t a_ps, a_ld;
    const __bf16* B; int64_t b_ps, b_ld;
    int64_t M; int32_t N; int32_t K;
    float* C; int64_t ldc;
    const float* bias; int32_t act;              // C = act(acc + bias[n])
    const float* mask; int64_t ld_mask;          // optional: C = 0 where mask[m][n] <= 0   (ReLU' of the layer below)
};

// =====================================================================================================================
// NT, three-stage pipeline ("pipe"): the same product on 128 x 128 x 32 tiles with THREE LDS stages, so that the HBM stream
// of the big operand runs one to two k-tiles ahead of the matrix pipe instead of in lock step with it.
//
// What the two-stage 128 x 256 kernel this one replaced measured (M = 65536, K = 1696, N = 256): 369 us, of which the
// pieces -- A stream from HBM 132 us (667 MB at 5.05 TB/s), B tiles from L2 75 us, barrier + fragment reads 106 us, MFMAs
// ~165 us at the clock the chip holds -- run essentially back to back: with two 72 KB stages a k-tile's LDS-DMA is issued one
// k-tile before the barrier that needs it, every wave waits vmcnt(0) there, and the two waves of a SIMD read fragments and
// issue MFMAs in phase with each other.
//
// Here a block's k-tiles form ONE stream of steps g = 0, 1, 2, ... over all its output tiles (stage = g mod 3):
//   H0(g):  fragment reads (g, k-step 1) -> set 1 | 12 MFMAs on set 0, pieces 3..5 of step g+2 between them
//           lgkmcnt(0) (this wave is done with stage g)  ;  vmcnt(6)  (step g+1 has landed; step g+2 may be in flight)
//           s_barrier                                     -> stage of step g+1 published, stage of step g free
//   H1(g):  fragment reads (g+1, k-step 0) -> set 0 | 12 MFMAs on set 1, pieces 0..2 of step g+3 (into step g's stage) between them
// One barrier per k-tile, fragment reads always one phase ahead of their MFMAs, every LDS-DMA piece one and a half to two
// k-tiles ahead of its barrier, the next output tile's first k-tiles in flight under this tile's epilogue.
// The fragment reads and the waits are inline asm: for a ds_read the compiler's wait-count pass conservatively waits for EVERY
// outstanding LDS-DMA (it cannot tell which stage a read touches), which would serialise the pipeline again.
// Ordering rules used (MI355X_MICROARCH.md, LDS-DMA): a staged buffer is read only after the issuing wave's counted vmcnt AND a
// barrier the reader has passed; a stage is re-filled only after a barrier that every wave reaches with its reads of that
// stage retired (the lgkmcnt(0) in front of it).  VMEM operations retire in issue order on gfx9 (one counter for loads and
// stores), so the epilogue's stores only make the counted waits conservative.
// =====================================================================================================================

// NW = 8 (2 x 4 waves of 64 x 32 outputs) or 16 (4 x 4 waves of 32 x 32, four per SIMD; the library launches only this one): an
// LDS-DMA piece costs its wave 100 - 350 cycles of issue time (address coalescer queue), during which only OTHER waves of the SIMD
// can feed the matrix pipe -- with two waves per SIMD the pipe idles about half of the time, with four the stalls overlap.
// DBG (tools/exp/bf3_ablate.hip only; 0 in the library): 1 = no LDS-DMA after the first k-tile, 2 = no MFMAs,
// 4 = LDS-DMA re-reads the first k-tile (cache hits)
template <int NW, int DBG = 0>
__global__ __launch_bounds__(64 * NW, NW / 4) void bf3_gemm_nt_pipe_kernel(NtArgs g) {
    constexpr int BM = 128, BN = 128, NS = 3;
    constexpr int WN = 4, WM = NW / WN, TM = BM / (32 * WM);            // wave grid, MFMA tiles per wave along m (n: one)
    constexpr int A_PLANE = BM * 64, B_PLANE = BN * 64;                 // bytes: rows x 64-byte rows (32 bf16)
    constexpr int STAGE = 3 * (A_PLANE + B_PLANE);                      // 48 KB
    constexpr int KB_A = 3 * A_PLANE / 1024, PW = STAGE / 1024 / NW;    // 24 of the 48 1-KB pieces are A; PW pieces per wave
    constexpr int P1 = (PW + 1) / 2, P0 = PW - P1;                      // issued in H1 (pieces 0..P1-1) / in H0 (the rest)
    static_assert((NW == 8 || NW == 16) && PW * NW * 1024 == STAGE, "wave layout");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, hi = lane >> 5;

    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_m = (int)((g.M + BM - 1) / BM);
    const int ntiles = tiles_m * tiles_n;
    const int nk = g.K / BK;
    if ((int)blockIdx.x >= ntiles) return;
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int total = my_tiles * nk;                                    // steps of this block

    // fragment read addresses (LDS byte address within stage 0), one per k-step: row = 32 TM wm + 32 t + l31 (A) / 32 wn + l31 (B),
    // logical 16-byte chunk 2 ks + hi at physical chunk (2 ks + hi) ^ ((row >> 2) & 3)
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
    const int sw = (l31 >> 2) & 3;
    unsigned a_addr[2], b_addr[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        a_addr[ks] = lds0 + (wm * 32 * TM + l31) * 64 + (((2 * ks + hi) ^ sw) << 4);
        b_addr[ks] = lds0 + 3 * A_PLANE + (wn * 32 + l31) * 64 + (((2 * ks + hi) ^ sw) << 4);
    }

    // ---- producer: the block's LDS-DMA stream -----------------------------------------------------------------------
    const __bf16* src[PW];
    int p_tile = blockIdx.x, p_kt = 0, p_stage = 0;                     // next step to issue, its stage
    auto setup_src = [&](int tile) {
        const int lid = xcd_remap(tile, ntiles);
        const int64_t m0 = (int64_t)(lid / tiles_n) * BM;
        const int n0 = (lid % tiles_n) * BN;
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int j = wave + NW * i;                                // 1-KB piece of the stage (wave-uniform)
            const bool is_a = j < KB_A;
            const int jj = is_a ? j : j - KB_A;
            const int plane = jj >> 3, rb = jj & 7;                     // 8 pieces of 16 rows per plane
            const int row = rb * 16 + (lane >> 2);
            const int c = (lane & 3) ^ ((row >> 2) & 3);
            int64_t grow = (is_a ? m0 : (int64_t)n0) + row;
            const int64_t lim = is_a ? g.M : (int64_t)g.N;
            grow = grow < lim ? grow : lim - 1;                         // rows past the edge only feed unstored outputs
            src[i] = is_a ? g.A + plane * g.a_ps + grow * g.a_ld + c * 8 : g.B + plane * g.b_ps + grow * g.b_ld + c * 8;
        }
    };
    auto issue_piece = [&](int i) {
        lds_dma16(src[i], smem + p_stage * STAGE + (wave + NW * i) * 1024);
        if constexpr (!(DBG & 4)) src[i] += BK;
    };
    auto advance = [&]() {                                              // after the last piece of a step
        p_stage = p_stage == NS - 1 ? 0 : p_stage + 1;
        if (++p_kt == nk) {
            p_kt = 0;
            p_tile += gridDim.x;
            if (p_tile < ntiles) setup_src(p_tile);
        }
    };

    bf16x8 fa[2][3][TM], fb[2][3];                                      // [set][plane][t]: set s holds k-step s of a k-tile
    auto read_set = [&](int set, int stage) {
        const unsigned aa = a_addr[set] + stage * STAGE, bb = b_addr[set] + stage * STAGE;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            BF3_DS_READ_B128(fa[set][p][0], aa, p * A_PLANE);
            if constexpr (TM == 2) BF3_DS_READ_B128(fa[set][p][TM - 1], aa, p * A_PLANE + 32 * 64);
            BF3_DS_READ_B128(fb[set][p], bb, p * B_PLANE);
        }
    };
    auto wait_set = [&](int set) {      // the reads into `set` have landed; ties the MFMAs that follow to the wait
        if constexpr (TM == 2)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(fa[set][0][0]), "+v"(fa[set][0][TM - 1]), "+v"(fa[set][1][0]), "+v"(fa[set][1][TM - 1]),
                           "+v"(fa[set][2][0]), "+v"(fa[set][2][TM - 1]), "+v"(fb[set][0]), "+v"(fb[set][1]), "+v"(fb[set][2]));
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(fa[set][0][0]), "+v"(fa[set][1][0]), "+v"(fa[set][2][0]), "+v"(fb[set][0]), "+v"(fb[set][1]),
                           "+v"(fb[set][2]));
    };
    f32x16 acc[TM];
    // 6 TM MFMAs on `set`; the LDS-DMA pieces [i0, i0 + n) of the producer's current step after terms 0, 2 and 4
    auto mma_phase = [&](int set, int i0, int n, bool dma) {
#pragma unroll
        for (int term = 0; term < 6; ++term) {
            if constexpr (!(DBG & 2)) {
#pragma unroll
                for (int t = 0; t < TM; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][rs_pa(term)][t], fb[set][rs_pb(term)], acc[t], 0, 0, 0);
            } else {
#pragma unroll
                for (int t = 0; t < TM; ++t) acc[t][term] += (float)fa[set][rs_pa(term)][t][0] + (float)fb[set][rs_pb(term)][0];
            }
            if ((term & 1) == 0 && (term >> 1) < n) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (!(DBG & 1)) {
                    if (dma) issue_piece(i0 + (term >> 1));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // ---- prologue: steps 0 and 1 entirely, the first P1 pieces of step 2 ---------------------------------------------------
    setup_src(p_tile);
#pragma unroll
    for (int i = 0; i < PW; ++i) issue_piece(i);
    advance();
    if (total > 1) {
#pragma unroll
        for (int i = 0; i < PW; ++i) issue_piece(i);
        advance();
    }
    if (total > 2) {
#pragma unroll
        for (int i = 0; i < P1; ++i) issue_piece(i);
    }
    if (total > 2) __builtin_amdgcn_s_waitcnt(0x0F70 | ((PW + P1) & 15) | ((((PW + P1) >> 4) & 3) << 14));   // vmcnt(PW + P1)
    else if (total > 1) __builtin_amdgcn_s_waitcnt(0x0F70 | PW);                                             // vmcnt(PW)
    else __builtin_amdgcn_s_waitcnt(0x0F70);                                                                 // vmcnt(0)
    asm volatile("s_barrier" ::: "memory");
    read_set(0, 0);

    int tile = blockIdx.x, kt = 0, stage = 0;
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;
    for (int step = 0; step < total; ++step) {
        // ---- H0 ----
        wait_set(0);
        read_set(1, stage);
        __builtin_amdgcn_sched_barrier(0);
        mma_phase(0, P1, P0, step + 2 < total);                         // the last P0 pieces of step + 2
        if (step + 2 < total) advance();
        wait_set(1);
        if (step + 2 < total) __builtin_amdgcn_s_waitcnt(0x0F70 | PW);  // vmcnt(PW): step + 1 landed, step + 2 may be in flight
        else __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("s_barrier" ::: "memory");
        // ---- H1 ----
        const int nstage = stage == NS - 1 ? 0 : stage + 1;
        if (step + 1 < total) read_set(0, nstage);
        __builtin_amdgcn_sched_barrier(0);
        mma_phase(1, 0, P1, step + 3 < total);                          // the first P1 pieces of step + 3 (into this step's stage)
        stage = nstage;
        if (++kt < nk) continue;
        // ---- epilogue of an output tile: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        kt = 0;
        {
            const int lid = xcd_remap(tile, ntiles);
            const int64_t tm0 = (int64_t)(lid / tiles_n) * BM;
            const int tn0 = (lid % tiles_n) * BN;
            const int col = tn0 + wn * 32 + l31;
            const bool cv = col < g.N;
            const int colc = cv ? col : g.N - 1;
            float bj = g.bias != nullptr ? g.bias[colc] : 0.f;
            // consume the load HERE on every path: left pending into a branch, its register keeps hipcc's wait-count pass
            // inserting a vmcnt(0) at the top of the main loop (which would drain the LDS-DMA pipeline every k-tile)
            asm volatile("" : "+v"(bj));
            const bool relu = g.act == 1;
            // interior tiles (all but the last row / column of tiles): every store unconditional -- a store under a divergent
            // branch makes hipcc wait vmcnt(0) in front of each one
            if (tm0 + BM <= g.M && tn0 + BN <= g.N) {
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
                    const int64_t r0 = tm0 + wm * 32 * TM + mi * 32 + 4 * hi;
                    float* crow = g.C + r0 * g.ldc + col;
                    float mk[16];
                    if (g.mask != nullptr) {
                        const float* mrow = g.mask + r0 * g.ld_mask + col;
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) mk[reg] = mrow[(int64_t)((reg & 3) + 8 * (reg >> 2)) * g.ld_mask];
                    }
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        float v = acc[mi][reg] + bj;
                        acc[mi][reg] = 0.f;
                        v = relu ? fmaxf(v, 0.f) : v;
                        if (g.mask != nullptr) v = mk[reg] > 0.f ? v : 0.f;
                        crow[(int64_t)((reg & 3) + 8 * (reg >> 2)) * g.ldc] = v;
                    }
                }
            } else {
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
                    const int64_t row_b = tm0 + wm * 32 * TM + mi * 32 + 4 * hi;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int64_t row = row_b + (reg & 3) + 8 * (reg >> 2);
                        float v = acc[mi][reg] + bj;
                        acc[mi][reg] = 0.f;
                        if (!cv || row >= g.M) continue;
                        v = relu ? fmaxf(v, 0.f) : v;
                        if (g.mask != nullptr && !(g.mask[row * g.ld_mask + col] > 0.f)) v = 0.f;
                        g.C[row * g.ldc + col] = v;
                    }
                }
            }
        }
        tile += gridDim.x;
    }
}

// =====================================================================================================================
// TN split-K:  partial[s][f][n] = sum_{r in slice s} X[r][f] Y[r][n]
// =====================================================================================================================
struct TnArgs {
    const __bf16* X; int64_t x_ps, x_ld;
    const __bf16* Y; int64_t y_ps, y_ld;
    int64_t R; int32_t F; int32_t N;
    int64_t per; int32_t split;                  // reduction rows per slice (multiple of 32), number of slices
    float* partial;                              // [split][F][N]
};

__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds_ptr_t)const_cast<unsigned char*>(p0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds_ptr_t)const_cast<unsigned char*>(p1));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int WM, int WN>
__global__ __launch_bounds__(NTHREADS, 2) void bf3_gemm_tn_kernel(TnArgs g) {
    constexpr int BM = 64 * WM, BN = 64 * WN;                           // BM: columns of X (output rows f), BN: columns of Y
    constexpr int ROW_A = BM * 2, ROW_B = BN * 2;                        // bytes per reduction row of a plane image
    constexpr int A_PLANE = BK * ROW_A, B_PLANE = BK * ROW_B;
    constexpr int STAGE = 3 * (A_PLANE + B_PLANE);
    constexpr int NKB = STAGE / 1024, KB_A = 3 * A_PLANE / 1024, PER_WAVE = NKB / NWAVES;
    static_assert(WM * WN == NWAVES && NKB % NWAVES == 0, "tile / wave layout");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, hi = lane >> 5, g16 = (lane >> 4) & 1, s = lane & 15;

    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_f = (g.F + BM - 1) / BM;
    const int per_slice = tiles_f * tiles_n;
    const int ntiles = per_slice * g.split;

    // transposing fragment reads: this lane supplies the address of row (8 hi + 4 q + (s >> 2)) of the k-step, 4 elements from
    // column 16 g16 + 4 (s & 3) of the 32-column MFMA tile; it receives column 16 g16 + s, rows 8 hi + 4 q + 0..3
    const int swz = (s >> 2) << 2;
    const int a_off = (8 * hi + (s >> 2)) * ROW_A + ((((wm * 8) ^ swz) + 2 * g16 + ((s & 3) >> 1)) << 4) + ((s & 1) << 3);
    const int b_off = 3 * A_PLANE + (8 * hi + (s >> 2)) * ROW_B + ((((wn * 8) ^ swz) + 2 * g16 + ((s & 3) >> 1)) << 4) + ((s & 1) << 3);

    const __bf16* src[PER_WAVE];
    int64_t src_step[2];
    src_step[0] = (int64_t)BK * g.x_ld;
    src_step[1] = (int64_t)BK * g.y_ld;
    int f0 = 0, n0 = 0, slice = 0, nk = 0;
    auto setup = [&](int tile) {
        const int lid = xcd_remap(tile, ntiles);                        // consecutive logical ids share a reduction slice
        slice = lid / per_slice;
        const int t = lid % per_slice;
        f0 = (t / tiles_n) * BM;
        n0 = (t % tiles_n) * BN;
        const int64_t r0 = (int64_t)slice * g.per;
        int64_t r1 = r0 + g.per;
        const int64_t rpad = (g.R + BK - 1) / BK * BK;
        if (r1 > rpad) r1 = rpad;
        nk = (int)((r1 - r0) / BK);
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int j = wave + NWAVES * i;
            const bool is_a = j < KB_A;
            const int jj = is_a ? j : j - KB_A;
            const int kbs = is_a ? A_PLANE / 1024 : B_PLANE / 1024;
            const int rowb = is_a ? ROW_A : ROW_B;
            const int plane = jj / kbs, kb = jj % kbs;
            const int o = kb * 1024 + lane * 16;
            const int row = o / rowb;
            const int pc = (o % rowb) >> 4;
            const int c = pc ^ ((row & 3) << 2);
            int64_t col = (is_a ? f0 : n0) + c * 8;
            const int64_t ld = is_a ? g.x_ld : g.y_ld;
            col = col <= ld - 8 ? col : ld - 8;                          // columns past the pitch only feed unstored outputs
            src[i] = is_a ? g.X + plane * g.x_ps + (r0 + row) * g.x_ld + col : g.Y + plane * g.y_ps + (r0 + row) * g.y_ld + col;
        }
    };
    auto issue = [&](int stage) {
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int j = wave + NWAVES * i;
            unsigned char* dst = smem + stage * STAGE + j * 1024;
            lds_dma16(src[i], dst);
            src[i] += (j < KB_A) ? src_step[0] : src_step[1];
        }
    };

    f32x16 acc[2][2];
    // same schedule as the NT kernel: fragment reads up front, the next k-tile's LDS-DMA pieces between the first MFMA groups
    auto compute = [&](int stage, bool prefetch) {
        const int sa = stage * STAGE + a_off, sb = stage * STAGE + b_off;
        bf16x8 af[2][3][2], bf[2][3][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const unsigned char* pa = &smem[(sa ^ (t * 64)) + p * A_PLANE + ks * 16 * ROW_A];
                    const unsigned char* pb = &smem[(sb ^ (t * 64)) + p * B_PLANE + ks * 16 * ROW_B];
                    af[ks][p][t] = tr_pair(pa, pa + 4 * ROW_A);
                    bf[ks][p][t] = tr_pair(pb, pb + 4 * ROW_B);
                }
        unsigned char* const dma_dst = smem + (stage ^ 1) * STAGE + wave * 1024;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int term = 0; term < 6; ++term) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][rs_pa(term)][a], bf[ks][rs_pb(term)][b], acc[a][b], 0, 0, 0);
                const int piece = ks * 6 + term;
                if (piece < PER_WAVE) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (prefetch) {
                        lds_dma16(src[piece], dma_dst + NWAVES * piece * 1024);
                        src[piece] += (wave + NWAVES * piece < KB_A) ? src_step[0] : src_step[1];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    };

    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    int buf = 0;
    setup(tile);
    if (nk > 0) issue(buf);
    for (;;) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[a][b][k] = 0.f;
        const int tf0 = f0, tn0 = n0, tslice = slice;
        const int tnk = nk;
        for (int kt = 0; kt < tnk; ++kt) {
            __syncthreads();
            compute(buf, kt + 1 < tnk);
            buf ^= 1;
        }
        const int next = tile + gridDim.x;
        if (next < ntiles) {
            setup(next);
            if (tnk == 1) __syncthreads();        // a one-k-tile tile: stage `buf` may still be read by a slower wave
            if (nk > 0) issue(buf);
        }
        __builtin_amdgcn_sched_barrier(0);
        float* out = g.partial + (int64_t)tslice * g.F * g.N;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int col = tn0 + wn * 64 + ni * 32 + l31;
                const int row_b = tf0 + wm * 64 + mi * 32 + 4 * hi;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int row = row_b + (reg & 3) + 8 * (reg >> 2);
                    if (col < g.N && row < g.F) out[(int64_t)row * g.N + col] = acc[mi][ni][reg];
                }
            }
        if (next >= ntiles) break;
        tile = next;
    }
}

// dst[f][n] += scale * sum_s partial[s][f][n]  (fixed order);  dstb[n] += scale * colsum[n]
__global__ __launch_bounds__(256) void bf3_splitk_reduce_kernel(const float* __restrict__ partial, int32_t split, int64_t F,
                                                                int32_t N, float scale, float* __restrict__ dst, int64_t ld,
                                                                const float* __restrict__ colsum, float* __restrict__ dstb) {
    const int64_t total = F * N;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        float acc = 0.f;
        int sidx = 0;
        for (; sidx + 4 <= split; sidx += 4) {       // four loads in flight, summed in slice order
            const float v0 = partial[(int64_t)sidx * total + i], v1 = partial[(int64_t)(sidx + 1) * total + i];
            const float v2 = partial[(int64_t)(sidx + 2) * total + i], v3 = partial[(int64_t)(sidx + 3) * total + i];
            acc = (((acc + v0) + v1) + v2) + v3;
        }
        for (; sidx < split; ++sidx) acc += partial[(int64_t)sidx * total + i];
        const int64_t f = i / N;
        const int n = (int)(i - f * N);
        dst[f * ld + n] = fmaf(scale, acc, dst[f * ld + n]);
    }
    if (blockIdx.x == 0 && colsum != nullptr && dstb != nullptr)
        for (int n = threadIdx.x; n < N; n += blockDim.x) dstb[n] = fmaf(scale, colsum[n], dstb[n]);
}

// fp32 [R][C] -> planes[p][r0 + r][c0 + c]   (transpose = 0)   or   planes[p][r0 + c][c0 + r]   (transpose = 1)
__global__ __launch_bounds__(256) void bf3_split_kernel(const float* __restrict__ src, int64_t ld_src, int64_t R, int32_t C,
                                                        __bf16* __restrict__ planes, int64_t ps, int64_t ldp, int64_t r0,
                                                        int64_t c0, int32_t transpose) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (!transpose) {
        const int cq = (C + 3) / 4;
        const int64_t total = R * cq;
        const bool vec = (C & 3) == 0 && (c0 & 3) == 0 && (ldp & 3) == 0;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int64_t r = i / cq;
            const int c = (int)(i - r * cq) * 4;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = c + j < C ? src[r * ld_src + c + j] : 0.f;
            const int64_t off = (r0 + r) * ldp + c0 + c;
            if (vec) {
                bf3::store4(planes, ps, off, v[0], v[1], v[2], v[3]);
            } else {
                bf3::bf16x4 p0, p1, p2;
                bf3::split4(v[0], v[1], v[2], v[3], p0, p1, p2);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < C) {
                        planes[off + j] = p0[j];
                        planes[ps + off + j] = p1[j];
                        planes[2 * ps + off + j] = p2[j];
                    }
            }
        }
    } else {
        // a thread takes 4 consecutive rows r of one column c: coalesced reads across c, one 8-byte store per plane
        const int64_t rq = (R + 3) / 4;
        const int64_t total = rq * C;
        const bool vec = (c0 & 3) == 0 && (ldp & 3) == 0;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            const int64_t q = i / C;
            const int c = (int)(i - q * C);
            const int64_t r = q * 4;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = r + j < R ? src[(r + j) * ld_src + c] : 0.f;
            const int64_t off = (r0 + c) * ldp + c0 + r;
            bf3::bf16x4 p0, p1, p2;
            bf3::split4(v[0], v[1], v[2], v[3], p0, p1, p2);
            if (vec && r + 4 <= R) {
                *reinterpret_cast<bf3::bf16x4*>(planes + off) = p0;
                *reinterpret_cast<bf3::bf16x4*>(planes + ps + off) = p1;
                *reinterpret_cast<bf3::bf16x4*>(planes + 2 * ps + off) = p2;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r + j < R) {
                        planes[off + j] = p0[j];
                        planes[ps + off + j] = p1[j];
                        planes[2 * ps + off + j] = p2[j];
                    }
            }
        }
    }
}

// ---- f16x2 mode: amax records and the weight split ---------------------------------------------------------------------------
// amax[0] = max(amax[0], max |src|) as float bits (non-negative floats order like their bit patterns; a NaN lands above inf)
__global__ __launch_bounds__(256) void h2_amax_kernel(const float* __restrict__ src, int64_t ld, int64_t R, int32_t C,
                                                      uint32_t* __restrict__ amax) {
    uint32_t m = 0u;
    const bool al16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    auto take4 = [&](const float4& v) {
        m = max(max(m, __float_as_uint(fabsf(v.x))), max(__float_as_uint(fabsf(v.y)), max(__float_as_uint(fabsf(v.z)), __float_as_uint(fabsf(v.w)))));
    };
    if (ld == C || R == 1) {                                            // contiguous: one flat stream, four 16-byte loads in flight
        const int64_t n = R * (int64_t)C, nv = al16 ? (n >> 2) : 0;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        for (; i + 3 * stride < nv; i += 4 * stride) {
            const float4 v0 = s4[i], v1 = s4[i + stride], v2 = s4[i + 2 * stride], v3 = s4[i + 3 * stride];
            take4(v0); take4(v1); take4(v2); take4(v3);
        }
        for (; i < nv; i += stride) take4(s4[i]);
        for (int64_t j = (nv << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) m = max(m, __float_as_uint(fabsf(src[j])));
    } else {                                                            // padded rows: a block per row (and stride)
        const bool vec = al16 && (ld & 3) == 0;
        const int cv = vec ? (C >> 2) : 0;
        for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
            const float* row = src + r * ld;
            for (int c = threadIdx.x; c < cv; c += blockDim.x) take4(reinterpret_cast<const float4*>(row)[c]);
            for (int c = (cv << 2) + threadIdx.x; c < C; c += blockDim.x) m = max(m, __float_as_uint(fabsf(row[c])));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
        if (m > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax, m);
    }
}

// fp32 [R][C] * s -> two fp16 planes; planes[p][r0 + r][c0 + c] (transpose = 0) or planes[p][r0 + c][c0 + r] (transpose = 1); s from the record
__global__ __launch_bounds__(256) void h2_split_kernel(const float* __restrict__ src, int64_t ld_src, int64_t R, int32_t C,
                                                       _Float16* __restrict__ planes, int64_t ps, int64_t ldp, int64_t r0,
                                                       int64_t c0, int32_t transpose, const uint32_t* __restrict__ amax) {
    float sc, inv;
    h2_scale_of(amax[0], sc, inv);
    h2_mode_on();
    const int64_t total = R * C, stride = (int64_t)gridDim.x * blockDim.x;
    if (!transpose && (C & 3) == 0 && (ldp & 3) == 0 && (c0 & 3) == 0 && (ld_src & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
        (reinterpret_cast<uintptr_t>(planes) & 7) == 0 && (ps & 3) == 0 && total < (int64_t)0x7fffffff) {
        // four columns per thread: one 16-byte load, one 8-byte store per plane (the top-K scan splits the whole corpus through here)
        typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const unsigned cq = (unsigned)C >> 2, tq = (unsigned)(total >> 2);
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < tq; i += (unsigned)stride) {
            const unsigned r = i / cq, c = (i - r * cq) << 2;
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + (int64_t)r * ld_src + c) * sc;
            const f16x4 h = __builtin_convertvector(v, f16x4);
            const f16x4 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x4), f16x4);
            const int64_t off = (r0 + r) * ldp + c0 + c;
            *reinterpret_cast<f16x4*>(planes + off) = h;
            *reinterpret_cast<f16x4*>(planes + ps + off) = l;
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        // consecutive threads: consecutive DESTINATION elements (2-byte stores coalesce; the source is small and cached)
        int64_t r, c, off;
        if (!transpose) { r = i / C; c = i - r * C; off = (r0 + r) * ldp + c0 + c; }
        else { c = i / R; r = i - c * R; off = (r0 + c) * ldp + c0 + r; }
        const float v = src[r * ld_src + c] * sc;
        const _Float16 h = (_Float16)v;
        planes[off] = h;
        planes[ps + off] = (_Float16)(v - (float)h);
    }
}

// ---- a weight's record and BOTH of its plane images in two launches (dr_h2_refresh_weight, round 5) -----------------------------------
// dr_h2_amax + two dr_h2_split are four launches (a 4-byte memset, the atomicMax pass, two splits); in the sharded engine they sit on
// the serial chain between the wgrad and the next forward, where each small launch waits its turn among the exchange's HBM-bound
// kernels (rocprofv3: memset 47 us, amax 30, splits 16 + 6).  Here: per-block maxima with plain stores, then ONE kernel that reduces
// them in every block (256 values), stores the record from block 0 and writes both orientations.  Same record, same planes.
constexpr int H2_REFRESH_PARTS = 256;
__global__ __launch_bounds__(256) void h2_amax_parts_kernel(const float* __restrict__ src, int64_t ld, int64_t R, int32_t C,
                                                            uint32_t* __restrict__ parts) {
    uint32_t m = 0u;
    const int64_t total = R * (int64_t)C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / C;
        m = max(m, __float_as_uint(fabsf(src[r * ld + (i - r * C)])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    __shared__ uint32_t wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
}
__global__ __launch_bounds__(256) void h2_split_both_kernel(const float* __restrict__ src, int64_t ld, int64_t R, int32_t C,
                                                            _Float16* __restrict__ w, int64_t w_ps, int64_t w_ld,
                                                            _Float16* __restrict__ wt, int64_t wt_ps, int64_t wt_ld,
                                                            const uint32_t* __restrict__ parts, int32_t nparts, uint32_t* __restrict__ amax) {
    // (the body lives in tn_rs_reduce.h: the rider blocks behind K4's hot-row launch run the same text)
    h2_split_both_block(H2RefreshRide{src, ld, R, C, w, w_ps, w_ld, wt, wt_ps, wt_ld, parts, nparts, amax},
                        (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x);
}

// planes -> fp32 (tests, debugging): dst[r][c] = (p2 + p1) + p0
__global__ __launch_bounds__(256) void bf3_join_kernel(const __bf16* __restrict__ planes, int64_t ps, int64_t ldp, int64_t R,
                                                       int32_t C, float* __restrict__ dst, int64_t ld_dst) {
    const int64_t total = R * C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        const int64_t off = r * ldp + c;
        dst[r * ld_dst + c] = bf3::join(planes[off], planes[ps + off], planes[2 * ps + off]);
    }
}

}  // namespace

extern "C" int dr_bf3_split(const float* src, int64_t ld_src, int64_t R, int32_t C, void* planes, int64_t plane_stride,
                            int64_t ld_planes, int64_t row_offset, int64_t col_offset, int32_t transpose,
                            dr_stream_t stream) {
    if (R < 0 || C < 0 || ld_src < C || row_offset < 0 || col_offset < 0 || ld_planes <= 0 || plane_stride <= 0) return DR_EINVAL;
    if (R == 0 || C == 0) return DR_OK;
    if (!src || !planes) return DR_EINVAL;
    if (!transpose && col_offset + C > ld_planes) return DR_EINVAL;
    if (transpose && col_offset + R > ld_planes) return DR_EINVAL;
    hipLaunchKernelGGL(bf3_split_kernel, dim3(dr_grid_for(R * ((C + 3) / 4), 256)), dim3(256), 0, dr_s(stream), src, ld_src, R, C,
                       static_cast<__bf16*>(planes), plane_stride, ld_planes, row_offset, col_offset, transpose);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_bf3_join(const void* planes, int64_t plane_stride, int64_t ld_planes, int64_t R, int32_t C, float* dst,
                           int64_t ld_dst, dr_stream_t stream) {
    if (R < 0 || C < 0 || ld_planes < C || ld_dst < C || plane_stride <= 0) return DR_EINVAL;
    if (R == 0 || C == 0) return DR_OK;
    if (!planes || !dst) return DR_EINVAL;
    hipLaunchKernelGGL(bf3_join_kernel, dim3(dr_grid_for(R * C, 256)), dim3(256), 0, dr_s(stream),
                       static_cast<const __bf16*>(planes), plane_stride, ld_planes, R, C, dst, ld_dst);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// C[m][n] = act(sum_k A[m][k] B[n][k] + bias[n]) (* (mask[m][n] > 0)).  K is the PADDED reduction length (multiple of 32);
// columns [true K, K) of both operands' planes must be zero.
extern "C" int dr_bf3_gemm_nt(const void* a_planes, int64_t a_plane_stride, int64_t a_ld, const void* b_planes,
                              int64_t b_plane_stride, int64_t b_ld, int64_t M, int32_t N, int32_t K, const float* bias,
                              int32_t act, const float* mask, int64_t ld_mask, float* C, int64_t ldc, dr_stream_t stream) {
    if (M < 0 || N <= 0 || K <= 0 || (K % BK) != 0 || act < 0 || act > 1) return DR_EINVAL;
    if (M == 0) return DR_OK;
    if (!planes_ok(a_planes, a_plane_stride, a_ld) || !planes_ok(b_planes, b_plane_stride, b_ld) || !C) return DR_EINVAL;
    if (a_ld < K || b_ld < K || ldc < N || (mask != nullptr && ld_mask < N)) return DR_EINVAL;
    NtArgs g{static_cast<const __bf16*>(a_planes), a_plane_stride, a_ld, static_cast<const __bf16*>(b_planes), b_plane_stride, b_ld,
             M, N, K, C, ldc, bias, act, mask, ld_mask};
    // three-stage 128 x 128 x 32 pipeline, 16 waves; consecutive tiles share an A row-panel (same XCD, L2)
    const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
    if (tiles > 0x7fffffff) return DR_EINVAL;
    const int grid = (int)(tiles < 256 ? tiles : 256);                  // persistent: one block per CU
    hipLaunchKernelGGL((bf3_gemm_nt_pipe_kernel<16>), dim3(grid), dim3(1024), 0, dr_s(stream), g);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_bf3_gemm_tn_workspace_bytes(int64_t R, int32_t F, int32_t N) {
    if (R <= 0 || F <= 0 || N <= 0) return 0;
    return (int64_t)tn_split_for(R, F, N, 128, 256) * F * N * (int64_t)sizeof(float);
}

// dst[f][n] += scale * sum_r X[r][f] Y[r][n];  dstb[n] += scale * y_colsum[n] (both optional).  Planes must hold rows up to the
// next multiple of 32 past R, zero-filled.
extern "C" int dr_bf3_gemm_tn(const void* x_planes, int64_t x_plane_stride, int64_t x_ld, const void* y_planes,
                              int64_t y_plane_stride, int64_t y_ld, int64_t R, int32_t F, int32_t N, float scale, float* dst,
                              int64_t ld_dst, const float* y_colsum, float* dstb, void* workspace, int64_t workspace_bytes,
                              dr_stream_t stream) {
    if (R <= 0 || F <= 0 || N <= 0) return DR_EINVAL;
    if (!planes_ok(x_planes, x_plane_stride, x_ld) || !planes_ok(y_planes, y_plane_stride, y_ld) || !dst || !workspace) return DR_EINVAL;
    if (x_ld < F || y_ld < N || ld_dst < N) return DR_EINVAL;
    if (workspace_bytes < dr_bf3_gemm_tn_workspace_bytes(R, F, N)) return DR_EINVAL;
    TnArgs g{static_cast<const __bf16*>(x_planes), x_plane_stride, x_ld, static_cast<const __bf16*>(y_planes), y_plane_stride, y_ld,
             R, F, N, 0, 0, static_cast<float*>(workspace)};
    int split = tn_split_for(R, F, N, 128, 256);
    const int64_t rpad = (R + BK - 1) / BK * BK;
    g.per = ((rpad + split - 1) / split + BK - 1) / BK * BK;
    g.split = (int32_t)((rpad + g.per - 1) / g.per);                    // every launched slice is non-empty
    const int64_t tiles = (int64_t)((F + 127) / 128) * ((N + 255) / 256) * g.split;
    const int grid = (int)(tiles < 256 ? tiles : 256);
    hipLaunchKernelGGL((bf3_gemm_tn_kernel<2, 4>), dim3(grid), dim3(NTHREADS), 0, dr_s(stream), g);
    hipLaunchKernelGGL(bf3_splitk_reduce_kernel, dim3(dr_grid_for((int64_t)F * N, 256)), dim3(256), 0, dr_s(stream), g.partial,
                       g.split, (int64_t)F, N, scale, dst, ld_dst, y_colsum, dstb);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// ---- f16x2 operand mode (see h2_split8): amax records, the weight split, forward / dgrad on fp32 activations -----------------------
// amax[0] = max(reset ? 0 : amax[0], max |src[r][c]|) as float bits.  The record of a GEMM operand must be >= its true largest
// magnitude when the GEMM runs (a producer may keep a running maximum instead of an exact one).
extern "C" int dr_h2_amax(const float* src, int64_t ld, int64_t R, int32_t C, uint32_t* amax, int32_t reset, dr_stream_t stream) {
    if (R < 0 || C < 0 || ld < C || !amax) return DR_EINVAL;
    if (reset && hipMemsetAsync(amax, 0, sizeof(uint32_t), dr_s(stream)) != hipSuccess) return DR_ELAUNCH;
    if (R == 0 || C == 0) return DR_OK;
    if (!src) return DR_EINVAL;
    const int grid = (ld == C || R == 1) ? dr_grid_for(R * ((C + 3) / 4), 256 * 4) : (int)(R < 4096 ? R : 4096);
    hipLaunchKernelGGL(h2_amax_kernel, dim3(grid), dim3(256), 0, dr_s(stream), src, ld, R, C, amax);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// Two fp16 planes of src * s(amax) -- the layout of dr_bf3_split with two planes instead of three.  The GEMMs that read the planes
// are handed the same record (unchanged since the split).
extern "C" int dr_h2_split(const float* src, int64_t ld_src, int64_t R, int32_t C, void* planes, int64_t plane_stride,
                           int64_t ld_planes, int64_t row_offset, int64_t col_offset, int32_t transpose, const uint32_t* amax,
                           dr_stream_t stream) {
    if (R < 0 || C < 0 || ld_src < C || row_offset < 0 || col_offset < 0 || ld_planes <= 0 || plane_stride <= 0 || !amax) return DR_EINVAL;
    if (R == 0 || C == 0) return DR_OK;
    if (!src || !planes) return DR_EINVAL;
    if (!transpose && col_offset + C > ld_planes) return DR_EINVAL;
    if (transpose && col_offset + R > ld_planes) return DR_EINVAL;
    hipLaunchKernelGGL(h2_split_kernel, dim3(dr_grid_for(R * (int64_t)C, 256)), dim3(256), 0, dr_s(stream), src, ld_src, R, C,
                       static_cast<_Float16*>(planes), plane_stride, ld_planes, row_offset, col_offset, transpose, amax);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

// A weight W [K, N] (row stride ldw): its amax record, its planes [2][K][w_ld] and the planes of its transpose [2][N][wt_ld] -- what
// dr_h2_amax(reset) + dr_h2_split + dr_h2_split(transpose) produce, in two launches without a memset or an atomic.  parts: 256 uint32 of scratch.
extern "C" int dr_h2_refresh_weight(const float* W, int64_t ldw, int64_t K, int32_t N, void* w_planes, int64_t w_ps, int64_t w_ld,
                                    void* wt_planes, int64_t wt_ps, int64_t wt_ld, uint32_t* amax, uint32_t* parts, dr_stream_t stream) {
    if (K <= 0 || N <= 0 || ldw < N || !W || !w_planes || !wt_planes || !amax || !parts) return DR_EINVAL;
    if (w_ld < N || wt_ld < K || w_ps <= 0 || wt_ps <= 0) return DR_EINVAL;
    const int64_t total = K * (int64_t)N;
    const int np = (int)(total < (int64_t)H2_REFRESH_PARTS * 256 ? (total + 255) / 256 : H2_REFRESH_PARTS);
    hipLaunchKernelGGL(h2_amax_parts_kernel, dim3(np), dim3(256), 0, dr_s(stream), W, ldw, K, N, parts);
    hipLaunchKernelGGL(h2_split_both_kernel, dim3(dr_grid_for(2 * total, 256, 2048)), dim3(256), 0, dr_s(stream), W, ldw, K, N,
                       static_cast<_Float16*>(w_planes), w_ps, w_ld, static_cast<_Float16*>(wt_planes), wt_ps, wt_ld, parts, np, amax);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
