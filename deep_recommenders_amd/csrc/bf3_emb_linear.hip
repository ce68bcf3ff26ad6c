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

__device__ __forceinline__ int sload_i32(const void* base, int byte_off) {      // scalar load of a wave-uniform word, on the spot
    int v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "s"(byte_off) : "memory");
    return v;
}

// H2: the f16x2 operand mode (h2_split8): two fp16 weight planes (32 KB stages, 4 pieces per wave and k-tile), three MFMAs per
// fragment pair; the activation scale comes from the larger of the table's and the dense features' amax records.
template <int H2>
__global__ __launch_bounds__(512, 2) void bf3_emb_linear_kernel(RsArgs g, EmbArgs e) {
    constexpr int NW = 8, BM = 32 * NW, BN = 256, NT = BN / 32, NS = 2;
    constexpr int NPL = RS_NPL<H2>, STAGE = RS_STAGE<H2>;               // the weight stages (bf3_rs_core.h)
    constexpr int PW = STAGE / 1024 / NW;                               // 6 (4) LDS-DMA pieces per wave and k-tile
    constexpr int A_WAVE = 32 * 128, A_STAGE = NW * A_WAVE;             // 4 KB per wave, 32 KB per stage
    constexpr int A_BASE = NS * STAGE;
    static_assert(PW == 2 * NPL, "piece schedule below assumes 2 pieces per plane, wave and k-tile");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE + 2 * A_STAGE];
    typedef float f32x4 __attribute__((ext_vector_type(4)));

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int grow = lane >> 3;                                         // gather layout: DMA i of this lane fetches row 8 i + grow,
    const int gchunk = (lane & 7) ^ grow;                               // 16-byte chunk gchunk ^ (i >> 1) (image slot lane & 7: emb_a_swizzle)

    const int tiles_n = (g.N + BN - 1) / BN;
    const int tiles_m = (int)((g.M + BM - 1) / BM);
    const int ntiles = tiles_m * tiles_n;
    const int nk = (g.K + BK - 1) / BK;
    const int nke = 2 * e.F;                                            // gathered k-tiles (nk == nke or nke + 1)
    if ((int)blockIdx.x >= ntiles) return;
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int total = my_tiles * nk;                                    // steps of this block

    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
    const int sw = rs_swizzle(l31);
    unsigned b_addr[2];                                                 // B fragment reads, one per k-step
#pragma unroll
    for (int s = 0; s < 2; ++s) b_addr[s] = rs_frag_addr(lds0, l31, hi, sw, s);
    // A image of this wave: position p = 8 row + (chunk ^ emb_a_swizzle(row)), 16 bytes each
    const unsigned a_rd = lds0 + A_BASE + wave * A_WAVE + emb_a_read_off(l31, hi, 0);                   // own row, chunk 4 hi (^ c << 4)
    const unsigned a_st = lds0 + A_BASE + wave * A_WAVE + lane * 16;                                    // position 64 i + lane

    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16*>(g.B), 0, (int)min((int64_t)0x7fffffff, NPL * g.b_ps * 2), 0x00020000);
    float h2_sa = 1.f, h2_out = 1.f;                                    // H2: the activations' scale, 1 / (s_a s_b)
    if constexpr (H2) {
        float sb;
        h2_prologue(g.a_amax, e.dense_amax, g.b_amax, h2_sa, sb, h2_out);
    }
    // (the table resource is built per FIELD, base = its first row: a buffer offset -- index x stride included -- is 32 bits
    // wide, so one resource reaches 4 GB = 2^24 rows; a resource over the whole 66 GB slab wraps, measured)
    const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(e.dense_pad != nullptr ? e.dense_pad : e.table), 128, 0x7fffffff, 0x00020000);
    const int b_lane = (int)((((int64_t)(wave * 16 + (lane >> 2))) * g.b_ld + ((lane & 3) ^ ((((wave * 16 + (lane >> 2))) >> 2) & 3)) * 8) * 2);

    // ---- the block's stream of steps (tile, k-tile): iterators for steps s + 1, s + 2, s + 3 ---------------------------------
    auto m0_of = [&](int tile) -> int { return (xcd_remap(tile, ntiles) / tiles_n) * BM; };
    auto n0_of = [&](int tile) -> int { return (xcd_remap(tile, ntiles) % tiles_n) * BN; };
    int kt1, tile1, m01, kt2, tile2, m02, kt3, tile3, m03;
    auto advance = [&](int& kt, int& tile, int& m0) {                   // past the end of the stream: stay on the last step
        if (kt + 1 < nk) { ++kt; return; }
        if (tile + (int)gridDim.x < ntiles) { tile += gridDim.x; kt = 0; m0 = m0_of(tile); }
    };
    auto grow_row = [&](int m0, int i) -> int { return min(m0 + wave * 32 + 8 * i + grow, (int)g.M - 1); };
    auto own_row = [&](int m0) -> int { return min(m0 + wave * 32 + l31, (int)g.M - 1); };
    const int* ids32 = reinterpret_cast<const int*>(e.ids);             // low words: bucket ids fit 31 bits, -1 stays negative
    int idg[4], ido = 0;                                                // ids in flight: gather layout (step s + 3), own row (step s + 2)
    auto load_idg = [&](int kt, int m0) {
        const int f = min(kt >> 1, e.F - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) idg[i] = ids32[2 * ((int64_t)grow_row(m0, i) * e.F + f)];
    };
    auto load_ido = [&](int kt, int m0) { ido = ids32[2 * ((int64_t)own_row(m0) * e.F + min(kt >> 1, e.F - 1))]; };
    int rb_next = 0;                                                    // row_base of step s + 1's field (step s + 2's when loaded)
    int m4q = 0;                                                        // missing bits of the gathers in flight: step s low nibble, s + 1 next
    bool mo_cur = false, mo_nxt = false;                                // own row missing: step s / s + 1
    float lwn = 0.f;                                                    // own row's first-order weight of the next step
    // Gather of step (KT, M0) into A stage AST from the ids IDS (gather layout) of the field whose first row is RB; M4 receives the
    // 4 missing bits.  One DMA with a selected resource, not one under each arm of a branch: with the branch hipcc's wait for
    // anything older than these DMAs comes out as vmcnt(0).  A macro, so that the prologue and the step loop's clump (which gathers
    // from its saved copy of the ids) share ONE text: as a lambda with the ids as a parameter the clump compiled to exactly that
    // branch, a DMA under each arm.
#define EMB_ISSUE_GATHER(IDS, KT, M0, RB, AST, M4)                                                                                   \
    {                                                                                                                                \
        const bool dense = (KT) >= nke;                                 /* (wave-uniform) */                                         \
        const __amdgpu_buffer_rsrc_t trsrc = __builtin_amdgcn_make_buffer_rsrc(                                                      \
            const_cast<float*>(e.table + (int64_t)(RB) * 64), 256, 0x7fffffff, 0x00020000);                                          \
        M4 = 0;                                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                              \
            const bool miss = !dense && IDS[i] < 0;                                                                                  \
            M4 |= (miss ? 1 : 0) << i;                                                                                               \
            const int idx = dense ? grow_row(M0, i) : max(IDS[i], 0);                                                                \
            unsigned char* dst = smem + A_BASE + (AST) * A_STAGE + wave * A_WAVE + i * 1024;                                         \
            __builtin_amdgcn_struct_ptr_buffer_load_lds(dense ? drsrc : trsrc, (lds_ptr_t)dst, 16, idx,                              \
                                                        (gchunk ^ (i >> 1)) * 16 + (dense ? 0 : ((KT) & 1) * 128), 0, 0, DR_NT_FWD_GATHER ? 2 : 0); \
        }                                                                                                                            \
    }
    auto issue_gather = [&](int kt, int m0, int rb, int ast) -> int {  // ... from the ids in idg; returns the 4 missing bits
        int m4;
        EMB_ISSUE_GATHER(idg, kt, m0, rb, ast, m4)
        return m4;
    };
    // (without first-order weights the load still happens, from the table: every step issues the same number of VMEM operations,
    // which is what makes the counted wait in front of the barrier a constant)
    const bool has_lw = e.lin_w != nullptr;
    const float* const lwp = has_lw ? e.lin_w : e.table;
    // own row (id IDO) of step (KT, .): first-order weight, missing flag.  (A macro for the same reason as EMB_ISSUE_GATHER.)
#define EMB_ISSUE_LW(IDO, KT, RB)                          \
    {                                                      \
        const bool dense = (KT) >= nke;                    \
        mo_nxt = !dense && (IDO) < 0;                      \
        lwn = lwp[dense ? 0 : (RB) + max((IDO), 0)];       \
    }
    auto issue_lw = [&](int kt, int rb) { EMB_ISSUE_LW(ido, kt, rb) };
    auto issue_b = [&](int i, int kt, int n0, int stage) {              // piece wave + 8 i of step (kt, tile with column base n0)
        unsigned char* dst = smem + stage * STAGE + (wave + NW * i) * 1024;
        const int uni = (int)(((int64_t)(i >> 1) * g.b_ps + ((int64_t)(i & 1) * 128 + n0) * g.b_ld) * 2) + kt * (BK * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(brsrc, (lds_ptr_t)dst, 16, b_lane, uni, 0, 0);
    };

    float S0[16], S1[16], ssq = 0.f, lin = 0.f;                         // FM terms of the lane's row (its 16 dims of each half row)
#pragma unroll
    for (int j = 0; j < 16; ++j) { S0[j] = 0.f; S1[j] = 0.f; }
    bf16x8 fa[2][3];                                                    // [k-step][plane] of the CURRENT step
    bf16x8 fb[2][3];                                                    // [buffer][plane]: group q uses buffer q & 1 (one group ahead)
    auto read_b = [&](int buf, int stage, int q) {                      // group q = (k-step q >> 3, column tile q & 7)
        const unsigned bb = b_addr[q >> 3] + stage * STAGE;
        rs_read_frag<NPL>(fb[buf], bb, q & 7);
    };
    f32x16 acc[NT];

    // ---- prologue: pieces of step 0, gathers of steps 0 and 1, ids of step 2 in flight --------------------------------------
    int kt = 0, tile = blockIdx.x, m0c = m0_of(tile);                   // consumer: step s
    kt1 = 0; tile1 = tile; m01 = m0c;
#pragma unroll
    for (int i = 0; i < PW; ++i) issue_b(i, 0, n0_of(tile), 0);
    {
        int rb = sload_i32(e.row_base, 0);
        load_idg(0, m0c);
        load_ido(0, m0c);
        m4q = issue_gather(0, m0c, rb, 0);
        issue_lw(0, rb);
        mo_cur = mo_nxt;
        advance(kt1, tile1, m01);                                       // step 1
        rb = sload_i32(e.row_base, 8 * min(kt1 >> 1, e.F - 1));
        load_idg(kt1, m01);
        m4q |= issue_gather(kt1, m01, rb, 1) << 4;
        load_ido(kt1, m01);                                             // consumed by step 0's clump (own row of step 1)
        rb_next = rb;
        kt2 = kt1; tile2 = tile1; m02 = m01;
        advance(kt2, tile2, m02);                                       // step 2
        load_idg(kt2, m02);                                             // consumed by step 0's clump (gather of step 2)
        kt3 = kt2; tile3 = tile2; m03 = m02;
        advance(kt3, tile3, m03);                                       // step 3
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                                 // everything landed (once per block)
    asm volatile("s_barrier" ::: "memory");
    read_b(0, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;

    int stage = 0;
    for (int step = 0; step < total; ++step) {
        const int astage = step & 1;
        const bool gathered = kt < nke;                                 // (wave-uniform)
        const bool c_fm = (xcd_remap(tile, ntiles) % tiles_n) == 0;     // the first column tile of a row panel owns concat / FM
        // ---- step start: this step's rows out of the LDS image ----------------------------------------------------------------
        f32x4 an[4];
        {
            const unsigned ra = a_rd + astage * A_STAGE;
            const unsigned r1 = ra ^ 16u, r2 = ra ^ 32u, r3 = ra ^ 48u;
            BF3_DS_READ_B128(an[0], ra, 0); BF3_DS_READ_B128(an[1], r1, 0);
            BF3_DS_READ_B128(an[2], r2, 0); BF3_DS_READ_B128(an[3], r3, 0);
        }
        if (gathered && c_fm && e.concat != nullptr) {                     // (kernel-uniform: concat == NULL skips the stores)
            // the image position-wise (8 lanes per 128-byte line) -> concat, for the backward kernels; missing ids store zeros
            const unsigned sa = a_st + astage * A_STAGE;
            f32x4 st[4];
            BF3_DS_READ_B128(st[0], sa, 0); BF3_DS_READ_B128(st[1], sa, 1024);
            BF3_DS_READ_B128(st[2], sa, 2048); BF3_DS_READ_B128(st[3], sa, 3072);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0c + wave * 32 + 8 * i + grow;
                if (row < g.M) {
                    float* dst = e.concat + (int64_t)row * e.ld_concat + kt * BK + 4 * (gchunk ^ (i >> 1));
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    const f32x4 v = ((m4q >> i) & 1) ? z : st[i];
                    // inline asm on purpose: stores the compiler can see make it treat vmcnt as unordered (loads + stores
                    // pending) and wait vmcnt(0) for everything in flight
                    // (s_nop: a VALU write to the data registers of a > 64-bit store needs a wait state after the store; the
                    // hazard recogniser does not look inside inline asm, and the next instruction did reuse v.x)
                    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" :: "v"(dst), "v"(v) : "memory");
                }
            }
        }
        // ("memory": the gather DMA that refills this A stage further down must not be moved above these reads)
        if constexpr (H2)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(an[0]), "+v"(an[1]), "+v"(an[2]), "+v"(an[3]), "+v"(fb[0][0]), "+v"(fb[0][1]) :: "memory");
        else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(an[0]), "+v"(an[1]), "+v"(an[2]), "+v"(an[3]), "+v"(fb[0][0]), "+v"(fb[0][1]), "+v"(fb[0][2])
                     :: "memory");
        if (gathered && mo_cur) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            an[0] = z; an[1] = z; an[2] = z; an[3] = z;
        }
        if (gathered && c_fm) {
            if ((kt & 1) == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { S0[4 * q] += an[q][0]; S0[4 * q + 1] += an[q][1]; S0[4 * q + 2] += an[q][2]; S0[4 * q + 3] += an[q][3]; }
                lin += (hi == 0 && !mo_cur && has_lw) ? lwn : 0.f;
                if (e.lin_vals != nullptr) {                                // (kernel-uniform)
                    // lanes l and l + 32 hold the same row's weight: both store it (same address, same value) -- no divergent
                    // branch around a memory operation; asm for the reason given at the concat stores above
                    float* lv = e.lin_vals + (int64_t)(kt >> 1) * g.M + min(m0c + wave * 32 + l31, (int)g.M - 1);
                    asm volatile("global_store_dword %0, %1, off" :: "v"(lv), "v"(lwn) : "memory");
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) { S1[4 * q] += an[q][0]; S1[4 * q + 1] += an[q][1]; S1[4 * q + 2] += an[q][2]; S1[4 * q + 3] += an[q][3]; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) ssq += (an[q][0] * an[q][0] + an[q][1] * an[q][1]) + (an[q][2] * an[q][2] + an[q][3] * an[q][3]);
        }
        asm volatile("" : "+v"(lwn));                                   // the weight load is consumed on every path
        {
            const float4 a0 = make_float4(an[0][0], an[0][1], an[0][2], an[0][3]), a1 = make_float4(an[1][0], an[1][1], an[1][2], an[1][3]);
            const float4 a2 = make_float4(an[2][0], an[2][1], an[2][2], an[2][3]), a3 = make_float4(an[3][0], an[3][1], an[3][2], an[3][3]);
            if constexpr (H2) {
                h2_split8(a0, a1, h2_sa, fa[0][0], fa[0][1]);
                h2_split8(a2, a3, h2_sa, fa[1][0], fa[1][1]);
            } else {
                rs_split8(a0, a1, fa[0][0], fa[0][1], fa[0][2]);
                rs_split8(a2, a3, fa[1][0], fa[1][1], fa[1][2]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const int nstage = stage ^ 1;
        const int n01 = n0_of(tile1);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            rs_wait_frag<NPL, 0>(fb[q & 1]);
            if (q < 15) {
                read_b((q + 1) & 1, stage, q + 1);
            } else {
                // this wave is done reading the stages of step `step`; publish step + 1.  vmcnt(10): the 6 weight pieces of step + 1
                // (and everything older: the gather of step + 1) have landed, the clump issued after them (5 id loads, the
                // first-order weight, the 4 gather DMAs of step + 2) stays in flight
                __builtin_amdgcn_s_waitcnt(0x0F70 | 10);
                asm volatile("s_barrier" ::: "memory");
                if (step + 1 < total) read_b(0, nstage, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (H2) {      // (the three terms written out: as a loop this instantiation allocates its registers differently)
                acc[q & 7] = rs_mma_term<1>(0, fa[q >> 3], fb[q & 1], acc[q & 7]);
                acc[q & 7] = rs_mma_term<1>(1, fa[q >> 3], fb[q & 1], acc[q & 7]);
                acc[q & 7] = rs_mma_term<1>(2, fa[q >> 3], fb[q & 1], acc[q & 7]);
            } else {
#pragma unroll
                for (int term = 0; term < 6; ++term) acc[q & 7] = rs_mma_term<0>(term, fa[q >> 3], fb[q & 1], acc[q & 7]);
            }
            __builtin_amdgcn_sched_barrier(0);    // keeps the next group's lgkmcnt wait from being hoisted between these MFMAs
            if (q < PW) {
                issue_b(q, kt1, n01, nstage);                           // weight pieces of step + 1 (a dummy re-fetch at the end of the stream)
                __builtin_amdgcn_sched_barrier(0);
            }
            if (q == PW) {
                // the clump: ids first (they are needed one step from now), then the weight, then the DMAs -- a wait for an
                // older operation never forces a younger one
                const int rb1 = rb_next;                                // field of step + 1
                const int rb2 = sload_i32(e.row_base, 8 * min(kt2 >> 1, e.F - 1));
                const int ido_use = ido;
                int idg_use[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) idg_use[i] = idg[i];
                load_idg(kt3, m03);                                     // gather layout, step + 3
                load_ido(kt2, m02);                                     // own row, step + 2
                EMB_ISSUE_LW(ido_use, kt1, rb1)                        // own row of step + 1
                {   // gather of step + 2 into the A stage this step has just consumed
                    int m4;
                    EMB_ISSUE_GATHER(idg_use, kt2, m02, rb2, astage, m4)
                    m4q = (m4q >> 4) | (m4 << 4);
                }
                rb_next = rb2;
                kt1 = kt2; tile1 = tile2; m01 = m02;
                kt2 = kt3; tile2 = tile3; m02 = m03;
                advance(kt3, tile3, m03);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        mo_cur = mo_nxt;
        stage = nstage;
        if (++kt < nk) continue;
        // ---- epilogue of an output tile: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        kt = 0;
        {
            const int lid = xcd_remap(tile, ntiles);
            const int64_t tm0 = (int64_t)(lid / tiles_n) * BM;
            const int tn0 = (lid % tiles_n) * BN;
            const bool relu = g.act == 1;
            const int64_t r0 = tm0 + wave * 32 + 4 * hi;
            // interior tiles: every load / store of the epilogue unconditional (a memory operation under a divergent branch makes
            // hipcc wait vmcnt(0) in front of each one); edge tiles take the guarded loop
            const bool interior = tm0 + BM <= g.M && tn0 + BN <= g.N;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = tn0 + nt * 32 + l31;
                const bool cv = col < g.N;
                float bj = g.bias != nullptr ? g.bias[cv ? col : g.N - 1] : 0.f;
                asm volatile("" : "+v"(bj));      // consume the load on every path (see bf3_gemm_nt_pipe_kernel, bf3_planes.hip)
                if (interior) {
                    float* crow = g.C + r0 * g.ldc + col;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        float v = H2 ? fmaf(acc[nt][reg], h2_out, bj) : acc[nt][reg] + bj;
                        acc[nt][reg] = 0.f;
                        crow[(int64_t)((reg & 3) + 8 * (reg >> 2)) * g.ldc] = relu ? fmaxf(v, 0.f) : v;
                    }
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int64_t row = r0 + (reg & 3) + 8 * (reg >> 2);
                        float v = H2 ? fmaf(acc[nt][reg], h2_out, bj) : acc[nt][reg] + bj;
                        acc[nt][reg] = 0.f;
                        if (!cv || row >= g.M) continue;
                        g.C[row * g.ldc + col] = relu ? fmaxf(v, 0.f) : v;
                    }
                }
            }
            if (c_fm) {
                // this row panel's FM outputs (keras/models/ranking/fm.py:28-37): sum_x for the backward, the logit part
                float t2 = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) t2 += S0[j] * S0[j] + S1[j] * S1[j];
                t2 += __shfl_xor(t2, 32, 64);
                const float ss_all = ssq + __shfl_xor(ssq, 32, 64);
                const int64_t row = tm0 + wave * 32 + l31;
                if (row < g.M) {
                    float* sx = e.sum_x + row * 64 + 16 * hi;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        *reinterpret_cast<float4*>(sx + 4 * q) = make_float4(S0[4 * q], S0[4 * q + 1], S0[4 * q + 2], S0[4 * q + 3]);
                        *reinterpret_cast<float4*>(sx + 32 + 4 * q) = make_float4(S1[4 * q], S1[4 * q + 1], S1[4 * q + 2], S1[4 * q + 3]);
                    }
                    if (hi == 0) e.fm_logit[row] = (e.lin_bias != nullptr ? e.lin_bias[0] : 0.f) + lin + 0.5f * (t2 - ss_all);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) { S0[j] = 0.f; S1[j] = 0.f; }
                ssq = 0.f;
                lin = 0.f;
            }
            // Stores and loads share vmcnt on gfx9 and hipcc treats a mix of the two as unordered: left pending into the next
            // k-tile, the stores turn every wait of the loop into vmcnt(0).  Draining here costs one refill per output tile.
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
        tile += gridDim.x;
        if (tile < ntiles) m0c = m0_of(tile);
    }
}

#undef EMB_ISSUE_GATHER
#undef EMB_ISSUE_LW

}  // namespace

// Fused K3 + first Dense layer (see bf3_emb_linear_kernel): h[m][n] = act(sum_k x[m][k] W[k][n] + bias[n]) with
// x = concat(field embeddings of ids[m], dense features = dense_pad[m, : K - 64 F]); also writes concat[:, : 64 F],
// sum_x [M, 64] and fm_logit [M] = lin_bias + sum_f lin_w[row] + 0.5 sum_d ((sum_f x_fd)^2 - sum_f x_fd^2).
static int emb_linear_fwd_impl(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                               const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad, float* concat,
                               int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride, int64_t ld_planes, int32_t N,
                               const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                               float* lin_vals_t, dr_stream_t stream, const uint32_t* table_amax = nullptr,
                               const uint32_t* dense_amax = nullptr, const uint32_t* w_amax = nullptr) {
    if (M < 0 || M > 0x7fffff00 || F <= 0 || N <= 0 || K < 64 * F || act < 0 || act > 1) return DR_EINVAL;
    // the k-tile <-> (field, half row) map is built for 64-wide rows; the dense features are one k-tile; a field is one 4 GB buffer
    if (D != 64 || K > 64 * F + 32 || field_rows_max <= 0 || field_rows_max > (1 << 24)) return DR_ESHAPE;
    if (M == 0) return DR_OK;
    // concat may be NULL: nothing then stores the gathered embeddings (the wgrad gathers them itself, dr_bf3_wgrad_emb)
    if (!ids || !row_base || !table || !sum_x || !fm_logit || !out || !planes_ok(wt_planes, plane_stride, ld_planes))
        return DR_EINVAL;
    if (K > 64 * F && (!dense_pad || (reinterpret_cast<uintptr_t>(dense_pad) & 15) != 0)) return DR_EINVAL;
    if ((concat != nullptr && ((reinterpret_cast<uintptr_t>(concat) & 15) != 0 || (ld_concat & 3) != 0 || ld_concat < K)) ||
        (reinterpret_cast<uintptr_t>(table) & 15) != 0 || (reinterpret_cast<uintptr_t>(sum_x) & 15) != 0)
        return DR_EINVAL;
    if (ld_planes < (K + BK - 1) / BK * BK || ld_out < N) return DR_EINVAL;
    RsArgs g{nullptr, 0, static_cast<const __bf16*>(wt_planes), plane_stride, ld_planes, M, N, K, out, ld_out, bias, act, nullptr, 0, 0,
             nullptr, nullptr, 0, 0.f, nullptr};
    EmbArgs e{ids, F, row_base, table, lin_w, lin_bias, K > 64 * F ? dense_pad : nullptr, concat, ld_concat, sum_x, fm_logit,
              lin_w != nullptr ? lin_vals_t : nullptr, K > 64 * F ? dense_amax : nullptr};
    const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
    if (tiles > 0x7fffffff) return DR_EINVAL;
    const int grid = (int)(tiles < 256 ? tiles : 256);
    if (table_amax != nullptr) {                                        // f16x2 operand mode
        if (!w_amax || (K > 64 * F && !dense_amax)) return DR_EINVAL;
        g.a_amax = table_amax;
        g.b_amax = w_amax;
        hipLaunchKernelGGL(bf3_emb_linear_kernel<1>, dim3(grid), dim3(512), 0, dr_s(stream), g, e);
    } else {
        hipLaunchKernelGGL(bf3_emb_linear_kernel<0>, dim3(grid), dim3(512), 0, dr_s(stream), g, e);
    }
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_bf3_emb_linear_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                                     const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad, float* concat,
                                     int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride, int64_t ld_planes, int32_t N,
                                     const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                                     dr_stream_t stream) {
    return emb_linear_fwd_impl(ids, M, F, row_base, field_rows_max, table, D, lin_w, lin_bias, dense_pad, concat, ld_concat, K, wt_planes,
                               plane_stride, ld_planes, N, bias, act, sum_x, fm_logit, out, ld_out, nullptr, stream);
}

// The same, also saving the first-order weight of every slot as it was read: lin_vals_t [F, M] field-major (lin_vals_t[f * M + m] =
// lin_w[row_base[f] + ids[m, f]]; undefined for a missing id).  dr_emb_pool_bwd_sorted_ex takes it as `lin_old_t`: the backward then
// updates a unique row's first-order weight with ONE write instead of a read-modify-write of a line it would have to fetch again.
extern "C" int dr_bf3_emb_linear_fwd_lv(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                                        const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad,
                                        float* concat, int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride,
                                        int64_t ld_planes, int32_t N, const float* bias, int32_t act, float* sum_x, float* fm_logit,
                                        float* out, int64_t ld_out, float* lin_vals_t, dr_stream_t stream) {
    return emb_linear_fwd_impl(ids, M, F, row_base, field_rows_max, table, D, lin_w, lin_bias, dense_pad, concat, ld_concat, K, wt_planes,
                               plane_stride, ld_planes, N, bias, act, sum_x, fm_logit, out, ld_out, lin_vals_t, stream);
}

// dr_bf3_emb_linear_fwd_lv in the f16x2 operand mode: wt_planes = two fp16 planes (dr_h2_split with w_amax); table_amax >= the largest
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
