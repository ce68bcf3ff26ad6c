// The body of bf3_emb_linear_kernel<H2> and of bf3_emb_linear_tail_kernel<H2> (bf3_emb_linear.hip, which describes it): included
// INSIDE both kernel definitions -- as one inlined function the existing instantiations compile to other code than before, and
// tools/asm_compare.py holds them to their text.  Expects in scope: the template parameter H2, `constexpr int TAIL`, the kernel
// arguments RsArgs g, EmbArgs e and FwdTailArgs tk (unused unless TAIL; the device pass reads it from the kernarg segment).
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
    const int total = TAIL ? nk : my_tiles * nk;                        // steps of this block (TAIL: one tile per block)

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
        // (TAIL: one tile per block.  m0 goes through an empty asm so that the row addresses derived from it stay what they are in the
        // other instantiations, values of the step: as loop invariants they are hoisted and cost ten registers the loop does not have)
        if constexpr (TAIL) { asm volatile("" : "+s"(m0)); return; }
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
    float fmv = 0.f;                                                    // (TAIL) this lane's row's fm_logit, valid in the lanes hi == 0
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
            if constexpr (TAIL) {
                // every DMA of this block has landed (the dummy re-fetches at the end of the stream included) and every wave is done
                // with the stages: from here on the whole LDS is the epilogue's
                __builtin_amdgcn_s_waitcnt(0x0F70);
                asm volatile("s_barrier" ::: "memory");
            }
            if constexpr (!TAIL) {
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
#define EMB_FM_LOGIT ((e.lin_bias != nullptr ? e.lin_bias[0] : 0.f) + lin + 0.5f * (t2 - ss_all))
                    if constexpr (TAIL) {                               // (kept in a register: the tail epilogue adds it to the tower's logit)
                        fmv = EMB_FM_LOGIT;
                        if (hi == 0) e.fm_logit[row] = fmv;
                    } else {
                        if (hi == 0) e.fm_logit[row] = EMB_FM_LOGIT;
                    }
#undef EMB_FM_LOGIT
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) { S0[j] = 0.f; S1[j] = 0.f; }
                ssq = 0.f;
                lin = 0.f;
            }
            if constexpr (TAIL) break;                                  // one tile per block; the tail epilogue follows the step loop
            // Stores and loads share vmcnt on gfx9 and hipcc treats a mix of the two as unordered: left pending into the next
            // k-tile, the stores turn every wait of the loop into vmcnt(0).  Draining here costs one refill per output tile.
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
        tile += gridDim.x;
        if (tile < ntiles) m0c = m0_of(tile);
    }
    // ---- TAIL: the tower tail on this wave's 32 rows (tower_tail_fused_kernel's stages; its wave index = our column tile).  Behind the
    // step loop, not inside its tile epilogue: there the compiler takes it for a part of the loop and keeps the pipeline's registers
    // alive through it.
    if constexpr (TAIL) {
        const int64_t tm0 = (int64_t)xcd_remap((int)blockIdx.x, ntiles) * BM;
        const bool relu = g.act == 1;
        float* const ldsf = reinterpret_cast<float*>(smem);
        float* const w1s = ldsf;                                // W1 [256][33], zero past H
        float* const red = w1s + 256 * 33;                      // [8 waves][32 x 32]: the waves' dW1 tiles of one column tile
        float* const wv = red + NW * 1024 + wave * (32 * 36);   // wave-private: an x slice [32][36], later d h1 [32][33]
        float* const blk = red + NW * 1024 + NW * (32 * 36);    // [8][34] head sums, [8][32] db1, [8] max |dx|
        static_assert((256 * 33 + NW * 1024 + NW * 32 * 36 + NW * 34 + NW * 32 + NW) * 4 <= NS * STAGE + 2 * A_STAGE, "tail epilogue LDS");
        // (lane-derived values of the epilogue start from laundered copies: computed from l31 / hi / tid they are loop invariants,
        // which the compiler hoists in front of the step loop and keeps in registers the main loop has no room for)
        int c = l31, h = hi, tidl = tid;
        asm volatile("" : "+v"(c), "+v"(h), "+v"(tidl));
        // (and the tail's 19 arguments are read from the kernarg segment HERE: as kernel parameters they are loaded at the kernel's
        // entry and held in ~34 SGPRs through the main loop, which then spills scalars into vector registers it does not have)
#if defined(__HIP_DEVICE_COMPILE__)
        typedef const __attribute__((address_space(4))) FwdTailKernargs* kernargs_t;
        kernargs_t ka = (kernargs_t)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const FwdTailArgs t = ka->t;
#else
        const FwdTailArgs t = tk;                               // (the host pass only parses the kernel)
#endif
        const int H = t.H;
        const int64_t wrow0 = tm0 + wave * 32;                  // (wave-uniform; M % 32 == 0: a wave is live or dead as a whole)
        const bool live = wrow0 < g.M;
        const int64_t lrow0 = live ? wrow0 : g.M - 32;          // a dead wave reads the last rows, stores nothing, contributes zeros
        const bool cvh = c < H;
        float labv = t.labels[lrow0 + c];
        float b1j = t.b1 != nullptr ? t.b1[cvh ? c : H - 1] : 0.f;
        float w2j = t.w2[(int64_t)(cvh ? c : H - 1) * t.ld_w2];
        float b2v = t.b2 != nullptr ? t.b2[0] : 0.f;
        {
            const int k = tidl >> 1, n0 = (tidl & 1) * 16;        // W1 -> LDS: thread = (row, half)
            float w[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = t.W1[(int64_t)k * t.ldw1 + (n0 + j < H ? n0 + j : H - 1)];
            // everything the epilogue loads, waited for HERE, by hand
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]),
                           "+v"(w[9]), "+v"(w[10]), "+v"(w[11]), "+v"(w[12]), "+v"(w[13]), "+v"(w[14]), "+v"(w[15]), "+v"(labv),
                           "+v"(b1j), "+v"(w2j), "+v"(b2v)
                         :: "memory");
#pragma unroll
            for (int j = 0; j < 16; ++j) w1s[k * 33 + n0 + j] = n0 + j < H ? w[j] : 0.f;
        }
        if (!cvh) w2j = 0.f;
        // (1) x = act(acc / scales + bias) in place; h0 leaves the CU only on request
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float bj = g.bias != nullptr ? g.bias[nt * 32 + c] : 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float v = fmaf(acc[nt][reg], h2_out, bj);
                acc[nt][reg] = relu ? fmaxf(v, 0.f) : v;
            }
            if (g.C != nullptr && live) {                       // (wave-uniform)
                float* crow = g.C + (wrow0 + 4 * h) * g.ldc + nt * 32 + c;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) crow[(int64_t)drtail::tt_row(reg, 0) * g.ldc] = acc[nt][reg];
            }
        }
        drtail::tail_lds_barrier();                             // W1 is in the LDS
        __builtin_amdgcn_sched_barrier(0);
        // (2) head product: one partial tile per 32-column slice, the partials added in slice order
        drtail::f32x16 hs;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) hs[reg] = 0.f;
#pragma unroll
        for (int sl = 0; sl < NT; ++sl) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) wv[drtail::tt_row(reg, h) * 36 + c] = acc[sl][reg];
            float w1f[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) w1f[j] = w1s[(32 * sl + 16 * h + j) * 33 + c];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the slice is wave-private: no barrier)
            drtail::f32x16 acc1;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc1[reg] = 0.f;
            const float* xr = wv + c * 36 + 16 * h;             // row m = c, this half's 16 columns of the slice
            DR_TAIL_HEAD_MFMA(4, acc1, xr, w1f)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) hs[reg] += acc1[reg];
            // one slice at a time (left free, the compiler runs all eight products before the first sum: 8 x 16 registers more), and
            // the next slice's LDS writes stay behind this slice's reads
            asm volatile("" : "+v"(hs) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        // (3) head epilogue of the wave's 32 rows; d h1 -> the wave's LDS
        float dw2_acc = 0.f, db2_acc = 0.f, loss_acc = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int ro = drtail::tt_row(reg, h);
            const float ext = __shfl(fmv, ro, 64), lab = __shfl(labv, ro, 64);
            float v = hs[reg];
            DR_TAIL_HEAD_ROW(true, v, b1j, cvh, w2j, b2v, ext, lab, t.loss_mode, t.inv_n, live, p, l, gs, dh)
            wv[ro * drtail::TT_P + c] = dh;
            if (live) {
                const int64_t row = wrow0 + ro;
                if (c == 0) {
                    t.prob[row] = p;
                    t.d_logit[row] = gs;
                }
                if (cvh && t.d_h != nullptr) t.d_h[row * t.ld_dh + c] = dh;
            }
            dw2_acc = fmaf(v, gs, dw2_acc);
            if (c == 0) { db2_acc += gs; loss_acc += l; }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // (4) narrow backward per column tile; the waves' dW1 tiles are summed through the LDS in wave order
        // (both operand forms of d h1 are re-read from the wave's LDS per column tile: held in registers across the eight tiles
        // they push the kernel past its 256)
        float db1 = 0.f, dx_max = 0.f;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) db1 += wv[r * drtail::TT_P + c];
        float* const pp = t.partial + (int64_t)blockIdx.x * ((BN + 1) * 32);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float wf[16], dxa[16], dwb[16];
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) {
                dwb[s2] = wv[drtail::tt_row(s2, h) * drtail::TT_P + c];     // d h1[m = row(s, h)][n = c]
                dxa[s2] = wv[c * drtail::TT_P + 2 * s2 + h];                // d h1[m = c][n = 2 s + h]
                wf[s2] = w1s[(32 * nt + c) * 33 + 2 * s2 + h];
            }
            drtail::f32x16 accw;
#pragma unroll
            for (int j = 0; j < 16; ++j) accw[j] = 0.f;
            DR_TAIL_BWD_TILE(16, acc[nt], dxa, dwb, wf, accw, dx_max)
            if (live) {
                float* base = t.dx + (wrow0 + 4 * h) * t.lddx + nt * 32 + c;
#pragma unroll
                for (int j = 0; j < 16; ++j) base[(int64_t)drtail::tt_row(j, 0) * t.lddx] = acc[nt][j];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) red[wave * 1024 + drtail::tt_row(j, h) * 32 + c] = accw[j];   // row = x column, n = c
            drtail::tail_lds_barrier();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int el = tidl + 512 * u;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) sum += red[w * 1024 + el];
                pp[(32 * nt) * 32 + el] = sum;
            }
            drtail::tail_lds_barrier();
            __builtin_amdgcn_sched_barrier(0);                  // (one column tile at a time, as above)
        }
        // (5) the block's remaining partials: Dense(1) gradient, db2, loss, db1, max |dx|
        dw2_acc += __shfl_xor(dw2_acc, 32, 64);
        db2_acc += __shfl_xor(db2_acc, 32, 64);
        loss_acc += __shfl_xor(loss_acc, 32, 64);
        uint32_t* const blk_amax = reinterpret_cast<uint32_t*>(blk + NW * 34 + NW * 32);
        if (h == 0) {
            blk[wave * 34 + c] = dw2_acc;
            if (c == 0) { blk[wave * 34 + 32] = db2_acc; blk[wave * 34 + 33] = loss_acc; }
            blk[NW * 34 + wave * 32 + c] = db1;
        }
        uint32_t mx = live ? __float_as_uint(dx_max) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        if (c == 0 && h == 0) blk_amax[wave] = mx;
        drtail::tail_lds_barrier();
        if (tidl < drtail::TAIL_HEAD_PART) {
            float sum = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) sum += blk[w * 34 + tidl];
            t.head_partial[(int64_t)blockIdx.x * drtail::TAIL_HEAD_PART + tidl] = sum;
        } else if (tidl >= 64 && tidl < 96) {
            float sum = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) sum += blk[NW * 34 + w * 32 + (tidl - 64)];
            pp[BN * 32 + (tidl - 64)] = sum;
        } else if (tidl == 128) {
            uint32_t mm = 0u;
#pragma unroll
            for (int w = 0; w < NW; ++w) mm = max(mm, blk_amax[w]);
            t.amax_part[blockIdx.x] = mm;
            // (kernel-uniform) part 1 alone: the reduce may run on another stream, later than the record's first reader -- the record
            // was reset in front of this launch and is raised here, one atomic per block and only if it would raise it
            if (t.dx_amax != nullptr && mm > __hip_atomic_load(t.dx_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t.dx_amax, mm);
        }
    }
#undef EMB_ISSUE_GATHER
#undef EMB_ISSUE_LW
