// Shared by the bf3_*.hip translation units (bf3_planes, bf3_gemm, bf3_emb_linear, bf3_wgrad): the operand format, the LDS images and
// the device code more than one of those kernel families uses, each thing once.
//
// The "planes" form of the bf16x3 product mode (gemm_f32_core.h):
//
// gemm_f32_core.h's bf16x3 kernel splits every fp32 operand value into three bf16 terms on its way into LDS: per k-tile 24
// v_cvt_pk + 48 exact subtractions + 24 ds_write_b64 per thread sit between the global loads and the 48 MFMAs, and the
// kernel reaches 0.33-0.38 of the bf16 pipe's fp32-equivalent ceiling (2.5 PFLOP/s / 6).  Here the PRODUCERS of the
// operands write the three planes once (K3 writes the pooled embeddings as planes, the tower-tail backward writes its
// dx as planes, a small kernel splits W after each update), so the GEMM's staging is pure LDS-DMA
// (global_load_lds_dwordx4: no VGPR round trip, no VALU, no ds_write) and its loop is
//     barrier -> issue next k-tile's DMA -> 24 ds_read_b128 (or 48 ds_read_b64_tr_b16) + 48 MFMAs
// with one barrier per k-tile and two LDS stages.  Three planes of x reproduce x exactly ((x2 + x1) + x0 == x), so the
// results are those of the bf16x3 mode: fp32 operands, fp32 accumulation, dropped terms below 2^-24 |ab|.
//
// Replaces, for the first (wide) Dense layer of keras/models/ranking/deepfm.py:30-34 / estimator dnn.py:17-29 of the
// reference and its autodiff:  y = act(x W + b),  dx = dy W^T,  dW = x^T dy,  db = colsum(dy).
//
// Operand format: planes[p][row][col], p = 0..2, bf16, `ld` elements per row (multiple of 8), plane stride `ps`.
//   NT kernel  C[m][n] = sum_k A[m][k] B[n][k]   both operands reduction-contiguous; K % 32 == 0 with ZERO padding in
//              both operands' planes (forward: A = x planes, B = W^T planes; dgrad: A = dy planes, B = W planes)
//   TN kernel  C[f][n] = sum_r X[r][f] Y[r][n]   both operands reduction-major (wgrad: X = x planes, Y = dy planes);
//              rows r >= R must exist up to the next multiple of 32 and be ZERO; split over r, fp32 partials + reduce
// Tile 64*WM x 64*WN x 32, 8 waves (2 per SIMD), each wave 64 x 64 = 2 x 2 MFMA tiles of 32 x 32 x 16 (bf16), 6 MFMAs per
// (A-fragment, B-fragment) pair.  LDS: 2 stages x 72 KB.
//
// LDS images (written by LDS-DMA: lane i of a wave-instruction lands at base + 16 i, so the image is lane-linear and
// any swizzle is applied to the per-lane SOURCE address and, identically, to the fragment read address):
//   NT: per plane [rows][32 k] = 64-byte rows; 16-byte chunk c of row r sits at chunk c ^ ((r >> 2) & 3)  -> the 16 rows
//       of a ds_read_b128 lane group fall on 16 distinct 16-byte slots of the 256-byte bank row (conflict-free)
//   TN: per plane [32 r][cols] = 256/512-byte rows; chunk c of row r sits at c ^ ((r & 3) << 2) -> the 4 rows x 64 bytes a
//       32-lane half of ds_read_b64_tr_b16 touches fall on 4 distinct 64-byte quarters of the bank row
#pragma once
#include "dr_common.h"
#include "bf3_split.h"
#include "rs_args.h"

namespace drrs {

using bf3::bf16x4;
using bf3::bf16x8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int BK = 32;

// 16-byte LDS-DMA: lane i's 16 bytes at `src` land at `dst` (wave-uniform) + 16 i.  A plain (non-template) device function:
// hipcc's host pass cannot substitute the builtin inside a kernel template and silently drops the instantiation.
__device__ __forceinline__ void lds_dma16(const void* src, unsigned char* dst) {
    __builtin_amdgcn_global_load_lds(src, (lds_ptr_t)dst, 16, 0, 0);
}

#define BF3_DS_READ_B128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))

__device__ __forceinline__ void h2_split8(const float4& lo, const float4& hi4, float s, bf16x8& p0, bf16x8& p1) {
    const f32x8 v = f32x8{lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w} * s;
    const f16x8 h = __builtin_convertvector(v, f16x8);
    const f32x8 r = v - __builtin_convertvector(h, f32x8);
    const f16x8 l = __builtin_convertvector(r, f16x8);
    p0 = __builtin_bit_cast(bf16x8, h);
    p1 = __builtin_bit_cast(bf16x8, l);
}
__device__ __forceinline__ f32x16 h2_mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void rs_split8(const float4& lo, const float4& hi4, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    bf16x4 a0, a1, a2, b0, b1, b2;
    bf3::split4(lo.x, lo.y, lo.z, lo.w, a0, a1, a2);
    bf3::split4(hi4.x, hi4.y, hi4.z, hi4.w, b0, b1, b2);
    p0 = __builtin_shufflevector(a0, b0, 0, 1, 2, 3, 4, 5, 6, 7);
    p1 = __builtin_shufflevector(a1, b1, 0, 1, 2, 3, 4, 5, 6, 7);
    p2 = __builtin_shufflevector(a2, b2, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ void rs_split8v(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    rs_split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), p0, p1, p2);
}

__device__ __forceinline__ void h2_split8v(const float (&v)[8], float s, bf16x8& p0, bf16x8& p1) {
    h2_split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), s, p0, p1);
}

// ---- the weight image of the register-split kernels (bf3_gemm_rs_kernel, bf3_emb_linear_kernel, bf3_gemm_tn_rs_kernel) ----------
// One stage holds NPL planes (three bf16 terms, or two fp16 terms in the f16x2 mode) of [256 n-rows][32 k] = 64-byte rows, the NT
// image above.  The k index inside a k-tile is permuted consistently on both operands: lane half `hi` holds k = 16 hi .. 16 hi + 15,
// k-step s uses 16 hi + 8 s .. + 7, i.e. the image's 16-byte chunk 2 hi + s.
// The helpers below only compute values or issue a fixed instruction sequence, and each is shaped so that the three kernels compile
// to the code they had with the text written out (tools/asm_compare.py).  Code with loops, branches and memory operations of its own
// did not survive the move into a function -- the same text came out as other machine code: the plain bias / ReLU store and
// bf3_gemm_rs_kernel's epilogues (the edge arm's `!cv || row >= M` guard split into two nested branches, addresses strength-reduced
// differently, other register allocation; by-reference and by-value arguments alike) stay inline, and the fused forward's gather
// is shared as a macro (bf3_emb_linear.hip) instead of a lambda.
constexpr int RS_B_PLANE = 256 * 64;                                    // bytes
template <int H2> constexpr int RS_NPL = H2 ? 2 : 3;                    // operand planes
template <int H2> constexpr int RS_STAGE = RS_NPL<H2> * RS_B_PLANE;     // 48 KB (32 KB)

// the image's swizzle: k-step s's chunk 2 hi + s of row r (a reader's 32 nt + l31, a writer's own row) sits at chunk ^ rs_swizzle(r).
// rs_swizzle belongs to the images LDS-DMA fills (bf3_gemm_rs_kernel, bf3_emb_linear_kernel, h2_occ.hip): their writes are lane-linear,
// only the fragment reads have to be spread.  bf3_gemm_tn_rs_kernel fills its dy image with ds_write_b128 from registers, 8 consecutive
// rows per lane group, and needs a swizzle that spreads those as well: tn_img_swizzle.
__host__ __device__ constexpr int rs_swizzle(int row) { return (row >> 2) & 3; }
__host__ __device__ constexpr int tn_img_swizzle(int row) { return ((row >> 1) & 3) ^ ((row >> 4) & 1); }
__host__ __device__ constexpr int rs_chunk_off(int hi, int sw, int s) { return ((2 * hi + s) ^ sw) << 4; }
// fragment read address of k-step s: stage 0, plane 0, column tile 0
__host__ __device__ constexpr unsigned rs_frag_addr(unsigned lds0, int l31, int hi, int sw, int s) { return lds0 + l31 * 64 + rs_chunk_off(hi, sw, s); }
// the fused forward's activation image (bf3_emb_linear_kernel): per wave [32 rows][8 chunks of 16 bytes]; chunk c of row r sits at
// position c ^ emb_a_swizzle(r).  The MFMA-operand read of lane (l31, hi) takes chunks 4 hi .. 4 hi + 3 of row l31.
__host__ __device__ constexpr int emb_a_swizzle(int row) { return (row & 7) ^ ((row >> 4) & 1); }
__host__ __device__ constexpr unsigned emb_a_read_off(int l31, int hi, int c) { return l31 * 128 + (((4 * hi + c) ^ emb_a_swizzle(l31)) << 4); }

// ---- bank model of the two 16-byte LDS instructions (CDNA4) -----------------------------------------------------------------------
// A wave's access is served in fixed lane groups, one LDS cycle per group when no two lanes of a group ask one bank for different
// addresses (equal addresses are one broadcast):
//   16-byte read:  4 groups of 16 lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; bank of byte a = (a / 4) % 64
//   16-byte write: 8 groups of 8 consecutive lanes;                                                  bank of byte a = (a / 4) % 32
// lds_b128_ways = 1 + the largest number of lanes that collide with one lane of their group: 1 means conflict-free.  Address
// arithmetic only; the static_asserts below evaluate it over every wave, k-step and column tile of the images above, so a swizzle that
// brings a conflict back does not compile.
constexpr int LDS_RD128_HALF[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
constexpr int lds_rd128_lane(int group, int i) { return LDS_RD128_HALF[group & 1][i] + 32 * (group >> 1); }
constexpr int lds_wr128_lane(int group, int i) { return 8 * group + i; }
typedef unsigned (*lds_addr_fn)(int lane, int p0, int p1);              // byte address of a lane's 16-byte access; p0, p1: the case
constexpr int lds_b128_ways(bool write, lds_addr_fn addr, int p0, int p1) {
    const int groups = write ? 8 : 4, lanes = write ? 8 : 16, banks = write ? 32 : 64;
    int worst = 1;
    for (int gq = 0; gq < groups; ++gq)
        for (int i = 0; i < lanes; ++i) {
            const unsigned ai = addr(write ? lds_wr128_lane(gq, i) : lds_rd128_lane(gq, i), p0, p1);
            int n = 1;
            for (int j = 0; j < lanes; ++j) {
                const unsigned aj = addr(write ? lds_wr128_lane(gq, j) : lds_rd128_lane(gq, j), p0, p1);
                if (aj != ai && (aj / 4) % banks == (ai / 4) % banks) ++n;
            }
            if (n > worst) worst = n;
        }
    return worst;
}
template <int SWZ> constexpr int img_swizzle(int row) { return SWZ ? tn_img_swizzle(row) : rs_swizzle(row); }
// the [256 rows][64 bytes] image: fragment read of k-step s, column tile nt; the TN kernel's write of k-step s by wave w
template <int SWZ> constexpr unsigned img_read_addr(int lane, int s, int nt) {
    return rs_frag_addr(0, lane & 31, lane >> 5, img_swizzle<SWZ>(lane & 31), s) + nt * 2048;
}
template <int SWZ> constexpr unsigned img_write_addr(int lane, int s, int w) {
    return (32 * w + (lane & 31)) * 64 + rs_chunk_off(lane >> 5, img_swizzle<SWZ>(32 * w + (lane & 31)), s);
}
constexpr unsigned emb_a_read_addr(int lane, int c, int w) { return w * 4096 + emb_a_read_off(lane & 31, lane >> 5, c); }
constexpr int lds_b128_worst(bool write, lds_addr_fn addr, int n0, int n1) {
    int worst = 1;
    for (int p0 = 0; p0 < n0; ++p0)
        for (int p1 = 0; p1 < n1; ++p1) {
            const int w = lds_b128_ways(write, addr, p0, p1);
            if (w > worst) worst = w;
        }
    return worst;
}
static_assert(lds_b128_worst(false, img_read_addr<0>, 2, 8) == 1, "NT weight image: fragment reads conflict");
static_assert(lds_b128_worst(false, img_read_addr<1>, 2, 8) == 1, "TN dy image: fragment reads conflict");
static_assert(lds_b128_worst(true, img_write_addr<1>, 2, 8) == 1, "TN dy image: ds_write_b128 conflicts");
static_assert(lds_b128_worst(false, emb_a_read_addr, 4, 8) == 1, "fused forward's activation image: operand reads conflict");

// the NP planes' fragments of column tile nt (bb: rs_frag_addr + the stage's offset).  Immediates must be literal: dispatch on nt
template <int NP>
__device__ __forceinline__ void rs_read_frag(bf16x8 (&f)[3], unsigned bb, int nt) {
#define RS_READ_NT(NTI)                                                           \
    BF3_DS_READ_B128(f[0], bb, 0 * RS_B_PLANE + NTI * 2048);                      \
    BF3_DS_READ_B128(f[1], bb, 1 * RS_B_PLANE + NTI * 2048);                      \
    if constexpr (NP == 3) BF3_DS_READ_B128(f[2], bb, 2 * RS_B_PLANE + NTI * 2048);
    switch (nt) {
        case 0: RS_READ_NT(0) break; case 1: RS_READ_NT(1) break; case 2: RS_READ_NT(2) break; case 3: RS_READ_NT(3) break;
        case 4: RS_READ_NT(4) break; case 5: RS_READ_NT(5) break; case 6: RS_READ_NT(6) break; default: RS_READ_NT(7) break;
    }
#undef RS_READ_NT
}
// the fragments in f's first NREG registers have landed once at most CNT younger LDS reads of this wave are pending; ties the
// MFMAs that follow to the wait
template <int NREG, int CNT>
__device__ __forceinline__ void rs_wait_frag(bf16x8 (&f)[3]) {
    static_assert((NREG == 2 || NREG == 3) && (CNT == 0 || CNT == 2 || CNT == 3), "the waits the kernels use");
#define RS_WAIT_LGKM(N)                                                                                     \
    if constexpr (NREG == 2) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(f[0]), "+v"(f[1]));            \
    else asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]));
    if constexpr (CNT == 0) { RS_WAIT_LGKM(0) } else if constexpr (CNT == 2) { RS_WAIT_LGKM(2) } else { RS_WAIT_LGKM(3) }
#undef RS_WAIT_LGKM
}

// f16x2 kernel prologue: the two operands' scales from their amax records (a2: a second record of operand a, may be null -- the
// larger one counts), 1 / (s_a s_b) for the epilogue, FP16_OVFL on
__device__ __forceinline__ void h2_prologue(const uint32_t* a, const uint32_t* a2, const uint32_t* b, float& sa, float& sb, float& inv_ab) {
    float ia, ib;
    h2_scale_of(max(a[0], a2 != nullptr ? a2[0] : 0u), sa, ia);
    h2_scale_of(b[0], sb, ib);
    inv_ab = ia * ib;
    h2_mode_on();
}

// The products of one (A-fragment, B-fragment) pair, smallest terms first: term t multiplies plane rs_pa(t) of a with plane
// rs_pb(t) of b.  bf16x3: six (a0 b2, a1 b1, a2 b0, a0 b1, a1 b0, a0 b0); f16x2: three (h_a l_b, l_a h_b, h_a h_b).
template <int H2> constexpr int RS_TERMS = H2 ? 3 : 6;
__device__ constexpr int rs_pa(int term) { constexpr int PA[6] = {0, 1, 2, 0, 1, 0}; return PA[term]; }
__device__ constexpr int rs_pb(int term) { constexpr int PB[6] = {2, 1, 0, 1, 0, 0}; return PB[term]; }
__device__ constexpr int h2_pa(int term) { constexpr int HA[3] = {0, 1, 0}; return HA[term]; }
__device__ constexpr int h2_pb(int term) { constexpr int HB[3] = {1, 0, 0}; return HB[term]; }
template <int H2>
__device__ __forceinline__ f32x16 rs_mma_term(int term, const bf16x8 (&a)[3], const bf16x8 (&b)[3], const f32x16& c) {
    if constexpr (H2) return h2_mfma(a[h2_pa(term)], b[h2_pb(term)], c);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rs_pa(term)], b[rs_pb(term)], c, 0, 0, 0);
}

inline bool planes_ok(const void* p, int64_t ps, int64_t ld) {
    return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld > 0 && (ld & 7) == 0 && (ps & 7) == 0;
}

inline int tn_split_for(int64_t R, int32_t F, int32_t N, int bm, int bn) {
    const int64_t tiles = (int64_t)((F + bm - 1) / bm) * ((N + bn - 1) / bn);
    int64_t max_split = (R + 16 * BK - 1) / (16 * BK);                  // at least 16 k-tiles per slice
    if (max_split < 1) max_split = 1;
    if (max_split > 128) max_split = 128;
    int64_t sp = 256 / tiles;                                           // one block per CU: fill the chip once
    if (sp < 1) sp = 1;
    if (sp > max_split) sp = max_split;
    return (int)sp;
}

}  // namespace drrs
