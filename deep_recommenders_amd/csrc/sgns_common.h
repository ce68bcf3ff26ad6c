// The device functions csrc/sgns.hip and csrc/eges.hip share: the four-column dot, its meeting inside a group of lanes, the loss term and
// coefficient of one slot, and a slot's share of the gradient rows.  Both files run these and nothing else on a slot, which is why
// dr_eges_fwd with one field, one positive and no attention writes dr_sgns_fwd's bits.
#pragma once
#include "dr_common.h"

constexpr int SGNS_MAX_D = 256;       // the slab's row width
constexpr int SGNS_U = 4;             // rows v_j a lane keeps in flight (8 measured no faster: DESIGN.md section 20)

__device__ __forceinline__ float sgns_dot4(const float4& a, const float4& b) {
    float acc = a.x * b.x;
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// the sum of s over the G lanes of a group (a power of two, 1 .. 64), in every lane of it: an xor butterfly
template <int G>
__device__ __forceinline__ float sgns_group_sum(float s) {
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, G);
    return s;
}

// slot with score s: adds softplus((1 - 2 z) s) to loss and returns g = w (sigmoid(s) - z), z = positive; a skipped slot adds nothing
// and returns 0
__device__ __forceinline__ float sgns_loss_term(float s, bool positive, bool skip, float w, float& loss) {
    const float z = positive ? 1.f : 0.f;
    const float x = positive ? -s : s;
    const float l = fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
    if (!skip) loss += l;
    return skip ? 0.f : w * (dr_sigmoidf(s) - z);
}

// slot j's share of the gradient rows, the same instructions in every kernel: one rounded multiply per d_ctx element, one fmaf per
// d_center element
__device__ __forceinline__ void sgns_grad_slot(float cj, bool skip, const float4& u, const float4& v, float4& acc, float4& dx) {
    dx = skip ? dr_zero4() : make_float4(cj * u.x, cj * u.y, cj * u.z, cj * u.w);
    if (!skip) {
        acc.x = fmaf(cj, v.x, acc.x);
        acc.y = fmaf(cj, v.y, acc.y);
        acc.z = fmaf(cj, v.z, acc.z);
        acc.w = fmaf(cj, v.w, acc.w);
    }
}
