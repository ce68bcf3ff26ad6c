// The CIN activations (act 0 none, 1 relu, 2 sigmoid, 3 tanh), shared by cin.hip and cin_pool.hip.
#pragma once
#include "dr_common.h"

__device__ __forceinline__ float cin_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return 1.f / (1.f + expf(-v));
    if (act == 3) return tanhf(v);
    return v;
}
// activation'(pre) expressed through out = activation(pre)
__device__ __forceinline__ float cin_act_grad(float out, int act) {
    if (act == 1) return out > 0.f ? 1.f : 0.f;
    if (act == 2) return out * (1.f - out);
    if (act == 3) return 1.f - out * out;
    return 1.f;
}
