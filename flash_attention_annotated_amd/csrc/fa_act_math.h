// fa_act_math.h — the activations of include/fa_act.h in fp32: a = act(x) and dg = act'(x) * g for a downstream factor g.
// The one definition for fa_act.hip and the epilogues of fa_gemm_act.hip, forward and backward, with contraction off: the
// backward's recomputed output has the forward's bits, whichever of the two units wrote the forward (modules.mlp mixes them).
// Inline functions only: including it adds no kernel to a unit.
#pragma once

#include "../../include/fa_act.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace fa_act_math {

struct Sig {
    float s, c;  // sigmoid(z) and 1 - sigmoid(z), neither by a subtraction
};

__device__ __forceinline__ Sig sigmoid_parts(float z) {
#pragma clang fp contract(off)
    const float e = expf(-fabsf(z));  // in [0, 1]: never overflows, 0 at saturation
    const float hi = 1.0f / (1.0f + e), lo = e * hi;
    Sig g;
    g.s = z >= 0.0f ? hi : lo;
    g.c = z >= 0.0f ? lo : hi;
    return g;
}

template <int ACT>
__device__ __forceinline__ void eval(float x, float g, float &a, float &dg) {
#pragma clang fp contract(off)
    float da;
    if constexpr (ACT == FA_ACT_GELU_TANH) {
        const float x2 = x * x;  // inf once |x| > 1.8e19: z is then +-inf, s (1 - s) is 0 and the second term is dropped
        const Sig g = sigmoid_parts((1.59576912f * x) * (1.0f + 0.044715f * x2));
        const float w = g.s * g.c;
        a = x * g.s;
        da = g.s + (w > 0.0f ? (x * w) * (1.59576912f + 0.2140644486f * x2) : 0.0f);
    } else if constexpr (ACT == FA_ACT_GELU_ERF) {
        const float y = x * 0.70710678118654752f;
        const float phi = x >= 0.0f ? 0.5f * (1.0f + erff(y)) : 0.5f * erfcf(-y);
        a = x * phi;
        da = phi + x * (0.39894228040143268f * expf(-0.5f * (x * x)));  // (x^2 = inf: exp is 0 and x is finite)
    } else if constexpr (ACT == FA_ACT_RELU) {
        a = x > 0.0f ? x : (x == x ? 0.0f : x);  // (NaN stays NaN)
        da = x > 0.0f ? 1.0f : 0.0f;
    } else if constexpr (ACT == FA_ACT_SQRELU) {
        const float r = x > 0.0f ? x : (x == x ? 0.0f : x);
        a = r * r;
        dg = (r * g) * 2.0f;  // (2 r alone overflows for r above half the largest value, where the product with g may not)
        return;
    } else if constexpr (ACT == FA_ACT_SILU) {
        const Sig g = sigmoid_parts(x);
        a = x * g.s;
        da = g.s + x * (g.s * g.c);
    } else if constexpr (ACT == FA_ACT_SIGMOID) {
        const Sig g = sigmoid_parts(x);
        a = g.s;
        da = g.s * g.c;
    } else {
        a = x;
        da = 1.0f;
    }
    dg = da * g;
}

// ... of NC elements, the activation a run-time (wave-uniform) argument
template <int NC>
__device__ __forceinline__ void eval_chunk(int act, const float (&x)[NC], const float (&g)[NC], float (&a)[NC], float (&dg)[NC]) {
#define FA_ACT_CASE(A)                                        \
    case A:                                                   \
        _Pragma("unroll") for (int i = 0; i < NC; ++i) eval<A>(x[i], g[i], a[i], dg[i]); \
        break;
    switch (act) {
        FA_ACT_CASE(FA_ACT_GELU_TANH)
        FA_ACT_CASE(FA_ACT_GELU_ERF)
        FA_ACT_CASE(FA_ACT_RELU)
        FA_ACT_CASE(FA_ACT_SQRELU)
        FA_ACT_CASE(FA_ACT_SILU)
        FA_ACT_CASE(FA_ACT_SIGMOID)
    default:
        _Pragma("unroll") for (int i = 0; i < NC; ++i) eval<FA_ACT_IDENTITY>(x[i], g[i], a[i], dg[i]);
    }
#undef FA_ACT_CASE
}

inline bool known_activation(int a) { return a >= FA_ACT_GELU_TANH && a <= FA_ACT_IDENTITY; }

}  // namespace fa_act_math
