// The plain activations of the FFN block (reference lib/tgt/layers/activations.py:21-25: `getattr(F, name)` for relu / silu / elu)
// as per-element fp32 device functions, shared by the streaming kernels (act.hip) and the TGT_EPI_ACT / TGT_EPI_ACT_BWD epilogues of
// the edge-row GEMM (edge_act.hip): all of them call act_fwd_vec / act_bwd_vec on the same stored values, which is what makes the
// fused launch bit-identical to the streaming pass.
//   relu  y = x > 0 ? x : 0 (NaN stays NaN),            y' = x > 0
//   silu  y = x sigma(x),                               y' = sigma (1 + x (1 - sigma))        (the swiglu gate of glu.hpp)
//   elu   y = x > 0 ? x : expm1(x)   (alpha = 1),       y' = x > 0 ? 1 : exp(x)
#pragma once
#include "glu.hpp"

namespace tgt {

// exp(x) - 1 for x <= 0.  exp(x) - 1.f cancels: at x = -2^-12 the float32 exp is 1 - 2^-12 rounded to 2^-24, a relative error of
// 2^-12 in the difference, far outside an fp16 half-ulp.  Below |x| = 1/2 the Taylor polynomial of degree 8 in Horner form (explicit
// fmas, so that every kernel evaluates the same expression tree): the first dropped term x^9 / 9! is 1.1e-8 |x| there, and every
// rounding is relative to a partial sum within [0.6, 1].  From 1/2 on the difference has magnitude >= 0.39 and exp's error (argument
// scaling + the 1-ulp exp2, together (|x| + 2) e^x 2^-24 <= 1.52 * 2^-24) plus the subtraction's stays below 5.1 * 2^-24 min(|x|, 1).
__device__ __forceinline__ float act_expm1_neg(float x) {
    if (x > -0.5f) {
        float p = 1.f / 40320.f;
        p = __builtin_fmaf(p, x, 1.f / 5040.f);
        p = __builtin_fmaf(p, x, 1.f / 720.f);
        p = __builtin_fmaf(p, x, 1.f / 120.f);
        p = __builtin_fmaf(p, x, 1.f / 24.f);
        p = __builtin_fmaf(p, x, 1.f / 6.f);
        p = __builtin_fmaf(p, x, 0.5f);
        p = __builtin_fmaf(p, x, 1.f);
        return p * x;
    }
    return __expf(x) - 1.f;
}

template <int KIND>
__device__ __forceinline__ float act_fwd(float x) {
    static_assert(KIND == TGT_ACT_RELU || KIND == TGT_ACT_SILU || KIND == TGT_ACT_ELU, "activation kind");
    if constexpr (KIND == TGT_ACT_RELU) {
        return x < 0.f ? 0.f : x;                       // (not fmaxf: that returns 0 for NaN, torch.relu returns NaN)
    } else if constexpr (KIND == TGT_ACT_SILU) {
        return x * fast_sigmoid(x);
    } else {
        return x > 0.f ? x : act_expm1_neg(x);
    }
}

template <int KIND>
__device__ __forceinline__ float act_grad(float x) {
    static_assert(KIND == TGT_ACT_RELU || KIND == TGT_ACT_SILU || KIND == TGT_ACT_ELU, "activation kind");
    if constexpr (KIND == TGT_ACT_RELU) {
        return x > 0.f ? 1.f : 0.f;                     // the derivative at 0 is 0
    } else if constexpr (KIND == TGT_ACT_SILU) {
        const float s = fast_sigmoid(x);
        return s * (1.f + x * (1.f - s));
    } else {
        return x > 0.f ? 1.f : __expf(x);
    }
}

// forward of one vector: out[t] = keep[t] ? act(x[t]) * ik : 0  (fp32 on the values as stored).  The product is pinned in a
// register as an fp32 value before it is narrowed, as in glu_fwd_vec (glu.hpp): one rounding form in every kernel.
template <typename T, int KIND, int V>
__device__ __forceinline__ void act_fwd_vec(const T (&xv)[V], const bool (&keep)[V], bool drop, float ik, T (&ov)[V]) {
#pragma unroll
    for (int t = 0; t < V; ++t) {
        float y = act_fwd<KIND>(to_f32(xv[t])) * ik;
        asm("" : "+v"(y));
        ov[t] = from_f32<T>((!drop || keep[t]) ? y : 0.f);
    }
}

// backward of one vector: dx[t] = keep[t] ? dy[t] * act'(x[t]) * ik : 0
template <typename T, int KIND, int V>
__device__ __forceinline__ void act_bwd_vec(const T (&xv)[V], const T (&dyv)[V], const bool (&keep)[V], bool drop, float ik, T (&dx)[V]) {
#pragma unroll
    for (int t = 0; t < V; ++t) {
        float d = to_f32(dyv[t]) * act_grad<KIND>(to_f32(xv[t])) * ik;
        asm("" : "+v"(d));
        dx[t] = from_f32<T>((!drop || keep[t]) ? d : 0.f);
    }
}

}  // namespace tgt
