// The gated activations of the FFN block (reference lib/tgt/layers/activations.py:4-17) as per-element device functions, shared by
// the streaming kernels (glu.hip) and the TGT_EPI_GLU epilogue of the 256 -> 512 edge-row GEMM (edge_glu.hip): both call
// glu_fwd_vec on the same stored values, which is what makes the fused launch bit-identical to the streaming pass.
//   x = [g | e],  y = e * act(g):   geglu act = gelu (erf form, gelu_cdf),  glu act = sigmoid,  swiglu act = g * sigmoid(g)
#pragma once
#include "common.hpp"

namespace tgt {

// dropout threshold (16 bit) and 1 / (1 - p): the values of elementwise.hip / edge_gemm.hip
__host__ __device__ inline uint32_t drop_thresh(float p) {
    return p <= 0.f ? 0u : (uint32_t)fminf(65535.f, fmaxf(1.f, rintf(p * 65536.f)));
}
__host__ __device__ inline float drop_inv_keep(float p) { return p <= 0.f ? 1.f : 1.f / (1.f - p); }

// act(g), and act'(g) when asked for
template <int KIND, bool GRAD>
__device__ __forceinline__ float glu_act(float g, float& d_act) {
    if constexpr (KIND == TGT_GLU_GEGLU) {
        float ex;
        const float cdf = gelu_cdf(g, ex);
        if constexpr (GRAD) d_act = cdf + g * 0.3989422804014327f * ex;
        return g * cdf;
    } else {
        const float s = fast_sigmoid(g);
        if constexpr (KIND == TGT_GLU_GLU) {
            if constexpr (GRAD) d_act = s * (1.f - s);
            return s;
        } else {
            if constexpr (GRAD) d_act = s * (1.f + g * (1.f - s));
            return g * s;
        }
    }
}

// forward of one vector: out[t] = keep[t] ? e[t] * act(g[t]) * ik : 0   (fp32 on the values as stored)
// The product r * ik is held in a register as an fp32 value before it is narrowed.  Left to itself hipcc folds the multiply
// into the fp16 conversion (v_fma_mixlo_f16: ONE rounding of the exact product) for some elements and keeps v_mul_f32 +
// v_cvt (two roundings) for others, differently per kernel: the geglu instance of edge_glu512_kernel came out with both forms
// in one vector and disagreed with the streaming kernel in the last fp16 bit wherever ik != 1.
template <typename T, int KIND, int V>
__device__ __forceinline__ void glu_fwd_vec(const T (&gv)[V], const T (&ev)[V], const bool (&keep)[V], bool drop, float ik, T (&ov)[V]) {
#pragma unroll
    for (int t = 0; t < V; ++t) {
        float unused;
        const float r = to_f32(ev[t]) * glu_act<KIND, false>(to_f32(gv[t]), unused);
        float y = r * ik;
        asm("" : "+v"(y));
        ov[t] = from_f32<T>((!drop || keep[t]) ? y : 0.f);
    }
}

// backward of one vector: d_e = dy * act(g) * k, d_g = dy * e * act'(g) * k, k = keep * ik
template <typename T, int KIND, int V>
__device__ __forceinline__ void glu_bwd_vec(const T (&gv)[V], const T (&ev)[V], const T (&dyv)[V], const bool (&keep)[V], bool drop,
                                            float ik, T (&dg)[V], T (&de)[V]) {
#pragma unroll
    for (int t = 0; t < V; ++t) {
        float d_act;
        const float act = glu_act<KIND, true>(to_f32(gv[t]), d_act);
        const float dy = to_f32(dyv[t]);
        const bool k = !drop || keep[t];
        de[t] = from_f32<T>(k ? dy * act * ik : 0.f);
        dg[t] = from_f32<T>(k ? dy * to_f32(ev[t]) * d_act * ik : 0.f);
    }
}

}  // namespace tgt
