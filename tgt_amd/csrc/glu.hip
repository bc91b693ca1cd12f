// Fused GLU-family activation + dropout (geglu / glu / swiglu: reference lib/tgt/layers/activations.py:4-17 followed by the
// nn.Dropout of lib/tgt/layers/layers.py:158) for gfx950.
//
//   x = [g | e] (rows, 2 cols)  ->  y (rows, cols) = keep(i) ? e * act(g) / (1-p) * sample_scale[i / elems_per_sample] : 0
//   dx = [d_g | d_e]:  d_e = dy * act(g) * k,  d_g = dy * e * act'(g) * k,  k = keep(i) / (1-p) * sample_scale[..]
//
// Pure streaming, as elementwise.hip: two reads + one write forward (3 half-row vectors per thread), three reads + two writes
// backward, no mask tensor -- keep(i) is the counter-based hash of (seed, i) over the OUTPUT index space (keep_vector on i / V),
// recomputed in the backward.  One 16-byte vector of g and one of e per thread; cols is a multiple of the vector width, so a
// vector never leaves its row and there is no scalar tail.
#include "glu.hpp"

namespace tgt {

// n / d for a divisor fixed per launch, constants computed on the HOST (FastDiv of common.hpp builds them with a 64-bit division
// per thread, which a one-vector-per-thread kernel cannot afford)
struct HostDiv {
    uint32_t mul, sh1, sh2;
    explicit HostDiv(uint32_t d) {
        uint32_t l = 0;
        while (l < 32 && ((uint64_t)1 << l) < d) ++l;                            // ceil(log2 d)
        mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / (d ? d : 1) + 1);
        sh1 = l < 1 ? l : 1;
        sh2 = l > 1 ? l - 1 : 0;
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const {
        const uint32_t t = __umulhi(mul, n);
        return (t + ((n - t) >> sh1)) >> sh2;
    }
};

// vpr: vectors per output row (cols / V); rows_per_sample: elems_per_sample / cols (1 without a scale)
template <typename T, int KIND, bool BWD>
__global__ void __launch_bounds__(256) glu_dropout_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out,
                                                         uint32_t n_vec, uint32_t vpr, HostDiv by_vpr, HostDiv by_sample,
                                                         uint64_t seed, uint32_t thresh, float inv_keep,
                                                         const float* __restrict__ sample_scale, const uint64_t* __restrict__ seed_ctr) {
    constexpr int V = 16 / (int)sizeof(T);
    const uint32_t vec = blockIdx.x * 256u + threadIdx.x;
    if (vec >= n_vec) return;
    const uint32_t row = by_vpr.div(vec), c = vec - row * vpr;
    const int64_t xo = ((int64_t)row * 2 * vpr + c) * V;          // the gate vector; the linear one sits cols = vpr * V further
    T gv[V], ev[V], dv[V];
    {
        const uint4 rg = *reinterpret_cast<const uint4*>(x + xo);
        const uint4 re = *reinterpret_cast<const uint4*>(x + xo + (int64_t)vpr * V);
        __builtin_memcpy(gv, &rg, 16);
        __builtin_memcpy(ev, &re, 16);
        if constexpr (BWD) {
            const uint4 rd = *reinterpret_cast<const uint4*>(dy + (int64_t)vec * V);
            __builtin_memcpy(dv, &rd, 16);
        }
    }
    bool keep[V];
    if (thresh != 0u) keep_vector<V>(step_seed(seed, seed_ctr), (int64_t)vec, thresh, keep);
    else
        for (int t = 0; t < V; ++t) keep[t] = true;
    const float ik = sample_scale ? inv_keep * sample_scale[by_sample.div(row)] : inv_keep;
    if constexpr (!BWD) {
        T ov[V];
        glu_fwd_vec<T, KIND, V>(gv, ev, keep, thresh != 0u, ik, ov);
        uint4 raw;
        __builtin_memcpy(&raw, ov, 16);
        *reinterpret_cast<uint4*>(out + (int64_t)vec * V) = raw;
    } else {
        T dg[V], de[V];
        glu_bwd_vec<T, KIND, V>(gv, ev, dv, keep, thresh != 0u, ik, dg, de);
        uint4 r0, r1;
        __builtin_memcpy(&r0, dg, 16);
        __builtin_memcpy(&r1, de, 16);
        *reinterpret_cast<uint4*>(out + xo) = r0;
        *reinterpret_cast<uint4*>(out + xo + (int64_t)vpr * V) = r1;
    }
}

template <typename T, int KIND>
static int glu_launch(const void* x, const void* dy, void* out, int64_t rows, int cols, float p, uint64_t seed, bool bwd,
                      const float* sample_scale, int64_t elems_per_sample, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const uint32_t vpr = (uint32_t)(cols / V), n_vec = (uint32_t)(rows * vpr);
    const HostDiv by_vpr(vpr), by_sample(sample_scale ? (uint32_t)(elems_per_sample / cols) : 1u);
    const uint32_t blocks = (n_vec + 255u) / 256u;
    const T* xp = reinterpret_cast<const T*>(x);
    if (!bwd)
        hipLaunchKernelGGL((glu_dropout_kernel<T, KIND, false>), dim3(blocks), dim3(256), 0, st, xp, nullptr, reinterpret_cast<T*>(out),
                           n_vec, vpr, by_vpr, by_sample, seed, drop_thresh(p), drop_inv_keep(p), sample_scale, seed_counter());
    else
        hipLaunchKernelGGL((glu_dropout_kernel<T, KIND, true>), dim3(blocks), dim3(256), 0, st, xp, reinterpret_cast<const T*>(dy),
                           reinterpret_cast<T*>(out), n_vec, vpr, by_vpr, by_sample, seed, drop_thresh(p), drop_inv_keep(p), sample_scale,
                           seed_counter());
    return check_launch(bwd ? "glu_dropout_bwd_kernel" : "glu_dropout_fwd_kernel");
}

template <typename T>
static int glu_kind(int kind, const void* x, const void* dy, void* out, int64_t rows, int cols, float p, uint64_t seed, bool bwd,
                    const float* sample_scale, int64_t eps_, hipStream_t st) {
    switch (kind) {
        case TGT_GLU_GEGLU: return glu_launch<T, TGT_GLU_GEGLU>(x, dy, out, rows, cols, p, seed, bwd, sample_scale, eps_, st);
        case TGT_GLU_GLU: return glu_launch<T, TGT_GLU_GLU>(x, dy, out, rows, cols, p, seed, bwd, sample_scale, eps_, st);
        default: return glu_launch<T, TGT_GLU_SWIGLU>(x, dy, out, rows, cols, p, seed, bwd, sample_scale, eps_, st);
    }
}

int glu_dropout_run(const void* x, const void* dy, void* out, int64_t rows, int cols, int kind, int dtype, float p, uint64_t seed,
                    bool bwd, const float* sample_scale, int64_t elems_per_sample, hipStream_t st) {
    if (!x || !out || (bwd && !dy)) return set_error(TGT_ERR_INVALID, "glu_dropout: null tensor");
    if (rows < 0 || cols <= 0) return set_error(TGT_ERR_INVALID, "glu_dropout: bad sizes (rows=%lld cols=%d)", (long long)rows, cols);
    if (!(p >= 0.f && p < 1.f)) return set_error(TGT_ERR_INVALID, "glu_dropout: p=%f outside [0,1)", p);
    if (kind != TGT_GLU_GEGLU && kind != TGT_GLU_GLU && kind != TGT_GLU_SWIGLU)
        return set_error(TGT_ERR_INVALID, "glu_dropout: bad kind %d", kind);
    if (dtype != TGT_F32 && dtype != TGT_BF16 && dtype != TGT_F16) return set_error(TGT_ERR_INVALID, "glu_dropout: bad dtype %d", dtype);
    const int V = dtype == TGT_F32 ? 4 : 8;
    if (cols % V) return set_error(TGT_ERR_UNSUPPORTED, "glu_dropout: cols=%d must be a multiple of %d (one 16-byte vector)", cols, V);
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)dy) % 16) return set_error(TGT_ERR_INVALID, "glu_dropout: tensors must be 16-byte aligned");
    if (rows * (int64_t)(cols / V) > 0xffffffffLL)
        return set_error(TGT_ERR_UNSUPPORTED, "glu_dropout: more than 2^32 output vectors (rows=%lld cols=%d)", (long long)rows, cols);
    if (sample_scale && (elems_per_sample <= 0 || elems_per_sample % cols))
        return set_error(TGT_ERR_INVALID, "glu_dropout: sample_scale needs elems_per_sample, a whole number of rows (%d elements)", cols);
    if (rows == 0) return TGT_OK;
    switch (dtype) {
        case TGT_F32: return glu_kind<float>(kind, x, dy, out, rows, cols, p, seed, bwd, sample_scale, elems_per_sample, st);
        case TGT_BF16: return glu_kind<bf16_t>(kind, x, dy, out, rows, cols, p, seed, bwd, sample_scale, elems_per_sample, st);
        default: return glu_kind<f16_t>(kind, x, dy, out, rows, cols, p, seed, bwd, sample_scale, elems_per_sample, st);
    }
}

}  // namespace tgt
