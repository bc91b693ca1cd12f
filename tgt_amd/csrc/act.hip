// Fused plain activation + dropout (relu / silu / elu: reference lib/tgt/layers/activations.py:21-25 followed by the nn.Dropout
// of lib/tgt/layers/layers.py:158) for gfx950 -- the GELU pair of elementwise.hip for the other names an FFN is configured with.
//
//   y  = keep(i) ? act(x) / (1-p) * sample_scale[i / elems_per_sample] : 0
//   dx = keep(i) ? dy * act'(x) / (1-p) * sample_scale[i / elems_per_sample] : 0
//
// Pure streaming: one read + one write forward, two reads + one write backward, no mask tensor -- keep(i) is the counter-based
// hash of (seed, i / V) of common.hpp, recomputed in the backward, which therefore needs only x and dy.  One 16-byte vector per
// thread; the arithmetic is act_fwd_vec / act_bwd_vec of act.hpp, shared with the edge-row epilogues (edge_act.hip).
#include "act.hpp"

namespace tgt {

template <typename T, int KIND, bool BWD>
__global__ void __launch_bounds__(256) act_dropout_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out, int64_t n,
                                                         uint64_t seed, uint32_t thresh, float inv_keep,
                                                         const float* __restrict__ sample_scale, uint32_t vecs_per_sample,
                                                         const uint64_t* __restrict__ seed_ctr) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t vec = (int64_t)blockIdx.x * 256 + threadIdx.x, i = vec * V;
    if (i >= n) return;
    const bool whole = i + V <= n;
    T xv[V], dv[V], ov[V];
    if (whole) {
        const uint4 raw = *reinterpret_cast<const uint4*>(x + i);
        __builtin_memcpy(xv, &raw, 16);
        if constexpr (BWD) {
            const uint4 rd = *reinterpret_cast<const uint4*>(dy + i);
            __builtin_memcpy(dv, &rd, 16);
        }
    } else {
        for (int t = 0; t < V; ++t) {
            xv[t] = i + t < n ? x[i + t] : from_f32<T>(0.f);
            if constexpr (BWD) dv[t] = i + t < n ? dy[i + t] : from_f32<T>(0.f);
        }
    }
    bool keep[V];
    if (thresh != 0u) keep_vector<V>(step_seed(seed, seed_ctr), vec, thresh, keep);
    else
        for (int t = 0; t < V; ++t) keep[t] = true;
    // (a vector never straddles samples: elems_per_sample is a multiple of 8; 32-bit division in vector units, host-checked)
    const float ik = sample_scale ? inv_keep * sample_scale[(uint32_t)vec / vecs_per_sample] : inv_keep;
    if constexpr (!BWD) act_fwd_vec<T, KIND, V>(xv, keep, thresh != 0u, ik, ov);
    else act_bwd_vec<T, KIND, V>(xv, dv, keep, thresh != 0u, ik, ov);
    if (whole) {
        uint4 raw;
        __builtin_memcpy(&raw, ov, 16);
        *reinterpret_cast<uint4*>(out + i) = raw;
    } else {
        for (int t = 0; t < V && i + t < n; ++t) out[i + t] = ov[t];
    }
}

template <typename T, int KIND>
static int act_launch(const void* x, const void* dy, void* out, int64_t n, float p, uint64_t seed, bool bwd, const float* sample_scale,
                      int64_t elems_per_sample, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t blocks = ((n + V - 1) / V + 255) / 256;
    const uint32_t vps = sample_scale ? (uint32_t)(elems_per_sample / V) : 1u;
    const T* xp = reinterpret_cast<const T*>(x);
    if (!bwd)
        hipLaunchKernelGGL((act_dropout_kernel<T, KIND, false>), dim3((unsigned)blocks), dim3(256), 0, st, xp, nullptr, reinterpret_cast<T*>(out),
                           n, seed, drop_thresh(p), drop_inv_keep(p), sample_scale, vps, seed_counter());
    else
        hipLaunchKernelGGL((act_dropout_kernel<T, KIND, true>), dim3((unsigned)blocks), dim3(256), 0, st, xp, reinterpret_cast<const T*>(dy),
                           reinterpret_cast<T*>(out), n, seed, drop_thresh(p), drop_inv_keep(p), sample_scale, vps, seed_counter());
    return check_launch(bwd ? "act_dropout_bwd_kernel" : "act_dropout_fwd_kernel");
}

template <typename T>
static int act_kind(int kind, const void* x, const void* dy, void* out, int64_t n, float p, uint64_t seed, bool bwd,
                    const float* sample_scale, int64_t eps_, hipStream_t st) {
    switch (kind) {
        case TGT_ACT_RELU: return act_launch<T, TGT_ACT_RELU>(x, dy, out, n, p, seed, bwd, sample_scale, eps_, st);
        case TGT_ACT_SILU: return act_launch<T, TGT_ACT_SILU>(x, dy, out, n, p, seed, bwd, sample_scale, eps_, st);
        default: return act_launch<T, TGT_ACT_ELU>(x, dy, out, n, p, seed, bwd, sample_scale, eps_, st);
    }
}

int act_dropout_run(const void* x, const void* dy, void* out, int64_t n, int kind, int dtype, float p, uint64_t seed, bool bwd,
                    const float* sample_scale, int64_t elems_per_sample, hipStream_t st) {
    if (!x || !out || n < 0 || (bwd && !dy)) return set_error(TGT_ERR_INVALID, "act_dropout: null tensor");
    if (!(p >= 0.f && p < 1.f)) return set_error(TGT_ERR_INVALID, "act_dropout: p=%f outside [0,1)", p);
    if (kind != TGT_ACT_RELU && kind != TGT_ACT_SILU && kind != TGT_ACT_ELU) return set_error(TGT_ERR_INVALID, "act_dropout: bad kind %d", kind);
    if (dtype != TGT_F32 && dtype != TGT_BF16 && dtype != TGT_F16) return set_error(TGT_ERR_INVALID, "act_dropout: bad dtype %d", dtype);
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)dy) % 16) return set_error(TGT_ERR_INVALID, "act_dropout: tensors must be 16-byte aligned");
    const int V = dtype == TGT_F32 ? 4 : 8;
    // (the grid is one thread per vector in a 32-bit block index, and the sample of a vector is a 32-bit division)
    if (n / V > 0xffffffffLL / 2) return set_error(TGT_ERR_UNSUPPORTED, "act_dropout: more than 2^31 vectors (n=%lld)", (long long)n);
    if (sample_scale && (elems_per_sample <= 0 || elems_per_sample % 8))
        return set_error(TGT_ERR_INVALID, "act_dropout: sample_scale needs elems_per_sample, a multiple of 8");
    if (n == 0) return TGT_OK;
    switch (dtype) {
        case TGT_F32: return act_kind<float>(kind, x, dy, out, n, p, seed, bwd, sample_scale, elems_per_sample, st);
        case TGT_BF16: return act_kind<bf16_t>(kind, x, dy, out, n, p, seed, bwd, sample_scale, elems_per_sample, st);
        default: return act_kind<f16_t>(kind, x, dy, out, n, p, seed, bwd, sample_scale, elems_per_sample, st);
    }
}

}  // namespace tgt
