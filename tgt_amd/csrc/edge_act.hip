// TGT_EPI_ACT / TGT_EPI_ACT_BWD: lin_W1 of an FFN with a plain activation (relu / silu / elu) on the edge rows and the data
// gradient through lin_W2 and that activation (reference lib/tgt/layers/layers.py:155-158 with lib/tgt/layers/activations.py:21-25),
// K in {64, 128, 256} -> N = 256, ONE launch each:
//     ACT      out2 (M, 256) = a W^T + bias          the pre-activation as stored, kept for the backward
//              out  (M, 256) = dropout(act(out2), p) * row_scale[m / rows_per_sample]
//     ACT_BWD  out  (M, 256) = round(a W^T * out_scale[m / rows_per_sample]) * act'(res) * keep / (1-p)
//              colsum_partial: per-workgroup column sums of `out` as stored (the bias gradient of lin_W1)
// The kernel is the row-phase kernel of edge_gemm.hip (two wave roles, weight slice resident in registers, accumulators out through
// a double-buffered staging tile, every global access through a tile-based buffer resource: see there and edge_common.hpp) with
// these two epilogues; it lives in a unit of its own so that no kernel of edge_gemm.hip is compiled differently.  Two differences:
// the bias is added AFTER the k-loop, the way the slice kernel behind TGT_EPI_BIAS does it, so that out2 equals such a launch bit
// for bit; and the row phase works on the staged 16-byte vector as stored (act.hpp: the arithmetic and the drop pattern of
// tgt_act_dropout_fwd on out2, bit for bit).
#include "edge_common.hpp"
#include "act.hpp"

namespace tgt {

template <typename T, int KS, int KIND, bool BWD, typename... TL>
__global__ void __launch_bounds__(1024, 4) edge_act_rows_kernel(const tgt_edge_linear_args a, const uint64_t* seed_ctr, TL... tl) {
    constexpr bool LV = sizeof...(TL) > 0;                // launched with a live tile list (edge_common.hpp)
    using F = frag_t<T>;
    constexpr int K = KS * 16, N = 256, kBM = 32, kABytes = kBM * K * 2, kSBytes = kBM * N * 2, kPass = 2;
    constexpr int kOffStage = 2 * kABytes;                                        // LDS: A tiles [2] | staging tiles [2]
    constexpr uint32_t kNone = 0xffffffffu;                                       // a byte offset outside every buffer
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
    const EgGeo g(K), gs(N);
    const int64_t row_tiles = (a.M + kBM - 1) / kBM;
    if (blockIdx.x >= row_tiles) return;
    const int32_t* live = edge_live_ptr(tl...);
    int n_live = 0;
    if constexpr (LV) {
        n_live = edge_live_count(live, row_tiles);
        edge_dead_tiles(live, n_live, row_tiles, [&](int64_t t) {      // all 16 waves, before the roles part: zeros, no operand read
            edge_zero_rows(a.out, a.ldo * 2, N * 2, t, a.M, tid);
            if constexpr (!BWD) edge_zero_rows(a.out2, a.ldo2 * 2, N * 2, t, a.M, tid);
        });
    }
    const int n_tiles = LV ? (int)(((int64_t)n_live - blockIdx.x + gridDim.x - 1) / gridDim.x)
                           : (int)((row_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    auto tile_of = [&](int s) {                            // (s >= n_tiles: past the last row -> empty buffers)
        if constexpr (LV) return edge_live_tile(live, (int64_t)blockIdx.x + (int64_t)s * gridDim.x, n_live, row_tiles);
        else return (int64_t)blockIdx.x + (int64_t)s * gridDim.x;
    };

    if (wave < 8) {
        // ------------------------------------------------------------------------------------------------ GEMM role
        const T* W = reinterpret_cast<const T*>(a.w);
        const int n0 = wave * 32;
        constexpr int spr = K >> 3, total = kBM * spr, kNA = (total + 511) / 512;
        F wr[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wr[ks] = load_frag<T>(W + (int64_t)(n0 + r) * a.ldw + ks * 16 + 8 * hi);
        uint2 braw[4];                                     // the bias of this lane's 16 columns, kept packed
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            braw[gq] = make_uint2(0, 0);
            if (a.bias) braw[gq] = *reinterpret_cast<const uint2*>(reinterpret_cast<const T*>(a.bias) + n0 + 8 * gq + 4 * hi);
        }
        const int64_t lda_b = a.lda * 2;
        uint32_t aoff[kNA];
        int loff[kNA];
#pragma unroll
        for (int q = 0; q < kNA; ++q) {
            const int pc = q * 512 + tid, row = pc / spr, ps = pc % spr;
            const bool mine = total % 512 == 0 || pc < total;
            aoff[q] = mine ? (uint32_t)row * (uint32_t)lda_b + (uint32_t)ps * 16u : kNone;
            loff[q] = g.off(row % kBM, ps);
        }
        uint4 pre[kNA];
        auto fetch = [&](int64_t tile) {
            const __amdgpu_buffer_rsrc_t rs = tile_rsrc(a.a, lda_b, K * 2, tile * kBM, a.M);
#pragma unroll
            for (int q = 0; q < kNA; ++q) pre[q] = rp_ld16(rs, aoff[q]);
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int q = 0; q < kNA; ++q)
                if (total % 512 == 0 || aoff[q] != kNone) *reinterpret_cast<uint4*>(smem + buf * kABytes + loff[q]) = pre[q];
        };
        fetch(tile_of(0));
        commit(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        for (int s = 0; s <= n_tiles; ++s) {
            if (s < n_tiles) {
                const char* xs = smem + (s & 1) * kABytes;
                char* sg = smem + kOffStage + (s & 1) * kSBytes;
                fetch(tile_of(s + 1));
                asm volatile("" ::: "memory");            // the prefetch is issued HERE, not sunk towards its use
                f32x16 acc;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    int rr = r;
                    asm volatile("" : "+v"(rr));           // (keeps the swizzled address arithmetic at its k-step: see edge_rows_kernel)
                    const F xf = load_frag<T>(reinterpret_cast<const T*>(xs + g.off(rr, 2 * ks + hi)));
                    acc = mma32(wr[ks], xf, acc);
                }
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {           // + bias, after the sum (the order of the slice kernel's TGT_EPI_BIAS)
                    float bv[4];
                    unpack4<T>(braw[gq], bv);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * gq + j] += bv[j];
                }
                // accumulators -> staging tile, rounded to the storage type; lanes (r, hi) of a row exchange halves so that each
                // holds 8 consecutive columns = one 16-byte slot
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    uint2 lo = pack4<T>(acc[8 * p], acc[8 * p + 1], acc[8 * p + 2], acc[8 * p + 3]);
                    uint2 up = pack4<T>(acc[8 * p + 4], acc[8 * p + 5], acc[8 * p + 6], acc[8 * p + 7]);
                    swap_halves(lo, up);
                    *reinterpret_cast<uint4*>(sg + gs.off(r, (n0 >> 3) + 2 * p + hi)) = make_uint4(lo.x, lo.y, up.x, up.y);
                }
                commit((s + 1) & 1);                       // (the A buffer of tile s-1: its k-loop ended before the last barrier)
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        return;
    }

    // ------------------------------------------------------------------------------------------------------ row role
    const int t4 = tid - 512;
    const int ch = t4 & 31, rsub = t4 >> 5;               // 16-byte chunk (8 columns) and row inside a group of 16
    const uint32_t thresh = drop_thresh(a.dropout_p);
    const float inv_keep = drop_inv_keep(a.dropout_p);
    const uint64_t seed = step_seed(a.dropout_seed, seed_ctr);
    float cs_x[BWD ? 8 : 1];                              // BWD: column sums of the result over every row this workgroup processes
#pragma unroll
    for (int j = 0; j < (BWD ? 8 : 1); ++j) cs_x[j] = 0.f;

    // per-graph factor (DropPath): one float per rows_per_sample rows, through a buffer of its own (absent: empty, and the 1.f below)
    const float* scale_ptr = BWD ? a.out_scale : a.row_scale;
    const bool has_scale = scale_ptr != nullptr;
    const FastDiv per_sample((uint32_t)(has_scale ? a.rows_per_sample : 1));      // (host-checked: M < 2^31 when a scale is given)
    const int64_t n_samples = has_scale ? (a.M + a.rows_per_sample - 1) / a.rows_per_sample : 0;
    const __amdgpu_buffer_rsrc_t rs_scale = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(scale_ptr), 0, (int)(n_samples * 4), 0x00020000);
    const int64_t ldr_b = a.ldr * 2, ldo_b = a.ldo * 2, ldo2_b = a.ldo2 * 2;
    const uint32_t c16 = (uint32_t)ch * 16u;
    const uint32_t o_res = (uint32_t)rsub * (uint32_t)ldr_b + c16;
    const uint32_t o_out = (uint32_t)rsub * (uint32_t)ldo_b + c16, o_out2 = (uint32_t)rsub * (uint32_t)ldo2_b + c16;

    struct Ops { uint4 o1[BWD ? kPass : 1]; float sc[kPass]; };
    auto fetch_ops = [&](int64_t tile, Ops& o) {          // the row phase's operands of `tile`: whole rows, straight from global memory
        const int64_t r0 = tile * kBM;
        const __amdgpu_buffer_rsrc_t rs1 = tile_rsrc(a.res, ldr_b, N * 2, r0, BWD ? a.M : 0);
#pragma unroll
        for (int i = 0; i < kPass; ++i) {
            if constexpr (BWD) o.o1[i] = rp_ld16(rs1, o_res + (uint32_t)i * 16u * (uint32_t)ldr_b);
            o.sc[i] = rp_ld_f32(rs_scale, per_sample.div((uint32_t)(r0 + i * 16 + rsub)) * 4u);      // (raw: 0 without a scale)
        }
    };
    Ops nxt;
    fetch_ops(tile_of(0), nxt);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // (the GEMM role's first A tile)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // stage 0: the GEMM role fills the first staging tile
    for (int s = 1; s <= n_tiles; ++s) {
        const Ops cur = nxt;                               // operands of tile s-1 (fetched a stage ago)
        fetch_ops(tile_of(s), nxt);
        asm volatile("" ::: "memory");
        const char* sg = smem + kOffStage + ((s - 1) & 1) * kSBytes;
        const int64_t m0 = tile_of(s - 1) * kBM;
        const __amdgpu_buffer_rsrc_t rs_out = tile_rsrc(a.out, ldo_b, N * 2, m0, a.M);
        const __amdgpu_buffer_rsrc_t rs_out2 = tile_rsrc(a.out2, ldo2_b, N * 2, m0, BWD ? 0 : a.M);
#pragma unroll
        for (int i = 0; i < kPass; ++i) {
            const int row = i * 16 + rsub;
            const int64_t m = m0 + row;
            const uint32_t po = (uint32_t)i * 16u;          // rows of this pass below the thread's pass-0 row
            const uint4 zraw = *reinterpret_cast<const uint4*>(sg + gs.off(row, ch));
            const float sc_i = has_scale ? cur.sc[i] : 1.f;
            bool keep[8] = {true, true, true, true, true, true, true, true};
            if (thresh) keep_vector<8>(seed, m * (N / 8) + ch, thresh, keep);              // vector index of (m, 8 ch) in (M, 256)
            T ov[8];
            if constexpr (!BWD) {
                rp_st16(rs_out2, o_out2 + po * (uint32_t)ldo2_b, zraw);                    // the pre-activation
                T zv[8];
                __builtin_memcpy(zv, &zraw, 16);
                const float ik = has_scale ? inv_keep * sc_i : inv_keep;                   // (as act_dropout_kernel forms it)
                act_fwd_vec<T, KIND, 8>(zv, keep, thresh != 0u, ik, ov);
            } else {
                T zv[8], pv[8], dyv[8];
                __builtin_memcpy(zv, &zraw, 16);
                __builtin_memcpy(pv, &cur.o1[i], 16);
#pragma unroll
                for (int t = 0; t < 8; ++t) dyv[t] = has_scale ? from_f32<T>(to_f32(zv[t]) * sc_i) : zv[t];      // z' as a stored value
                act_bwd_vec<T, KIND, 8>(pv, dyv, keep, thresh != 0u, inv_keep, ov);
#pragma unroll
                for (int t = 0; t < 8; ++t) cs_x[t] += to_f32(ov[t]);                      // (of the values AS STORED)
            }
            uint4 raw;
            __builtin_memcpy(&raw, ov, 16);
            rp_st16(rs_out, o_out + po * (uint32_t)ldo_b, raw);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    if constexpr (BWD) {
        if (a.colsum_partial) {
            // fold the 16 row groups, fixed order: [16][256] floats in LDS (the A / staging tiles are dead: every wave is past the last
            // barrier; only the row role takes part from here on -- the GEMM waves have exited, and an exited wave counts as arrived)
            float* red = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int t = 0; t < 8; ++t) red[rsub * N + ch * 8 + t] = cs_x[t];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            float* part = a.colsum_partial + (int64_t)blockIdx.x * N;
            if (t4 < N) {
                float t = 0.f;
#pragma unroll
                for (int s_ = 0; s_ < 16; ++s_) t += red[s_ * N + t4];
                part[t4] = t;
            }
        }
    }
}

template <typename T, int KS, int KIND, bool BWD, typename... TL>
static int eact_launch(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    constexpr int lds = 2 * 32 * KS * 16 * 2 + 2 * 32 * 256 * 2;          // >= the 16 KB of the column-sum fold
    return launch_lds<edge_act_rows_kernel<T, KS, KIND, BWD, TL...>>("edge_act_rows_kernel", dim3((unsigned)grid), dim3(1024), lds, st, a,
                                                                      seed_counter(), tl...);
}

template <typename T, int KS, int KIND, typename... TL>
static int eact_dir(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    return a.epilogue == EPI_ACT ? eact_launch<T, KS, KIND, false>(a, grid, st, tl...) : eact_launch<T, KS, KIND, true>(a, grid, st, tl...);
}

template <typename T, int KS, typename... TL>
static int eact_kind(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    switch ((a.flags & TGT_EDGE_ACT_KIND_MASK) >> TGT_EDGE_ACT_KIND_SHIFT) {
        case TGT_ACT_RELU: return eact_dir<T, KS, TGT_ACT_RELU>(a, grid, st, tl...);
        case TGT_ACT_SILU: return eact_dir<T, KS, TGT_ACT_SILU>(a, grid, st, tl...);
        case TGT_ACT_ELU: return eact_dir<T, KS, TGT_ACT_ELU>(a, grid, st, tl...);
        default: return set_error(TGT_ERR_INVALID, "edge linear (TGT_EPI_ACT): bad kind in flags 0x%x", a.flags);
    }
}

template <typename T, typename... TL>
static int eact_k(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    switch (a.K) {
        case 64: return eact_kind<T, 4>(a, grid, st, tl...);
        case 128: return eact_kind<T, 8>(a, grid, st, tl...);
        default: return eact_kind<T, 16>(a, grid, st, tl...);
    }
}

// K in {64, 128, 256} -> N = 256, 16-bit, a kind the header names, no LayerNorm / pre-scaled bias / fused weight gradient attached
// (the caller, edge_linear_run, checks pointers, alignment and p)
bool edge_act_eligible(const tgt_edge_linear_args& a) {
    return (a.epilogue == EPI_ACT || a.epilogue == EPI_ACT_BWD) && (a.K == 64 || a.K == 128 || a.K == 256) && a.N == 256 &&
           (a.dtype == TGT_BF16 || a.dtype == TGT_F16) && !a.gamma && !a.dw_partial && !(a.flags & TGT_EDGE_BIAS_SCALED) &&
           ((a.flags & TGT_EDGE_ACT_KIND_MASK) >> TGT_EDGE_ACT_KIND_SHIFT) <= TGT_ACT_ELU &&
           !(a.epilogue == EPI_ACT ? a.out_scale != nullptr : a.row_scale != nullptr);
}

// tiles: NULL, or the live tile list of tgt_edge_linear_live
int edge_act_run(const tgt_edge_linear_args& a, int grid, hipStream_t st, const int32_t* tiles) {
    if (tiles) return a.dtype == TGT_BF16 ? eact_k<bf16_t>(a, grid, st, tiles) : eact_k<f16_t>(a, grid, st, tiles);
    return a.dtype == TGT_BF16 ? eact_k<bf16_t>(a, grid, st) : eact_k<f16_t>(a, grid, st);
}

}  // namespace tgt
