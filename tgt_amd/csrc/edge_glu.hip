// TGT_EPI_GLU: lin_W1 of an FFN with a gated activation on the edge rows (256 -> 512 channels; reference
// lib/tgt/layers/layers.py:155-158 with lib/tgt/layers/activations.py:4-17) as ONE launch:
//     out2 (M, 512) = a W^T + bias = [g | e]   the pre-activation as stored, kept for the backward
//     out  (M, 256) = dropout(e * act(g), p) * row_scale[m / rows_per_sample]
// The GEMM is edge_wide512_kernel (edge_gemm.hip) unchanged: 16 waves hold 32 output columns x 256 k each, one k-loop per
// 32-row tile, the accumulators leave through ONE storage-type tile in LDS (32 rows x 1 KB, 16-byte slots XOR-swizzled by the
// row).  In that kernel's store phase thread (row, ch) reads slot ch and slot ch + 32 of its row: the eight gate columns
// 8 ch .. 8 ch + 7 and the eight linear columns 256 + 8 ch ..: exactly the pair the activation needs.  So the activation lives
// in the store phase -- two 16-byte stores to out2, one to out -- with no further barrier, LDS or cross-lane traffic, on the
// values as stored (glu.hpp: the arithmetic and the drop pattern of tgt_glu_dropout_fwd on out2, bit for bit).
#include "edge_common.hpp"
#include "glu.hpp"

namespace tgt {

template <typename T, int KIND, typename... TL>
__global__ void __launch_bounds__(1024, 4) edge_glu512_kernel(const tgt_edge_linear_args a, const uint64_t* __restrict__ seed_ctr, TL... tl) {
    constexpr bool LV = sizeof...(TL) > 0;                // launched with a live tile list (edge_common.hpp), as edge_wide512_kernel
    using F = frag_t<T>;
    constexpr int K = 256, KS = 16, N = 512, NO = 256, kBM = 32;
    constexpr int kABytes = kBM * K * 2, kOBytes = kBM * N * 2;
    constexpr int kOffO = 2 * kABytes, kOffB = kOffO + kOBytes;               // LDS: A tiles [2] | output tile | bias (fp32)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
    const int n0 = wave * 32;                             // column block of this wave's k-loop
    const int row = tid >> 5, ch = tid & 31;              // row and 16-byte chunk of this thread's loads / stores
    const EgGeo g(K);
    const int64_t row_tiles = (a.M + kBM - 1) / kBM;
    float* bs = reinterpret_cast<float*>(smem + kOffB);
    if (blockIdx.x >= row_tiles) return;
    const int32_t* live = edge_live_ptr(tl...);
    int n_live = 0;
    if constexpr (LV) {
        n_live = edge_live_count(live, row_tiles);
        edge_dead_tiles(live, n_live, row_tiles, [&](int64_t t) {
            edge_zero_rows(a.out2, a.ldo2 * 2, N * 2, t, a.M, tid);
            edge_zero_rows(a.out, a.ldo * 2, NO * 2, t, a.M, tid);
        });
    }
    const int n_tiles = LV ? (int)(((int64_t)n_live - blockIdx.x + gridDim.x - 1) / gridDim.x)
                           : (int)((row_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x);
    auto tile_of = [&](int s) {
        if constexpr (LV) return edge_live_tile(live, (int64_t)blockIdx.x + (int64_t)s * gridDim.x, n_live, row_tiles);
        else return (int64_t)blockIdx.x + (int64_t)s * gridDim.x;
    };
    if (tid < N) bs[tid] = a.bias ? to_f32(reinterpret_cast<const T*>(a.bias)[tid]) : 0.f;
    const T* W = reinterpret_cast<const T*>(a.w);
    F wr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wr[ks] = load_frag<T>(W + (int64_t)(n0 + r) * a.ldw + ks * 16 + 8 * hi);
    const int64_t lda_b = a.lda * 2, ldo_b = a.ldo * 2, ldo2_b = a.ldo2 * 2;
    const uint32_t aoff = (uint32_t)row * (uint32_t)lda_b + (uint32_t)ch * 16u;
    const int loff = g.off(row, ch);
    const uint32_t o_out = (uint32_t)row * (uint32_t)ldo_b + (uint32_t)ch * 16u;
    const uint32_t o_out2 = (uint32_t)row * (uint32_t)ldo2_b + (uint32_t)ch * 16u;
    auto ooff = [&](int prow, int slot) { return prow * 1024 + ((slot ^ (prow & 31)) << 4); };
    const uint32_t thresh = drop_thresh(a.dropout_p);
    const float inv_keep = drop_inv_keep(a.dropout_p);
    const uint64_t seed = step_seed(a.dropout_seed, seed_ctr);
    const bool has_scale = a.row_scale != nullptr;
    const FastDiv per_sample((uint32_t)(has_scale ? a.rows_per_sample : 1));
    const int64_t n_samples = has_scale ? (a.M + a.rows_per_sample - 1) / a.rows_per_sample : 0;
    const __amdgpu_buffer_rsrc_t rs_scale = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.row_scale), 0, (int)(n_samples * 4), 0x00020000);
    uint4 pre;
    float op_sc;
    auto fetch_a = [&](int64_t tile) { pre = rp_ld16(tile_rsrc(a.a, lda_b, K * 2, tile * kBM, a.M), aoff); };
    // the per-graph factor of this thread's row of a tile (raw: 0 without a scale or past the last sample; selected where it is used)
    auto fetch_scale = [&](int64_t tile) { op_sc = rp_ld_f32(rs_scale, per_sample.div((uint32_t)(tile * kBM + row)) * 4u); };
    auto commit = [&](int buf) { *reinterpret_cast<uint4*>(smem + buf * kABytes + loff) = pre; };
    fetch_a(tile_of(0));
    fetch_scale(tile_of(0));
    commit(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    char* ot = smem + kOffO;
    for (int s = 0; s < n_tiles; ++s) {
        fetch_a(tile_of(s + 1));                           // (past the last tile: an empty buffer)
        asm volatile("" ::: "memory");
        const char* xs = smem + (s & 1) * kABytes;
        f32x16 acc;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 bv = *reinterpret_cast<const float4*>(bs + n0 + 8 * gq + 4 * hi);
            acc[4 * gq] = bv.x; acc[4 * gq + 1] = bv.y; acc[4 * gq + 2] = bv.z; acc[4 * gq + 3] = bv.w;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            int rr = r;
            asm volatile("" : "+v"(rr));                   // (keeps the swizzled address arithmetic at its k-step: see edge_rows_kernel)
            const F xf = load_frag<T>(reinterpret_cast<const T*>(xs + g.off(rr, 2 * ks + hi)));
            acc = mma32(wr[ks], xf, acc);
        }
        // accumulator element 4 gq + e = (tile row r, column n0 + 8 gq + 4 hi + e): 8 bytes of slot n0/8 + gq
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            f32x2 lo = {acc[4 * gq], acc[4 * gq + 1]}, hi2 = {acc[4 * gq + 2], acc[4 * gq + 3]};
            *reinterpret_cast<uint2*>(ot + ooff(r, (n0 >> 3) + gq) + 8 * hi) = make_uint2(rp_pack2<T>(lo), rp_pack2<T>(hi2));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const int64_t m0 = tile_of(s) * kBM;
            const __amdgpu_buffer_rsrc_t rs_out2 = tile_rsrc(a.out2, ldo2_b, N * 2, m0, a.M);
            const __amdgpu_buffer_rsrc_t rs_out = tile_rsrc(a.out, ldo_b, NO * 2, m0, a.M);
            const uint4 v0 = *reinterpret_cast<const uint4*>(ot + ooff(row, ch));           // gate columns 8 ch ..
            const uint4 v1 = *reinterpret_cast<const uint4*>(ot + ooff(row, ch + 32));      // linear columns 256 + 8 ch ..
            rp_st16(rs_out2, o_out2, v0);
            rp_st16(rs_out2, o_out2 + 512u, v1);
            T gv[8], ev[8], ov[8];
            __builtin_memcpy(gv, &v0, 16);
            __builtin_memcpy(ev, &v1, 16);
            bool keep[8] = {true, true, true, true, true, true, true, true};
            if (thresh) keep_vector<8>(seed, (m0 + row) * (NO / 8) + ch, thresh, keep);     // vector index of (m, 8 ch) in (M, 256)
            const float ik = has_scale ? inv_keep * op_sc : inv_keep;
            glu_fwd_vec<T, KIND, 8>(gv, ev, keep, thresh != 0u, ik, ov);
            uint4 raw;
            __builtin_memcpy(&raw, ov, 16);
            rp_st16(rs_out, o_out, raw);
        }
        fetch_scale(tile_of(s + 1));
        asm volatile("" ::: "memory");
        commit((s + 1) & 1);                               // (the A buffer of tile s-1; its k-loop ended two barriers ago)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

template <typename T, int KIND, typename... TL>
static int eglu_launch(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    constexpr int lds = 2 * 32 * 256 * 2 + 32 * 512 * 2 + 512 * 4;
    return launch_lds<edge_glu512_kernel<T, KIND, TL...>>("edge_glu512_kernel", dim3((unsigned)grid), dim3(1024), lds, st, a, seed_counter(), tl...);
}

template <typename T, typename... TL>
static int eglu_kind(const tgt_edge_linear_args& a, int grid, hipStream_t st, TL... tl) {
    switch ((a.flags & TGT_EDGE_GLU_KIND_MASK) >> TGT_EDGE_GLU_KIND_SHIFT) {
        case TGT_GLU_GEGLU: return eglu_launch<T, TGT_GLU_GEGLU>(a, grid, st, tl...);
        case TGT_GLU_GLU: return eglu_launch<T, TGT_GLU_GLU>(a, grid, st, tl...);
        case TGT_GLU_SWIGLU: return eglu_launch<T, TGT_GLU_SWIGLU>(a, grid, st, tl...);
        default: return set_error(TGT_ERR_INVALID, "edge linear (TGT_EPI_GLU): bad kind in flags 0x%x", a.flags);
    }
}

// K = 256 -> N = 512, 16-bit, nothing else attached (the caller, edge_linear_run, has checked pointers, alignment and p)
bool edge_glu_eligible(const tgt_edge_linear_args& a) {
    return a.epilogue == EPI_GLU && a.K == 256 && a.N == 512 && (a.dtype == TGT_BF16 || a.dtype == TGT_F16) && !a.gamma &&
           !a.out_scale && !(a.flags & TGT_EDGE_BIAS_SCALED) &&
           ((a.flags & TGT_EDGE_GLU_KIND_MASK) >> TGT_EDGE_GLU_KIND_SHIFT) <= TGT_GLU_SWIGLU;
}

// tiles: NULL, or the live tile list of tgt_edge_linear_live
int edge_glu_run(const tgt_edge_linear_args& a, int grid, hipStream_t st, const int32_t* tiles) {
    if (tiles) return a.dtype == TGT_BF16 ? eglu_kind<bf16_t>(a, grid, st, tiles) : eglu_kind<f16_t>(a, grid, st, tiles);
    return a.dtype == TGT_BF16 ? eglu_kind<bf16_t>(a, grid, st) : eglu_kind<f16_t>(a, grid, st);
}

}  // namespace tgt
