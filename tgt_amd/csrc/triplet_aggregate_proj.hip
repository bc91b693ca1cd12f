// Triplet aggregate forward with the V projection fused in -- gfx950, inference only (no backward follows the call).
//
// Reference lib/tgt/layers/triplet.py:45-73 (gated) / :100-127 (ungated): `lin_V(e_ln)` followed by softmax * gate over the third
// arm and the two einsums.  The unfused path writes the 512 projected V channels of every edge with a library GEMM and reads
// them straight back in tri_agg_fwd_kernel; here the workgroup that walks node j projects the V rows it needs from the
// LayerNorm'd edge rows itself and nothing of V ever reaches global memory.
//
//   workgroup = (graph b, direction): all 16 heads, so every X row is fetched by ONE workgroup per direction;
//   8 waves, wave = the head PAIR (2w, 2w + 1):
//     * the pair's 32 weight rows [W_V(2w); W_V(2w+1)] x 256 k stay resident as the B operands of 16 v_mfma_f32_32x32x16
//       (64 registers), the pair's two 32 x 32 weight tiles A[i,k] as operand fragments (16 registers) -- they do not depend on j;
//     * per step j: V[k][(head, d)] = X_tile(32 x 256) W^T + b from the X tile of step j in LDS (rows padded to 528 bytes, as
//       proj2::xoff), which comes out of the matrix core in the layout tri_agg_fwd_kernel transposes its V slab INTO -- lane =
//       channel, registers = k -- so the accumulator is packed into operand fragments in registers, without a trip through LDS;
//       then O^T[(head, d)][i] = V^T A_head^T, one 32-row product per head of which that head's 16 rows are kept;
//     * the O rows leave as whole 512-byte rows through an O slab; X tiles and O slabs are double-buffered: ONE barrier per step.
//   512 threads at <= 128 registers and 68.25 KB of LDS (the third-arm stage): two workgroups per CU.
// Supported: C = 256, D = 16, H = 16, N <= 32, 16-bit dtypes, gated and ungated, attention dropout (the plain kernel's pattern).
#include "triplet_common.hpp"

namespace tgt {

namespace aggproj {
constexpr int kC = 256, kD = 16, kH = 16, kWaves = 8, kThreads = kWaves * 64;
constexpr int kRowBytes = kC * 2;                            // an X row and an O row of one direction: 512 bytes
constexpr int kXPitch = kRowBytes + 16;                      // (see proj2::xoff in triplet_attention_proj.hip)
constexpr int kXTile = 32 * kXPitch;
constexpr int kOSlab = 32 * kRowBytes;
constexpr int kOffO = 2 * kXTile;
constexpr int kWalk = kOffO + 2 * kOSlab;
constexpr uint32_t kNone = 0xffffffffu;
__device__ __forceinline__ int xoff(int row, int slot) { return row * kXPitch + (slot << 4); }
// the 16-head slab geometry of triplet_common.hpp, walked by this kernel's 512 threads
template <typename T>
struct Geo : TriGeo<T, kD, kH> {
    static constexpr int kThreads = aggproj::kThreads;
};
}  // namespace aggproj

template <typename T, typename... GS>
__global__ void __launch_bounds__(aggproj::kThreads, 4) tri_agg_proj_fwd_kernel(const tgt_triplet_aggregate_args a, const T* x, const T* w,
                                                                             const T* bias, const uint64_t* seed_ctr, GS... gs) {
    using namespace aggproj;
    using G = Geo<T>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<kH>(a, 0);                      // one head group: blockIdx.x = b*2 + dir
    const int N = c.N, dir = c.dir;
    // a graph DropPath dropped (triplet_common.hpp, agg_dead): zeros to this direction's C columns of every row of the graph.  Its
    // E/G, where they wait inside those columns, are overwritten unread: only this workgroup would have read them.
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        slab_zero_units<G>(0, N, 0, N, tid, agg_o_slab<T, kD, kH>(a.out, a.ld_out, a.o_off[dir], c));
        return;
    }
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);

    // ---- the weights A[i,k] of the two heads, once (the stage aliases the walk's buffers).
    // INVARIANT (part of the entry point's contract, include/tgt_hip.h): ALL of this direction's E/G is read here, and the barrier
    // below is passed, before this workgroup writes its first O row; and this workgroup is the only writer of the columns
    // [o_off[dir], o_off[dir] + C) of its graph.  eg[dir] may therefore live in those columns of `out` (ops.py puts it there).
    // Staging E/G per step, splitting a (graph, direction) over several workgroups, or reading another direction's E/G here would
    // break that silently: such a change must take the aliasing out of the header and of ops._agg_proj_eg_view first.
    static_assert(kH * 64 == 2 * kThreads, "arm_stage_load<T, kH, 1> strides by kH * 64 threads: the two calls below cover it exactly");
    F pa[2][2];
    arm_stage_load<T, kH, 1>(c.ta, c.b, dir, 0, N, 0, smem, tid);
    arm_stage_load<T, kH, 1>(c.ta, c.b, dir, 0, N, 0, smem, tid + kThreads);      // (the loader strides by 1024 threads)
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int h = 2 * wave + hh;
        float p[1][16], gate[16];
        arm_stage_read<T, kH, 1, false>(c.ta, smem, dir, h, N, r, hi, 0, 0, p[0], gate);
        tile_softmax<1>(p);
        f32x16 wgt;
#pragma unroll
        for (int q = 0; q < 16; ++q) wgt[q] = p[0][q] * gate[q];
        if (drop.on) {
            const uint32_t keep = tri_drop_bits(drop, (uint32_t)((c.b * 2 + dir) * a.H + h), r, 0, hi);
#pragma unroll
            for (int q = 0; q < 16; ++q) wgt[q] = (keep >> q) & 1u ? wgt[q] * drop.scale : 0.f;
        }
        pa[hh][0] = pack_chunk<T>(wgt, 0);
        pa[hh][1] = pack_chunk<T>(wgt, 1);
    }
    __syncthreads();

    // ---- resident projection: B[kk][n = r] = W[dir*C + 32*wave + r][16 s + 8 hi + t]
    const int ch = dir * kC + 32 * wave + r;
    F wv[16];
    {
        const T* wr = w + (int64_t)ch * kC + 8 * hi;
#pragma unroll
        for (int s = 0; s < 16; ++s) wv[s] = load_frag<T>(wr + 16 * s);
    }
    const float bv = to_f32(bias[ch]);

    // ---- X tile of step j: rows k of x[j,k,:] (inward) / x[k,j,:] (outward); rows k >= N are zeros (out-of-range loads)
    const __amdgpu_buffer_rsrc_t r_x = graph_rsrc(x, (int64_t)N * N * kRowBytes, c.b);
    const uint32_t x_row = dir == 0 ? (uint32_t)kRowBytes : (uint32_t)N * kRowBytes;
    const uint32_t x_j = dir == 0 ? (uint32_t)N * kRowBytes : (uint32_t)kRowBytes;
    // (the per-thread offsets are rebuilt from the thread index at every use -- a few VALU instructions -- instead of living in
    // registers through the walk next to the resident weights: `t_` is opaque so that nothing is hoisted, as in proj2_walk)
    uint4 px[2];
    auto x_issue = [&](int jx) {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int row = it * 16 + (t_ >> 5), slot = t_ & 31;
            const uint32_t vo = row < N ? (uint32_t)row * x_row + (uint32_t)slot * 16u : kNone;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r_x, (int)vo, (int)((uint32_t)jx * x_j), 0);
            px[it] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    auto x_commit = [&](int jx) {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        char* xt = smem + (jx & 1) * kXTile;
#pragma unroll
        for (int it = 0; it < 2; ++it) *reinterpret_cast<uint4*>(xt + xoff(it * 16 + (t_ >> 5), t_ & 31)) = px[it];
    };
    const SlabBuf bO = agg_o_slab<T, kD, kH>(a.out, a.ld_out, a.o_off[dir], c);

    // Hazards with ONE barrier per step (B_j = the barrier of iteration j): X tile (j+1)&1 is committed in iteration j and was last
    // read in iteration j-1, before B_{j-1}; O slab j&1 is stored after B_j and written again in iteration j+2, after B_{j+1}.
    x_issue(0);
    x_commit(0);
    if (N > 1) x_issue(1);
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        if (j + 1 < N) x_commit(j + 1);
        if (j + 2 < N) x_issue(j + 2);
        const char* xt = smem + (j & 1) * kXTile + xoff(r, hi);
        char* sO = smem + kOffO + (j & 1) * kOSlab;
        f32x16 vt = {0};                                     // V[k = acc_row(q, hi)][channel r of the pair]
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            vt = mma32(load_frag<T>(reinterpret_cast<const T*>(xt + 32 * s)), wv[s], vt);
            // (left alone the scheduler hoists all 16 fragment reads to the top of the step: 64 registers next to the 64 of weights)
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        // (the bias joins V here, before the weighted sum: seeded into the accumulator it is kept as 16 registers through the walk)
#pragma unroll
        for (int q = 0; q < 16; ++q) vt[q] += bv;
        const F va[2] = {pack_chunk<T>(vt, 0), pack_chunk<T>(vt, 1)};
        // O^T[channel][i = r] = V^T A_head^T, one head after the other (one accumulator alive): rows 0..15 of the first product and
        // rows 16..31 of the second are the heads' own, the other halves are dropped
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            f32x16 o = {0};
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) o = mma32(va[cc], pa[hh][cc], o);
            f32x16 own;
#pragma unroll
            for (int q = 0; q < 8; ++q) own[q] = o[8 * hh + q], own[8 + q] = 0.f;
            write_rows<T, kD, kH>(sO, own, 2 * wave + hh, r, hi);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        slab_store<G, 32>(sO, bO, j, 0, N, t_);
    }
}

int triplet_aggregate_proj_supported(const tgt_triplet_aggregate_args* a, int C) {
    return a && a->N >= 0 && a->N <= 32 && a->D == aggproj::kD && a->H == aggproj::kH && (a->dtype == TGT_BF16 || a->dtype == TGT_F16) &&
           C == aggproj::kC;
}

template <typename T, typename... GS>
static int launch_agg_proj(const tgt_triplet_aggregate_args& a, const void* x, const void* w, const void* bias, hipStream_t st, GS... gs) {
    constexpr int kArm = ArmStage<T, aggproj::kH, 1>::kBytes;
    constexpr int kLds = cmax(aggproj::kWalk, kArm);
    return launch_lds<tri_agg_proj_fwd_kernel<T, GS...>>("tri_agg_proj_fwd_kernel", dim3(a.B * 2), dim3(aggproj::kThreads), kLds, st, a,
                                                         reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(w), reinterpret_cast<const T*>(bias), seed_counter(), gs...);
}

int triplet_aggregate_proj_run(const tgt_triplet_aggregate_args* a, const float* graph_scale, const void* x, int C, const void* w, const void* bias,
                               hipStream_t st) {
    if (!a) return set_error(TGT_ERR_INVALID, "projected triplet aggregate: null args");
    if (a->B < 0 || a->N < 0 || a->H <= 0 || C <= 0) return set_error(TGT_ERR_INVALID, "projected triplet aggregate: bad sizes");
    if (!triplet_aggregate_proj_supported(a, C))
        return set_error(TGT_ERR_UNSUPPORTED,
                         "projected triplet aggregate needs N <= 32, D = 16, H = 16, a 16-bit dtype and C = 256 (got N=%d D=%d H=%d dtype=%d C=%d)",
                         a->N, a->D, a->H, a->dtype, C);
    if (a->B == 0 || a->N == 0) return TGT_OK;
    if (!x || !w || !bias || !a->eg[0] || !a->eg[1] || !a->mask || !a->out)       // (a->v is never examined)
        return set_error(TGT_ERR_INVALID, "projected triplet aggregate: null tensor");
    if ((a->ld_out * 2) % 16 || (a->o_off[0] * 2) % 16 || (a->o_off[1] * 2) % 16 || ((uintptr_t)a->out % 16) ||
        (((uintptr_t)x | (uintptr_t)w) % 16) || ((uintptr_t)bias % 2))
        return set_error(TGT_ERR_INVALID, "projected triplet aggregate: x / w / out rows and offsets must be 16-byte aligned");
    const bool gated = (a->flags & TGT_TRI_GATED) != 0;
    for (int dir = 0; dir < 2; ++dir)                       // every E / G column of a pair must lie inside its row of ld_eg elements
        if (a->ld_eg[dir] < aggproj::kH || a->e_off[dir] < 0 || a->e_off[dir] + aggproj::kH > a->ld_eg[dir] ||
            (gated && (a->g_off[dir] < 0 || a->g_off[dir] + aggproj::kH > a->ld_eg[dir])))
            return set_error(TGT_ERR_INVALID, "projected triplet aggregate: e_off / g_off + H outside the E/G row (ld_eg=%lld)", (long long)a->ld_eg[dir]);
    if ((uintptr_t)graph_scale % 4) return set_error(TGT_ERR_INVALID, "projected triplet aggregate: graph_scale must be 4-byte aligned");
    // (without factors: the kernel's instantiation without the argument -- triplet_common.hpp, agg_dead)
    if (graph_scale) return a->dtype == TGT_BF16 ? launch_agg_proj<bf16_t>(*a, x, w, bias, st, graph_scale) : launch_agg_proj<f16_t>(*a, x, w, bias, st, graph_scale);
    return a->dtype == TGT_BF16 ? launch_agg_proj<bf16_t>(*a, x, w, bias, st) : launch_agg_proj<f16_t>(*a, x, w, bias, st);
}

}  // namespace tgt
