// Triplet aggregate forward with the V projection fused in, 33 <= N <= 64 -- gfx950, inference only (no backward follows).
//
// The two-tile sibling of triplet_aggregate_proj.hip.  The unfused path at these node counts is a library GEMM
// that writes the 576-channel fused row and tri_agg_fwd_kernel<T, 16, 4, 2>, which walks the graph once per 32-row query tile
// and so reads every V slab twice; here V never reaches global memory and every X row is projected ONCE per step j.
//
//   workgroup = (graph b, direction): all 16 heads, so every X row is fetched by ONE workgroup per direction;
//   8 waves, wave = the head PAIR (2w, 2w + 1), at up to 256 registers (one workgroup per CU, two waves per SIMD):
//     * resident through the walk: the pair's 32 weight rows x 256 k as the B operands of 16 v_mfma_f32_32x32x16 (64 registers)
//       and the pair's weights A[i,k] of BOTH 32-row query tiles x BOTH 32-key tiles as operand fragments (2 heads x 2 x 2 tiles
//       x 8 registers = 64 registers) -- neither depends on j;
//     * per step j: the X tile of up to 64 rows k (LDS, rows padded to 528 bytes as aggproj::xoff) is projected once, key tile by
//       key tile: V[k][(head, d)] = X W^T + b comes out of the matrix core as lane = channel, registers = k, and is packed into
//       operand fragments in registers; then, per head and query tile, O^T[(head, d)][i] = sum over both key tiles of V^T A^T, of
//       which that head's 16 rows are kept (one accumulator alive);
//     * the O rows of both query tiles leave as whole 512-byte rows through a 64-row O slab; X tiles and O slabs are
//       double-buffered: ONE barrier per step.
//   Keys k >= N: their X rows load as zeros, so their V is the projection bias, not 0 -- their WEIGHT is exactly 0
//   (arm_stage_read gives them a logit of -inf and a gate of 0), which is what keeps them out of every sum.
// Supported: C = 256, D = 16, H = 16, 33 <= N <= 64, 16-bit dtypes, gated and ungated, attention dropout (the plain kernel's
// pattern at this N: unit (b*2 + dir)*H + h, word (i*64 + k) >> 1).
#include "triplet_common.hpp"

namespace tgt {

namespace aggproj64 {
constexpr int kC = 256, kD = 16, kH = 16, kWaves = 8, kThreads = kWaves * 64;
constexpr int kRows = 64;                                    // rows of an X tile (keys k) and of an O slab (queries i)
constexpr int kRowBytes = kC * 2;                            // an X row and an O row of one direction: 512 bytes
constexpr int kXPitch = kRowBytes + 16;                      // (see proj2::xoff in triplet_attention_proj.hip)
constexpr int kXTile = kRows * kXPitch;
constexpr int kOSlab = kRows * kRowBytes;
constexpr int kOffO = 2 * kXTile;
constexpr int kWalk = kOffO + 2 * kOSlab;
constexpr int kXIters = kRows * (kRowBytes / 16) / kThreads;  // 16-byte pieces of an X tile per thread
constexpr uint32_t kNone = 0xffffffffu;
__device__ __forceinline__ int xoff(int row, int slot) { return row * kXPitch + (slot << 4); }
// the 16-head slab geometry of triplet_common.hpp, walked by this kernel's 512 threads
template <typename T>
struct Geo : TriGeo<T, kD, kH> {
    static constexpr int kThreads = aggproj64::kThreads;
};
}  // namespace aggproj64

template <typename T, typename... GS>
__global__ void __launch_bounds__(aggproj64::kThreads, 2) tri_agg_proj64_fwd_kernel(const tgt_triplet_aggregate_args a, const T* x, const T* w,
                                                                                 const T* bias, const uint64_t* seed_ctr, GS... gs) {
    using namespace aggproj64;
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
        const SlabBuf zO = agg_o_slab<T, kD, kH>(a.out, a.ld_out, a.o_off[dir], c);
        for (int i0 = 0; i0 < N; i0 += 32) slab_zero_units<G>(0, N, i0, N, tid, zO);
        return;
    }
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);

    // ---- the weights A[i,k] of the two heads, both query tiles x both key tiles, once (the stage aliases the walk's buffers; it
    // holds one 32-row query pass, so two passes).
    // INVARIANT (part of the entry point's contract, include/tgt_hip.h): ALL of this direction's E/G is read here -- both passes --
    // and the barrier that ends the second pass is passed, before this workgroup writes its first O row; and this workgroup is the
    // only writer of the columns [o_off[dir], o_off[dir] + C) of its graph.  eg[dir] may therefore live in those columns of `out`
    // (ops.py puts it there).  See triplet_aggregate_proj.hip for what would break that.
    static_assert(kH * 64 == 2 * kThreads, "arm_stage_load<T, kH, 2> strides by kH * 64 threads: the two calls below cover it exactly");
    F pa[2][2][2][2];                                        // [head of the pair][query tile][key tile][16-key chunk]
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i0 = 32 * it;
        arm_stage_load<T, kH, 2>(c.ta, c.b, dir, 0, N, i0, smem, tid);
        arm_stage_load<T, kH, 2>(c.ta, c.b, dir, 0, N, i0, smem, tid + kThreads);  // (the loader strides by 1024 threads)
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int h = 2 * wave + hh;
            float p[2][16], gate[2][16];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) arm_stage_read<T, kH, 2, false>(c.ta, smem, dir, h, N, r, hi, i0, kt, p[kt], gate[kt]);
            tile_softmax<2>(p);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                f32x16 wgt;
#pragma unroll
                for (int q = 0; q < 16; ++q) wgt[q] = p[kt][q] * gate[kt][q];
                if (drop.on) {
                    const uint32_t keep = tri_drop_bits(drop, (uint32_t)((c.b * 2 + dir) * a.H + h), i0 + r, kt, hi);
#pragma unroll
                    for (int q = 0; q < 16; ++q) wgt[q] = (keep >> q) & 1u ? wgt[q] * drop.scale : 0.f;
                }
                pa[hh][it][kt][0] = pack_chunk<T>(wgt, 0);
                pa[hh][it][kt][1] = pack_chunk<T>(wgt, 1);
            }
        }
        __syncthreads();
    }

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
    // (the per-thread offsets are rebuilt from the thread index at every use instead of living in registers through the walk:
    // `t_` is opaque so that nothing is hoisted, as in tri_agg_proj_fwd_kernel)
    uint4 px[kXIters];
    auto x_issue = [&](int jx) {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
#pragma unroll
        for (int it = 0; it < kXIters; ++it) {
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
        for (int it = 0; it < kXIters; ++it) *reinterpret_cast<uint4*>(xt + xoff(it * 16 + (t_ >> 5), t_ & 31)) = px[it];
    };
    const SlabBuf bO = agg_o_slab<T, kD, kH>(a.out, a.ld_out, a.o_off[dir], c);

    // Hazards with ONE barrier per step (B_j = the barrier of iteration j): X tile (j+1)&1 is committed in iteration j and was last
    // read in iteration j-1, before B_{j-1}; O slab j&1 is stored after B_j and written again in iteration j+2, after B_{j+1}.
    x_issue(0);
    x_commit(0);
    x_issue(1);                                              // (N >= 33)
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        if (j + 1 < N) x_commit(j + 1);
        if (j + 2 < N) x_issue(j + 2);
        char* sO = smem + kOffO + (j & 1) * kOSlab;
        // V[k = 32 kt + acc_row(q, hi)][channel r of the pair], both key tiles, as operand fragments
        F va[2][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const char* xt = smem + (j & 1) * kXTile + xoff(32 * kt + r, hi);
            f32x16 vt = {0};
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                vt = mma32(load_frag<T>(reinterpret_cast<const T*>(xt + 32 * s)), wv[s], vt);
                // (left alone the scheduler hoists all fragment reads to the top of the step)
                if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            // (the bias joins V here, after the projection: seeded into the accumulator it is kept as 16 registers through the walk)
#pragma unroll
            for (int q = 0; q < 16; ++q) vt[q] += bv;
            va[kt][0] = pack_chunk<T>(vt, 0);
            va[kt][1] = pack_chunk<T>(vt, 1);
        }
        // O^T[channel][i = 32 it + r] = sum_kt V_kt^T A_head[it][kt]^T, one (head, query tile) after the other: rows 0..15 of a
        // first-head product and rows 16..31 of a second-head product are the heads' own, the other halves are dropped
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f32x16 o = {0};
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) o = mma32(va[kt][cc], pa[hh][it][kt][cc], o);
                f32x16 own;
#pragma unroll
                for (int q = 0; q < 8; ++q) own[q] = o[8 * hh + q], own[8 + q] = 0.f;
                write_rows<T, kD, kH>(sO, own, 2 * wave + hh, 32 * it + r, hi);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        slab_store<G, kRows>(sO, bO, j, 0, N, t_);           // rows i >= N are not stored
    }
}

int triplet_aggregate_proj64_supported(const tgt_triplet_aggregate_args* a, int C) {
    return a && a->N >= 33 && a->N <= 64 && a->D == aggproj64::kD && a->H == aggproj64::kH && (a->dtype == TGT_BF16 || a->dtype == TGT_F16) &&
           C == aggproj64::kC;
}

template <typename T, typename... GS>
static int launch_agg_proj64(const tgt_triplet_aggregate_args& a, const void* x, const void* w, const void* bias, hipStream_t st, GS... gs) {
    constexpr int kArm = ArmStage<T, aggproj64::kH, 2>::kBytes;
    constexpr int kLds = cmax(aggproj64::kWalk, kArm);
    static_assert(kLds <= 160 * 1024, "one workgroup must fit the LDS of a CU");
    return launch_lds<tri_agg_proj64_fwd_kernel<T, GS...>>("tri_agg_proj64_fwd_kernel", dim3(a.B * 2), dim3(aggproj64::kThreads), kLds, st, a,
                                                           reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(w), reinterpret_cast<const T*>(bias), seed_counter(), gs...);
}

// (check order and words: triplet_aggregate_proj_run)
int triplet_aggregate_proj64_run(const tgt_triplet_aggregate_args* a, const float* graph_scale, const void* x, int C, const void* w, const void* bias,
                                 hipStream_t st) {
    if (!a) return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): null args");
    if (a->B < 0 || a->N < 0 || a->H <= 0 || C <= 0) return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): bad sizes");
    if (!triplet_aggregate_proj64_supported(a, C))
        return set_error(TGT_ERR_UNSUPPORTED,
                         "projected triplet aggregate (33..64 nodes) needs 33 <= N <= 64, D = 16, H = 16, a 16-bit dtype and C = 256 (got N=%d D=%d H=%d dtype=%d C=%d)",
                         a->N, a->D, a->H, a->dtype, C);
    if (a->B == 0) return TGT_OK;
    if (!x || !w || !bias || !a->eg[0] || !a->eg[1] || !a->mask || !a->out)       // (a->v is never examined)
        return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): null tensor");
    if ((a->ld_out * 2) % 16 || (a->o_off[0] * 2) % 16 || (a->o_off[1] * 2) % 16 || ((uintptr_t)a->out % 16) ||
        (((uintptr_t)x | (uintptr_t)w) % 16) || ((uintptr_t)bias % 2))
        return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): x / w / out rows and offsets must be 16-byte aligned");
    const bool gated = (a->flags & TGT_TRI_GATED) != 0;
    for (int dir = 0; dir < 2; ++dir)                       // every E / G column of a pair must lie inside its row of ld_eg elements
        if (a->ld_eg[dir] < aggproj64::kH || a->e_off[dir] < 0 || a->e_off[dir] + aggproj64::kH > a->ld_eg[dir] ||
            (gated && (a->g_off[dir] < 0 || a->g_off[dir] + aggproj64::kH > a->ld_eg[dir])))
            return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): e_off / g_off + H outside the E/G row (ld_eg=%lld)",
                             (long long)a->ld_eg[dir]);
    if ((uintptr_t)graph_scale % 4) return set_error(TGT_ERR_INVALID, "projected triplet aggregate (33..64 nodes): graph_scale must be 4-byte aligned");
    // (without factors: the kernel's instantiation without the argument -- triplet_common.hpp, agg_dead)
    if (graph_scale) return a->dtype == TGT_BF16 ? launch_agg_proj64<bf16_t>(*a, x, w, bias, st, graph_scale) : launch_agg_proj64<f16_t>(*a, x, w, bias, st, graph_scale);
    return a->dtype == TGT_BF16 ? launch_agg_proj64<bf16_t>(*a, x, w, bias, st) : launch_agg_proj64<f16_t>(*a, x, w, bias, st);
}

}  // namespace tgt
