// Triplet aggregate core (TripletAggregate / TripletAggregateUngated) for
// gfx950 -- forward and backward.
//
// Replaces reference lib/tgt/layers/triplet.py:56-70 and :107-123: the
// softmax*gate over the third arm followed by einsum('bikh,bjkdh->bijdh') /
// einsum('bkih,bkjdh->bijdh'), and their autograd backward.  SURVEY App. A.3.
//
// Same decomposition as triplet_attention.hip (workgroup = (graph, direction,
// head group), wave = head, walk over the shared node j), but the weights
// A[i,k] do not depend on j: each wave computes its 32x32 weight tile ONCE
// from E/G/M, keeps it in registers as matrix-core operand fragments, and per
// j only streams the V slab:   O^T[d][i] = sum_k V^T[d][k] A^T[k][i].
// Backward: dA^T[k][i] = sum_j V[j,k,:].dO[i,j,:] accumulates across the walk
// inside the MFMA accumulator; dV^T[d][k] = sum_i dO^T[d][i] A[i][k] per j.
#include "triplet_common.hpp"

namespace tgt {

// weights of query tile it / key tile kt in (lane = i) layout: softmax over ALL key tiles
// (the E/G/mask tiles come through the LDS stage: two barriers inside, `lds` aliases the slabs)
template <typename T, int HG, int NT, bool PAD>
__device__ __forceinline__ void agg_weights(const AggCtx& c, int N, int wave, int tid, int r, int hi, int i0, char* lds,
                                            float (&p)[NT][16], float (&gate)[NT][16]) {
    arm_stage_load<T, HG, NT>(c.ta, c.b, c.dir, c.g, N, i0, lds, tid);
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
        arm_stage_read<T, HG, NT, PAD>(c.ta, lds, c.dir, wave, N, r, hi, i0, kt, p[kt], gate[kt]);
    __syncthreads();
    tile_softmax<NT>(p);
}

template <typename T, int D, int HG, int NT, typename... GS>
__global__ void __launch_bounds__(HG * 64) tri_agg_fwd_kernel(const tgt_triplet_aggregate_args a, const uint64_t* seed_ctr, GS... gs) {
    using G = TriGeo<T, D, HG>;
    using F = frag_t<T>;
    constexpr int KR = 32 * NT;
    // two LDS sets {V | O}: set j&1 is computed on while slab j+1 lands in the other one -> ONE barrier per j
    // (hazards as in triplet_attention.hip)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kSet = (NT + 1) * G::kSlabBytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<HG>(a, wave);
    const int N = c.N;
    // a graph DropPath dropped (triplet_common.hpp, agg_dead): zeros to this head group's O columns of every (i, j) row
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        const SlabBuf zO = agg_o_slab<T, D, HG>(a.out, a.ld_out, a.o_off[c.dir], c);
        for (int i0 = 0; i0 < N; i0 += 32) slab_zero_units<G>(0, N, i0, N, tid, zO);
        return;
    }
    F ident_d[G::kDC];
    make_ident_d<T, G::kDC>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit = (uint32_t)((c.b * 2 + c.dir) * a.H + c.h);
    const SlabBuf bV = agg_v_slab<T, D, HG>(a.v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
    const SlabBuf bO = agg_o_slab<T, D, HG>(a.out, a.ld_out, a.o_off[c.dir], c);

    for (int it = 0; it < NT; ++it) {
        const int i0 = 32 * it;
        if (i0 >= N) break;
        F pa[NT][2];
        {
            float p[NT][16], gate[NT][16];
            agg_weights<T, HG, NT, false>(c, N, wave, tid, r, hi, i0, smem, p, gate);
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                f32x16 w;
#pragma unroll
                for (int q = 0; q < 16; ++q) w[q] = p[kt][q] * gate[kt][q];
                if (drop.on) {
                    const uint32_t keep = tri_drop_bits(drop, drop_unit, i0 + r, kt, hi);
#pragma unroll
                    for (int q = 0; q < 16; ++q) w[q] = (keep >> q) & 1u ? w[q] * drop.scale : 0.f;
                }
                pa[kt][0] = pack_chunk<T>(w, 0);
                pa[kt][1] = pack_chunk<T>(w, 1);
            }
        }
        uint4 pv[SlabIO<G, KR>::kIters];
        slab_issue<G, KR>(pv, bV, 0, 0, N, tid);
        slab_commit<G, KR>(pv, smem, tid);
        if (N > 1) slab_issue<G, KR>(pv, bV, 1, 0, N, tid);
        __syncthreads();
        for (int j = 0; j < N; ++j) {
            char* sV = smem + (j & 1) * kSet;
            char* sOut = sV + NT * G::kSlabBytes;
            if (j + 1 < N) slab_commit<G, KR>(pv, smem + ((j + 1) & 1) * kSet, tid);
            if (j + 2 < N) slab_issue<G, KR>(pv, bV, j + 2, 0, N, tid);
            f32x16 o = {0};
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                F fv[G::kDC];
                read_frags<T, D, HG>(fv, sV, wave, 32 * kt + r, hi);
                f32x16 vt = {0};
#pragma unroll
                for (int dc = 0; dc < G::kDC; ++dc) vt = mma32(fv[dc], ident_d[dc], vt);
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) o = mma32(pack_chunk<T>(vt, cc), pa[kt][cc], o);
            }
            write_rows<T, D, HG>(sOut, o, wave, r, hi);
            __syncthreads();
            slab_store<G, 32>(sOut, bO, j, i0, N, tid);
        }
        __syncthreads();      // the next query-tile pass re-fills the stage and both sets
    }
}

template <typename T, int D, int HG, int NT, typename... GS>
__global__ void __launch_bounds__(HG * 64) tri_agg_bwd_kernel(const tgt_triplet_aggregate_args a, const uint64_t* seed_ctr, GS... gs) {
    using G = TriGeo<T, D, HG>;
    using F = frag_t<T>;
    constexpr int KR = 32 * NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kSet = (NT + 1) * G::kSlabBytes;        // {dO | V}, two sets (see forward)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<HG>(a, wave);
    const int N = c.N;
    // a graph DropPath dropped receives an all-zero d_out, which is not read: zeros to this head group's d_v columns of every
    // (j, k) row and, through the stage (several workgroups can share a 16-byte piece of a narrow E/G row), to its heads' E/G
    // columns of d_eg
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        const SlabBuf zV = agg_v_slab<T, D, HG>(a.d_v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
        for (int j = 0; j < N; ++j) slab_store_zero<G, KR>(zV, j, 0, N, tid);
        for (int i0 = 0; i0 < N; i0 += 32)
            arm_stage_zero_grad<T, HG, NT>(c.ta, a.d_eg[c.dir], c.b, c.dir, c.g, N, i0, smem, wave, tid, r, hi);
        return;
    }

    F ident_d[G::kDC];
    make_ident_d<T, G::kDC>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit = (uint32_t)((c.b * 2 + c.dir) * a.H + c.h);
    const SlabBuf bV = agg_v_slab<T, D, HG>(a.v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
    const SlabBuf dV = agg_v_slab<T, D, HG>(a.d_v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);      // d_v mirrors v
    const SlabBuf dO = agg_o_slab<T, D, HG>(a.d_out, a.ld_out, a.o_off[c.dir], c);

    for (int it = 0; it < NT; ++it) {
        const int i0 = 32 * it;
        if (i0 >= N) break;
        // weights in (lane = k, registers = i) layout, as operand fragments over i
        F a2f[NT][2];
        {
            float p[NT][16], gate[NT][16];
            agg_weights<T, HG, NT, true>(c, N, wave, tid, r, hi, i0, smem, p, gate);
            F ident_k[2];
            make_ident_k<T>(ident_k, r, hi);
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                f32x16 w, a2 = {0};
#pragma unroll
                for (int q = 0; q < 16; ++q) w[q] = p[kt][q] * gate[kt][q];
                if (drop.on) {
                    const uint32_t keep = tri_drop_bits(drop, drop_unit, i0 + r, kt, hi);
#pragma unroll
                    for (int q = 0; q < 16; ++q) w[q] = (keep >> q) & 1u ? w[q] * drop.scale : 0.f;
                }
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) a2 = mma32(pack_chunk<T>(w, cc), ident_k[cc], a2);
                a2f[kt][0] = pack_chunk<T>(a2, 0);
                a2f[kt][1] = pack_chunk<T>(a2, 1);
            }
        }
        f32x16 dacc[NT];          // dA^T[k][i], summed over j
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int q = 0; q < 16; ++q) dacc[kt][q] = 0.f;

        uint4 pv[SlabIO<G, KR>::kIters], po[SlabIO<G, 32>::kIters];
        slab_issue<G, 32>(po, dO, 0, i0, N, tid);
        slab_issue<G, KR>(pv, bV, 0, 0, N, tid);
        slab_commit<G, 32>(po, smem, tid);
        slab_commit<G, KR>(pv, smem + G::kSlabBytes, tid);
        if (N > 1) {
            slab_issue<G, 32>(po, dO, 1, i0, N, tid);
            slab_issue<G, KR>(pv, bV, 1, 0, N, tid);
        }
        __syncthreads();
        for (int j = 0; j < N; ++j) {
            char* sO = smem + (j & 1) * kSet;
            char* sV = sO + G::kSlabBytes;
            if (j + 1 < N) {
                char* nO = smem + ((j + 1) & 1) * kSet;
                slab_commit<G, 32>(po, nO, tid);
                slab_commit<G, KR>(pv, nO + G::kSlabBytes, tid);
            }
            if (j + 2 < N) {
                slab_issue<G, 32>(po, dO, j + 2, i0, N, tid);
                slab_issue<G, KR>(pv, bV, j + 2, 0, N, tid);
            }
            // partial dV the previous query-tile pass stored for THIS j (added at the store below)
            uint4 curv[NT > 1 ? SlabIO<G, KR>::kIters : 1];
            if constexpr (NT > 1) {
                if (it > 0) slab_issue<G, KR>(curv, dV, j, 0, N, tid);
            }
            F fo[G::kDC];
            read_frags<T, D, HG>(fo, sO, wave, r, hi);
            f32x16 t2 = {0};
#pragma unroll
            for (int dc = 0; dc < G::kDC; ++dc) t2 = mma32(fo[dc], ident_d[dc], t2);   // dO^T
            F oTf[2] = {pack_chunk<T>(t2, 0), pack_chunk<T>(t2, 1)};
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                F fv[G::kDC];
                read_frags<T, D, HG>(fv, sV, wave, 32 * kt + r, hi);
#pragma unroll
                for (int dc = 0; dc < G::kDC; ++dc) dacc[kt] = mma32(fv[dc], fo[dc], dacc[kt]);
                f32x16 dv = {0};
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) dv = mma32(oTf[cc], a2f[kt][cc], dv);
                // (in place: this wave only reads its own columns, and only of rows it has not overwritten yet)
                write_rows<T, D, HG>(sV, dv, wave, 32 * kt + r, hi);
            }
            __syncthreads();
            bool plain = true;
            if constexpr (NT > 1) {
                if (it > 0) {
                    plain = false;
                    slab_store_add<G, KR, T>(sV, curv, dV, j, 0, N, tid);
                }
            }
            if (plain) slab_store<G, KR>(sV, dV, j, 0, N, tid);
        }
        __syncthreads();      // the stage below aliases both sets

        // softmax*gate backward on the accumulated dA (recompute P, g)
        float p[NT][16], gate[NT][16];
        agg_weights<T, HG, NT, true>(c, N, wave, tid, r, hi, i0, smem, p, gate);
        float delta = 0.f;
        float dG[NT][16];
        if (drop.on) {            // dacc is the gradient of the DROPPED weights
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                const uint32_t keep = tri_drop_bits(drop, drop_unit, i0 + r, kt, hi);
#pragma unroll
                for (int q = 0; q < 16; ++q) dacc[kt][q] = (keep >> q) & 1u ? dacc[kt][q] * drop.scale : 0.f;
            }
        }
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                dG[kt][q] = dacc[kt][q] * p[kt][q] * gate[kt][q] * (1.f - gate[kt][q]);
                dacc[kt][q] *= gate[kt][q];
                delta += p[kt][q] * dacc[kt][q];
            }
        delta += xhalf(delta);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            float dE[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) dE[q] = p[kt][q] * (dacc[kt][q] - delta);
            arm_stage_put_grad<T, HG, NT>(smem, c.dir, wave, r, hi, kt, dE, dG[kt]);
        }
        __syncthreads();
        arm_stage_store_grad<T, HG, NT>(c.ta, a.d_eg[c.dir], c.b, c.dir, c.g, N, i0, smem, tid);
        __syncthreads();
    }
}

template <typename T, int D, int HG, int NT, typename... GS>
static int launch_agg_nt(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    using G = TriGeo<T, D, HG>;
    const int grid = a.B * 2 * (a.H / HG);
    constexpr int kArm = ArmStage<T, HG, NT>::kBytes;
    constexpr int kLds = 2 * (NT + 1) * G::kSlabBytes > kArm ? 2 * (NT + 1) * G::kSlabBytes : kArm;
    if (!bwd) hipLaunchKernelGGL((tri_agg_fwd_kernel<T, D, HG, NT, GS...>), dim3(grid), dim3(G::kThreads), kLds, st, a, seed_counter(), gs...);
    else      hipLaunchKernelGGL((tri_agg_bwd_kernel<T, D, HG, NT, GS...>), dim3(grid), dim3(G::kThreads), kLds, st, a, seed_counter(), gs...);
    return check_launch(bwd ? "tri_agg_bwd_kernel" : "tri_agg_fwd_kernel");
}
template <typename T, int D, int HG, typename... GS>
static int launch_agg(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    if (a.N <= 32) return launch_agg_nt<T, D, HG, 1>(a, bwd, st, gs...);
    return launch_agg_nt<T, D, HG, 2>(a, bwd, st, gs...);
}
template <typename T, int D, typename... GS>
static int agg_dispatch_hg(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    if constexpr (D == 16 && sizeof(T) == 2) {
        if (a.H % 8 == 0 && a.N <= 32) return launch_agg_nt<T, D, 8, 1>(a, bwd, st, gs...);     // 256-byte row pieces
    }
    if (a.H % 4 == 0) return launch_agg<T, D, 4>(a, bwd, st, gs...);
    if constexpr (D * sizeof(T) >= 16) return launch_agg<T, D, 1>(a, bwd, st, gs...);
    return set_error(TGT_ERR_UNSUPPORTED, "triplet aggregate: H=%d not a multiple of 4 with D=%d", a.H, D);
}
template <typename T, typename... GS>
static int agg_dispatch_d(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    switch (a.D) {
        case 8: return agg_dispatch_hg<T, 8>(a, bwd, st, gs...);
        case 16: return agg_dispatch_hg<T, 16>(a, bwd, st, gs...);
        case 32: return agg_dispatch_hg<T, 32>(a, bwd, st, gs...);
        default: return set_error(TGT_ERR_UNSUPPORTED, "triplet aggregate: D=%d not in {8,16,32}", a.D);
    }
}

int tri_agg_kb_run(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st);      // triplet_aggregate_kb.hip: 65 <= N <= 128, D = 16

template <typename... GS>
static int agg_dispatch_dtype(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    switch (a.dtype) {
        case TGT_F32: return agg_dispatch_d<float>(a, bwd, st, gs...);
        case TGT_BF16: return agg_dispatch_d<bf16_t>(a, bwd, st, gs...);
        case TGT_F16: return agg_dispatch_d<f16_t>(a, bwd, st, gs...);
        default: return set_error(TGT_ERR_INVALID, "triplet aggregate: bad dtype %d", a.dtype);
    }
}

// The kernels with the factors compile in a translation unit of their own (TGT_AGG_INST: bit 0 the kernels without factors and
// the entry point, bit 1 the kernels with them): co-compiled with their siblings, every tri_agg_bwd_kernel WITHOUT the argument
// came out of hipcc with another scalar register allocation and more spills than it was measured with.
#ifndef TGT_AGG_INST
#define TGT_AGG_INST 3
#endif
int triplet_aggregate_skip_run(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st);
#if TGT_AGG_INST & 2
// N <= 64, arguments already validated by triplet_aggregate_run, graph_scale not NULL
int triplet_aggregate_skip_run(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) {
    return agg_dispatch_dtype(a, bwd, st, graph_scale);
}
#endif

#if TGT_AGG_INST & 1
// graph_scale: (B) float32 device memory or NULL (tgt_triplet_aggregate_fwd_skip / _bwd_skip); never read on the host
int triplet_aggregate_run(const tgt_triplet_aggregate_args* a, const float* graph_scale, bool bwd, hipStream_t st) {
    if (!a) return set_error(TGT_ERR_INVALID, "triplet aggregate: null args");
    if (a->B < 0 || a->N < 0 || a->H <= 0) return set_error(TGT_ERR_INVALID, "triplet aggregate: bad sizes");
    if (a->B == 0 || a->N == 0) return TGT_OK;
    if (a->N > 128) return set_error(TGT_ERR_UNSUPPORTED, "triplet aggregate: N=%d > 128 not supported", a->N);
    if (a->N > 64 && a->D != 16)
        return set_error(TGT_ERR_UNSUPPORTED, "triplet aggregate: N=%d > 64 is supported for D = 16 only (D=%d)", a->N, a->D);
    const int64_t esz = a->dtype == TGT_F32 ? 4 : 2;
    for (int dir = 0; dir < 2; ++dir) {
        if (!a->v[dir] || !a->eg[dir] || !a->out || !a->mask) return set_error(TGT_ERR_INVALID, "triplet aggregate: null tensor");
        if ((a->ld_v[dir] * esz) % 16 || (a->v_off[dir] * esz) % 16 || (a->ld_out * esz) % 16 ||
            (a->o_off[dir] * esz) % 16 || ((uintptr_t)a->v[dir] % 16) || ((uintptr_t)a->out % 16))
            return set_error(TGT_ERR_INVALID, "triplet aggregate: rows/offsets must be 16-byte aligned");
        if (bwd && (!a->d_out || !a->d_v[dir] || !a->d_eg[dir] || ((uintptr_t)a->d_v[dir] % 16) || ((uintptr_t)a->d_out % 16)))
            return set_error(TGT_ERR_INVALID, "triplet aggregate bwd: null/misaligned gradient tensor");
    }
    if ((uintptr_t)graph_scale % 4) return set_error(TGT_ERR_INVALID, "triplet aggregate: graph_scale must be 4-byte aligned");
    if (a->N > 64) return tri_agg_kb_run(*a, graph_scale, bwd, st);                // key-blocked kernels
    // (without factors: the kernels' instantiations without the argument)
    return graph_scale ? triplet_aggregate_skip_run(*a, graph_scale, bwd, st) : agg_dispatch_dtype(*a, bwd, st);
}
#endif

}  // namespace tgt
