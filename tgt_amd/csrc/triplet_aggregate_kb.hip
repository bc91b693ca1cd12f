// Triplet aggregate core for 65 <= N <= 128 (D = 16): key-blocked kernels for gfx950.
//
// Same arithmetic, operand layouts and matrix-core mapping as triplet_aggregate.hip (read its header first); what changes is
// what a workgroup owns, because four key tiles of everything do not fit one wave next to each other.
//   forward   workgroup = (graph, direction, head group, query tile of 32).  The wave of a head computes the 32 x 128 weight
//             strip of its query tile once, keeps it as operand fragments and walks j, streaming the 128-row V slab
//             (double-buffered, one barrier per j).  One query tile per workgroup: four times the workgroups to fill the CUs
//             at the batch sizes these graphs allow, the V slabs of the other three tiles come out of L2.
//   backward  two launches, no atomics, every sum in a fixed order inside one wave:
//     A sweep  owns a query tile, walks j: dA^T[k][i] = sum_j V[j,k,:].dO[i,j,:] in four accumulators, then dropout, gate and
//              softmax backward, dE / dG stored once.
//     V sweep  owns 32 consecutive j, holds the weights of ALL (i, k) of its head as operand fragments (lane = k), and per j
//              sums dV[j,k,:] = sum_i A[i,k] dO[i,j,:] over the four query tiles in the fp32 accumulator; dV is stored once,
//              nothing is read back from HBM.
// The softmax runs over all live keys: the E / G / mask tiles come through LDS one (query tile, key tile) block at a time
// (32 x 32 pairs, ArmStage<T, HG, 1>: arm_stage_* of triplet_common.hpp with key origin k0 = 32*kt), the raw logits stay in
// registers until the row maximum and sum are known (tile_softmax).  AggCtx and the slab descriptors are those of N <= 64.
// Dropout: unit (b*2 + dir)*H + h as for N <= 64, word index (i*128 + k) >> 1 (triplet_common.hpp).
#include "triplet_common.hpp"

namespace tgt {

// softmax weights p and gates of query tile i0 against ALL key tiles, (lane = i) layout.  Key tiles past N are never staged:
// their logits are -inf (weight exactly 0) and their gates 0.  Two barriers per staged tile; `lds` aliases the slab sets.
template <typename T, int HG, bool PAD>
__device__ __forceinline__ void agg_kb_softmax(const AggCtx& c, int wave, int tid, int r, int hi, int i0, char* lds,
                                               float (&p)[4][16], float (&gate)[4][16]) {
    const int N = c.N;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (32 * kt < N) {
            arm_stage_load<T, HG, 1>(c.ta, c.b, c.dir, c.g, N, i0, lds, tid, 32 * kt);
            __syncthreads();
            arm_stage_read<T, HG, 1, PAD>(c.ta, lds, c.dir, wave, N, r, hi, i0, 0, p[kt], gate[kt], 32 * kt);
            __syncthreads();
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) { p[kt][q] = -INFINITY; gate[kt][q] = 0.f; }
        }
    }
    tile_softmax<4>(p);
}
// the weights the aggregate multiplies with: softmax * gate, dropout applied
__device__ __forceinline__ f32x16 agg_kb_dropped(const float (&p)[16], const float (&gate)[16], const TriDrop& drop, uint32_t unit,
                                                 int i, int kt, int hi) {
    f32x16 w;
#pragma unroll
    for (int q = 0; q < 16; ++q) w[q] = p[q] * gate[q];
    if (drop.on) {
        const uint32_t keep = tri_drop_bits(drop, unit, i, kt, hi, kTriDropStrideKb);
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = (keep >> q) & 1u ? w[q] * drop.scale : 0.f;
    }
    return w;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int HG, typename... GS>
__global__ void __launch_bounds__(HG * 64) tri_agg_kb_fwd_kernel(const tgt_triplet_aggregate_args a, const uint64_t* seed_ctr, GS... gs) {
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    // two LDS sets {V (128 rows) | O (32)}: set j&1 is computed on while slab j+1 lands in the other one -> ONE barrier per j
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kSet = 5 * G::kSlabBytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<HG, true>(a, wave);
    const int N = c.N, i0 = 32 * c.tile;
    // a graph DropPath dropped (triplet_common.hpp, agg_dead): zeros to the O rows i0..i0+31 of this head group for every j
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        slab_zero_units<G>(0, N, i0, N, tid, agg_o_slab<T, 16, HG>(a.out, a.ld_out, a.o_off[c.dir], c));
        return;
    }
    F ident_d[1];
    make_ident_d<T, 1>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit = (uint32_t)((c.b * 2 + c.dir) * a.H + c.h);
    const SlabBuf bV = agg_v_slab<T, 16, HG>(a.v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
    const SlabBuf bO = agg_o_slab<T, 16, HG>(a.out, a.ld_out, a.o_off[c.dir], c);

    F pa[4][2];
    {
        float p[4][16], gate[4][16];
        agg_kb_softmax<T, HG, false>(c, wave, tid, r, hi, i0, smem, p, gate);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const f32x16 w = agg_kb_dropped(p[kt], gate[kt], drop, drop_unit, i0 + r, kt, hi);
            pa[kt][0] = pack_chunk<T>(w, 0);
            pa[kt][1] = pack_chunk<T>(w, 1);
        }
    }
    uint4 pv[SlabIO<G, 128>::kIters];
    slab_issue<G, 128>(pv, bV, 0, 0, N, tid);
    slab_commit<G, 128>(pv, smem, tid);
    slab_issue<G, 128>(pv, bV, 1, 0, N, tid);           // (N > 64)
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        char* sV = smem + (j & 1) * kSet;
        char* sOut = sV + 4 * G::kSlabBytes;
        if (j + 1 < N) slab_commit<G, 128>(pv, smem + ((j + 1) & 1) * kSet, tid);
        if (j + 2 < N) slab_issue<G, 128>(pv, bV, j + 2, 0, N, tid);
        f32x16 o = {0};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (32 * kt < N) {
                F fv[1];
                read_frags<T, 16, HG>(fv, sV, wave, 32 * kt + r, hi);
                f32x16 vt = {0};
                vt = mma32(fv[0], ident_d[0], vt);          // V[k][d] -> lane d
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) o = mma32(pack_chunk<T>(vt, cc), pa[kt][cc], o);     // O^T[d][i]
            }
        }
        write_rows<T, 16, HG>(sOut, o, wave, r, hi);
        __syncthreads();
        slab_store<G, 32>(sOut, bO, j, i0, N, tid);
    }
}

// ---------------------------------------------------------------------------
// backward, A sweep: dE / dG of (query tile, all keys)
// ---------------------------------------------------------------------------
template <typename T, int HG, typename... GS>
__global__ void __launch_bounds__(HG * 64) tri_agg_kb_bwd_a_kernel(const tgt_triplet_aggregate_args a, const uint64_t* seed_ctr, GS... gs) {
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kSet = 5 * G::kSlabBytes;               // {dO (32 rows) | V (128)}, two sets (see forward)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<HG, true>(a, wave);
    const int N = c.N, i0 = 32 * c.tile;
    // a graph DropPath dropped: d_out is not read, zeros to the d_eg rows of this query tile, key tile by key tile through the
    // stage as the live store below
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        for (int kt = 0; 32 * kt < N; ++kt)
            arm_stage_zero_grad<T, HG, 1>(c.ta, a.d_eg[c.dir], c.b, c.dir, c.g, N, i0, smem, wave, tid, r, hi, 32 * kt);
        return;
    }
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit = (uint32_t)((c.b * 2 + c.dir) * a.H + c.h);
    const SlabBuf bV = agg_v_slab<T, 16, HG>(a.v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
    const SlabBuf dO = agg_o_slab<T, 16, HG>(a.d_out, a.ld_out, a.o_off[c.dir], c);

    f32x16 dacc[4];           // dA^T[k][i], summed over j
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) dacc[kt][q] = 0.f;

    uint4 pv[SlabIO<G, 128>::kIters], po[SlabIO<G, 32>::kIters];
    slab_issue<G, 32>(po, dO, 0, i0, N, tid);
    slab_issue<G, 128>(pv, bV, 0, 0, N, tid);
    slab_commit<G, 32>(po, smem, tid);
    slab_commit<G, 128>(pv, smem + G::kSlabBytes, tid);
    slab_issue<G, 32>(po, dO, 1, i0, N, tid);
    slab_issue<G, 128>(pv, bV, 1, 0, N, tid);
    __syncthreads();
    for (int j = 0; j < N; ++j) {
        char* sO = smem + (j & 1) * kSet;
        char* sV = sO + G::kSlabBytes;
        if (j + 1 < N) {
            char* nO = smem + ((j + 1) & 1) * kSet;
            slab_commit<G, 32>(po, nO, tid);
            slab_commit<G, 128>(pv, nO + G::kSlabBytes, tid);
        }
        if (j + 2 < N) {
            slab_issue<G, 32>(po, dO, j + 2, i0, N, tid);
            slab_issue<G, 128>(pv, bV, j + 2, 0, N, tid);
        }
        F fo[1];
        read_frags<T, 16, HG>(fo, sO, wave, r, hi);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (32 * kt < N) {
                F fv[1];
                read_frags<T, 16, HG>(fv, sV, wave, 32 * kt + r, hi);
                dacc[kt] = mma32(fv[0], fo[0], dacc[kt]);
            }
        }
        __syncthreads();
    }
    // (the barrier that ended the walk: the stage below aliases both sets)

    // dropout, gate and softmax backward on the accumulated dA (recompute P, g)
    float p[4][16], gate[4][16];
    agg_kb_softmax<T, HG, true>(c, wave, tid, r, hi, i0, smem, p, gate);
    if (drop.on) {            // dacc is the gradient of the DROPPED weights
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const uint32_t keep = tri_drop_bits(drop, drop_unit, i0 + r, kt, hi, kTriDropStrideKb);
#pragma unroll
            for (int q = 0; q < 16; ++q) dacc[kt][q] = (keep >> q) & 1u ? dacc[kt][q] * drop.scale : 0.f;
        }
    }
    float delta = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) delta += p[kt][q] * (dacc[kt][q] * gate[kt][q]);
    delta += xhalf(delta);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (32 * kt < N) {
            float dE[16], dG[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                dG[q] = dacc[kt][q] * p[kt][q] * gate[kt][q] * (1.f - gate[kt][q]);
                dE[q] = p[kt][q] * (dacc[kt][q] * gate[kt][q] - delta);
            }
            arm_stage_put_grad<T, HG, 1>(smem, c.dir, wave, r, hi, 0, dE, dG);
            __syncthreads();
            arm_stage_store_grad<T, HG, 1>(c.ta, a.d_eg[c.dir], c.b, c.dir, c.g, N, i0, smem, tid, 32 * kt);
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------
// backward, V sweep: dV of 32 consecutive j, summed over all query tiles in registers.  KT = key tiles a workgroup owns
// (blockIdx.y picks which): 4 = all of them for the 16-bit types; fp32 fragments are twice the size and sixteen weight
// tiles of them spill, so fp32 takes 2 and twice the workgroups.
// ---------------------------------------------------------------------------
template <typename T, int HG, int KT, typename... GS>
__global__ void __launch_bounds__(HG * 64, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) tri_agg_kb_bwd_v_kernel(const tgt_triplet_aggregate_args a, const uint64_t* seed_ctr, GS... gs) {
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kSet = 4 * G::kSlabBytes;               // {dO (128 rows i), overwritten in place by dV (128 rows k)}, two sets
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const AggCtx c = agg_ctx<HG, true>(a, wave);
    const int N = c.N, j0 = 32 * c.tile, j1 = j0 + 32 < N ? j0 + 32 : N;
    const int kpart = blockIdx.y;                         // owns key tiles [KT*kpart, KT*kpart + KT)
    if (32 * KT * kpart >= N) return;                     // (the whole workgroup, before any barrier)
    // a graph DropPath dropped: d_out is not read, zeros to the rows the store below owns -- the keys of `kpart` of its 32 j
    if constexpr (sizeof...(GS) > 0) if (agg_dead(c.b, gs...)) {
        const SlabBuf zV = agg_v_slab<T, 16, HG>(a.d_v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);
        for (int j = j0; j < j1; ++j) slab_store_zero<G, 32 * KT>(zV, j, 32 * KT * kpart, N, tid);
        return;
    }
    F ident_d[1];
    make_ident_d<T, 1>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit = (uint32_t)((c.b * 2 + c.dir) * a.H + c.h);
    const SlabBuf dV = agg_v_slab<T, 16, HG>(a.d_v[c.dir], a.ld_v[c.dir], a.v_off[c.dir], c);      // d_v mirrors v
    const SlabBuf dO = agg_o_slab<T, 16, HG>(a.d_out, a.ld_out, a.o_off[c.dir], c);

    // the weights of every (query tile it, owned key tile kt) in (lane = k, registers = i) layout, as operand fragments over i
    F a2f[4][KT][2];
    {
        F ident_k[2];
        make_ident_k<T>(ident_k, r, hi);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (32 * it < N) {
                float p[4][16], gate[4][16];
                agg_kb_softmax<T, HG, true>(c, wave, tid, r, hi, 32 * it, smem, p, gate);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    if (kt / KT == kpart) {               // (kt is a constant here: the register index stays static)
                        const f32x16 w = agg_kb_dropped(p[kt], gate[kt], drop, drop_unit, 32 * it + r, kt, hi);
                        f32x16 a2 = {0};
#pragma unroll
                        for (int cc = 0; cc < 2; ++cc) a2 = mma32(pack_chunk<T>(w, cc), ident_k[cc], a2);
                        a2f[it][kt % KT][0] = pack_chunk<T>(a2, 0);
                        a2f[it][kt % KT][1] = pack_chunk<T>(a2, 1);
                    }
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < KT; ++kk) a2f[it][kk][0] = a2f[it][kk][1] = zero_frag<T>();
            }
        }
    }

    uint4 po[SlabIO<G, 128>::kIters];
    slab_issue<G, 128>(po, dO, j0, 0, N, tid);
    slab_commit<G, 128>(po, smem + (j0 & 1) * kSet, tid);
    if (j0 + 1 < j1) slab_issue<G, 128>(po, dO, j0 + 1, 0, N, tid);
    __syncthreads();
    for (int j = j0; j < j1; ++j) {
        char* sO = smem + (j & 1) * kSet;
        // (set (j+1)&1 was last read by the store of j-1: by the thread that overwrites the same chunks here -- same chunk map)
        if (j + 1 < j1) slab_commit<G, 128>(po, smem + ((j + 1) & 1) * kSet, tid);
        if (j + 2 < j1) slab_issue<G, 128>(po, dO, j + 2, 0, N, tid);
        F oTf[4][2];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (32 * it < N) {
                F fo[1];
                read_frags<T, 16, HG>(fo, sO, wave, 32 * it + r, hi);
                f32x16 t2 = {0};
                t2 = mma32(fo[0], ident_d[0], t2);          // dO^T
                oTf[it][0] = pack_chunk<T>(t2, 0);
                oTf[it][1] = pack_chunk<T>(t2, 1);
            } else {
                oTf[it][0] = oTf[it][1] = zero_frag<T>();
            }
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt / KT == kpart && 32 * kt < N) {
                f32x16 dv = {0};
#pragma unroll
                for (int it = 0; it < 4; ++it)
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) dv = mma32(oTf[it][cc], a2f[it][kt % KT][cc], dv);      // dV^T[d][k], all i
                // (in place: this wave reads only its own columns, and has read every row of them above)
                write_rows<T, 16, HG>(sO, dv, wave, 32 * kt + r, hi);
            }
        }
        __syncthreads();
        // the owned rows, by the chunk map of the 128-row commit (slab_store<G, 128> restricted to them)
        const uint32_t so = dV.chan + (uint32_t)j * dV.j_stride;
#pragma unroll
        for (int it = 0; it < SlabIO<G, 128>::kIters; ++it) {
            const int ch = it * G::kThreads + tid;
            const int row = ch / G::kSlots, slot = ch % G::kSlots;
            if (row / (32 * KT) == kpart && row < N)
                buf_store16(dV, *reinterpret_cast<const uint4*>(sO + G::lds_off(row, slot)), (uint32_t)row * dV.row_stride + (uint32_t)slot * 16u, so);
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <typename T, int HG, typename... GS>
static int launch_agg_kb(const tgt_triplet_aggregate_args& a, bool bwd, hipStream_t st, GS... gs) {
    using G = TriGeo<T, 16, HG>;
    const int grid = a.B * 2 * (a.H / HG) * ((a.N + 31) / 32);
    constexpr int kArm = ArmStage<T, HG, 1>::kBytes;
    constexpr int kWalkLds = cmax(10 * G::kSlabBytes, kArm), kVLds = cmax(8 * G::kSlabBytes, kArm);
    static_assert(kWalkLds <= 160 * 1024 && kVLds <= 160 * 1024, "LDS of a CU");
    if (!bwd) return launch_lds<tri_agg_kb_fwd_kernel<T, HG, GS...>>("tri_agg_kb_fwd_kernel", dim3(grid), dim3(G::kThreads), kWalkLds, st, a, seed_counter(), gs...);
    constexpr int KT = sizeof(T) == 2 ? 4 : 2;
    // (both reservations before the first launch: a failed one leaves nothing half-written)
    if (int rc = reserve_lds<tri_agg_kb_bwd_a_kernel<T, HG, GS...>>("tri_agg_kb_bwd_a_kernel", kWalkLds)) return rc;
    if (int rc = reserve_lds<tri_agg_kb_bwd_v_kernel<T, HG, KT, GS...>>("tri_agg_kb_bwd_v_kernel", kVLds)) return rc;
    if (int rc = launch_lds<tri_agg_kb_bwd_a_kernel<T, HG, GS...>>("tri_agg_kb_bwd_a_kernel", dim3(grid), dim3(G::kThreads), kWalkLds, st, a, seed_counter(), gs...)) return rc;
    return launch_lds<tri_agg_kb_bwd_v_kernel<T, HG, KT, GS...>>("tri_agg_kb_bwd_v_kernel", dim3(grid, 4 / KT), dim3(G::kThreads), kVLds, st, a, seed_counter(), gs...);
}
// graph_scale NULL: the kernels' instantiations without the argument (triplet_common.hpp, agg_dead)
template <typename T>
static int dispatch_agg_kb(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) {
    if (graph_scale) return a.H % 4 == 0 ? launch_agg_kb<T, 4>(a, bwd, st, graph_scale) : launch_agg_kb<T, 1>(a, bwd, st, graph_scale);
    if (a.H % 4 == 0) return launch_agg_kb<T, 4>(a, bwd, st);
    return launch_agg_kb<T, 1>(a, bwd, st);
}

// one dtype per translation unit in the build, as triplet_attention_kb.hip (TGT_AGGKB_INST: bit 0 fp32, bit 1 bf16, bit 2 fp16,
// bit 3 the dispatch)
#ifndef TGT_AGGKB_INST
#define TGT_AGGKB_INST 15
#endif
int tri_agg_kb_run_f32(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st);
int tri_agg_kb_run_bf16(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st);
int tri_agg_kb_run_f16(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st);
#if TGT_AGGKB_INST & 1
int tri_agg_kb_run_f32(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) { return dispatch_agg_kb<float>(a, graph_scale, bwd, st); }
#endif
#if TGT_AGGKB_INST & 2
int tri_agg_kb_run_bf16(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) { return dispatch_agg_kb<bf16_t>(a, graph_scale, bwd, st); }
#endif
#if TGT_AGGKB_INST & 4
int tri_agg_kb_run_f16(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) { return dispatch_agg_kb<f16_t>(a, graph_scale, bwd, st); }
#endif

#if TGT_AGGKB_INST & 8
// 65 <= N <= 128, D = 16, arguments already validated by triplet_aggregate_run
int tri_agg_kb_run(const tgt_triplet_aggregate_args& a, const float* graph_scale, bool bwd, hipStream_t st) {
    switch (a.dtype) {
        case TGT_F32: return tri_agg_kb_run_f32(a, graph_scale, bwd, st);
        case TGT_BF16: return tri_agg_kb_run_bf16(a, graph_scale, bwd, st);
        case TGT_F16: return tri_agg_kb_run_f16(a, graph_scale, bwd, st);
        default: return set_error(TGT_ERR_INVALID, "triplet aggregate: bad dtype %d", a.dtype);
    }
}
#endif

}  // namespace tgt
