// Triplet attention core for 65 <= N <= 128 (D = 16): key-blocked kernels for gfx950.
//
// Same arithmetic, operand layouts and matrix-core mapping as triplet_attention.hip (read its header first); what changes
// is what a workgroup owns.  The generic kernel keeps the (i,k) third-arm tile of ALL key tiles and, in the backward, the
// dE / dG accumulators AND the dK / dV partial sums of one query tile in registers -- that does not fit four key tiles.
// Here:
//   forward   workgroup = (graph, direction, head group, query tile of 32); walks j; the key axis goes by in blocks of 32
//             with a running max / sum and rescaled O accumulators (online softmax).  (B,N,N,N,H) is never written.
//   backward  three sweeps over the same data, no floating-point atomics, every sum in a fixed order:
//     E sweep  owns a query tile, walks j, loops the key blocks twice per j: pass 1 = softmax statistics (row max, 1 / row
//              sum) and delta = sum_k P dP by the same online recurrence; pass 2 = dS -> dE / dG of its (query tile, all
//              keys) summed over j in registers (256 of them: the reason dQ is not produced here as well -- together they
//              spill).  It leaves (max, 1/sum, delta) per (b, dir, h, j, i) in the caller's workspace.  The row maximum
//              and the sum are stored SEPARATELY: next to a finfo.min-sized maximum (a fully masked row) a log-sum-exp
//              would absorb log(sum) and lose the uniform softmax.
//     Q sweep  owns a query tile, walks j, loops the key blocks with those statistics: dQ (sum over k).
//     K sweep  owns a key tile, walks j, loops the query tiles with those statistics: dK, dV (sum over i).
//              S is produced directly as S[i][k] (lane = k), so no re-layout through the identity is needed.
//   workspace layout: float [B][2][H][N (j)][3 (max, 1/sum, delta)][Np (i)], Np = N rounded up to 32.
// Dropout: word index (i*128 + k) >> 1 inside a unit (triplet_common.hpp).  In-kernel column sums are not provided here.
//
// Ragged batches (TGT_TRI_COUNTS_KB with node counts, tgt_hip.h): every kernel has a second instantiation that takes the per-graph
// counts as a trailing argument (`NC... nc`, RG = true: triplet_common.hpp, tri_node_count; without it the pack is empty and the
// kernel is the one it was before the counts existed).  With n = clamp(node_counts[b], 0, N) and n32 = n rounded up to 32 it
// bounds all three axes of the work:
//   owned tile   a workgroup whose tile starts at or past n32 (query tile i0; K sweep: key tile k0) holds padded nodes only: it
//                writes the zeros a dropped graph gets and returns;
//   walk         j ends at n (the register prefetch of j + 1 too); the rows of the units n..N-1 get zeros, in the backward ahead
//                of the walk;
//   inner tiles  key blocks (forward, E sweep, Q sweep) / query tiles (K sweep) at or past n32 are neither loaded nor computed:
//                their third-arm tiles take the -inf / 0 of blocks past N and the 128-row slabs are loaded up to min(n32, N).
// Why skipping a key block keeps the bits of a real query row (i < n; the mask closes every key k >= n and opens at least one
// k < n): every logit of the block is finfo.min, so its maximum cannot raise the running maximum; alpha = exp(m - m) = exp(0)
// is exactly 1; every exp(finfo.min - m) underflows to exactly 0; the row sum gains 0 and the matrix-core product adds
// 0 * V (finite) = 0 to O.  The backward is the same argument on P = 0: dS = P (...) = 0, so dE, dG, dQ, dK gain zeros, and dV
// gains dO^T A with A = P gate = 0.  A skipped QUERY tile (K sweep) has d_out = 0 (the contract) and delta = 0, so dS = 0 and
// dV gains 0 * A.  Rows n <= i < n32 of a computed tile see fewer keys than without counts (finite, different) and, with their
// zero d_out, contribute zeros either way.  N keeps every stride, row bound, Np and dropout index; the E sweep writes and the
// other two sweeps read the statistics of (j < n, i < n32) only.
#include "triplet_common.hpp"

namespace tgt {

__device__ __forceinline__ float* kb_stats(const tgt_triplet_attention_args& a, int b, int dir, int h, int j, int Np) {
    return reinterpret_cast<float*>(a.workspace) + ((((int64_t)b * 2 + dir) * a.H + h) * a.N + j) * 3 * Np;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int HG, bool PF, typename... NC>
__global__ void __launch_bounds__(HG * 64, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) tri_kb_fwd_kernel(const tgt_triplet_attention_args a, const uint64_t* seed_ctr, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;          // ragged: launched with the node counts as a trailing argument (triplet_common.hpp)
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem;                              // {Q (32 rows) | K (128) | V (128)}
    char* sK = sQ + G::kSlabBytes;
    char* sV = sK + 4 * G::kSlabBytes;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const TriCtx c = tri_ctx<T, 16, HG, true>(a, wave);
    const int N = c.N, i0 = 32 * c.tile;
    const ThirdArm ta = tri_third_arm(a, c.dir);
    F ident_d[1];
    make_ident_d<T, 1>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit0 = (uint32_t)(((c.b * 2 + c.dir) * a.H + c.h) * N);

    const int64_t sz = sizeof(T), Nl = N;
    const uint32_t hch = (uint32_t)(c.g * HG * 16 * sz), lds_ = (uint32_t)(a.ld_qkv[c.dir] * sz), ldo_ = (uint32_t)(a.ld_out * sz);
    const __amdgpu_buffer_rsrc_t r_src = graph_rsrc(a.qkv[c.dir], Nl * Nl * a.ld_qkv[c.dir] * sz, c.b);
    const SlabBuf bQ = {r_src, (uint32_t)(a.q_off[c.dir] * sz) + hch, (uint32_t)N * lds_, lds_};
    const SlabBuf bK = {r_src, (uint32_t)(a.k_off[c.dir] * sz) + hch, c.dir == 0 ? lds_ : (uint32_t)N * lds_,
                        c.dir == 0 ? (uint32_t)N * lds_ : lds_};
    const SlabBuf bV = {r_src, (uint32_t)(a.v_off[c.dir] * sz) + hch, bK.row_stride, bK.j_stride};
    const SlabBuf bO = {graph_rsrc(a.out, Nl * Nl * a.ld_out * sz, c.b), (uint32_t)(a.o_off[c.dir] * sz) + hch, (uint32_t)N * ldo_, ldo_};

    // n real nodes (RG; else N): key blocks at or past nkb are skipped, the 128-row slabs are loaded up to row nrow
    const int n = tri_node_count<RG>(tri_counts_ptr(nc...), c.b, N);
    const int nkb = RG ? tri_count32(n) : N, nrow = RG ? min(nkb, N) : N;
    if ((RG && i0 >= nkb) || (a.graph_scale && a.graph_scale[c.b] == 0.f)) {          // DropPath-dropped graph / query tile of padded nodes: zero rows, nothing read
        slab_zero_units<G>(0, N, i0, N, tid, bO);
        return;
    }

    float biasM[4][16], gate[4][16];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (32 * kt < nkb) {
            load_third_arm<T, false>(ta, c.b, c.dir, c.h, N, r, hi, biasM[kt], gate[kt], i0, 32 * kt);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) { biasM[kt][q] = -INFINITY; gate[kt][q] = 0.f; }
        }
    }

    uint4 pq[SlabIO<G, 32>::kIters], pk[SlabIO<G, 128>::kIters], pv[SlabIO<G, 128>::kIters];
    if constexpr (PF) {
        slab_issue<G, 32>(pq, bQ, 0, i0, N, tid);
        slab_issue<G, 128>(pk, bK, 0, 0, nrow, tid);
        slab_issue<G, 128>(pv, bV, 0, 0, nrow, tid);
    }
    // one LDS set, two barriers per j: the commit of j+1 follows barrier 2 of j (every wave is done reading K / V);
    // the O rows in sQ are stored by the thread that overwrites the same chunk next (same chunk map)
    for (int j = 0; j < n; ++j) {
        if constexpr (!PF) {
            slab_issue<G, 32>(pq, bQ, j, i0, N, tid);
            slab_issue<G, 128>(pk, bK, j, 0, nrow, tid);
            slab_issue<G, 128>(pv, bV, j, 0, nrow, tid);
        }
        slab_commit<G, 32>(pq, sQ, tid);
        slab_commit<G, 128>(pk, sK, tid);
        slab_commit<G, 128>(pv, sV, tid);
        if constexpr (PF) {
            if (j + 1 < n) {
                slab_issue<G, 32>(pq, bQ, j + 1, i0, N, tid);
                slab_issue<G, 128>(pk, bK, j + 1, 0, nrow, tid);
                slab_issue<G, 128>(pv, bV, j + 1, 0, nrow, tid);
            }
        }
        __syncthreads();

        F fq[1];
        read_frags<T, 16, HG>(fq, sQ, wave, r, hi);
        float m = -INFINITY, l = 0.f;
        f32x16 o = {0};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (32 * kt < nkb) {
                F fk[1], fv[1];
                read_frags<T, 16, HG>(fk, sK, wave, 32 * kt + r, hi);
                read_frags<T, 16, HG>(fv, sV, wave, 32 * kt + r, hi);
                f32x16 s = {0}, vt = {0};
                s = mma32(fk[0], fq[0], s);                 // S^T[k][i]
                vt = mma32(fv[0], ident_d[0], vt);          // V[k][d] -> lane d
                float bm = -INFINITY;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    s[q] = s[q] * a.scale + biasM[kt][q];
                    bm = fmaxf(bm, s[q]);
                }
                bm = fmaxf(bm, xhalf(bm));
                // running max: the first block always holds a key < N, whose logit is finite (finfo.min at the least), so
                // mn is finite from block 0 on and exp(m - mn) is exp(-inf) = 0 there; later blocks past N are all -inf
                const float mn = fmaxf(m, bm);
                const float alpha = fast_exp(m - mn);
                float sum = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    s[q] = fast_exp(s[q] - mn);
                    sum += s[q];
                    s[q] *= gate[kt][q];
                }
                l = l * alpha + sum;             // in-lane partial: alpha is the same in both lane halves
                m = mn;
                if (drop.on) {
                    const uint32_t keep = tri_drop_bits(drop, drop_unit0 + j, i0 + r, kt, hi, kTriDropStrideKb);
#pragma unroll
                    for (int q = 0; q < 16; ++q) s[q] = (keep >> q) & 1u ? s[q] * drop.scale : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) o[q] *= alpha;
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) o = mma32(pack_chunk<T>(vt, cc), pack_chunk<T>(s, cc), o);      // O^T[d][i]
            }
        }
        l += xhalf(l);
        const float inv = fast_rcp(l);
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] *= inv;
        write_rows<T, 16, HG>(sQ, o, wave, r, hi);
        __syncthreads();
        slab_store<G, 32>(sQ, bO, j, i0, N, tid);
    }
    if constexpr (RG) slab_zero_units<G>(n, N, i0, N, tid, bO);          // the padded units of a ragged batch
}

// ---------------------------------------------------------------------------
// backward, E sweep (EG = true): statistics, dE / dG;  Q sweep (EG = false): dQ from the E sweep's statistics
// ---------------------------------------------------------------------------
template <typename T, int HG, bool PF, bool EG, typename... NC>
__global__ void __launch_bounds__(HG * 64, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) tri_kb_bwd_q_kernel(const tgt_triplet_attention_args a, const uint64_t* seed_ctr, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;          // ragged: as tri_kb_fwd_kernel
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem;                              // {Q | dO (32 rows each) | K (128) | V (128)}
    char* sO = sQ + G::kSlabBytes;
    char* sK = sO + G::kSlabBytes;
    char* sV = sK + 4 * G::kSlabBytes;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const TriCtx c = tri_ctx<T, 16, HG, true>(a, wave);
    const int N = c.N, i0 = 32 * c.tile, Np = (N + 31) & ~31;
    const ThirdArm ta = tri_third_arm(a, c.dir);
    F ident_d[1];
    make_ident_d<T, 1>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit0 = (uint32_t)(((c.b * 2 + c.dir) * a.H + c.h) * N);

    const int64_t sz = sizeof(T), Nl = N;
    const int64_t ldq = a.ld_dqkv[c.dir] ? a.ld_dqkv[c.dir] : a.ld_qkv[c.dir];
    const int64_t lde = a.ld_deg[c.dir] ? a.ld_deg[c.dir] : a.ld_eg[c.dir];
    const uint32_t hch = (uint32_t)(c.g * HG * 16 * sz);
    const uint32_t lds_ = (uint32_t)(a.ld_qkv[c.dir] * sz), ldg_ = (uint32_t)(ldq * sz), ldo_ = (uint32_t)(a.ld_out * sz);
    const __amdgpu_buffer_rsrc_t r_src = graph_rsrc(a.qkv[c.dir], Nl * Nl * a.ld_qkv[c.dir] * sz, c.b);
    const __amdgpu_buffer_rsrc_t r_grd = graph_rsrc(a.d_qkv[c.dir], Nl * Nl * ldq * sz, c.b);
    const __amdgpu_buffer_rsrc_t r_do = graph_rsrc(a.d_out, Nl * Nl * a.ld_out * sz, c.b);
    const uint32_t qo = (uint32_t)(a.q_off[c.dir] * sz) + hch, ko = (uint32_t)(a.k_off[c.dir] * sz) + hch,
                   vo = (uint32_t)(a.v_off[c.dir] * sz) + hch;
    const SlabBuf bQ = {r_src, qo, (uint32_t)N * lds_, lds_};
    const SlabBuf bK = {r_src, ko, c.dir == 0 ? lds_ : (uint32_t)N * lds_, c.dir == 0 ? (uint32_t)N * lds_ : lds_};
    const SlabBuf bV = {r_src, vo, bK.row_stride, bK.j_stride};
    const SlabBuf dO = {r_do, (uint32_t)(a.o_off[c.dir] * sz) + hch, (uint32_t)N * ldo_, ldo_};
    const SlabBuf gQ = {r_grd, qo, (uint32_t)N * ldg_, ldg_};
    ThirdArm dta = ta;
    dta.ld = lde;

    float dE[EG ? 4 : 1][16], dG[EG ? 4 : 1][16];
#pragma unroll
    for (int kt = 0; kt < (EG ? 4 : 1); ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) dE[kt][q] = dG[kt][q] = 0.f;

    const int n = tri_node_count<RG>(tri_counts_ptr(nc...), c.b, N);
    const int nkb = RG ? tri_count32(n) : N, nrow = RG ? min(nkb, N) : N;
    if ((RG && i0 >= nkb) || (a.graph_scale && a.graph_scale[c.b] == 0.f)) {          // dropped graph / query tile of padded nodes: zero gradient rows, nothing read
        if constexpr (EG) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
                if (32 * kt < N) store_third_arm_grad<T>(dta, a.d_eg[c.dir], c.b, c.dir, c.h, N, r, hi, dE[kt], dG[kt], i0, 32 * kt);
        } else {
            slab_zero_units<G>(0, N, i0, N, tid, gQ);
        }
        return;
    }
    // the padded units of a ragged batch, ahead of the walk (its stores go to other rows)
    if constexpr (RG && !EG) slab_zero_units<G>(n, N, i0, N, tid, gQ);

    float biasM[4][16], gate[4][16];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (32 * kt < nkb) {
            load_third_arm<T, true>(ta, c.b, c.dir, c.h, N, r, hi, biasM[kt], gate[kt], i0, 32 * kt);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) { biasM[kt][q] = -INFINITY; gate[kt][q] = 0.f; }
        }
    }

    uint4 pq[SlabIO<G, 32>::kIters], po[SlabIO<G, 32>::kIters], pk[SlabIO<G, 128>::kIters], pv[SlabIO<G, 128>::kIters];
    if constexpr (PF) {
        slab_issue<G, 32>(pq, bQ, 0, i0, N, tid);
        slab_issue<G, 32>(po, dO, 0, i0, N, tid);
        slab_issue<G, 128>(pk, bK, 0, 0, nrow, tid);
        slab_issue<G, 128>(pv, bV, 0, 0, nrow, tid);
    }
    for (int j = 0; j < n; ++j) {
        if constexpr (!PF) {
            slab_issue<G, 32>(pq, bQ, j, i0, N, tid);
            slab_issue<G, 32>(po, dO, j, i0, N, tid);
            slab_issue<G, 128>(pk, bK, j, 0, nrow, tid);
            slab_issue<G, 128>(pv, bV, j, 0, nrow, tid);
        }
        slab_commit<G, 32>(pq, sQ, tid);
        slab_commit<G, 32>(po, sO, tid);
        slab_commit<G, 128>(pk, sK, tid);
        slab_commit<G, 128>(pv, sV, tid);
        if constexpr (PF) {
            if (j + 1 < n) {
                slab_issue<G, 32>(pq, bQ, j + 1, i0, N, tid);
                slab_issue<G, 32>(po, dO, j + 1, i0, N, tid);
                slab_issue<G, 128>(pk, bK, j + 1, 0, nrow, tid);
                slab_issue<G, 128>(pv, bV, j + 1, 0, nrow, tid);
            }
        }
        __syncthreads();

        F fq[1], fo[1];
        read_frags<T, 16, HG>(fq, sQ, wave, r, hi);
        read_frags<T, 16, HG>(fo, sO, wave, r, hi);
        // pass 1: row max m, row sum l and dl = sum_k exp(s - m) dP, all by the online recurrence
        float m = -INFINITY, l = 0.f, dl = 0.f;
        float ms, inv, delta;
        if constexpr (EG) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (32 * kt < nkb) {
                F fk[1], fv[1];
                read_frags<T, 16, HG>(fk, sK, wave, 32 * kt + r, hi);
                read_frags<T, 16, HG>(fv, sV, wave, 32 * kt + r, hi);
                f32x16 s = {0}, da = {0};
                s = mma32(fk[0], fq[0], s);                 // S^T[k][i]
                da = mma32(fv[0], fo[0], da);               // dA^T[k][i]
                float bm = -INFINITY;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    s[q] = s[q] * a.scale + biasM[kt][q];
                    bm = fmaxf(bm, s[q]);
                }
                bm = fmaxf(bm, xhalf(bm));
                const float mn = fmaxf(m, bm);
                const float ms = mn == -INFINITY ? 0.f : mn;        // padding column (i >= N): every weight is exactly 0
                const float alpha = fast_exp(m - ms);
                uint32_t keep = 0xffffu;
                if (drop.on) keep = tri_drop_bits(drop, drop_unit0 + j, i0 + r, kt, hi, kTriDropStrideKb);
                float sum = 0.f, dsum = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float e = fast_exp(s[q] - ms);
                    const float dp = (keep >> q) & 1u ? da[q] * gate[kt][q] * drop.scale : 0.f;
                    sum += e;
                    dsum += e * dp;
                }
                l = l * alpha + sum;
                dl = dl * alpha + dsum;
                m = mn;
            }
        }
        l += xhalf(l);
        dl += xhalf(dl);
        ms = m == -INFINITY ? 0.f : m;
        inv = l > 0.f ? fast_rcp(l) : 0.f;
        delta = dl * inv;
        if (hi == 0) {
            float* st = kb_stats(a, c.b, c.dir, c.h, j, Np);
            st[i0 + r] = ms;
            st[Np + i0 + r] = inv;
            st[2 * Np + i0 + r] = delta;
        }
        } else {
            const float* st = kb_stats(a, c.b, c.dir, c.h, j, Np);
            ms = st[i0 + r];
            inv = st[Np + i0 + r];
            delta = st[2 * Np + i0 + r];
        }
        // pass 2: P, dS -> dE, dG (E sweep) or dQ (Q sweep)
        f32x16 dq = {0};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (32 * kt < nkb) {
                F fk[1], fv[1];
                read_frags<T, 16, HG>(fk, sK, wave, 32 * kt + r, hi);
                read_frags<T, 16, HG>(fv, sV, wave, 32 * kt + r, hi);
                f32x16 s = {0}, da = {0};
                s = mma32(fk[0], fq[0], s);
                da = mma32(fv[0], fo[0], da);
                uint32_t keep = 0xffffu;
                if (drop.on) keep = tri_drop_bits(drop, drop_unit0 + j, i0 + r, kt, hi, kTriDropStrideKb);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float p = fast_exp(s[q] * a.scale + biasM[kt][q] - ms) * inv;
                    const float dad = (keep >> q) & 1u ? da[q] * drop.scale : 0.f;      // dA with the dropout mask
                    const float ds = p * (dad * gate[kt][q] - delta);
                    if constexpr (EG) {
                        if (ta.gated) dG[kt][q] += dad * p;        // the gate factor is applied once, after the walk
                        if (ta.biased) dE[kt][q] += ds;
                    }
                    s[q] = ds * a.scale;
                }
                if constexpr (!EG) {
                    f32x16 kT = {0};
                    kT = mma32(fk[0], ident_d[0], kT);          // K[k][d] -> lane d
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) dq = mma32(pack_chunk<T>(kT, cc), pack_chunk<T>(s, cc), dq);    // dQ^T[d][i]
                }
            }
        }
        if constexpr (!EG) write_rows<T, 16, HG>(sQ, dq, wave, r, hi);
        __syncthreads();
        if constexpr (!EG) slab_store<G, 32>(sQ, gQ, j, i0, N, tid);
    }
    if constexpr (EG)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (32 * kt < N) {
            if (ta.gated) {
#pragma unroll
                for (int q = 0; q < 16; ++q) dG[kt][q] *= gate[kt][q] * (1.f - gate[kt][q]);       // d sigmoid
            }
            store_third_arm_grad<T>(dta, a.d_eg[c.dir], c.b, c.dir, c.h, N, r, hi, dE[kt], dG[kt], i0, 32 * kt);
        }
    }
}

// ---------------------------------------------------------------------------
// backward, K sweep: dK, dV.  Lane = key k of the owned tile, register q <-> query i = 32*it + acc_row(q, hi).
// ---------------------------------------------------------------------------
template <typename T, int HG, bool PF, typename... NC>
__global__ void __launch_bounds__(HG * 64, 1) __attribute__((amdgpu_waves_per_eu(1, 1))) tri_kb_bwd_k_kernel(const tgt_triplet_attention_args a, const uint64_t* seed_ctr, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;          // ragged: as tri_kb_fwd_kernel, with the roles of query and key tiles exchanged
    using G = TriGeo<T, 16, HG>;
    using F = frag_t<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sK = smem;                              // {K | V (32 rows each) | Q (128) | dO (128) | statistics}
    char* sV = sK + G::kSlabBytes;
    char* sQ = sV + G::kSlabBytes;
    char* sO = sQ + 4 * G::kSlabBytes;
    float* sS = reinterpret_cast<float*>(sO + 4 * G::kSlabBytes);       // [HG][3][128]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hi = lane >> 5;
    const TriCtx c = tri_ctx<T, 16, HG, true>(a, wave);
    const int N = c.N, k0 = 32 * c.tile, Np = (N + 31) & ~31;
    const ThirdArm ta = tri_third_arm(a, c.dir);
    F ident_d[1];
    make_ident_d<T, 1>(ident_d, r, hi);
    const TriDrop drop = tri_drop(a.dropout_p, a.dropout_seed, seed_ctr);
    const uint32_t drop_unit0 = (uint32_t)(((c.b * 2 + c.dir) * a.H + c.h) * N);

    const int64_t sz = sizeof(T), Nl = N;
    const int64_t ldq = a.ld_dqkv[c.dir] ? a.ld_dqkv[c.dir] : a.ld_qkv[c.dir];
    const uint32_t hch = (uint32_t)(c.g * HG * 16 * sz);
    const uint32_t lds_ = (uint32_t)(a.ld_qkv[c.dir] * sz), ldg_ = (uint32_t)(ldq * sz), ldo_ = (uint32_t)(a.ld_out * sz);
    const __amdgpu_buffer_rsrc_t r_src = graph_rsrc(a.qkv[c.dir], Nl * Nl * a.ld_qkv[c.dir] * sz, c.b);
    const __amdgpu_buffer_rsrc_t r_grd = graph_rsrc(a.d_qkv[c.dir], Nl * Nl * ldq * sz, c.b);
    const __amdgpu_buffer_rsrc_t r_do = graph_rsrc(a.d_out, Nl * Nl * a.ld_out * sz, c.b);
    const uint32_t qo = (uint32_t)(a.q_off[c.dir] * sz) + hch, ko = (uint32_t)(a.k_off[c.dir] * sz) + hch,
                   vo = (uint32_t)(a.v_off[c.dir] * sz) + hch;
    const SlabBuf bQ = {r_src, qo, (uint32_t)N * lds_, lds_};
    const SlabBuf bK = {r_src, ko, c.dir == 0 ? lds_ : (uint32_t)N * lds_, c.dir == 0 ? (uint32_t)N * lds_ : lds_};
    const SlabBuf bV = {r_src, vo, bK.row_stride, bK.j_stride};
    const SlabBuf dO = {r_do, (uint32_t)(a.o_off[c.dir] * sz) + hch, (uint32_t)N * ldo_, ldo_};
    const SlabBuf dK = {r_grd, ko, c.dir == 0 ? ldg_ : (uint32_t)N * ldg_, c.dir == 0 ? (uint32_t)N * ldg_ : ldg_};
    const SlabBuf dV = {r_grd, vo, dK.row_stride, dK.j_stride};

    // n real nodes (RG; else N): query tiles at or past nqt are skipped, the 128-row slabs are loaded up to row nrow
    const int n = tri_node_count<RG>(tri_counts_ptr(nc...), c.b, N);
    const int nqt = RG ? tri_count32(n) : N, nrow = RG ? min(nqt, N) : N;
    if ((RG && k0 >= nqt) || (a.graph_scale && a.graph_scale[c.b] == 0.f)) {          // dropped graph / key tile of padded nodes: zero gradient rows, nothing read
        slab_zero_units<G>(0, N, k0, N, tid, dK, dV);
        return;
    }
    // the padded units of a ragged batch, ahead of the walk (its stores go to other rows)
    if constexpr (RG) slab_zero_units<G>(n, N, k0, N, tid, dK, dV);

    // third-arm tiles with the roles of the two indices exchanged: load_third_arm's "lane" index is the key here and its
    // "register" index the query, which is the other direction's pair order
    float biasT[4][16], gateT[4][16];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        if (32 * it < nqt) {
            load_third_arm<T, true>(ta, c.b, 1 - c.dir, c.h, N, r, hi, biasT[it], gateT[it], k0, 32 * it);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) { biasT[it][q] = -INFINITY; gateT[it][q] = 0.f; }
        }
    }

    uint4 pk[SlabIO<G, 32>::kIters], pv[SlabIO<G, 32>::kIters], pq[SlabIO<G, 128>::kIters], po[SlabIO<G, 128>::kIters];
    if constexpr (PF) {
        slab_issue<G, 32>(pk, bK, 0, k0, N, tid);
        slab_issue<G, 32>(pv, bV, 0, k0, N, tid);
        slab_issue<G, 128>(pq, bQ, 0, 0, nrow, tid);
        slab_issue<G, 128>(po, dO, 0, 0, nrow, tid);
    }
    for (int j = 0; j < n; ++j) {
        if constexpr (!PF) {
            slab_issue<G, 32>(pk, bK, j, k0, N, tid);
            slab_issue<G, 32>(pv, bV, j, k0, N, tid);
            slab_issue<G, 128>(pq, bQ, j, 0, nrow, tid);
            slab_issue<G, 128>(po, dO, j, 0, nrow, tid);
        }
        slab_commit<G, 32>(pk, sK, tid);
        slab_commit<G, 32>(pv, sV, tid);
        slab_commit<G, 128>(pq, sQ, tid);
        slab_commit<G, 128>(po, sO, tid);
        // the E sweep's statistics of (j, every i) for this group's heads; ragged: of the i < nqt it wrote
        if constexpr (RG) {
            // idx = the LDS slot: no division by a run-time count, and no branch around the load (the loads of one step go out
            // back to back).  Slots i >= nqt, which nothing reads, get a copy of entry nqt - 1 -- an entry the E sweep wrote.
            for (int idx = tid; idx < HG * 384; idx += HG * 64) {
                const int hh = idx / 384, t = (idx >> 7) % 3, i = min(idx & 127, nqt - 1);
                sS[idx] = kb_stats(a, c.b, c.dir, c.g * HG + hh, j, Np)[t * Np + i];
            }
        } else {
            for (int idx = tid; idx < HG * 3 * Np; idx += HG * 64) {
                const int hh = idx / (3 * Np), rem = idx - hh * 3 * Np, t = rem / Np, i = rem - t * Np;
                sS[hh * 384 + t * 128 + i] = kb_stats(a, c.b, c.dir, c.g * HG + hh, j, Np)[rem];
            }
        }
        if constexpr (PF) {
            if (j + 1 < n) {
                slab_issue<G, 32>(pk, bK, j + 1, k0, N, tid);
                slab_issue<G, 32>(pv, bV, j + 1, k0, N, tid);
                slab_issue<G, 128>(pq, bQ, j + 1, 0, nrow, tid);
                slab_issue<G, 128>(po, dO, j + 1, 0, nrow, tid);
            }
        }
        __syncthreads();

        F fk[1], fv[1];
        read_frags<T, 16, HG>(fk, sK, wave, r, hi);
        read_frags<T, 16, HG>(fv, sV, wave, r, hi);
        const float* st = sS + wave * 384;
        f32x16 dk = {0}, dv = {0};
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (32 * it < nqt) {
                F fq[1], fo[1];
                read_frags<T, 16, HG>(fq, sQ, wave, 32 * it + r, hi);
                read_frags<T, 16, HG>(fo, sO, wave, 32 * it + r, hi);
                f32x16 s = {0}, da = {0}, qT = {0}, oT = {0};
                s = mma32(fq[0], fk[0], s);                 // S[i][k]
                da = mma32(fo[0], fv[0], da);               // dA[i][k]
                qT = mma32(fq[0], ident_d[0], qT);          // Q[i][d] -> lane d
                oT = mma32(fo[0], ident_d[0], oT);          // dO[i][d] -> lane d
                uint32_t keep = 0xffffu;
                if (drop.on) keep = tri_drop_bits_t(drop, drop_unit0 + j, 32 * it, k0 + r, hi);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int ib = 32 * it + 8 * g4 + 4 * hi;          // acc_row(4*g4 + t, hi) = 8*g4 + 4*hi + t
                    const float4 mm = *reinterpret_cast<const float4*>(st + ib);
                    const float4 iv = *reinterpret_cast<const float4*>(st + 128 + ib);
                    const float4 dl = *reinterpret_cast<const float4*>(st + 256 + ib);
                    const float m4[4] = {mm.x, mm.y, mm.z, mm.w}, i4[4] = {iv.x, iv.y, iv.z, iv.w}, d4[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int q = 4 * g4 + t;
                        const float p = fast_exp(s[q] * a.scale + biasT[it][q] - m4[t]) * i4[t];
                        const float kd = (keep >> q) & 1u ? drop.scale : 0.f;
                        const float gd = gateT[it][q] * kd;            // gate with the dropout mask
                        s[q] = p * (da[q] * gd - d4[t]) * a.scale;      // dS * scale
                        da[q] = p * gd;                                 // A
                    }
                }
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    dk = mma32(pack_chunk<T>(qT, cc), pack_chunk<T>(s, cc), dk);       // dK^T[d][k] = sum_i Q^T[d][i] dS[i][k]
                    dv = mma32(pack_chunk<T>(oT, cc), pack_chunk<T>(da, cc), dv);      // dV^T[d][k] = sum_i dO^T[d][i] A[i][k]
                }
            }
        }
        write_rows<T, 16, HG>(sK, dk, wave, r, hi);
        write_rows<T, 16, HG>(sV, dv, wave, r, hi);
        __syncthreads();
        slab_store<G, 32>(sK, dK, j, k0, N, tid);
        slab_store<G, 32>(sV, dV, j, k0, N, tid);
        // (the statistics of j+1 are written before the next barrier 1 by other threads than those that read them above:
        //  every wave is past barrier 2, i.e. done reading them)
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// nc: the node counts of a call with TGT_TRI_COUNTS_KB (a trailing kernel argument: the RG instantiations), or nothing
template <typename T, int HG, typename... NC>
static int launch_kb(const tgt_triplet_attention_args& a, bool bwd, hipStream_t st, NC... nc) {
    using G = TriGeo<T, 16, HG>;
    // register prefetch of slab j+1 under the math of j where the register file has room for it (16-bit); fp32 loads in place
    constexpr bool kPF = sizeof(T) == 2;
    const int grid = a.B * 2 * (a.H / HG) * ((a.N + 31) / 32);
    constexpr int kFwdLds = 9 * G::kSlabBytes, kBwdQLds = 10 * G::kSlabBytes, kBwdKLds = 10 * G::kSlabBytes + HG * 384 * 4;
    const dim3 blocks(grid), threads(G::kThreads);
    if (!bwd) return launch_lds<tri_kb_fwd_kernel<T, HG, kPF, NC...>>("tri_kb_fwd_kernel", blocks, threads, kFwdLds, st, a, seed_counter(), nc...);
    // (all three reservations before the first launch: a failed one leaves nothing half-written)
    if (int rc = reserve_lds<tri_kb_bwd_q_kernel<T, HG, kPF, true, NC...>>("tri_kb_bwd_e_kernel", kBwdQLds)) return rc;
    if (int rc = reserve_lds<tri_kb_bwd_q_kernel<T, HG, kPF, false, NC...>>("tri_kb_bwd_q_kernel", kBwdQLds)) return rc;
    if (int rc = reserve_lds<tri_kb_bwd_k_kernel<T, HG, kPF, NC...>>("tri_kb_bwd_k_kernel", kBwdKLds)) return rc;
    if (int rc = launch_lds<tri_kb_bwd_q_kernel<T, HG, kPF, true, NC...>>("tri_kb_bwd_e_kernel", blocks, threads, kBwdQLds, st, a, seed_counter(), nc...)) return rc;    // E sweep: statistics first
    if (int rc = launch_lds<tri_kb_bwd_q_kernel<T, HG, kPF, false, NC...>>("tri_kb_bwd_q_kernel", blocks, threads, kBwdQLds, st, a, seed_counter(), nc...)) return rc;
    return launch_lds<tri_kb_bwd_k_kernel<T, HG, kPF, NC...>>("tri_kb_bwd_k_kernel", blocks, threads, kBwdKLds, st, a, seed_counter(), nc...);
}
template <typename T>
static int dispatch_kb(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st) {
    if (nc) return a.H % 4 == 0 ? launch_kb<T, 4>(a, bwd, st, nc) : launch_kb<T, 1>(a, bwd, st, nc);
    if (a.H % 4 == 0) return launch_kb<T, 4>(a, bwd, st);
    return launch_kb<T, 1>(a, bwd, st);
}

// one dtype per translation unit in the build, as triplet_attention.hip (TGT_TRIKB_INST: bit 0 fp32, bit 1 bf16, bit 2 fp16,
// bit 3 the checks + dispatch)
#ifndef TGT_TRIKB_INST
#define TGT_TRIKB_INST 15
#endif
int tri_att_kb_run_f32(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st);
int tri_att_kb_run_bf16(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st);
int tri_att_kb_run_f16(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st);
#if TGT_TRIKB_INST & 1
int tri_att_kb_run_f32(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st) { return dispatch_kb<float>(a, nc, bwd, st); }
#endif
#if TGT_TRIKB_INST & 2
int tri_att_kb_run_bf16(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st) { return dispatch_kb<bf16_t>(a, nc, bwd, st); }
#endif
#if TGT_TRIKB_INST & 4
int tri_att_kb_run_f16(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st) { return dispatch_kb<f16_t>(a, nc, bwd, st); }
#endif

#if TGT_TRIKB_INST & 8
// host only; reads B, N, H, D, dtype, flags
int64_t tri_att_kb_workspace_bytes(const tgt_triplet_attention_args* a, int bwd) {
    if (!a || a->B < 0 || a->N < 0 || a->H <= 0) return -1;
    if (a->dtype != TGT_F32 && a->dtype != TGT_BF16 && a->dtype != TGT_F16) return -1;
    if (a->N > 128) return -1;
    if (a->N <= 64) return (a->D == 8 || a->D == 16 || a->D == 32) ? 0 : -1;
    if (a->D != 16) return -1;
    if (!bwd) return 0;
    const int64_t Np = (a->N + 31) & ~31;
    return (int64_t)a->B * 2 * a->H * a->N * 3 * Np * (int64_t)sizeof(float);
}

// 65 <= N <= 128, arguments already validated by triplet_attention_run.  nc: the node counts of a *_counts call or nullptr; they
// reach the kernels only with TGT_TRI_COUNTS_KB in a.flags (DEVICE memory, never read here)
int tri_att_kb_run(const tgt_triplet_attention_args& a, const int32_t* nc, bool bwd, hipStream_t st) {
    if (!(a.flags & TGT_TRI_COUNTS_KB)) nc = nullptr;
    if (a.D != 16) return set_error(TGT_ERR_UNSUPPORTED, "triplet attention: N=%d > 64 is supported for D = 16 only (D=%d)", a.N, a.D);
    if (bwd) {
        if (a.d_qkv_colsum[0] || a.d_qkv_colsum[1] || a.d_eg_colsum[0] || a.d_eg_colsum[1])
            return set_error(TGT_ERR_UNSUPPORTED, "triplet attention bwd: d_qkv_colsum / d_eg_colsum are not produced for N=%d > 64 (use tgt_colsum)", a.N);
        const int64_t need = tri_att_kb_workspace_bytes(&a, 1);
        if (!a.workspace || a.workspace_bytes < need || ((uintptr_t)a.workspace % 16))
            return set_error(TGT_ERR_INVALID, "triplet attention bwd: N=%d needs a 16-byte aligned workspace of %lld bytes (tgt_triplet_attention_workspace_bytes), got %lld",
                             a.N, (long long)need, (long long)a.workspace_bytes);
    }
    switch (a.dtype) {
        case TGT_F32: return tri_att_kb_run_f32(a, nc, bwd, st);
        case TGT_BF16: return tri_att_kb_run_bf16(a, nc, bwd, st);
        case TGT_F16: return tri_att_kb_run_f16(a, nc, bwd, st);
        default: return set_error(TGT_ERR_INVALID, "triplet attention: bad dtype %d", a.dtype);
    }
}
#endif

}  // namespace tgt
