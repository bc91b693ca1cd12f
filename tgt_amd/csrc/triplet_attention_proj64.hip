// Triplet attention forward with the Q/K/V projection fused in, 33 <= N <= 64 -- gfx950, inference only (no backward follows).
//
// The two-tile sibling of triplet_attention_proj.hip's STORE = false form.  The unfused path at these node
// counts is a library GEMM that writes the (B,N,N,6C) Q/K/V tensor and tri_att16_fwd_kernel, which reads it straight back; here
// the workgroup that walks shared node j projects the LayerNorm'd edge rows it needs itself and Q, K, V never leave the CU --
// most of them never leave the register file.
//
//   workgroup = (graph b, direction, 4 heads), 8 waves at up to 256 registers (one workgroup per CU, two waves per SIMD);
//   wave = (head hw = wave & 3, half = wave >> 2): the half owns the query blocks {2 half, 2 half + 1} of 16 rows and projects
//   the key blocks of the same numbers.  Resident through the walk: the head's 48 weight rows [W_Q; W_K; W_V] x 256 k as operand
//   fragments of v_mfma_f32_16x16x32 (96 registers) and the third arm (bias + mask, gate) of 2 query blocks x 4 key blocks in
//   fp32 (64 registers).  Per step j, two phases and two barriers:
//     phase A  (reads the X tile of step j: rows 0..63 = edges (i, j); inward also rows 64..127 = edges (j, k))
//              Q^T[d][i] = W_Q X_q^T per own query block: the accumulator (lane = query, d = 4g + q) IS the B operand of the
//              16x16x16 score product and stays in registers;  K^T[d][k] = W_K X_kv^T and V[k][d] = X_kv W_V^T per own key block
//              -- the same weight fragment serves as A or as B -- come out as the A operands of the score and of the P V product
//              and go, 8 bytes per lane and lane-linear, into a 16 KB exchange area for the other half of the head;
//     barrier 1; the X tile of step j + 1 goes from registers to LDS and the loads of step j + 2 are issued: ONE X tile, a
//              register prefetch a whole step deep;
//     phase B  the core of tri_att16_fwd_kernel for (head, own query blocks) against the 4 key blocks of the exchange area:
//              S^T = K Q^T, softmax over keys (in-lane + two lane exchanges), gate, O^T = V^T P^T; O rows into a 64-row O slab;
//     barrier 2; the O rows of step j leave as whole 128-byte row pieces (slab_store: rows i >= N are not stored).
//   Every X row is projected ONCE per step and workgroup (no loop over query tiles around the walk).
//   The four head groups of a (graph, direction) read the same X rows: they are consecutive workgroups of one XCD (unit_of_block).
//   Keys k >= N of a partly filled key block: their X rows load as zeros, so their K and V are the projection bias, not 0 --
//   their WEIGHT is exactly 0 (a logit of -inf and a gate of 0, as tri_att16_fwd_kernel); key blocks wholly past N are skipped.
// Supported: C = 256, D = 16, H = 16, 33 <= N <= 64, 16-bit dtypes, gated / ungated / axial, no attention dropout,
// TGT_TRI_NO_QKV_STORE set (a->qkv is never dereferenced).
//
// The TRAINING form (TGT_TRI_PROJ64_INST == 2, a translation unit of its own so that the kernels above keep
// the instruction streams they were measured with): the same walk with STORE = true.  Phase A additionally puts the packed Q, K
// and V values it consumes into three 64-row slabs next to the O slab -- Q and K as the 8 bytes per lane of the O-slab write, V
// (lane column = d, four keys per lane) element by element, which is its transpose -- and after barrier 1 they leave as whole
// 128-byte row pieces through slab_store into a->qkv[dir], the layout tri_att16_bwd_kernel reads.  The slabs are written before
// B1_j, read by the stores between B1_j and B2_j and written again after B2_j: no third barrier.  Over the walk every row is
// projected once (inward: Q of (i, j), K / V of (j, k); outward: all three of (t, j)), so no element has two writers; rows >= N,
// a dropped graph's rows and the units j >= n of a ragged graph are never written.
#include "node_tiles16.hpp"
#include "triplet_common.hpp"

#ifndef TGT_TRI_PROJ64_INST
#define TGT_TRI_PROJ64_INST 1      // 1: the inference kernels and their entry; 2: the training (storing) kernels and theirs
#endif

namespace tgt {

namespace proj64 {
using na16::frag4_t;
using na16::mma16;
using na16::pack4;
constexpr int kC = xtile::kC, kD = 16, kH = 16, kHG = 4, kWaves = 2 * kHG, kThreads = kWaves * 64;
constexpr int kRows = 64;                                    // rows of one part of the X tile and of the O slab
constexpr int kRowBytes = xtile::kRowBytes;
constexpr int kXTile = 2 * kRows * xtile::kPitch;            // inward: rows (i, j) then rows (j, k); outward uses the first half
constexpr int kKvx = kHG * 4 * 2 * 512;                      // exchange area: [head][key block][K | V] x (64 lanes x 8 bytes)
constexpr int kOSlab = kRows * kHG * kD * 2;
constexpr int kOffKvx = kXTile, kOffO = kOffKvx + kKvx, kWalk = kOffO + kOSlab;
constexpr int kOffQkv = kWalk, kWalkStore = kOffQkv + 3 * kOSlab;           // training form: the Q | K | V row slabs behind the O slab
constexpr uint32_t kNone = 0xffffffffu;
// the 4-head slab geometry of triplet_common.hpp, walked by this kernel's 512 threads
template <typename T>
struct Geo : TriGeo<T, kD, kHG> {
    static constexpr int kThreads = proj64::kThreads;
};
template <typename T> using Arm = ArmStage<T, kHG, 2>;       // one 32-row query pass against both 32-key tiles

// third arm of (query 32 half + 16 qbl + x, keys 16 kb + 4g + q) of head hh from the stage image of pass i0 = 32 half
// (arm_stage_load's layout), in the accumulator layout of the 16-wide tiles
template <typename T>
__device__ __forceinline__ void arm_read16(const ThirdArm& ta, const char* lds, int dir, int hh, int N, int i0, int qbl, int x, int g,
                                           float (&biasM)[4][4], float (&gate)[4][4]) {
    using A = Arm<T>;
    const int pitch = A::pitch(dir), mpitch = A::mpitch(dir);
    const int ri = 16 * qbl + x, i = i0 + ri;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 16 * kb + 4 * g + q;
            const int xx = dir == 0 ? ri : k, yy = dir == 0 ? k : ri;
            const char* pp = lds + xx * pitch + yy * A::kPairBytes;
            const float e = to_f32(*reinterpret_cast<const T*>(pp + hh * (int)sizeof(T)));
            const float gl = to_f32(*reinterpret_cast<const T*>(pp + (kHG + hh) * (int)sizeof(T)));
            const float m = *reinterpret_cast<const float*>(lds + A::kOffM + xx * mpitch + yy * 4);
            biasM[kb][q] = k < N ? e + m : -INFINITY;
            gate[kb][q] = (i < N && k < N) ? (ta.gated ? fast_sigmoid(gl + m) : 1.f) : 0.f;
        }
}

// arm_stage_load<T, kHG, 2> for both query passes (i0 = 0 into the first stage image, i0 = 32 into the second) by all 512 threads.
// The E columns of the group's 4 heads are 8 contiguous bytes of a pair's row, the G columns another 8: where those are 8-byte
// aligned a thread fetches them whole, 8 pairs per thread with every load in flight at once -- the element-wise loader waits for
// each 2-byte load in turn, 64 times per thread at this size.  Any other
// alignment: the element-wise loader, threads 0..255 for the first pass and 256..511 for the second.
template <typename T, int DIR>
__device__ __forceinline__ void arm_stage_load2(const ThirdArm& ta, int b, int g, int N, char* smem, int tid) {
    using A = Arm<T>;
    const bool vec = (ta.ld % 4 == 0) && (ta.e_off % 4 == 0) && (ta.g_off % 4 == 0) && ((uintptr_t)ta.eg % 8 == 0);
    if (!vec) {
        arm_stage_load<T, kHG, 2>(ta, b, DIR, g, N, 32 * (tid >> 8), smem + (tid >> 8) * A::kBytes, tid & 255);
        return;
    }
    constexpr int ny = DIR == 0 ? 64 : 32, kPairs = 2 * 32 * 64, kIt = kPairs / kThreads;
    const int pitch = A::pitch(DIR), mpitch = A::mpitch(DIR);
    const char* eg = reinterpret_cast<const char*>(ta.eg);
    uint2 e[kIt], gl[kIt];
    float m[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int p = it * kThreads + tid, pass = p >> 11, pp = p & 2047, yy = pp % ny, xx = pp / ny;
        const int x = (DIR == 0 ? 32 * pass : 0) + xx, y = (DIR == 0 ? 0 : 32 * pass) + yy;
        const bool valid = x < N && y < N;
        const int64_t pair = ((int64_t)b * N + x) * N + y;
        e[it] = gl[it] = make_uint2(0, 0);
        m[it] = 0.f;
        if (valid && ta.biased) e[it] = *reinterpret_cast<const uint2*>(eg + (pair * ta.ld + ta.e_off + g * kHG) * (int64_t)sizeof(T));
        if (valid && ta.gated) gl[it] = *reinterpret_cast<const uint2*>(eg + (pair * ta.ld + ta.g_off + g * kHG) * (int64_t)sizeof(T));
        if (valid && ta.mask) m[it] = ta.mask[pair];
    }
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int p = it * kThreads + tid, pass = p >> 11, pp = p & 2047, yy = pp % ny, xx = pp / ny;
        uint32_t* rec = reinterpret_cast<uint32_t*>(smem + pass * A::kBytes + xx * pitch + yy * A::kPairBytes);      // (4-byte aligned: the pitch)
        rec[0] = e[it].x; rec[1] = e[it].y; rec[2] = gl[it].x; rec[3] = gl[it].y;
        *reinterpret_cast<float*>(smem + pass * A::kBytes + A::kOffM + xx * mpitch + yy * 4) = m[it];
    }
}
}  // namespace proj64

template <typename T, int DIR, bool RG, bool STORE = false>
__device__ __forceinline__ void proj64_walk(const tgt_triplet_attention_args& a, const int32_t* node_counts, const TriCtx& c, const T* x,
                                            const T* w, const T* bias, char* smem, int tid) {
    using namespace proj64;
    using G = Geo<T>;
    using F = frag_t<T>;
    using F4 = frag4_t<T>;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), x16 = lane & 15, g = lane >> 4;
    const int hw = wave & 3, half = wave >> 2;                              // (wave-uniform: the block tests below are scalar branches)
    const int N = c.N;
    const int64_t sz = sizeof(T), Nl = N;
    const uint32_t ldo_ = (uint32_t)(a.ld_out * sz);
    const SlabBuf bO = {graph_rsrc(a.out, Nl * Nl * a.ld_out * sz, c.b), (uint32_t)((a.o_off[DIR] + c.g * kHG * kD) * sz), (uint32_t)N * ldo_, ldo_};

    // a graph DropPath dropped (graph_scale[b] == 0): zeros to its O rows, nothing is read or computed.  Ragged batches
    // (node_counts): the walk ends at the graph's own n -- the X rows of the units j >= n are not read -- and those units get the
    // same zeros after it.
    const int n = tri_node_count<RG>(node_counts, c.b, N);
    if ((a.graph_scale && a.graph_scale[c.b] == 0.f) || (RG && n == 0)) {
        for (int j = 0; j < N; ++j) slab_store_zero<G, kRows>(bO, j, 0, N, tid);
        return;
    }

    // ---- third arm: both 32-row query passes of ArmStage side by side in the area the walk's buffers take afterwards
    float biasM[2][4][4], gate[2][4][4];
    {
        const ThirdArm ta = tri_third_arm(a, DIR);
        arm_stage_load2<T, DIR>(ta, c.b, c.g, N, smem, tid);
        __syncthreads();
#pragma unroll
        for (int qbl = 0; qbl < 2; ++qbl)
            arm_read16<T>(ta, smem + half * Arm<T>::kBytes, DIR, hw, N, 32 * half, qbl, x16, g, biasM[qbl], gate[qbl]);
        __syncthreads();
    }

    // ---- resident projection of head c.h: fragment s of part p holds W_p[row x16][k = 32 s + 8 g ..]
    F wq[8], wk[8], wv[8];
    float bq[4], bk[4];
    {
        const int hrow = c.h * kD + x16;
        const T* rq = w + (int64_t)(a.q_off[DIR] + hrow) * kC + 8 * g;
        const T* rk = w + (int64_t)(a.k_off[DIR] + hrow) * kC + 8 * g;
        const T* rv = w + (int64_t)(a.v_off[DIR] + hrow) * kC + 8 * g;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            wq[s] = load_frag<T>(rq + 32 * s);
            wk[s] = load_frag<T>(rk + 32 * s);
            wv[s] = load_frag<T>(rv + 32 * s);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bq[q] = to_f32(bias[a.q_off[DIR] + c.h * kD + 4 * g + q]);       // Q^T, K^T: d = 4g + q
            bk[q] = to_f32(bias[a.k_off[DIR] + c.h * kD + 4 * g + q]);
        }
    }
    const float bv = to_f32(bias[a.v_off[DIR] + c.h * kD + x16]);            // V: d = the lane's column

    // ---- X tile of step j: part 0 = rows t of x[t, j, :], part 1 (inward) = rows t of x[j, t, :]; rows t >= N are zeros
    // (out-of-range loads).  The per-thread offsets are rebuilt from the thread index at every use instead of living in
    // registers through the walk (`t_` is opaque so that nothing is hoisted, as in tri_agg_proj64_fwd_kernel).
    constexpr int kXIt = (DIR == 0 ? 2 : 1) * kRows * (kRowBytes / 16) / kThreads;     // 8 inward, 4 outward
    const __amdgpu_buffer_rsrc_t r_x = graph_rsrc(x, Nl * Nl * kRowBytes, c.b);
    uint4 px[kXIt];
    auto x_issue = [&](int jx) {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        const bool live = jx < n;
#pragma unroll
        for (int it = 0; it < kXIt; ++it) {
            const int row = (it & 3) * 16 + (t_ >> 5), slot = t_ & 31;      // it < 4: part 0, it >= 4: part 1
            const uint32_t rs = it < 4 ? (uint32_t)N * kRowBytes : (uint32_t)kRowBytes;
            const uint32_t js = it < 4 ? (uint32_t)kRowBytes : (uint32_t)N * kRowBytes;
            const uint32_t vo = (live && row < N) ? (uint32_t)row * rs + (uint32_t)slot * 16u : kNone;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r_x, (int)vo, (int)(live ? (uint32_t)jx * js : 0u), 0);
            px[it] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    auto x_commit = [&]() {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
#pragma unroll
        for (int it = 0; it < kXIt; ++it) *reinterpret_cast<uint4*>(smem + xtile::off(it * 16 + (t_ >> 5), t_ & 31)) = px[it];
    };

    char* kvx = smem + kOffKvx + hw * (4 * 2 * 512) + lane * 8;              // this lane's 8 bytes of [key block][K | V] of its head
    char* sO = smem + kOffO;
    // STORE: the Q / K / V rows of step j, as rows of this head group's 64 channels (the O slab's geometry).  Q rows are the
    // edges (i, j); K / V rows the edges (j, k) inward, (k, j) outward
    auto qkv_slab = [&](int part) {
        const uint32_t ldq = (uint32_t)(a.ld_qkv[DIR] * sz);
        const int off = part == 0 ? a.q_off[DIR] : part == 1 ? a.k_off[DIR] : a.v_off[DIR];
        const bool rows_ij = part == 0 || DIR == 1;
        return SlabBuf{graph_rsrc(a.qkv[DIR], Nl * Nl * a.ld_qkv[DIR] * sz, c.b), (uint32_t)((off + c.g * kHG * kD) * sz),
                       rows_ij ? (uint32_t)N * ldq : ldq, rows_ij ? ldq : (uint32_t)N * ldq};
    };
    const int nblk = (N + 15) >> 4;                                         // blocks of 16 rows that hold a real node (3 or 4)
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};

    // Hazards with two barriers per step (B1_j, B2_j): the X tile is read in phase A alone, before B1_j, and rewritten between
    // B1_j and B2_j; the exchange area is written in phase A and read in phase B, between B1_j and B2_j; the O slab is written
    // in phase B, stored after B2_j, and written again after B1_{j+1}.
    x_issue(0);
    x_commit();
    x_issue(1);                                                             // (1 >= n: nothing is read)
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        // ---- phase A
        F4 fq[2];
#pragma unroll
        for (int bl = 0; bl < 2; ++bl) {
            const int blk = 2 * half + bl;
            if (blk < nblk) {
                const char* xq = smem + xtile::off(16 * blk + x16, g);
                const char* xkv = smem + xtile::off((DIR == 0 ? kRows : 0) + 16 * blk + x16, g);
                f32x4 qa, ka, va;
#pragma unroll
                for (int q = 0; q < 4; ++q) { qa[q] = bq[q]; ka[q] = bk[q]; va[q] = bv; }
                // the fragment reads run two k-steps ahead of the products (a ring of three): left to itself hipcc either waits for
                // every pair of reads in front of its products or hoists all sixteen next to the resident weights
                F fx[3], fkv[3];
                auto frags = [&](int s) {
                    fx[s % 3] = load_frag<T>(reinterpret_cast<const T*>(xq + 64 * s));
                    if constexpr (DIR == 0) fkv[s % 3] = load_frag<T>(reinterpret_cast<const T*>(xkv + 64 * s));
                };
                frags(0);
                frags(1);
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    if (s + 2 < 8) frags(s + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    const F fa = fx[s % 3], fb = DIR == 0 ? fkv[s % 3] : fa;
                    qa = mma16x32(wq[s], fa, qa);                           // Q^T[d][i]
                    ka = mma16x32(wk[s], fb, ka);                           // K^T[d][k]
                    va = mma16x32(fb, wv[s], va);                           // V[k][d]
                    __builtin_amdgcn_sched_barrier(0);
                }
                fq[bl] = pack4<T>(qa);
                const F4 fk = pack4<T>(ka), fv = pack4<T>(va);
                uint2 r0, r1;
                __builtin_memcpy(&r0, &fk, 8);
                __builtin_memcpy(&r1, &fv, 8);
                *reinterpret_cast<uint2*>(kvx + (blk * 2 + 0) * 512) = r0;
                *reinterpret_cast<uint2*>(kvx + (blk * 2 + 1) * 512) = r1;
                if constexpr (STORE) {
                    // the packed values themselves.  Q^T, K^T: lane (row x16, g) holds channels 4g .. 4g+3 of its row, 8 bytes;
                    // V: lane (d = x16, g) holds keys 4g .. 4g+3 of the block, one element each into their rows
                    // (the slab offsets are rebuilt from an opaque copy of the lane index: hoisted out of the walk they would live
                    // next to the resident weights and the third arm, and the register file is full)
                    int l_ = lane;
                    asm volatile("" : "+v"(l_));
                    const int x16 = l_ & 15, g = l_ >> 4;
                    char* sQkv = smem + kOffQkv;
                    uint2 rq;
                    __builtin_memcpy(&rq, &fq[bl], 8);
                    const int o8 = G::lds_elem(16 * blk + x16, hw * kD + 4 * g);
                    *reinterpret_cast<uint2*>(sQkv + o8) = rq;
                    *reinterpret_cast<uint2*>(sQkv + kOSlab + o8) = r0;
                    uint16_t tv[4];
                    __builtin_memcpy(tv, &r1, 8);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<uint16_t*>(sQkv + 2 * kOSlab + G::lds_elem(16 * blk + 4 * g + q, hw * kD + x16)) = tv[q];
                }
            } else {
                fq[bl] = pack4<T>(z);
            }
        }
        __syncthreads();                                                    // B1
        x_commit();                                                         // X tile of step j + 1
        x_issue(j + 2);                                                     // (a whole step ahead of its commit; j + 2 >= n: nothing is read)
        asm volatile("" ::: "memory");
        if constexpr (STORE) {
            // the Q / K / V rows of step j (written before B1, not rewritten before B2); rows >= N are not stored.  Behind the X
            // loads of step j + 2, so that the loads are not queued behind 24 KB of stores
            int t_ = tid;
            asm volatile("" : "+v"(t_));
#pragma unroll
            for (int part = 0; part < 3; ++part) slab_store<G, kRows>(smem + kOffQkv + part * kOSlab, qkv_slab(part), j, 0, N, t_);
            asm volatile("" ::: "memory");
        }
        // ---- phase B
#pragma unroll
        for (int bl = 0; bl < 2; ++bl) {
            const int qb = 2 * half + bl;
            if (qb < nblk) {
                f32x4 s[4];
                float mx = -INFINITY;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    if (kb < nblk) {
                        F4 fk;
                        const uint2 raw = *reinterpret_cast<const uint2*>(kvx + (kb * 2 + 0) * 512);
                        __builtin_memcpy(&fk, &raw, 8);
                        s[kb] = mma16(fk, fq[bl], z);                       // S^T[key][query]
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            s[kb][q] = s[kb][q] * a.scale + biasM[bl][kb][q];
                            mx = fmaxf(mx, s[kb][q]);
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) s[kb][q] = -INFINITY;
                    }
                }
                mx = xor16_max(mx);
                mx = fmaxf(mx, xhalf(mx));
                float sum = 0.f;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        s[kb][q] = fast_exp(s[kb][q] - mx);
                        sum += s[kb][q];
                    }
                sum = xor16_sum(sum);
                sum += xhalf(sum);
                const float inv = fast_rcp(sum);
                f32x4 o = z;
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) {
                    if (kb < nblk) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) s[kb][q] = s[kb][q] * inv * gate[bl][kb][q];
                        F4 fv;
                        const uint2 raw = *reinterpret_cast<const uint2*>(kvx + (kb * 2 + 1) * 512);
                        __builtin_memcpy(&fv, &raw, 8);
                        o = mma16(fv, pack4<T>(s[kb]), o);                  // O^T[d][query]
                    }
                }
                // lane (query, g) holds channels 4g .. 4g+3 of its query: 8 bytes into the head's columns of the O slab
                const F4 of = pack4<T>(o);
                uint2 raw;
                __builtin_memcpy(&raw, &of, 8);
                *reinterpret_cast<uint2*>(sO + G::lds_elem(16 * qb + x16, hw * kD + 4 * g)) = raw;
            }
        }
        __syncthreads();                                                    // B2
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        slab_store<G, kRows>(sO, bO, j, 0, N, t_);                          // rows i >= N are not stored
    }
    if constexpr (RG) {
        int t_ = tid;
        asm volatile("" : "+v"(t_));
        for (int j = n; j < N; ++j) slab_store_zero<G, kRows>(bO, j, 0, N, t_);
    }
}

// what both entry points ask of the tensors every form reads or writes, after their predicate and the empty batch
static int proj64_check_tensors(const tgt_triplet_attention_args* a, const void* x, const void* w, const void* bias) {
    if (!x || !w || !bias || !a->mask || !a->out)                           // (a->qkv: the training entry's own check)
        return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): null tensor");
    if ((a->flags & (TGT_TRI_BIASED | TGT_TRI_GATED)) && (!a->eg[0] || !a->eg[1]))
        return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): eg missing");
    if ((a->ld_out * 2) % 16 || (a->o_off[0] * 2) % 16 || (a->o_off[1] * 2) % 16 || ((uintptr_t)a->out % 16) ||
        (((uintptr_t)x | (uintptr_t)w) % 16) || ((uintptr_t)bias % 2) || ((uintptr_t)a->mask % 4))
        return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): x / w / out rows and offsets must be 16-byte aligned");
    if ((uintptr_t)a->graph_scale % 4) return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): graph_scale must be 4-byte aligned");
    return TGT_OK;
}

#if TGT_TRI_PROJ64_INST == 1
template <typename T, typename... NC>
__global__ void __launch_bounds__(proj64::kThreads, 2) tri_att_proj64_fwd_kernel(const tgt_triplet_attention_args a, const T* x, const T* w,
                                                                                 const T* bias, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;          // ragged: launched with the node counts as a trailing argument (triplet_common.hpp)
    const int32_t* node_counts = tri_counts_ptr(nc...);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    // Unit order (node_tiles16.hpp, unit_of_block): the four head groups of a (graph, direction) read the SAME X rows, so they are
    // consecutive workgroups of ONE XCD and share them through its L2
    TriCtx c;
    {
        int pair, grp;
        if (!na16::unit_of_block(2 * a.B, proj64::kH / proj64::kHG, pair, grp)) return;
        c.b = pair >> 1; c.dir = pair & 1; c.g = grp; c.h = grp * proj64::kHG + ((tid >> 6) & 3); c.N = a.N; c.tile = 0;
    }
    if (c.dir == 0) proj64_walk<T, 0, RG>(a, node_counts, c, x, w, bias, smem, tid);
    else proj64_walk<T, 1, RG>(a, node_counts, c, x, w, bias, smem, tid);
}

int triplet_attention_proj64_supported(const tgt_triplet_attention_args* a, int C) {
    return a && a->dropout_p == 0.f && a->N >= 33 && a->N <= 64 && a->D == proj64::kD && a->H == proj64::kH &&
           (a->dtype == TGT_BF16 || a->dtype == TGT_F16) && C == proj64::kC && (a->flags & TGT_TRI_NO_QKV_STORE);
}

template <typename T>
static int launch_proj64(const tgt_triplet_attention_args& a, const int32_t* nc, const void* x, const void* w, const void* bias, hipStream_t st) {
    constexpr int kLds = cmax(proj64::kWalk, 2 * proj64::Arm<T>::kBytes);
    static_assert(kLds <= 160 * 1024, "one workgroup must fit the LDS of a CU");
    const T *xp = reinterpret_cast<const T*>(x), *wp = reinterpret_cast<const T*>(w), *bp = reinterpret_cast<const T*>(bias);
    const dim3 g(8 * ((a.B * 2 + 7) / 8) * (proj64::kH / proj64::kHG)), blk(proj64::kThreads);      // (unit_of_block: blocks past an XCD's share exit)
    // (without counts: the kernel's instantiation without the argument -- triplet_common.hpp, tri_counts_ptr)
    return nc ? launch_lds<tri_att_proj64_fwd_kernel<T, const int32_t*>>("tri_att_proj64_fwd_kernel", g, blk, kLds, st, a, xp, wp, bp, nc)
              : launch_lds<tri_att_proj64_fwd_kernel<T>>("tri_att_proj64_fwd_kernel", g, blk, kLds, st, a, xp, wp, bp);
}

int triplet_attention_proj64_run(const tgt_triplet_attention_args* a, const int32_t* nc, const void* x, int C, const void* w,
                                 const void* bias, hipStream_t st) {
    if (!a) return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): null args");
    if (a->B < 0 || a->N < 0 || a->H <= 0 || C <= 0) return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes): bad sizes");
    if (!triplet_attention_proj64_supported(a, C))
        return set_error(TGT_ERR_UNSUPPORTED,
                         "projected triplet attention (33..64 nodes) needs 33 <= N <= 64, D = 16, H = 16, a 16-bit dtype, C = 256, no attention "
                         "dropout and TGT_TRI_NO_QKV_STORE set: it has no form that writes Q/K/V (got N=%d D=%d H=%d dtype=%d C=%d flags=%d dropout_p=%g)",
                         a->N, a->D, a->H, a->dtype, C, a->flags, (double)a->dropout_p);
    if (a->B == 0) return TGT_OK;
    if (int rc = proj64_check_tensors(a, x, w, bias)) return rc;
    return a->dtype == TGT_BF16 ? launch_proj64<bf16_t>(*a, nc, x, w, bias, st) : launch_proj64<f16_t>(*a, nc, x, w, bias, st);
}

#else   // TGT_TRI_PROJ64_INST == 2: the training form
// tri_att_proj64_fwd_kernel with STORE = true: a kernel of another name, so that the inference kernels keep theirs
template <typename T, typename... NC>
__global__ void __launch_bounds__(proj64::kThreads, 2) tri_att_proj64_train_fwd_kernel(const tgt_triplet_attention_args a, const T* x, const T* w,
                                                                                       const T* bias, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;
    const int32_t* node_counts = tri_counts_ptr(nc...);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    TriCtx c;
    {
        int pair, grp;
        if (!na16::unit_of_block(2 * a.B, proj64::kH / proj64::kHG, pair, grp)) return;
        c.b = pair >> 1; c.dir = pair & 1; c.g = grp; c.h = grp * proj64::kHG + ((tid >> 6) & 3); c.N = a.N; c.tile = 0;
    }
    if (c.dir == 0) proj64_walk<T, 0, RG, true>(a, node_counts, c, x, w, bias, smem, tid);
    else proj64_walk<T, 1, RG, true>(a, node_counts, c, x, w, bias, smem, tid);
}

int triplet_attention_proj64_train_supported(const tgt_triplet_attention_args* a, int C) {
    return a && a->dropout_p == 0.f && a->N >= 33 && a->N <= 64 && a->D == proj64::kD && a->H == proj64::kH &&
           (a->dtype == TGT_BF16 || a->dtype == TGT_F16) && C == proj64::kC && !(a->flags & TGT_TRI_NO_QKV_STORE);
}

template <typename T>
static int launch_proj64_train(const tgt_triplet_attention_args& a, const int32_t* nc, const void* x, const void* w, const void* bias,
                               hipStream_t st) {
    constexpr int kLds = cmax(proj64::kWalkStore, 2 * proj64::Arm<T>::kBytes);
    static_assert(kLds <= 160 * 1024, "one workgroup must fit the LDS of a CU");
    const T *xp = reinterpret_cast<const T*>(x), *wp = reinterpret_cast<const T*>(w), *bp = reinterpret_cast<const T*>(bias);
    const dim3 g(8 * ((a.B * 2 + 7) / 8) * (proj64::kH / proj64::kHG)), blk(proj64::kThreads);
    return nc ? launch_lds<tri_att_proj64_train_fwd_kernel<T, const int32_t*>>("tri_att_proj64_train_fwd_kernel", g, blk, kLds, st, a, xp, wp, bp, nc)
              : launch_lds<tri_att_proj64_train_fwd_kernel<T>>("tri_att_proj64_train_fwd_kernel", g, blk, kLds, st, a, xp, wp, bp);
}

int triplet_attention_proj64_train_run(const tgt_triplet_attention_args* a, const int32_t* nc, const void* x, int C, const void* w,
                                       const void* bias, hipStream_t st) {
    if (!a) return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes, training): null args");
    if (a->B < 0 || a->N < 0 || a->H <= 0 || C <= 0)
        return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes, training): bad sizes");
    if (!triplet_attention_proj64_train_supported(a, C))
        return set_error(TGT_ERR_UNSUPPORTED,
                         "projected triplet attention (33..64 nodes, training) needs 33 <= N <= 64, D = 16, H = 16, a 16-bit dtype, C = 256, no "
                         "attention dropout and TGT_TRI_NO_QKV_STORE clear: it writes Q/K/V (got N=%d D=%d H=%d dtype=%d C=%d flags=%d dropout_p=%g)",
                         a->N, a->D, a->H, a->dtype, C, a->flags, (double)a->dropout_p);
    if (a->B == 0) return TGT_OK;
    if (int rc = proj64_check_tensors(a, x, w, bias)) return rc;
    // the Q/K/V rows: 128-byte row pieces of whole 16-byte chunks, inside a graph the kernel addresses with 32-bit offsets
    for (int dir = 0; dir < 2; ++dir) {
        if (!a->qkv[dir]) return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes, training): null qkv");
        const int64_t ld = a->ld_qkv[dir];
        const int offs[3] = {a->q_off[dir], a->k_off[dir], a->v_off[dir]};
        bool ok = ld > 0 && (ld * 2) % 16 == 0 && (uintptr_t)a->qkv[dir] % 16 == 0 && (int64_t)a->N * a->N * ld * 2 <= INT32_MAX;
        for (int p = 0; p < 3; ++p) ok = ok && offs[p] >= 0 && (offs[p] * 2) % 16 == 0 && offs[p] + proj64::kH * proj64::kD <= ld;
        if (!ok)
            return set_error(TGT_ERR_INVALID, "projected triplet attention (33..64 nodes, training): qkv rows and offsets must be 16-byte aligned, "
                                              "inside a row of ld_qkv, and a graph below 2 GB");
    }
    return a->dtype == TGT_BF16 ? launch_proj64_train<bf16_t>(*a, nc, x, w, bias, st) : launch_proj64_train<f16_t>(*a, nc, x, w, bias, st);
}
#endif

}  // namespace tgt
