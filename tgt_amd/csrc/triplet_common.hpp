// Shared machinery of the triplet kernels (attention + aggregate) for gfx950:
// slab geometry, HBM<->register<->LDS staging, matrix-core operand fragments.
// See triplet_attention.hip for the design notes.
#pragma once
#include "common.hpp"

namespace tgt {

template <typename T, int D, int HG>
struct TriGeo {
    static constexpr int kThreads = HG * 64;
    static constexpr int kRowBytes = HG * D * (int)sizeof(T);   // this group's bytes of one row
    static constexpr int kSlots = kRowBytes / 16;               // 16-byte slots per row
    static constexpr int kSlabBytes = 32 * kRowBytes;
    static constexpr int kChunks = 32 * kSlots;
    static constexpr int kIters = (kChunks + kThreads - 1) / kThreads;
    static constexpr int kRowsPerBankRow = kRowBytes >= 256 ? 1 : 256 / kRowBytes;
    static constexpr int kSwzMask = (kSlots < 16 ? kSlots : 16) - 1;
    static constexpr int kDC = (D + 15) / 16;                   // 16-wide d chunks
    static_assert(kRowBytes % 16 == 0, "row piece must be a multiple of 16 bytes");
    static_assert(D % 8 == 0 && D <= 32, "D in {8,16,24,32}");

    // XOR swizzle of the 16-byte slot index so that ds_read_b128 of one slot
    // column over 16 different rows is bank-conflict free.
    __device__ static __forceinline__ int lds_off(int row, int slot) {
        const int f = (row / kRowsPerBankRow) & kSwzMask;
        return row * kRowBytes + ((slot ^ f) << 4);
    }
    // byte offset (inside a slab) of element `col` (in T units, < HG*D) of `row`
    __device__ static __forceinline__ int lds_elem(int row, int col) {
        const int bo = col * (int)sizeof(T);
        return lds_off(row, bo >> 4) + (bo & 15);
    }
};

// Slab staging.  ROWS = rows of the slab (32 per node tile); slab row `row`
// is global row `row0 + row` (rows >= N are zero-filled / not stored).
template <typename G, int ROWS>
struct SlabIO {
    static constexpr int kChunks = ROWS * G::kSlots;
    static constexpr int kIters = (kChunks + G::kThreads - 1) / G::kThreads;
};

template <typename G, int ROWS, int IT = SlabIO<G, ROWS>::kIters>
__device__ __forceinline__ void slab_commit(const uint4 (&pre)[IT], char* slab, int tid) {
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        if (c < SlabIO<G, ROWS>::kChunks) *reinterpret_cast<uint4*>(slab + G::lds_off(row, slot)) = pre[it];
    }
}
// Column sums folded into the slab stores (the bias gradient of the projection that produced the slab's
// tensor): a thread always owns the same 16-byte column chunk (slot = tid % kSlots), so it keeps E private
// fp32 accumulators -- in LDS, the register file is full -- at cs[tid*E .. +E); the workgroup reduces them
// once at the end (slab_colsum_finish).  Fixed order -> deterministic.
// floats of one accumulator plane (one of dQ/dK/dV): E per thread
template <typename G, typename T> constexpr int slab_colsum_plane_floats() { return G::kThreads * (16 / (int)sizeof(T)); }
// sum the per-thread accumulators of plane `cs` over the threads that share a slot and write the
// kSlots*E column sums to out[0 .. kSlots*E)
template <typename G, typename T>
__device__ __forceinline__ void slab_colsum_finish(const float* cs, float* out, int tid) {
    constexpr int E = 16 / (int)sizeof(T), W = G::kSlots * E;
    for (int col = tid; col < W; col += G::kThreads) {
        const int slot = col / E, e = col % E;
        float v = 0.f;
        for (int t = slot; t < G::kThreads; t += G::kSlots) v += cs[t * E + e];
        out[col] = v;
    }
}

// ---------------------------------------------------------------------------
// Buffer-addressed slab IO (the backward kernel is VALU-bound: 64-bit vector address arithmetic
// per slab and j is work it cannot afford).  A slab lives in ONE graph of a (B,N,N,ld) tensor:
//   buffer resource = that graph (base, N*N*ld bytes; accesses past it read 0 / are dropped),
//   soffset (scalar)  = channel offset + j*j_stride + row0*row_stride   -- changes with j
//   voffset (vector)  = row*row_stride + slot*16                        -- fixed per thread
// so the walk over j issues buffer_load/store ... s[rsrc], s_off offen with no vector address math.
// ---------------------------------------------------------------------------
// 16 x 16 matrix-core tile with 32-deep k (the projection-fused kernels): lane l = (x = l & 15, g = l >> 4) supplies
// A[m = x][kk = 8g + t] / B[kk = 8g + t][n = x], t = 0..7, and holds C[m = 4g + q][n = x], q = 0..3
__device__ __forceinline__ f32x4 mma16x32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma16x32(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// LDS image of a tile of LayerNorm'd edge rows X (C = 256, 16-bit: 512 bytes = 32 slots of 16) that a projection-fused kernel
// reads as matrix-core operand fragments.  Rows PADDED by one 16-byte slot instead of XOR-swizzled: the 16 rows a ds_read_b128
// lane group touches land in 16 different bank slots (pitch 528 = 33 slots), and a fragment address is
// lane base + k-step x constant -- the k-loop's reads take immediate offsets.  (With the XOR form every k-step needs its own
// address register or three VALU instructions; hipcc chose the registers, hoisted them out of the walk and spilled them next to
// the resident weights.)
namespace xtile {
constexpr int kC = 256, kRowBytes = kC * 2, kPitch = kRowBytes + 16;
__device__ __forceinline__ int off(int row, int slot) { return row * kPitch + (slot << 4); }
}  // namespace xtile

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
struct SlabBuf {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t chan;         // byte offset of this group's first channel of the tensor in a row
    uint32_t row_stride;   // bytes between consecutive slab rows
    uint32_t j_stride;     // bytes between consecutive j
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t graph_rsrc(const void* tensor, int64_t graph_bytes, int b) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(tensor)) + (int64_t)b * graph_bytes, 0,
                                             (int)graph_bytes, 0x00020000);
}
// (N is used as the ROW bound only -- never in an address: the backward passes 0 to issue a step that must read nothing)
template <typename G, int ROWS, int IT = SlabIO<G, ROWS>::kIters>
__device__ __forceinline__ void slab_issue(uint4 (&pre)[IT], const SlabBuf& s, int j, int row0, int N, int tid) {
    const uint32_t so = s.chan + (uint32_t)j * s.j_stride + (uint32_t)row0 * s.row_stride;
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        u32x4_t v = {0, 0, 0, 0};
        if (c < SlabIO<G, ROWS>::kChunks && row0 + row < N)
            v = __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, (int)((uint32_t)row * s.row_stride + (uint32_t)slot * 16u), (int)so, TGT_LD_AUX);
        pre[it] = make_uint4(v.x, v.y, v.z, v.w);
    }
}
__device__ __forceinline__ void buf_store16(const SlabBuf& s, uint4 v, uint32_t voff, uint32_t so) {
    u32x4_t d = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(d, s.rsrc, (int)voff, (int)so, TGT_ST_AUX);
}
template <typename G, int ROWS>
__device__ __forceinline__ void slab_store(const char* slab, const SlabBuf& s, int j, int row0, int N, int tid) {
    const uint32_t so = s.chan + (uint32_t)j * s.j_stride + (uint32_t)row0 * s.row_stride;
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        if (c < SlabIO<G, ROWS>::kChunks && row0 + row < N)
            buf_store16(s, *reinterpret_cast<const uint4*>(slab + G::lds_off(row, slot)),
                        (uint32_t)row * s.row_stride + (uint32_t)slot * 16u, so);
    }
}
// zeros to the slab's rows (a DropPath-dropped graph: tgt_triplet_attention_args.graph_scale)
template <typename G, int ROWS>
__device__ __forceinline__ void slab_store_zero(const SlabBuf& s, int j, int row0, int N, int tid) {
    const uint32_t so = s.chan + (uint32_t)j * s.j_stride + (uint32_t)row0 * s.row_stride;
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        if (c < SlabIO<G, ROWS>::kChunks && row0 + row < N)
            buf_store16(s, make_uint4(0, 0, 0, 0), (uint32_t)row * s.row_stride + (uint32_t)slot * 16u, so);
    }
}
template <typename G, int ROWS, typename T, int IT = SlabIO<G, ROWS>::kIters>
__device__ __forceinline__ void slab_store_add(const char* slab, const uint4 (&prior)[IT], const SlabBuf& s, int j,
                                               int row0, int N, int tid) {
    constexpr int E = 16 / (int)sizeof(T);
    const uint32_t so = s.chan + (uint32_t)j * s.j_stride + (uint32_t)row0 * s.row_stride;
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        if (c < SlabIO<G, ROWS>::kChunks && row0 + row < N) {
            uint4 a = *reinterpret_cast<const uint4*>(slab + G::lds_off(row, slot)), b = prior[it], o;
            T xa[E], xb[E];
            __builtin_memcpy(xa, &a, 16);
            __builtin_memcpy(xb, &b, 16);
#pragma unroll
            for (int t = 0; t < E; ++t) xa[t] = from_f32<T>(to_f32(xa[t]) + to_f32(xb[t]));
            __builtin_memcpy(&o, xa, 16);
            buf_store16(s, o, (uint32_t)row * s.row_stride + (uint32_t)slot * 16u, so);
        }
    }
}
template <typename G, int ROWS, typename T, bool ADD, int IT = SlabIO<G, ROWS>::kIters>
__device__ __forceinline__ void slab_store_sum(const char* slab, const uint4 (&prior)[IT], const SlabBuf& s, int j, int row0,
                                               int N, int tid, float* cs) {
    constexpr int E = 16 / (int)sizeof(T);
    static_assert(G::kThreads % G::kSlots == 0, "a thread must own one column chunk");
    float4* mine = reinterpret_cast<float4*>(cs + tid * E);
    const uint32_t so = s.chan + (uint32_t)j * s.j_stride + (uint32_t)row0 * s.row_stride;
    float acc[E];
#pragma unroll
    for (int t = 0; t < E / 4; ++t) *reinterpret_cast<float4*>(acc + 4 * t) = mine[t];
#pragma unroll
    for (int it = 0; it < SlabIO<G, ROWS>::kIters; ++it) {
        const int c = it * G::kThreads + tid;
        const int row = c / G::kSlots, slot = c % G::kSlots;
        if (c < SlabIO<G, ROWS>::kChunks && row0 + row < N) {
            uint4 a = *reinterpret_cast<const uint4*>(slab + G::lds_off(row, slot));
            T xa[E];
            __builtin_memcpy(xa, &a, 16);
            if constexpr (ADD) {
                T xb[E];
                __builtin_memcpy(xb, &prior[it], 16);
#pragma unroll
                for (int t = 0; t < E; ++t) {
                    const float old = to_f32(xb[t]);
                    xa[t] = from_f32<T>(to_f32(xa[t]) + old);
                    acc[t] += to_f32(xa[t]) - old;
                }
                __builtin_memcpy(&a, xa, 16);
            } else {
#pragma unroll
                for (int t = 0; t < E; ++t) acc[t] += to_f32(xa[t]);
            }
            buf_store16(s, a, (uint32_t)row * s.row_stride + (uint32_t)slot * 16u, so);
        }
    }
#pragma unroll
    for (int t = 0; t < E / 4; ++t) mine[t] = *reinterpret_cast<const float4*>(acc + 4 * t);
}

// operand fragments of head `wave` for slab row r: d in [16*dc + 8*hi, +8)
template <typename T, int D, int HG>
__device__ __forceinline__ void read_frags(frag_t<T> (&f)[(D + 15) / 16], const char* slab,
                                           int wave, int r, int hi) {
    using G = TriGeo<T, D, HG>;
#pragma unroll
    for (int dc = 0; dc < G::kDC; ++dc) {
        const int d0 = 16 * dc + 8 * hi;
        if (d0 < D) {
            if constexpr (sizeof(T) == 2) {
                f[dc] = load_frag<T>(reinterpret_cast<const T*>(slab + G::lds_elem(r, wave * D + d0)));
            } else {
                frag_t<T> v;
                uint4 r0 = *reinterpret_cast<const uint4*>(slab + G::lds_elem(r, wave * D + d0));
                uint4 r1 = *reinterpret_cast<const uint4*>(slab + G::lds_elem(r, wave * D + d0 + 4));
                __builtin_memcpy(&v, &r0, 16);
                __builtin_memcpy(reinterpret_cast<char*>(&v) + 16, &r1, 16);
                f[dc] = v;
            }
        } else {
            f[dc] = zero_frag<T>();
        }
    }
}

// write a transposed result tile X^T[d][row] (lane = row r, registers = d) as
// T into columns [wave*D, wave*D + D) of slab row r.
template <typename T, int D, int HG>
__device__ __forceinline__ void write_rows(char* slab, const f32x16& acc, int wave, int r, int hi) {
    using G = TriGeo<T, D, HG>;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
        const int d0 = 8 * q + 4 * hi;      // registers 4q..4q+3 hold d0..d0+3
        T tmp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) tmp[t] = from_f32<T>(acc[4 * q + t]);
        char* dst = slab + G::lds_elem(r, wave * D + d0);
        if constexpr (sizeof(T) == 2) {
            uint2 v;
            __builtin_memcpy(&v, tmp, 8);
            *reinterpret_cast<uint2*>(dst) = v;
        } else {
            uint4 v;
            __builtin_memcpy(&v, tmp, 16);
            *reinterpret_cast<uint4*>(dst) = v;
        }
    }
}

// identity fragments.  ident_d[dc]: B[kk = d][n = d'] = (d == d') for the d-chunk dc.
template <typename T, int DC>
__device__ __forceinline__ void make_ident_d(frag_t<T> (&f)[DC], int r, int hi) {
#pragma unroll
    for (int dc = 0; dc < DC; ++dc)
#pragma unroll
        for (int t = 0; t < 8; ++t) f[dc][t] = from_f32<T>(r == 16 * dc + 8 * hi + t ? 1.f : 0.f);
}
// ident_k[c]: B[kk][n = k'] = 1 where the fragment element (hi,t) of chunk c
// stands for row k' in the accumulator order: k = 16c + (t&3) + 8(t>>2) + 4hi.
template <typename T>
__device__ __forceinline__ void make_ident_k(frag_t<T> (&f)[2], int r, int hi) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < 8; ++t) f[c][t] = from_f32<T>(r == acc_row(8 * c + t, hi) ? 1.f : 0.f);
}


// ---------------------------------------------------------------------------
// Third-arm tile (bias E, gate logit G, additive mask M over node pairs) of one
// head in accumulator layout: lane column i = r, register q <-> k = acc_row(q,hi).
//   inward  (dir 0): element (i,k) is stored at pair (x,y) = (i,k)
//   outward (dir 1): element (i,k) is stored at pair (x,y) = (k,i)
// biasM = E + M (or -inf past N), gate = sigmoid(G + M) (1 if ungated).
// Entries past N: k >= N gets -inf (weight exactly 0).  Lanes i >= N are padding
// columns whose results are never stored; PAD_COLS_NEG_INF makes their weights
// exactly 0 (backward, where they feed reductions over i).
// ---------------------------------------------------------------------------
struct ThirdArm {
    const void* eg;
    int64_t ld;
    int e_off, g_off;
    const float* mask;     // (B,N,N) or nullptr (no mask in this direction)
    bool biased, gated;
};

template <typename T, bool PAD_COLS_NEG_INF>
__device__ __forceinline__ void load_third_arm(const ThirdArm& ta, int b, int dir, int h, int N, int r, int hi,
                                               float (&biasM)[16], float (&gate)[16], int i0 = 0, int k0 = 0) {
    const T* eg = reinterpret_cast<const T*>(ta.eg);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int k = k0 + acc_row(q, hi), i = i0 + r;
        const bool valid = i < N && k < N;
        const int x = dir == 0 ? i : k, y = dir == 0 ? k : i;
        const int64_t idx = ((int64_t)b * N + x) * N + y;
        const float m = (valid && ta.mask) ? ta.mask[idx] : 0.f;
        float e = 0.f, gl = 0.f;
        if (valid && ta.biased) e = to_f32(eg[idx * ta.ld + ta.e_off + h]);
        if (valid && ta.gated) gl = to_f32(eg[idx * ta.ld + ta.g_off + h]);
        biasM[q] = (k < N && (!PAD_COLS_NEG_INF || i < N)) ? e + m : -INFINITY;
        gate[q] = valid ? (ta.gated ? fast_sigmoid(gl + m) : 1.f) : 0.f;
    }
}

// scatter a per-head (i,k) tile of third-arm gradients back (as T)
template <typename T>
__device__ __forceinline__ void store_third_arm_grad(const ThirdArm& ta, void* d_eg, int b, int dir, int h, int N,
                                                     int r, int hi, const float (&dE)[16], const float (&dG)[16],
                                                     int i0 = 0, int k0 = 0) {
    if (!(ta.biased || ta.gated)) return;
    T* deg = reinterpret_cast<T*>(d_eg);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int k = k0 + acc_row(q, hi), i = i0 + r;
        if (i < N && k < N) {
            const int x = dir == 0 ? i : k, y = dir == 0 ? k : i;
            const int64_t idx = ((int64_t)b * N + x) * N + y;
            if (ta.biased) deg[idx * ta.ld + ta.e_off + h] = from_f32<T>(dE[q]);
            if (ta.gated) deg[idx * ta.ld + ta.g_off + h] = from_f32<T>(dG[q]);
        }
    }
}

// ---------------------------------------------------------------------------
// Staged third arm.  The per-lane gathers above touch one cache line per lane
// per value (48 instructions x 64 lines per wave).  Instead the WORKGROUP pulls
// the E/G columns of its HG heads and the mask for the pair region of one
// query-tile pass through LDS (8 pairs per wave instruction), and each wave
// then picks its head's tile in accumulator layout from LDS; the backward
// scatters dE/dG back the same way.  The staging area aliases the slab
// buffers (used strictly before / after the walk over j).
//   region of pass i0: inward  x in [i0,i0+32), y in [k0,k0+32NT)
//                      outward x in [k0,k0+32NT), y in [i0,i0+32)
// k0 = key origin of the staged region: 0 where all NT key tiles are staged at once, 32*kt with NT = 1 where they go
// through one by one (N > 64).
// row pitch + 4 bytes: lanes that differ in x hit different banks.
// ---------------------------------------------------------------------------
template <typename T, int HG, int NT>
struct ArmStage {
    static constexpr int kVals = 2 * HG;
    static constexpr int kPairBytes = kVals * (int)sizeof(T);
    static constexpr int kOffM = ((32 * NT * 32 * kPairBytes + 4 * 32 * NT + 15) / 16) * 16;
    static constexpr int kBytes = kOffM + 32 * NT * 32 * 4 + 4 * 32 * NT;
    __device__ static __forceinline__ int nx(int dir) { return dir == 0 ? 32 : 32 * NT; }
    __device__ static __forceinline__ int ny(int dir) { return dir == 0 ? 32 * NT : 32; }
    __device__ static __forceinline__ int pitch(int dir) { return ny(dir) * kPairBytes + 4; }
    __device__ static __forceinline__ int mpitch(int dir) { return ny(dir) * 4 + 4; }
};

template <typename T, int HG, int NT>
__device__ __forceinline__ void arm_stage_load(const ThirdArm& ta, int b, int dir, int g, int N, int i0, char* lds,
                                               int tid, int k0 = 0) {
    using A = ArmStage<T, HG, NT>;
    const int nx = A::nx(dir), ny = A::ny(dir), x0 = dir == 0 ? i0 : k0, y0 = dir == 0 ? k0 : i0;
    const int pitch = A::pitch(dir), mpitch = A::mpitch(dir);
    const T* eg = reinterpret_cast<const T*>(ta.eg);
    for (int idx = tid; idx < nx * ny * A::kVals; idx += HG * 64) {
        const int v = idx % A::kVals, p = idx / A::kVals, yy = p % ny, xx = p / ny;
        const int x = x0 + xx, y = y0 + yy;
        T val = from_f32<T>(0.f);
        if (x < N && y < N) {
            const bool is_e = v < HG;
            if (is_e ? ta.biased : ta.gated)
                val = eg[(((int64_t)b * N + x) * N + y) * ta.ld + (is_e ? ta.e_off + g * HG + v : ta.g_off + g * HG + v - HG)];
        }
        *reinterpret_cast<T*>(lds + xx * pitch + yy * A::kPairBytes + v * (int)sizeof(T)) = val;
    }
    for (int idx = tid; idx < nx * ny; idx += HG * 64) {
        const int yy = idx % ny, xx = idx / ny, x = x0 + xx, y = y0 + yy;
        float m = 0.f;
        if (x < N && y < N && ta.mask) m = ta.mask[((int64_t)b * N + x) * N + y];
        *reinterpret_cast<float*>(lds + A::kOffM + xx * mpitch + yy * 4) = m;
    }
}

// tile (query tile at i0, key tile kt of the staged region) of head `hh` of the group, accumulator layout
template <typename T, int HG, int NT, bool PAD_COLS_NEG_INF>
__device__ __forceinline__ void arm_stage_read(const ThirdArm& ta, const char* lds, int dir, int hh, int N, int r, int hi,
                                               int i0, int kt, float (&biasM)[16], float (&gate)[16], int k0 = 0) {
    using A = ArmStage<T, HG, NT>;
    const int pitch = A::pitch(dir), mpitch = A::mpitch(dir);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int kl = 32 * kt + acc_row(q, hi), k = k0 + kl, i = i0 + r;
        const bool valid = i < N && k < N;
        const int xx = dir == 0 ? r : kl, yy = dir == 0 ? kl : r;
        const char* pp = lds + xx * pitch + yy * A::kPairBytes;
        const float e = to_f32(*reinterpret_cast<const T*>(pp + hh * (int)sizeof(T)));
        const float gl = to_f32(*reinterpret_cast<const T*>(pp + (HG + hh) * (int)sizeof(T)));
        const float m = *reinterpret_cast<const float*>(lds + A::kOffM + xx * mpitch + yy * 4);
        biasM[q] = (k < N && (!PAD_COLS_NEG_INF || i < N)) ? e + m : -INFINITY;
        gate[q] = valid ? (ta.gated ? fast_sigmoid(gl + m) : 1.f) : 0.f;
    }
}

// (kt counts from the staged region's first key tile, as in arm_stage_read)
template <typename T, int HG, int NT>
__device__ __forceinline__ void arm_stage_put_grad(char* lds, int dir, int hh, int r, int hi, int kt,
                                                   const float (&dE)[16], const float (&dG)[16]) {
    using A = ArmStage<T, HG, NT>;
    const int pitch = A::pitch(dir);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int kl = 32 * kt + acc_row(q, hi);
        const int xx = dir == 0 ? r : kl, yy = dir == 0 ? kl : r;
        char* pp = lds + xx * pitch + yy * A::kPairBytes;
        *reinterpret_cast<T*>(pp + hh * (int)sizeof(T)) = from_f32<T>(dE[q]);
        *reinterpret_cast<T*>(pp + (HG + hh) * (int)sizeof(T)) = from_f32<T>(dG[q]);
    }
}

// Returns this thread's sum of the values it stored: idx % kVals is fixed per thread
// ((HG*64) % kVals == 0), i.e. a partial column sum of dE (v < HG) or dG of head g*HG + v % HG.
template <typename T, int HG, int NT>
__device__ __forceinline__ float arm_stage_store_grad(const ThirdArm& ta, void* d_eg, int b, int dir, int g, int N,
                                                      int i0, const char* lds, int tid, int k0 = 0) {
    using A = ArmStage<T, HG, NT>;
    static_assert((HG * 64) % A::kVals == 0, "a thread must own one E/G column");
    float part = 0.f;
    if (!(ta.biased || ta.gated)) return part;
    const int nx = A::nx(dir), ny = A::ny(dir), x0 = dir == 0 ? i0 : k0, y0 = dir == 0 ? k0 : i0;
    const int pitch = A::pitch(dir);
    T* deg = reinterpret_cast<T*>(d_eg);
#pragma nounroll
    for (int idx = tid; idx < nx * ny * A::kVals; idx += HG * 64) {
        const int v = idx % A::kVals, p = idx / A::kVals, yy = p % ny, xx = p / ny;
        const int x = x0 + xx, y = y0 + yy;
        const bool is_e = v < HG;
        if (x < N && y < N && (is_e ? ta.biased : ta.gated)) {
            const T val = *reinterpret_cast<const T*>(lds + xx * pitch + yy * A::kPairBytes + v * (int)sizeof(T));
            deg[(((int64_t)b * N + x) * N + y) * ta.ld + (is_e ? ta.e_off + g * HG + v : ta.g_off + g * HG + v - HG)] = val;
            part += to_f32(val);
        }
    }
    return part;
}

// Softmax over the NT key tiles of logits a lane holds in accumulator layout (lane column i, both lane halves), in place.
// A padding column (every logit -inf) gets weights of exactly 0: no exp(-inf + inf), no 0 * inf.
template <int NT>
__device__ __forceinline__ void tile_softmax(float (&p)[NT][16]) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) mx = fmaxf(mx, p[kt][q]);
    mx = fmaxf(mx, xhalf(mx));
    if (mx == -INFINITY) mx = 0.f;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            p[kt][q] = fast_exp(p[kt][q] - mx);
            sum += p[kt][q];
        }
    sum += xhalf(sum);
    const float inv = sum > 0.f ? fast_rcp(sum) : 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) p[kt][q] *= inv;
}

// ---------------------------------------------------------------------------
// Attention dropout (reference lib/tgt/layers/triplet.py:223-225, :242-244, :59-60: F.dropout on
// the gated weights).  Counter-based, so the backward recomputes the forward's pattern from the
// seed and nothing is stored.  Element (unit, i, k): `unit` numbers the (graph, direction, head
// [, shared node j]) the weights belong to; one hash word serves the pair (k even, k + 1):
//   word = mix32( mix32(seed_lo ^ mix32(unit)) + seed_hi + ((i*64 + k) >> 1) * 0x9e3779b9 )
//   keep(k even) = (word & 0xffff) >= thresh16,  keep(k odd) = (word >> 16) >= thresh16,
//   thresh16 = clamp(round(p * 65536), 1, 65535); kept weights are scaled by 1/(1-p).
// Word stride of a row: 64 for N <= 64 (as above).  With k >= 64 that index would alias (i, k) with (i+1, k-64), so the
// kernels for N > 64 (triplet_attention_kb.hip, triplet_aggregate_kb.hip) use ((i*128 + k) >> 1): `stride` below =
// kTriDropStrideKb.  Patterns for N <= 64 are unchanged.
// (tests/golden_util.py::triplet_dropout_keep restates it in numpy for the parity tests.)
// Returns the keep bits of the 16 accumulator elements of one lane: bit q <-> k = 32*kt + acc_row(q,hi).
// ---------------------------------------------------------------------------
constexpr int kTriDropStrideKb = 128;
struct TriDrop {
    uint32_t thresh16, seed_lo, seed_hi;
    float scale;
    bool on;
};
__device__ __forceinline__ TriDrop tri_drop(float p, uint64_t seed) {
    TriDrop d;
    d.on = p > 0.f;
    float t = rintf(p * 65536.f);
    t = t < 1.f ? 1.f : (t > 65535.f ? 65535.f : t);
    d.thresh16 = (uint32_t)t;
    d.seed_lo = (uint32_t)seed;
    d.seed_hi = (uint32_t)(seed >> 32);
    d.scale = d.on ? 1.f / (1.f - p) : 1.f;
    return d;
}
// The same with the registered device step counter (common.hpp, step_seed; the launchers pass seed_counter()) mixed into the seed:
// a replayed hipGraph draws a new pattern per replay, and forward and backward of one step agree.  p == 0: the counter is not read.
__device__ __forceinline__ TriDrop tri_drop(float p, uint64_t seed, const uint64_t* ctr) {
    return tri_drop(p, p > 0.f ? step_seed(seed, ctr) : seed);
}
__device__ __forceinline__ uint32_t tri_drop_bits(const TriDrop& d, uint32_t unit, int i, int kt, int hi, int stride = 64) {
    const uint32_t base = mix32(d.seed_lo ^ mix32(unit)) + d.seed_hi;
    uint32_t bits = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const int k = 32 * kt + acc_row(2 * w, hi);
        const uint32_t r = mix32(base + (uint32_t)((i * stride + k) >> 1) * 0x9e3779b9u);
        bits |= ((r & 0xffffu) >= d.thresh16 ? 1u : 0u) << (2 * w);
        bits |= ((r >> 16) >= d.thresh16 ? 1u : 0u) << (2 * w + 1);
    }
    return bits;
}
// the same bits transposed, for N > 64: lane = key k, bit q <-> i = i0 + acc_row(q, hi)
__device__ __forceinline__ uint32_t tri_drop_bits_t(const TriDrop& d, uint32_t unit, int i0, int k, int hi) {
    const uint32_t base = mix32(d.seed_lo ^ mix32(unit)) + d.seed_hi;
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + acc_row(q, hi);
        const uint32_t r = mix32(base + (uint32_t)((i * kTriDropStrideKb + k) >> 1) * 0x9e3779b9u);
        bits |= (((k & 1) ? (r >> 16) : (r & 0xffffu)) >= d.thresh16 ? 1u : 0u) << q;
    }
    return bits;
}
// the same elements in the 16 x 16 x 16 accumulator layout of triplet_attention16.hip: lane (query i, g = lane >> 4) holds keys
// k = 16*blk + 4g + q of key block `blk`, q = 0..3 -- two hash words per block and lane; bit q <-> key q.  N <= 64: stride 64.
// The word index (i*64 + k) >> 1 = (i*32 + 2g) + (8*blk + w) splits into a part of the lane and a part of the block, and the
// unit's base is the same in every lane, so a kernel keeps ONE vector register of generator state (tri_drop_lane16: fixed for the
// whole walk) and everything else in scalar ones (tri_drop_base: once per unit).
__device__ __forceinline__ uint32_t tri_drop_base(const TriDrop& d, uint32_t unit) { return mix32(d.seed_lo ^ mix32(unit)) + d.seed_hi; }
__device__ __forceinline__ uint32_t tri_drop_lane16(int i, int g) { return (uint32_t)(i * 32 + 2 * g) * 0x9e3779b9u; }
__device__ __forceinline__ uint32_t tri_drop_bits16(const TriDrop& d, uint32_t base, uint32_t lane16, int blk) {
    uint32_t bits = 0;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const uint32_t r = mix32((base + (uint32_t)(8 * blk + w) * 0x9e3779b9u) + lane16);
        bits |= ((r & 0xffffu) >= d.thresh16 ? 1u : 0u) << (2 * w);
        bits |= ((r >> 16) >= d.thresh16 ? 1u : 0u) << (2 * w + 1);
    }
    return bits;
}

// ---------------------------------------------------------------------------
// workgroup coordinates and slab sources of the triplet kernels
// ---------------------------------------------------------------------------
struct TriCtx {
    int b, dir, g, h, tile, N;
};
// blockIdx.x = ((b*2 + dir)*ngroups + g)*ntiles + tile.  ntiles = 1 where a workgroup owns all of (graph, direction, head
// group) (N <= 64); TILED: the number of 32-row tiles, where it owns one of them (N > 64).
template <typename T, int D, int HG, bool TILED = false>
__device__ __forceinline__ TriCtx tri_ctx(const tgt_triplet_attention_args& a, int wave) {
    TriCtx c;
    const int ngroups = a.H / HG, ntiles = TILED ? (a.N + 31) / 32 : 1;
    int bid = blockIdx.x;
    c.tile = bid % ntiles;
    bid /= ntiles;
    c.g = bid % ngroups;
    bid /= ngroups;
    c.dir = bid & 1;
    c.b = bid >> 1;
    c.h = c.g * HG + wave;
    c.N = a.N;
    return c;
}

// Units j of graph b a triplet ATTENTION kernel computes (tgt_hip.h, tgt_triplet_attention_*_counts): clamp(node_counts[b], 0, N).
// Units past it are not read or computed; their rows get the zeros a dropped graph gets.  Workgroup-uniform (b comes from
// blockIdx): one scalar load.  N keeps every stride, row bound and dropout unit index.
// RG (ragged) is a compile-time flag of every kernel that takes counts: a call without counts launches the RG = false
// instantiation, where n IS N and all of the count handling folds away -- the instruction streams of the kernels every caller
// without counts runs are the ones they were before the counts existed (hipcc's register allocation of these kernels moves with
// any added live scalar: profiles/tri_ragged_ab.txt).  Where even an unused kernel ARGUMENT moved the allocation (a longer
// argument segment lets hipcc widen its scalar loads), the counts are a trailing parameter pack `NC... nc`: empty without counts,
// so that instantiation has the argument list it always had; `const int32_t*` with them.
__device__ __forceinline__ const int32_t* tri_counts_ptr() { return nullptr; }
__device__ __forceinline__ const int32_t* tri_counts_ptr(const int32_t* p) { return p; }
// The same device for the step counter of attention dropout in tri_att_bwd2_kernel: its DROP instantiations take a TriSeedCtr
// AHEAD of the counts in that pack, the p == 0 instantiations keep the argument list they had.
struct TriSeedCtr {
    const uint64_t* p;
};
__device__ __forceinline__ const int32_t* tri_counts_ptr(TriSeedCtr) { return nullptr; }
__device__ __forceinline__ const int32_t* tri_counts_ptr(TriSeedCtr, const int32_t* p) { return p; }
__device__ __forceinline__ const uint64_t* tri_seed_ptr() { return nullptr; }
__device__ __forceinline__ const uint64_t* tri_seed_ptr(const int32_t*) { return nullptr; }
__device__ __forceinline__ const uint64_t* tri_seed_ptr(TriSeedCtr s) { return s.p; }
__device__ __forceinline__ const uint64_t* tri_seed_ptr(TriSeedCtr s, const int32_t*) { return s.p; }
// TGT_TRI_DROP_FAST (A/B): attention dropout inside tri_att_bwd2_kernel (N <= 32); 0: a backward with p > 0 is routed as before
// that kernel had it, to tri_att_bwd_kernel (triplet_attention_bwd2.hip).  Host logic only.
bool tri_drop_fast();
// TGT_TRI_DROP16 (A/B, default off): attention dropout inside the 16-wide-tile kernels for 33..64 nodes (the DROP instantiations of
// triplet_attention16.hip, same pack convention as above); unset / 0: a call with p > 0 at those sizes goes to the general kernels.
// Read per call.  Host logic only.
bool tri_drop16();
template <bool RG>
__device__ __forceinline__ int tri_node_count(const int32_t* node_counts, int b, int N) {
    if constexpr (RG) return min(max(node_counts[b], 0), N);
    else return N;
}

// Key-blocked kernels (triplet_attention_kb.hip) with TGT_TRI_COUNTS_KB: tiles of 32 rows at or past n rounded up to 32 hold
// padded nodes only and are skipped as query tiles, key blocks and owned tiles.
__device__ __forceinline__ int tri_count32(int n) { return (n + 31) & ~31; }
// zeros to rows [row0, row0 + 32) of the units j0 <= j < j1 of the slab tensors `bufs`: every unit of a tile that is not
// computed (a DropPath-dropped graph, a tile of padded nodes) or the padded units n..N-1 of one that is
template <typename G, typename... Bufs>
__device__ __forceinline__ void slab_zero_units(int j0, int j1, int row0, int N, int tid, const Bufs&... bufs) {
    for (int j = j0; j < j1; ++j) (slab_store_zero<G, 32>(bufs, j, row0, N, tid), ...);
}

__device__ __forceinline__ ThirdArm tri_third_arm(const tgt_triplet_attention_args& a, int dir) {
    return ThirdArm{a.eg[dir], a.ld_eg[dir], a.e_off[dir], a.g_off[dir], a.mask,
                    (a.flags & TGT_TRI_BIASED) != 0, (a.flags & TGT_TRI_GATED) != 0};
}

// The same for the triplet-aggregate kernels (both files), plus their third arm.  The decode is spelled out a second time on
// purpose: built on TriCtx (as a base or a member) or filled by a decode function shared with tri_ctx, every aggregate
// kernel, N <= 64 included, came out of hipcc with a different schedule and register assignment; this form compiles to the
// instruction streams the kernels were measured with.
struct AggCtx {
    int b, dir, g, h, N;
    ThirdArm ta;
    int tile;
};
template <int HG, bool TILED = false>
__device__ __forceinline__ AggCtx agg_ctx(const tgt_triplet_aggregate_args& a, int wave) {
    AggCtx c;
    const int ngroups = a.H / HG, ntiles = TILED ? (a.N + 31) / 32 : 1;
    int bid = blockIdx.x;
    c.tile = bid % ntiles;
    bid /= ntiles;
    c.g = bid % ngroups;
    bid /= ngroups;
    c.dir = bid & 1;
    c.b = bid >> 1;
    c.h = c.g * HG + wave;
    c.N = a.N;
    const bool use_mask = c.dir == 0 || (a.flags & TGT_TRI_MASK_OUT);
    c.ta = ThirdArm{a.eg[c.dir], a.ld_eg[c.dir], a.e_off[c.dir], a.g_off[c.dir], use_mask ? a.mask : nullptr,
                    true, (a.flags & TGT_TRI_GATED) != 0};
    return c;
}
// A graph DropPath dropped (tgt_hip.h, tgt_triplet_aggregate_*_skip: graph_scale[b] == 0): its workgroups read and compute
// nothing and write zeros to what they own.  Workgroup-uniform (b comes from blockIdx): one scalar load, tested before the first
// barrier.  The factors are a trailing parameter pack `GS... gs` of every aggregate kernel, as the attention kernels' counts
// (`NC... nc` above): a call without factors launches the instantiation with the empty pack, whose argument list and
// instruction stream are the ones the kernel had before the factors existed; with them the pack is one `const float*`, never null.
// The test sits behind `if constexpr (sizeof...(GS) > 0)`: the dead branch is not even instantiated without factors (merely
// folded away as dead code, it still moved the register allocation of every tri_agg_bwd_kernel).
__device__ __forceinline__ bool agg_dead(int b, const float* graph_scale) { return graph_scale[b] == 0.f; }
// zeros to the E/G gradient columns of this head group for the staged pair region of pass (i0, k0): the staged path of the live
// kernels (arm_stage_put_grad / arm_stage_store_grad) with a zero tile per head, so the ownership map of the store is theirs.
// Two barriers; `lds` is the stage.
template <typename T, int HG, int NT>
__device__ __forceinline__ void arm_stage_zero_grad(const ThirdArm& ta, void* d_eg, int b, int dir, int g, int N, int i0, char* lds,
                                                    int wave, int tid, int r, int hi, int k0 = 0) {
    float z[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) z[q] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) arm_stage_put_grad<T, HG, NT>(lds, dir, wave, r, hi, kt, z, z);
    __syncthreads();
    arm_stage_store_grad<T, HG, NT>(ta, d_eg, b, dir, g, N, i0, lds, tid, k0);
    __syncthreads();
}
// buffer-addressed slabs: rows k of V[j,k] (inward) / V[k,j] (outward) of this head group
template <typename T, int D, int HG>
__device__ __forceinline__ SlabBuf agg_v_slab(const void* tensor, int64_t ld, int off, const AggCtx& c) {
    const int64_t sz = sizeof(T), N = c.N;
    const uint32_t ldb = (uint32_t)(ld * sz);
    return SlabBuf{graph_rsrc(tensor, N * N * ld * sz, c.b), (uint32_t)((off + c.g * HG * D) * sz),
                   c.dir == 0 ? ldb : (uint32_t)N * ldb, c.dir == 0 ? (uint32_t)N * ldb : ldb};
}
// rows i of X[i,j] (the aggregate's output and its gradient)
template <typename T, int D, int HG>
__device__ __forceinline__ SlabBuf agg_o_slab(const void* tensor, int64_t ld, int off, const AggCtx& c) {
    const int64_t sz = sizeof(T), N = c.N;
    const uint32_t ldb = (uint32_t)(ld * sz);
    return SlabBuf{graph_rsrc(tensor, N * N * ld * sz, c.b), (uint32_t)((off + c.g * HG * D) * sz), (uint32_t)N * ldb, ldb};
}

}  // namespace tgt
