// Shared pieces of the 16-wide-tile node attention kernels (node_attention16.hip: whole key rows per query block;
// node_attention_kb.hip: key-blocked forward, all heads of a pair's 128-byte rows in one workgroup; node_attention_kb_bwd.hip: the
// backward of 65..128 nodes, key chunks of 64): operand fragments of
// v_mfma_f32_16x16x16, the 4 x 8 half-word transposes of the staging threads, 16-byte buffer accesses, the launch order.
#pragma once
#include "common.hpp"
#include "triplet_common.hpp"

namespace tgt {
namespace na16 {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
template <typename T> struct F4;
template <> struct F4<bf16_t> { typedef s16x4 type; };
template <> struct F4<f16_t> { typedef h16x4 type; };
template <typename T> using frag4_t = typename F4<T>::type;
template <typename T> inline constexpr bool kIsBf16 = false;
template <> inline constexpr bool kIsBf16<bf16_t> = true;

// C[m][n] += sum_kk A[m][kk] B[kk][n], kk in [0,16): lane l = (x = l & 15, g = l >> 4) supplies A[m = x][kk = 4g + t] /
// B[kk = 4g + t][n = x], t = 0..3, and holds C[m = 4g + q][n = x], q = 0..3
__device__ __forceinline__ f32x4 mma16(s16x4 a, s16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma16(h16x4 a, h16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }

template <typename T>
__device__ __forceinline__ frag4_t<T> pack4(const f32x4& v) {
    T t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = from_f32<T>(v[i]);
    frag4_t<T> f;
    __builtin_memcpy(&f, t, 8);
    return f;
}
template <typename T>
__device__ __forceinline__ uint2 pack4u(const float (&v)[4]) {
    T t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = from_f32<T>(v[i]);
    uint2 u;
    __builtin_memcpy(&u, t, 8);
    return u;
}
template <typename T>
__device__ __forceinline__ void unpack4(const uint2& u, float (&v)[4]) {
    T t[4];
    __builtin_memcpy(t, &u, 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = to_f32(t[i]);
}
template <typename T>
__device__ __forceinline__ frag4_t<T> ident4(int x, int g) {     // B[kk][n] = (kk == n)
    T t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = from_f32<T>(4 * g + i == x ? 1.f : 0.f);
    frag4_t<T> f;
    __builtin_memcpy(&f, t, 8);
    return f;
}
// half-wave / quarter-wave exchanges of the softmax statistics: lanes x, x + 16, x + 32, x + 48 hold one query
// (v_permlane16_swap / v_permlane32_swap: VALU, not the LDS crossbar -- common.hpp)
__device__ __forceinline__ float qsum(float v) {
    float a, b;
    lane_swap_pair<true>(v, a, b); v = a + b;
    lane_swap_pair<false>(v, a, b); return a + b;
}
__device__ __forceinline__ float qmax(float v) {
    float a, b;
    lane_swap_pair<true>(v, a, b); v = fmaxf(a, b);
    lane_swap_pair<false>(v, a, b); return fmaxf(a, b);
}

constexpr uint32_t kOob = 0x7ffffff0u;
// Ragged batches (tgt_hip.h, tgt_node_attention_*_counts): the loaders below have a compile-time flag RG (of the class) and take the graph's node
// count n as a last argument.  With RG, rows and pairs at or past n are not loaded (offset kOob: zeros come back, no memory is
// touched) and their mask entries are the -inf of the keys past N; N keeps every stride.  Without RG (the default: every caller
// without counts) n does not appear in the code at all -- the task's row and pair indices come from an opaque thread index, so a
// comparison with a constant would NOT fold away.

__device__ __forceinline__ uint4 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void buf_st16(__amdgpu_buffer_rsrc_t r, uint32_t off, const uint4& v) {
    const u32x4_t d = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)off, 0, 0);
}
__device__ __forceinline__ uint32_t dw(const uint4& v, int p) { return p == 0 ? v.x : p == 1 ? v.y : p == 2 ? v.z : v.w; }
// v[i] = the 8 halves (heads 0..7) of row i  ->  o[j] = the 4 halves (rows 0..3) of head j
__device__ __forceinline__ void tr4x8(const uint4 (&v)[4], uint2 (&o)[8]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        o[2 * p].x = __builtin_amdgcn_perm(dw(v[1], p), dw(v[0], p), 0x05040100u);
        o[2 * p].y = __builtin_amdgcn_perm(dw(v[3], p), dw(v[2], p), 0x05040100u);
        o[2 * p + 1].x = __builtin_amdgcn_perm(dw(v[1], p), dw(v[0], p), 0x07060302u);
        o[2 * p + 1].y = __builtin_amdgcn_perm(dw(v[3], p), dw(v[2], p), 0x07060302u);
    }
}
// a[j] = the 4 halves (rows 0..3) of head j  ->  the 8 halves of row i
__device__ __forceinline__ uint4 tr8x4_row(const uint2 (&a)[8], int i) {
    const uint32_t sel = (i & 1) ? 0x07060302u : 0x05040100u;
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = (i >> 1) ? a[j].y : a[j].x;
    return make_uint4(__builtin_amdgcn_perm(s[1], s[0], sel), __builtin_amdgcn_perm(s[3], s[2], sel),
                      __builtin_amdgcn_perm(s[5], s[4], sel), __builtin_amdgcn_perm(s[7], s[6], sel));
}
// eight 8-byte LDS accesses of a staging thread: head j at p + j * head_pitch
__device__ __forceinline__ void lds_put8x8(char* p, int head_pitch, const uint2 (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<uint2*>(p + j * head_pitch) = o[j];
}
__device__ __forceinline__ void lds_get8x8(const char* p, int head_pitch, uint2 (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = *reinterpret_cast<const uint2*>(p + j * head_pitch);
}

// Unit order: XCD x (= block index & 7) owns the graphs b = x mod 8 and hands their units to its workgroups in order, so that the
// units of one graph (the head groups of a query block share its 128-byte E / G rows, the query blocks its K / V rows) run
// together on one XCD.
__device__ __forceinline__ bool unit_of_block(int B, int per_graph, int& b, int& sub) {
    const int x = blockIdx.x & 7, t = blockIdx.x >> 3;
    const int nt = ((B - x + 7) >> 3) * per_graph;
    b = (t / per_graph) * 8 + x;
    sub = t % per_graph;
    return t < nt;
}

// ---- staging of the 8-heads-per-workgroup kernels (node_attention16.hip, node_attention_kb_bwd.hip): workgroup = 8 waves, wave = head
constexpr int HG = 8, kThreads = HG * 64;

struct Unit { int b, hg; };

// ---- pair planes.  A staging task = (plane, query l, key quad mq): the 16-byte records of pairs (16 qb + l, m0 + 4 mq + i), i < 4
// (m0: the first key of the staged key range; 0 where the planes hold every key).
// `chan[plane]` = element offset of this head group's 8 channels inside a pair's row of the tensor (ld elements per pair).
template <typename T, int NQ, int PLANES, bool RG = false>
struct PairIO {
    static constexpr int NK = 16 * NQ, MQ = NK / 4, kPerPlane = 16 * MQ, kTasks = PLANES * kPerPlane;
    static constexpr int kIters = (kTasks + kThreads - 1) / kThreads;
    uint4 v[kIters][4];

    __device__ __forceinline__ void issue(const void* x, int64_t ld, const int (&chan)[PLANES], int N, int b, int qb, int tid, int m0 = 0,
                                          int n = 0) {
        asm volatile("" : "+v"(tid));            // (opaque: the task's addresses are recomputed here, not kept live across the query-block walk)
        const __amdgpu_buffer_rsrc_t rs = graph_rsrc(x, (int64_t)N * N * ld * sizeof(T), b);
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            const int task = it * kThreads + tid, plane = task / kPerPlane, r = task % kPerPlane, l = r / MQ, mq = r % MQ, q = 16 * qb + l;
            int ch = chan[0];
#pragma unroll
            for (int p = 1; p < PLANES; ++p) ch = plane == p ? chan[p] : ch;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + 4 * mq + i;
                bool ok;
                if constexpr (RG) ok = x && task < kTasks && q < n && m < n;         // (n <= N)
                else ok = x && task < kTasks && q < N && m < N;
                v[it][i] = buf_ld16(rs, ok ? (uint32_t)(((int64_t)(q * N + m) * ld + ch) * (int64_t)sizeof(T)) : kOob);
            }
        }
    }
    template <int PITCH>
    __device__ __forceinline__ void land(char* const (&planes)[PLANES], int tid) {
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            const int task = it * kThreads + tid, plane = task / kPerPlane, r = task % kPerPlane, l = r / MQ, mq = r % MQ;
            char* base = planes[0];
#pragma unroll
            for (int p = 1; p < PLANES; ++p) base = plane == p ? planes[p] : base;
            uint2 o[8];
            tr4x8(v[it], o);
            if (task < kTasks) lds_put8x8(base + l * PITCH + mq * 8, NK * 2, o);
        }
    }
    // LDS planes -> the tensor
    template <int PITCH>
    static __device__ __forceinline__ void store(const char* const (&planes)[PLANES], void* x, int64_t ld, const int (&chan)[PLANES], int N, int b,
                                                 int qb, int tid, int m0 = 0) {
        asm volatile("" : "+v"(tid));            // (opaque: the task's addresses are recomputed here, not kept live across the query-block walk)
        const __amdgpu_buffer_rsrc_t rs = graph_rsrc(x, (int64_t)N * N * ld * sizeof(T), b);
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            const int task = it * kThreads + tid, plane = task / kPerPlane, r = task % kPerPlane, l = r / MQ, mq = r % MQ, q = 16 * qb + l;
            const char* base = planes[0];
            int ch = chan[0];
#pragma unroll
            for (int p = 1; p < PLANES; ++p) { base = plane == p ? planes[p] : base; ch = plane == p ? chan[p] : ch; }
            if (task < kTasks) {
                uint2 o[8];
                lds_get8x8(base + l * PITCH + mq * 8, NK * 2, o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + 4 * mq + i;
                    const bool ok = q < N && m < N;
                    buf_st16(rs, ok ? (uint32_t)(((int64_t)(q * N + m) * ld + ch) * (int64_t)sizeof(T)) : kOob, tr8x4_row(o, i));
                }
            }
        }
    }
};

// ---- node rows.  A staging task = (segment, row, d quad dq): the 16-byte (8 heads) records of (row, d = 4 dq + i), i < 4, of a
// (B, N, ld) tensor whose row holds [d][H heads] from element `off[segment]`.  Segment s covers `rows[s]` rows from row0[s] into region[s].
template <typename T, int D, int SEGS, int MAXROWS, bool RG = false>
struct NodeIO {
    static constexpr int DQ = D / 4, kTasks = MAXROWS * DQ, kIters = (kTasks + kThreads - 1) / kThreads;
    uint4 v[kIters][4];

    static __device__ __forceinline__ void decode(int task, const int (&rows)[SEGS], int& seg, int& row, int& dq) {
        int r = task / DQ;
        dq = task % DQ;
        seg = 0;
#pragma unroll
        for (int s = 0; s + 1 < SEGS; ++s)
            if (seg == s && r >= rows[s]) { r -= rows[s]; seg = s + 1; }
        row = r;
    }
    __device__ __forceinline__ void issue(const void* x, int64_t ld, const int (&off)[SEGS], const int (&rows)[SEGS], const int (&row0)[SEGS], int N,
                                          int H, const Unit& u, int tid, int n = 0) {
        asm volatile("" : "+v"(tid));            // (opaque: the task's addresses are recomputed here, not kept live across the query-block walk)
        const __amdgpu_buffer_rsrc_t rs = graph_rsrc(x, (int64_t)N * ld * sizeof(T), u.b);
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            int seg, row, dq;
            decode(it * kThreads + tid, rows, seg, row, dq);
            int o = off[0], r0 = row0[0], nr = rows[0];
#pragma unroll
            for (int s = 1; s < SEGS; ++s) { o = seg == s ? off[s] : o; r0 = seg == s ? row0[s] : r0; nr = seg == s ? rows[s] : nr; }
            bool ok;
            if constexpr (RG) ok = x && row < nr && r0 + row < n;                    // (n <= N)
            else ok = x && row < nr && r0 + row < N;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                v[it][i] = buf_ld16(rs, ok ? (uint32_t)(((int64_t)(r0 + row) * ld + o + (4 * dq + i) * H + u.hg * HG) * (int64_t)sizeof(T)) : kOob);
        }
    }
    template <int PITCH>
    __device__ __forceinline__ void land(char* const (&region)[SEGS], const int (&rows)[SEGS], int tid) {
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            int seg, row, dq;
            decode(it * kThreads + tid, rows, seg, row, dq);
            char* base = region[0];
            int nr = rows[0];
#pragma unroll
            for (int s = 1; s < SEGS; ++s) { base = seg == s ? region[s] : base; nr = seg == s ? rows[s] : nr; }
            uint2 o[8];
            tr4x8(v[it], o);
            if (row < nr) lds_put8x8(base + row * PITCH + dq * 8, D * 2, o);
        }
    }
    template <int PITCH>
    static __device__ __forceinline__ void store(const char* const (&region)[SEGS], void* x, int64_t ld, const int (&off)[SEGS], const int (&rows)[SEGS],
                                                 const int (&row0)[SEGS], int N, int H, const Unit& u, int tid) {
        asm volatile("" : "+v"(tid));            // (opaque: the task's addresses are recomputed here, not kept live across the query-block walk)
        const __amdgpu_buffer_rsrc_t rs = graph_rsrc(x, (int64_t)N * ld * sizeof(T), u.b);
#pragma unroll
        for (int it = 0; it < kIters; ++it) {
            int seg, row, dq;
            decode(it * kThreads + tid, rows, seg, row, dq);
            const char* base = region[0];
            int o = off[0], r0 = row0[0], nr = rows[0];
#pragma unroll
            for (int s = 1; s < SEGS; ++s) {
                base = seg == s ? region[s] : base; o = seg == s ? off[s] : o; r0 = seg == s ? row0[s] : r0; nr = seg == s ? rows[s] : nr;
            }
            if (row < nr) {
                uint2 t[8];
                lds_get8x8(base + row * PITCH + dq * 8, D * 2, t);
                const bool ok = r0 + row < N;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    buf_st16(rs, ok ? (uint32_t)(((int64_t)(r0 + row) * ld + o + (4 * dq + i) * H + u.hg * HG) * (int64_t)sizeof(T)) : kOob,
                             tr8x4_row(t, i));
            }
        }
    }
};

// mask tile of the query block (keys from m0): pairs past N get -inf (weight exactly 0, gate sigmoid(-inf) = 0)
template <int NQ, int PITCH, bool RG = false>
__device__ __forceinline__ void mask_load(char* lds_m, const tgt_node_attention_args& a, int b, int qb, int tid, int m0 = 0, int n = 0) {
    constexpr int NK = 16 * NQ, MQ = NK / 4;
    const int N = a.N;
    asm volatile("" : "+v"(tid));
    const __amdgpu_buffer_rsrc_t rs = graph_rsrc(a.mask, (int64_t)N * N * 4, b);
    for (int task = tid; task < 16 * MQ; task += kThreads) {
        const int l = task / MQ, mq = task % MQ, q = 16 * qb + l;
        float mk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + 4 * mq + i;
            bool ok;
            if constexpr (RG) ok = q < n && m < n;                                   // (n <= N)
            else ok = q < N && m < N;
            const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ok ? (q * N + m) * 4 : (int)kOob, 0, 0));
            mk[i] = ok ? v : -INFINITY;
        }
        *reinterpret_cast<float4*>(lds_m + l * PITCH + mq * 16) = make_float4(mk[0], mk[1], mk[2], mk[3]);
    }
}

// operand fragment of head hh from a node region: lane (x, g) holds X[row][d = 4g + t], t = 0..3 (0 past D)
template <typename T, int D, int PITCH>
__device__ __forceinline__ frag4_t<T> node_frag(const char* region, int row, int g, int hh) {
    const int gg = 4 * g < D ? g : 0;
    uint2 u = *reinterpret_cast<const uint2*>(region + row * PITCH + hh * (D * 2) + gg * 8);
    if (4 * g >= D) u = make_uint2(0u, 0u);
    frag4_t<T> f;
    __builtin_memcpy(&f, &u, 8);
    return f;
}
// transposed result X^T[d = 4g + q][row] into head hh of a node region
template <typename T, int D, int PITCH>
__device__ __forceinline__ void node_put(char* region, const f32x4& acc, int row, int g, int hh) {
    const float v[4] = {acc[0], acc[1], acc[2], acc[3]};
    if (4 * g < D) *reinterpret_cast<uint2*>(region + row * PITCH + hh * (D * 2) + g * 8) = pack4u<T>(v);
}

}  // namespace na16
}  // namespace tgt
