// TriangularUpdate core on staged matrix-core tiles (gfx950), 16-bit, N <= 64.  Math: the header of triangular_update.hip
// (reference lib/tgt/layers/triplet.py:156-170).  That kernel gives one lane per (pair, head) and gates all four operands again
// in every k iteration; here every operand element is gated ONCE, while it is staged into LDS:
//
//   workgroup = (graph b, group of 4 heads, direction).  Per head it keeps N x N planes in LDS in the element type (rows padded
//   to NP = 32 / 64, row stride NP + 8 elements); a plane holds X[x][y] = sigmoid(gate[x,y] + M[x,y]) * lin[x,y] -- the mask
//   index is the element's own pair in all four planes ([a,k] inward, [k,a] outward) -- or, stored transposed, X[y][x].
//   Both operands of v_mfma_f32_32x32x16 want the contraction index contiguous, so every product is P_a . P_b^T of two planes:
//     forward   O_in  = E_in . V_in^T                      O_out = E_out^T . V_out          (outward planes stored transposed)
//     backward  dE_in = dO_in . (V_in^T)^T                 dV_in  = dO_in^T . (E_in^T)^T    (V_in, E_in, one dO copy transposed)
//               dE_out = V_out . dO_out^T                  dV_out = E_out . (dO_out^T)^T    (one dO copy transposed)
//   then, in the backward, the split into gate and linear gradients with the gate recomputed from the operand in global memory.
//   One wave per 32 x 32 result tile, four heads' accumulators per lane: the four heads of a pair leave as one 8-byte store.
//
// Rows and columns of a plane past N are WRITTEN as zeros (never left as they were): a stale NaN times a zero gate would be NaN.
// A closed position contributes exactly 0: sigmoid(finfo.min + g) = rcp(1 + inf) = 0.  No atomics; every sum in a fixed order.
//
// Ragged batches (tgt_hip.h, tgt_triangular_update_tiled_*_counts).  The per-graph node counts are a trailing parameter pack
// `NC... nc` of both kernels (the convention of triplet_common.hpp): empty without counts -- that instantiation has the argument
// list and the instruction stream it always had -- `const int32_t*` with them.  n = clamp(node_counts[b], 0, N) is uniform per
// workgroup (b comes from blockIdx), so every __syncthreads() stays outside anything that depends on it.  With counts only the
// real block [0, n) x [0, n) of a plane is loaded (the rest of the NP x NP plane is zeros, as past N), the contraction runs over
// ceil(n / 16) chunks, and a result tile whose first row or column is at or past n is not multiplied; every output position
// inside [0, N) x [0, N) is still stored, zeros at a pair with a node >= n, and nothing is read there -- not the operands, not
// the mask, not d_out.  N keeps every stride and bound.
#include "common.hpp"

namespace tgt {

namespace {

constexpr int TT_HG = 4;          // heads per workgroup (8-byte global accesses: 4 x 16 bit)

struct TriTiledArgs {
    const void* e4; const void* v4; const float* mask; void* out;
    const void* d_out; void* d_e4; void* d_v4;
    int64_t ld_e, ld_v, ld_de, ld_dv;
    int B, N, H;
};

template <typename T>
__device__ __forceinline__ void ld4(const T* p, float (&f)[TT_HG]) {
    const uint2 raw = *reinterpret_cast<const uint2*>(p);
    T t[TT_HG];
    __builtin_memcpy(t, &raw, 8);
#pragma unroll
    for (int h = 0; h < TT_HG; ++h) f[h] = to_f32(t[h]);
}
template <typename T>
__device__ __forceinline__ void st4(T* p, const float (&f)[TT_HG]) {
    T t[TT_HG];
#pragma unroll
    for (int h = 0; h < TT_HG; ++h) t[h] = from_f32<T>(f[h]);
    uint2 raw;
    __builtin_memcpy(&raw, t, 8);
    *reinterpret_cast<uint2*>(p) = raw;
}

// TT_HG planes (consecutive, NP x (NP + 8) each) from the rows of one graph: element [x][y] (transposed: [y][x]) of head h is
// sigmoid(src[pair, col_gate + h] + mask[pair]) * src[pair, col_lin + h], pair = x*N + y; col_lin < 0: src[pair, col_gate + h] as
// it is (a gradient plane).  Everything at or past n (the graph's node count; N without counts): zero, and not read.
template <typename T, int NP>
__device__ __forceinline__ void stage_planes(T* planes, const T* src, int64_t ld, int col_gate, int col_lin, const float* mask,
                                             int N, int n, bool transposed) {
    constexpr int LD = NP + 8, PL = NP * LD;
    for (int p = threadIdx.x; p < NP * NP; p += blockDim.x) {
        const int x = p / NP, y = p % NP;
        float val[TT_HG];
#pragma unroll
        for (int h = 0; h < TT_HG; ++h) val[h] = 0.f;
        if (x < n && y < n) {
            const int64_t pair = (int64_t)x * N + y;
            const T* row = src + pair * ld;
            ld4(row + col_gate, val);
            if (col_lin >= 0) {
                float lin[TT_HG];
                ld4(row + col_lin, lin);
                const float m = mask[pair];
#pragma unroll
                for (int h = 0; h < TT_HG; ++h) val[h] = fast_sigmoid(val[h] + m) * lin[h];
            }
        }
        const int at = transposed ? y * LD + x : x * LD + y;
#pragma unroll
        for (int h = 0; h < TT_HG; ++h) planes[h * PL + at] = from_f32<T>(val[h]);
    }
}

// acc[h][m][n] = sum_k A_h[tm*32 + m][k] * B_h[tn*32 + n][k], k < 16*kchunks, for the TT_HG heads of two plane groups
template <typename T, int NP>
__device__ __forceinline__ void tile_products(const T* pa, const T* pb, int tm, int tn, int kchunks, f32x16 (&acc)[TT_HG]) {
    constexpr int LD = NP + 8, PL = NP * LD;
    const int lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int h = 0; h < TT_HG; ++h) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[h][q] = 0.f;
        const T* ra = pa + h * PL + (tm * 32 + r) * LD + 8 * hi;
        const T* rb = pb + h * PL + (tn * 32 + r) * LD + 8 * hi;
        for (int kc = 0; kc < kchunks; ++kc)
            acc[h] = mma32(load_frag<T>(ra + kc * 16), load_frag<T>(rb + kc * 16), acc[h]);
    }
}

__device__ __forceinline__ const int32_t* tt_counts_ptr() { return nullptr; }
__device__ __forceinline__ const int32_t* tt_counts_ptr(const int32_t* p) { return p; }
// nodes of graph b the workgroup computes: clamp(node_counts[b], 0, N) (one scalar load); N without counts
template <bool RG>
__device__ __forceinline__ int tt_node_count(const int32_t* node_counts, int b, int N) {
    if constexpr (RG) return min(max(node_counts[b], 0), N);
    else return N;
}
template <typename T, int NP, typename... NC>
__global__ void __launch_bounds__(256) tri_tiled_fwd_kernel(const TriTiledArgs a, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char tt_smem[];
    constexpr int LD = NP + 8, PL = NP * LD, NT = NP / 32;
    T* pa = reinterpret_cast<T*>(tt_smem);
    T* pb = pa + TT_HG * PL;
    const int N = a.N, H = a.H, groups = H / TT_HG;
    const int dir = blockIdx.x & 1, hg = (blockIdx.x >> 1) % groups, b = (blockIdx.x >> 1) / groups;
    const int h0 = hg * TT_HG;
    const int64_t gbase = (int64_t)b * N * N;
    const float* mask = a.mask + gbase;
    const int n = tt_node_count<RG>(tt_counts_ptr(nc...), b, N);
    stage_planes<T, NP>(pa, reinterpret_cast<const T*>(a.e4) + gbase * a.ld_e, a.ld_e, dir * 2 * H + h0, dir * 2 * H + H + h0, mask, N, n, dir == 1);
    stage_planes<T, NP>(pb, reinterpret_cast<const T*>(a.v4) + gbase * a.ld_v, a.ld_v, dir * 2 * H + h0, dir * 2 * H + H + h0, mask, N, n, dir == 1);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5;
    const int kchunks = (n + 15) / 16;
    T* out = reinterpret_cast<T*>(a.out) + gbase * 2 * H + dir * H + h0;
    for (int t = wave; t < NT * NT; t += 4) {
        const int tm = t / NT, tn = t % NT;
        if (tm * 32 >= N || tn * 32 >= N) continue;
        const int c = tn * 32 + r;
        if (RG && (tm * 32 >= n || tn * 32 >= n)) {      // (uniform per wave) a tile of padded nodes only: zeros, nothing multiplied
            const float zero[TT_HG] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = tm * 32 + acc_row(q, hi);
                if (m < N && c < N) st4(out + ((int64_t)m * N + c) * 2 * H, zero);
            }
            continue;
        }
        f32x16 acc[TT_HG];
        tile_products<T, NP>(pa, pb, tm, tn, kchunks, acc);      // (positions at or past n inside a live tile: sums over zero planes, +0)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = tm * 32 + acc_row(q, hi);
            if (m < N && c < N) {
                float o[TT_HG];
#pragma unroll
                for (int h = 0; h < TT_HG; ++h) o[h] = acc[h][q];
                st4(out + ((int64_t)m * N + c) * 2 * H, o);
            }
        }
    }
}

template <typename T, int NP, typename... NC>
__global__ void __launch_bounds__(256) tri_tiled_bwd_kernel(const TriTiledArgs a, NC... nc) {
    constexpr bool RG = sizeof...(NC) > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char tt_smem[];
    constexpr int LD = NP + 8, PL = NP * LD, NT = NP / 32;
    T* p0 = reinterpret_cast<T*>(tt_smem);
    T* p1 = p0 + TT_HG * PL;
    T* p2 = p1 + TT_HG * PL;
    T* p3 = p2 + TT_HG * PL;
    const int N = a.N, H = a.H, groups = H / TT_HG;
    const int dir = blockIdx.x & 1, hg = (blockIdx.x >> 1) % groups, b = (blockIdx.x >> 1) / groups;
    const int h0 = hg * TT_HG;
    const int64_t gbase = (int64_t)b * N * N;
    const float* mask = a.mask + gbase;
    const T* e = reinterpret_cast<const T*>(a.e4) + gbase * a.ld_e;
    const T* v = reinterpret_cast<const T*>(a.v4) + gbase * a.ld_v;
    const T* dO = reinterpret_cast<const T*>(a.d_out) + gbase * 2 * H;
    const int cg = dir * 2 * H + h0, cl = cg + H, co = dir * H + h0;
    const int n = tt_node_count<RG>(tt_counts_ptr(nc...), b, N);
    if (dir == 0) {
        stage_planes<T, NP>(p0, dO, 2 * H, co, -1, mask, N, n, false);       // dE_in [i,k] = sum_j dO_in[i,j] V_in[j,k]
        stage_planes<T, NP>(p1, v, a.ld_v, cg, cl, mask, N, n, true);
        stage_planes<T, NP>(p2, dO, 2 * H, co, -1, mask, N, n, true);        // dV_in [j,k] = sum_i dO_in[i,j] E_in[i,k]
        stage_planes<T, NP>(p3, e, a.ld_e, cg, cl, mask, N, n, true);
    } else {
        stage_planes<T, NP>(p0, v, a.ld_v, cg, cl, mask, N, n, false);       // dE_out[k,i] = sum_j V_out[k,j] dO_out[i,j]
        stage_planes<T, NP>(p1, dO, 2 * H, co, -1, mask, N, n, false);
        stage_planes<T, NP>(p2, e, a.ld_e, cg, cl, mask, N, n, false);       // dV_out[k,j] = sum_i E_out[k,i] dO_out[i,j]
        stage_planes<T, NP>(p3, dO, 2 * H, co, -1, mask, N, n, true);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5;
    const int kchunks = (n + 15) / 16;
    for (int job = wave; job < 2 * NT * NT; job += 4) {
        const int prod = job / (NT * NT), t = job % (NT * NT), tm = t / NT, tn = t % NT;
        if (tm * 32 >= N || tn * 32 >= N) continue;
        const bool tile_live = !RG || (tm * 32 < n && tn * 32 < n);      // (uniform per wave; a tile of padded nodes only is not multiplied)
        f32x16 acc[TT_HG];
        if (tile_live) tile_products<T, NP>(prod ? p2 : p0, prod ? p3 : p1, tm, tn, kchunks, acc);
        // the result of product 0 is the gradient of the gated E element at pair (m, n), of product 1 that of the gated V element
        const T* src = prod ? v : e;
        const int64_t ld_s = prod ? a.ld_v : a.ld_e, ld_d = prod ? a.ld_dv : a.ld_de;
        T* dst = reinterpret_cast<T*>(prod ? a.d_v4 : a.d_e4) + gbase * ld_d;
        const int c = tn * 32 + r;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = tm * 32 + acc_row(q, hi);
            if (m < N && c < N) {
                const int64_t pair = (int64_t)m * N + c;
                float g[TT_HG], l[TT_HG], dg[TT_HG], dl[TT_HG];
                if (RG && !(tile_live && m < n && c < n)) {      // a pair with a padded node: zeros, operand and mask not read
#pragma unroll
                    for (int h = 0; h < TT_HG; ++h) dg[h] = dl[h] = 0.f;
                    st4(dst + pair * ld_d + cg, dg);
                    st4(dst + pair * ld_d + cl, dl);
                    continue;
                }
                ld4(src + pair * ld_s + cg, g);
                ld4(src + pair * ld_s + cl, l);
                const float mk = mask[pair];
#pragma unroll
                for (int h = 0; h < TT_HG; ++h) {
                    const float s = fast_sigmoid(g[h] + mk), d = acc[h][q];
                    dg[h] = d * l[h] * s * (1.f - s);
                    dl[h] = d * s;
                }
                st4(dst + pair * ld_d + cg, dg);
                st4(dst + pair * ld_d + cl, dl);
            }
        }
    }
}

template <typename T, int NP, typename... NC>
int tri_tiled_launch(const TriTiledArgs& a, bool bwd, hipStream_t st, NC... nc) {
    const int grid = a.B * (a.H / TT_HG) * 2;
    const int lds = (bwd ? 4 : 2) * TT_HG * NP * (NP + 8) * (int)sizeof(T);
    if (!bwd) return launch_lds<tri_tiled_fwd_kernel<T, NP, NC...>>("tri_tiled_fwd_kernel", dim3(grid), dim3(256), lds, st, a, nc...);
    return launch_lds<tri_tiled_bwd_kernel<T, NP, NC...>>("tri_tiled_bwd_kernel", dim3(grid), dim3(256), lds, st, a, nc...);
}
template <typename T, typename... NC>
int tri_tiled_dispatch(const TriTiledArgs& a, bool bwd, hipStream_t st, NC... nc) {
    return a.N <= 32 ? tri_tiled_launch<T, 32>(a, bwd, st, nc...) : tri_tiled_launch<T, 64>(a, bwd, st, nc...);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int triangular_update_tiled_supported(int N, int H, int dtype) {
    return (dtype == TGT_BF16 || dtype == TGT_F16) && N >= 1 && N <= 64 && H >= TT_HG && H <= 64 && H % TT_HG == 0;
}

int triangular_update_tiled_run(const void* e4, int64_t ld_e, const void* v4, int64_t ld_v, const float* mask, void* out,
                                const void* d_out, void* d_e4, int64_t ld_de, void* d_v4, int64_t ld_dv, int B, int N, int H,
                                int dtype, bool bwd, const int32_t* node_counts, hipStream_t st) {
    const char* what = bwd ? "triangular update (tiled) bwd" : "triangular update (tiled) fwd";
    if (B < 0 || N < 0 || H <= 0) return set_error(TGT_ERR_INVALID, "%s: bad size", what);
    if (dtype != TGT_F32 && dtype != TGT_BF16 && dtype != TGT_F16) return set_error(TGT_ERR_INVALID, "%s: bad dtype %d", what, dtype);
    if (!triangular_update_tiled_supported(N > 0 ? N : 1, H, dtype))
        return set_error(TGT_ERR_UNSUPPORTED, "%s: N = %d, H = %d, dtype %d (16-bit, N <= 64, H a multiple of %d up to 64)", what, N, H, dtype, TT_HG);
    if (B == 0 || N == 0) return TGT_OK;
    if ((int64_t)B * (H / TT_HG) * 2 > 0x7fffffffLL) return set_error(TGT_ERR_UNSUPPORTED, "%s: too many workgroups", what);
    if (!e4 || !v4 || !mask) return set_error(TGT_ERR_INVALID, "%s: null tensor", what);
    if (!bwd && !out) return set_error(TGT_ERR_INVALID, "%s: null out", what);
    if (bwd && (!d_out || !d_e4 || !d_v4)) return set_error(TGT_ERR_INVALID, "%s: null gradient tensor", what);
    const int64_t lds[4] = {ld_e, ld_v, bwd ? ld_de : ld_e, bwd ? ld_dv : ld_v};
    for (int64_t ld : lds)
        if (ld < 4 * (int64_t)H || ld % 8) return set_error(TGT_ERR_INVALID, "%s: row stride %lld (at least 4H, a multiple of 8)", what, (long long)ld);
    const void* ptrs[5] = {e4, v4, bwd ? d_out : out, bwd ? d_e4 : out, bwd ? d_v4 : out};
    for (const void* p : ptrs)
        if (!aligned16(p)) return set_error(TGT_ERR_INVALID, "%s: tensor not 16-byte aligned", what);
    if (reinterpret_cast<uintptr_t>(mask) & 3) return set_error(TGT_ERR_INVALID, "%s: mask not 4-byte aligned", what);
    if (reinterpret_cast<uintptr_t>(node_counts) & 3) return set_error(TGT_ERR_INVALID, "%s: node_counts not 4-byte aligned", what);
    TriTiledArgs a = {e4, v4, mask, out, d_out, d_e4, d_v4, ld_e, ld_v, ld_de, ld_dv, B, N, H};
    if (node_counts) return dtype == TGT_BF16 ? tri_tiled_dispatch<bf16_t>(a, bwd, st, node_counts) : tri_tiled_dispatch<f16_t>(a, bwd, st, node_counts);
    return dtype == TGT_BF16 ? tri_tiled_dispatch<bf16_t>(a, bwd, st) : tri_tiled_dispatch<f16_t>(a, bwd, st);
}

}  // namespace tgt
