// tgt_edge_live_tiles: which 32-row tiles of the (B*N*N, C) edge rows of a ragged batch hold a real row -- gfx950.
//
// Row r of an edge tensor is the pair (b, i, j) = (r / N^2, (r % N^2) / N, r % N); it is DEAD when i >= n_b or j >= n_b with
// n_b = clamp(node_counts[b], 0, N): padding of graph b.  Tile t = rows [32 t, 32 t + 32); it is dead when every one of its
// rows is dead or at / past M = B N^2.  The persistent row kernels (edge_gemm.hip, edge_glu.hip: tgt_edge_linear_live) walk
//     tiles[0]                 number of live tiles L
//     tiles[1 .. L]            the live tile indices, ascending
//     tiles[L + 1 .. T]        the dead tile indices, ascending          (T = ceil(M / 32))
// ONE workgroup builds the list, so that both halves come out in order without a second launch: thread k owns the contiguous
// range of tiles [k c, (k + 1) c), counts its live ones, the workgroup takes the exclusive prefix sums of the 1024 counts, and
// every thread writes its range behind the live (dead) tiles of the ranges in front of it.  Deterministic, nothing read on the
// host: the launch can be captured in a hipGraph.
//
// Liveness of a tile without looking at 32 rows: inside one node row (b, i, .) the rows are ordered by j, so the piece of the
// tile that lies in that node row holds a live row iff its FIRST row does (i < n_b and j0 < n_b) -- one test per node row the
// tile touches, 32 / N + 2 at most.
#include "common.hpp"

namespace tgt {

__device__ __forceinline__ bool edge_tile_live(const int32_t* node_counts, int N, int64_t M, int64_t tile) {
    const int64_t nn = (int64_t)N * N;
    int64_t r = tile * 32;
    const int64_t end = r + 32 < M ? r + 32 : M;
    while (r < end) {
        const int64_t b = r / nn, ij = r - b * nn;
        const int i = (int)(ij / N), j = (int)(ij - (int64_t)i * N);
        const int n = min(max(node_counts[b], 0), N);
        if (i < n && j < n) return true;
        r += N - j;                                        // the first row of the next node row
    }
    return false;
}

__global__ void __launch_bounds__(1024) edge_live_tiles_kernel(const int32_t* node_counts, int N, int64_t M, int T, int32_t* tiles) {
    __shared__ int wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (T + 1023) / 1024;
    const int64_t t0 = (int64_t)tid * per;
    const int t1 = (int)(t0 + per < T ? t0 + per : T);
    int mine = 0;
    for (int64_t t = t0; t < t1; ++t) mine += edge_tile_live(node_counts, N, M, t) ? 1 : 0;
    // exclusive prefix sum over the 1024 threads: inside the wave by shuffles, across the 16 waves through LDS
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        before += w < wave ? wave_sum[w] : 0;
        total += wave_sum[w];
    }
    if (tid == 0) tiles[0] = total;
    // tiles in front of t0: `before` live ones, t0 - before dead ones
    int32_t* lv = tiles + 1 + before;
    int32_t* dd = tiles + 1 + total + (t0 < T ? t0 - before : 0);
    for (int64_t t = t0; t < t1; ++t) {
        if (edge_tile_live(node_counts, N, M, t)) *lv++ = (int32_t)t;
        else *dd++ = (int32_t)t;
    }
}

int edge_live_tiles_run(const int32_t* node_counts, int B, int N, int32_t* tiles, hipStream_t st) {
    if (B < 0 || N < 0 || N > 32768) return set_error(TGT_ERR_INVALID, "edge live tiles: bad sizes B=%d N=%d", B, N);
    if (!tiles || (B > 0 && !node_counts)) return set_error(TGT_ERR_INVALID, "edge live tiles: null tensor");
    const int64_t M = (int64_t)B * N * N, T = (M + 31) / 32;
    if (T > 0x7ffffffeLL) return set_error(TGT_ERR_INVALID, "edge live tiles: %lld tiles do not fit the int32 list", (long long)T);
    hipLaunchKernelGGL(edge_live_tiles_kernel, dim3(1), dim3(1024), 0, st, node_counts, N, M, (int)T, tiles);
    return check_launch("edge_live_tiles_kernel");
}

}  // namespace tgt
