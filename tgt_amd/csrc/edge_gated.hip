// Gated output stage of TriangularUpdate on the edge rows (gfx950), 16-bit, C = 256, K = 2H in {16, 32, 64}:
//   z = a w^T + bias = [z_g | z_l]   (fp32, never stored)          reference lib/tgt/layers/triplet.py:174-175
//   t = sigmoid(z_g) * z_l
//   s = res + row_scale[row / rows_per_sample] * t                  DropPath + residual, layers.py:284-287
//   y = LayerNorm(s as stored; gamma, beta, eps), mean / rstd       the edge FFN's opening LayerNorm, layers.py:150
// ONE launch; nothing of width 2C reaches memory.  Backward (one launch): z and sigma recomputed from a,
//   dz = [dt z_l sigma (1 - sigma) | dt sigma] rounded once to the element type,  d_a = dz w,
//   dw_partial / db_partial: per persistent workgroup dz^T a and the column sums of dz, summed by tgt_sum_planes / tgt_sum_rows.
//
// Shape of both kernels: 4 waves walk 32-row tiles persistently (tile = blockIdx.x + s * gridDim.x, as the row kernels of
// edge_gemm.hip).  Wave w owns output columns [64 w, 64 w + 64): its gate and linear weight rows stay resident in registers as the
// A operands of v_mfma_f32_32x32x16 (weights = M side, activation rows = N side, so a lane holds 16 columns of ONE row: the row
// phase is in-lane up to one half exchange and one LDS exchange between the waves).  The activation fragments come straight from
// global memory (a tile is 32 x K: 1-4 KB).
//   backward  d_a: dz of a lane IS the B operand of the next product (pack_chunk: the contraction index permuted the way the
//             accumulator holds it, the resident W fragments permuted alike); the four waves' partial sums meet in LDS, fixed order.
//             dw:  dz^T and a^T go through LDS (the contraction index is the row), accumulators persist over the tiles.
// Rows at or past M: a and dt read as zeros, so dz is zero there and nothing of them enters d_a / dw / db; no store leaves M rows.
//
// Ragged batches (tgt_hip.h, tgt_edge_gated_out_fwd_live / _bwd_live): the live tile list of edge_common.hpp as a trailing parameter
// pack `TL... tl` of both kernels, empty without a list -- that instantiation has the argument list and the instruction stream it
// always had.  With a list workgroup w walks list[1 + w + s * gridDim] below list[0] (the dealing of tgt_edge_linear_live, same
// grid) and first gives its share of the DEAD tiles zeros in every output (s, y, mean, rstd; d_a) without reading an operand of
// them.  The trip count of the tile loop is uniform per workgroup, so its barriers are too; a workgroup without a live tile still
// writes its (zero) dw_partial plane and db_partial row.  Entries are clamped where they are read (edge_live_tile): a tile index
// past the last row loads zeros and stores nothing.
#include "edge_common.hpp"

namespace tgt {

int edge_linear_parts(int64_t M, int N);          // edge_gemm.hip: the persistent grid of the N = 256 row kernels (honours the grid cap)

namespace {

constexpr int GO_C = 256;          // output channels
constexpr int GO_TP = 40;          // row stride (elements) of the transposed tiles in LDS: 32 rows + 8

template <typename T>
__device__ __forceinline__ void go_cols(const T* base, int nbase, int hi, float* v) {      // the lane's 16 columns of a (C) vector
#pragma unroll
    for (int g = 0; g < 4; ++g) unpack4<T>(*reinterpret_cast<const uint2*>(base + nbase + 8 * g + 4 * hi), v + 4 * g);
}
__device__ __forceinline__ void go_cols_f32(const float* base, int nbase, int hi, float* v) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 f = *reinterpret_cast<const float4*>(base + nbase + 8 * g + 4 * hi);
        v[4 * g] = f.x; v[4 * g + 1] = f.y; v[4 * g + 2] = f.z; v[4 * g + 3] = f.w;
    }
}

// resident forward operands of a wave: w[part][blk][kc] = rows part*C + (2 wave + blk)*32 + r of the weight, k chunk kc
template <typename T, int K>
struct GoWeights {
    static constexpr int KC = K / 16;
    frag_t<T> w[2][2][KC];
    __device__ __forceinline__ void load(const T* wp, int64_t ldw, int wave, int r, int hi) {
#pragma unroll
        for (int part = 0; part < 2; ++part)
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int kc = 0; kc < KC; ++kc)
                    w[part][blk][kc] = load_frag<T>(wp + (int64_t)(part * GO_C + (2 * wave + blk) * 32 + r) * ldw + kc * 16 + 8 * hi);
    }
    // z[part] of column block blk for the tile whose activation fragments are af: lane (r, hi), register q = row r, column acc_row(q, hi)
    __device__ __forceinline__ f32x16 z(int part, int blk, const frag_t<T> (&af)[KC], const T* bias, int wave, int hi) const {
        f32x16 acc;
        float b[16];
        go_cols<T>(bias + part * GO_C, (2 * wave + blk) * 32, hi, b);
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = b[q];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) acc = mma32(w[part][blk][kc], af[kc], acc);
        return acc;
    }
};

template <typename T, int KC>
__device__ __forceinline__ void go_load_a(const T* a, int64_t lda, int64_t m, int64_t M, int hi, frag_t<T> (&af)[KC]) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) af[kc] = m < M ? load_frag<T>(a + m * lda + kc * 16 + 8 * hi) : zero_frag<T>();
}

// zeros into columns [0, cols) of rows [32 tile, 32 tile + 32) of an (M, ld) tensor, by the 256 threads of a workgroup: 16 bytes each
template <typename T>
__device__ __forceinline__ void go_zero_rows(T* base, int64_t ld, int cols, int64_t tile, int64_t M, int tid) {
    const int per_row = cols / 8;
    for (int i = tid; i < 32 * per_row; i += 256) {
        const int64_t mr = tile * 32 + i / per_row;
        if (mr < M) *reinterpret_cast<uint4*>(base + mr * ld + (i % per_row) * 8) = make_uint4(0, 0, 0, 0);
    }
}

// The LIVE walk reads the list through the constant address space.  These kernels store through plain pointers, so hipcc cannot
// prove a plain `list[i]` untouched by them and reads it with a VECTOR load and a full `s_waitcnt vmcnt(0)` at the top of every
// tile -- which also drains the stores of the tile before (read off the ISA; +6 us on the 175 us backward with a list that names
// every tile).  The kernels never write the list, so it IS constant for them: a uniform index is then one scalar load, issued a
// tile ahead.  Same clamping as edge_live_count / edge_live_tile (edge_common.hpp), which the dead walk uses as they are.
typedef const __attribute__((address_space(4))) int32_t* go_list_t;
__device__ __forceinline__ go_list_t go_const_list(const int32_t* p) { return (go_list_t)reinterpret_cast<uintptr_t>(p); }
__device__ __forceinline__ int go_live_count(go_list_t list, int64_t row_tiles) {
    const int n = list[0];
    return n < 0 ? 0 : (n > row_tiles ? (int)row_tiles : n);
}
// entry `idx` as it stands in the list (0 at or past `end`: never used); it becomes a tile -- go_clamp_tile -- only where it is
// USED, a tile later, so the wait for the load sits there and not behind the load
__device__ __forceinline__ int go_live_raw(go_list_t list, int64_t idx, int64_t end) { return idx < end ? list[1 + idx] : 0; }
__device__ __forceinline__ int64_t go_clamp_tile(int t, int64_t row_tiles) {
    return t < 0 ? row_tiles : (t > row_tiles ? row_tiles : (int64_t)t);
}
// The list's count and this workgroup's first entry, read at the TOP of a kernel: two independent scalar loads whose latency the
// weight loads hide.  The entry is read whether or not it is live: index blockIdx.x is below the row tiles (the grid never exceeds
// them), so inside the list.
struct GoLiveHead {
    int n_live;
    int first_raw;
};
__device__ __forceinline__ GoLiveHead go_live_head(go_list_t list, int64_t row_tiles) {
    const int64_t w = (int64_t)blockIdx.x < row_tiles ? (int64_t)blockIdx.x : row_tiles - 1;
    const int raw = list[1 + w];
    return {go_live_count(list, row_tiles), raw};
}

__device__ __forceinline__ float go_wave_sum4(const float* red, int r) {          // the four waves' partials of row r, fixed order
    return ((red[r] + red[32 + r]) + red[64 + r]) + red[96 + r];
}

template <typename T, int K, typename... TL>
__global__ void __launch_bounds__(256) edge_gated_fwd_kernel(const tgt_edge_gated_args a, TL... tl) {
    constexpr int KC = K / 16;
    constexpr bool LV = sizeof...(TL) > 0;
    __shared__ float red[2][4 * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5;
    const T* bias = reinterpret_cast<const T*>(a.bias);
    const T* res = reinterpret_cast<const T*>(a.res);
    T* s_out = reinterpret_cast<T*>(a.s);
    T* y_out = reinterpret_cast<T*>(a.y);
    const int64_t M = a.M, tiles = (M + 31) / 32;
    const int32_t* live = edge_live_ptr(tl...);
    int64_t n_walk = tiles;                                // entries this launch deals: all tiles, or the live ones of the list
    int raw_next = 0;
    if constexpr (LV) {
        const GoLiveHead head = go_live_head(go_const_list(live), tiles);
        n_walk = head.n_live;
        raw_next = head.first_raw;
    }
    GoWeights<T, K> W;
    W.load(reinterpret_cast<const T*>(a.w), a.ldw, wave, r, hi);
    if constexpr (LV) {
        edge_dead_tiles(live, (int)n_walk, tiles, [&](int64_t t) {      // zeros, no operand read
            go_zero_rows<T>(s_out, GO_C, GO_C, t, M, threadIdx.x);
            go_zero_rows<T>(y_out, GO_C, GO_C, t, M, threadIdx.x);
            const int64_t mr = t * 32 + threadIdx.x;
            if (threadIdx.x < 32 && mr < M) { a.mean[mr] = 0.f; a.rstd[mr] = 0.f; }
        });
    }
    // (with a list: the NEXT entry is read while this tile computes -- a scalar load whose latency the tile hides)
    for (int64_t it = blockIdx.x; it < n_walk; it += gridDim.x) {
        int64_t tile = it;
        if constexpr (LV) {
            tile = go_clamp_tile(raw_next, tiles);
            raw_next = go_live_raw(go_const_list(live), it + gridDim.x, n_walk);
        }
        const int64_t m = tile * 32 + r;
        frag_t<T> af[KC];
        go_load_a<T, KC>(reinterpret_cast<const T*>(a.a), a.lda, m, M, hi, af);
        float sc = 1.f;
        if (a.row_scale && m < M) sc = a.row_scale[m / a.rows_per_sample];
        float sv[2][16];
        float sum = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int nbase = (2 * wave + blk) * 32;
            const f32x16 zg = W.z(0, blk, af, bias, wave, hi), zl = W.z(1, blk, af, bias, wave, hi);
            float rv[16];
            load_block<T>(res, GO_C, m, M, nbase, GO_C, hi, rv);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float t = fast_sigmoid(zg[q]) * zl[q];
                sv[blk][q] = to_f32(from_f32<T>(rv[q] + sc * t));          // s as stored: what the LayerNorm sees
                sum += sv[blk][q];
            }
            store_block<T>(s_out, GO_C, m, M, nbase, GO_C, hi, sv[blk]);
        }
        sum += xhalf(sum);
        if (hi == 0) red[0][wave * 32 + r] = sum;
        __syncthreads();
        const float mean = go_wave_sum4(red[0], r) * (1.f / GO_C);
        float sq = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int q = 0; q < 16; ++q) { const float d = sv[blk][q] - mean; sq += d * d; }
        sq += xhalf(sq);
        if (hi == 0) red[1][wave * 32 + r] = sq;
        __syncthreads();
        const float rstd = rsqrtf(go_wave_sum4(red[1], r) * (1.f / GO_C) + a.eps);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int nbase = (2 * wave + blk) * 32;
            float g[16], be[16], yv[16];
            go_cols_f32(a.gamma, nbase, hi, g);
            go_cols_f32(a.beta, nbase, hi, be);
#pragma unroll
            for (int q = 0; q < 16; ++q) yv[q] = (sv[blk][q] - mean) * rstd * g[q] + be[q];
            store_block<T>(y_out, GO_C, m, M, nbase, GO_C, hi, yv);
        }
        if (wave == 0 && hi == 0 && m < M) { a.mean[m] = mean; a.rstd[m] = rstd; }
    }
}

template <typename T, int K, typename... TL>
__global__ void __launch_bounds__(256) edge_gated_bwd_kernel(const tgt_edge_gated_args a, TL... tl) {
    constexpr int KC = K / 16, KB = K > 32 ? K / 32 : 1;
    constexpr bool LV = sizeof...(TL) > 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char go_smem[];
    T* dzT = reinterpret_cast<T*>(go_smem);                       // [2C][GO_TP]: dz transposed, row = weight row
    T* aT = dzT + 2 * GO_C * GO_TP;                               // [64][GO_TP]: the a tile transposed (rows at or past K stay zero)
    float* red = reinterpret_cast<float*>(aT + 64 * GO_TP);       // [4 waves][32 rows][64]: partial d_a
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hi = lane >> 5;
    const T* wp = reinterpret_cast<const T*>(a.w);
    const T* bias = reinterpret_cast<const T*>(a.bias);
    const T* dt = reinterpret_cast<const T*>(a.dt);
    T* d_a = reinterpret_cast<T*>(a.d_a);
    const int64_t M = a.M, tiles = (M + 31) / 32;
    const int32_t* live = edge_live_ptr(tl...);
    int64_t n_walk = tiles;
    int raw_next = 0;
    if constexpr (LV) {
        const GoLiveHead head = go_live_head(go_const_list(live), tiles);
        n_walk = head.n_live;
        raw_next = head.first_raw;
    }
    for (int i = tid; i < 64 * GO_TP; i += 256) aT[i] = from_f32<T>(0.f);
    GoWeights<T, K> W;
    W.load(wp, a.ldw, wave, r, hi);
    // resident operands of d_a = dz w: wd[part][blk][c][kb], lane (r, hi) = output column k = kb*32 + r, contraction element t =
    // the weight row that accumulator register 8c + t of lane-half hi belongs to
    frag_t<T> wd[2][2][2][KB];
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const int k = kb * 32 + r;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int row = part * GO_C + (2 * wave + blk) * 32 + c * 16 + (t & 3) + 8 * (t >> 2) + 4 * hi;
                        wd[part][blk][c][kb][t] = k < K ? wp[(int64_t)row * a.ldw + k] : from_f32<T>(0.f);
                    }
                }
    f32x16 dw[4][KB];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int q = 0; q < 16; ++q) dw[j][kb][q] = 0.f;
    float db[2] = {0.f, 0.f};
    __syncthreads();
    if constexpr (LV) edge_dead_tiles(live, (int)n_walk, tiles, [&](int64_t t) { go_zero_rows<T>(d_a, a.ld_da, K, t, M, tid); });      // dt / a / s not read
    // (with a list: the NEXT entry is read while this tile computes -- a scalar load whose latency the tile hides)
    for (int64_t it = blockIdx.x; it < n_walk; it += gridDim.x) {
        int64_t tile = it;
        if constexpr (LV) {
            tile = go_clamp_tile(raw_next, tiles);
            raw_next = go_live_raw(go_const_list(live), it + gridDim.x, n_walk);
        }
        const int64_t m = tile * 32 + r;
        frag_t<T> af[KC];
        go_load_a<T, KC>(reinterpret_cast<const T*>(a.a), a.lda, m, M, hi, af);
        f32x16 da[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int q = 0; q < 16; ++q) da[kb][q] = 0.f;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int nbase = (2 * wave + blk) * 32;
            const f32x16 zg = W.z(0, blk, af, bias, wave, hi), zl = W.z(1, blk, af, bias, wave, hi);
            float dtv[16];
            load_block<T>(dt, GO_C, m, M, nbase, GO_C, hi, dtv);
            f32x16 dz[2];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float sg = fast_sigmoid(zg[q]);
                dz[0][q] = dtv[q] * zl[q] * sg * (1.f - sg);
                dz[1][q] = dtv[q] * sg;
            }
#pragma unroll
            for (int part = 0; part < 2; ++part) {
#pragma unroll
                for (int q = 0; q < 16; ++q) dzT[(part * GO_C + nbase + acc_row(q, hi)) * GO_TP + r] = from_f32<T>(dz[part][q]);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const frag_t<T> f = pack_chunk<T>(dz[part], c);
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) da[kb] = mma32(wd[part][blk][c][kb], f, da[kb]);
                }
            }
        }
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
            if ((kc & 3) == wave) {
#pragma unroll
                for (int t = 0; t < 8; ++t) aT[(kc * 16 + 8 * hi + t) * GO_TP + r] = af[kc][t];
            }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int q = 0; q < 16; ++q) red[(wave * 32 + r) * 64 + kb * 32 + acc_row(q, hi)] = da[kb][q];
        __syncthreads();
        // dw += dz^T a over the tile's 32 rows: weight-row blocks 4 wave .. 4 wave + 3
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const frag_t<T> fa = load_frag<T>(dzT + ((4 * wave + j) * 32 + r) * GO_TP + ch * 16 + 8 * hi);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
                    dw[j][kb] = mma32(fa, load_frag<T>(aT + (kb * 32 + r) * GO_TP + ch * 16 + 8 * hi), dw[j][kb]);
            }
#pragma unroll
        for (int u = 0; u < 2; ++u) {                      // db: weight rows tid and tid + 256
            float v[32];
#pragma unroll
            for (int p = 0; p < 4; ++p) rp_unpack8<T>(*reinterpret_cast<const uint4*>(dzT + (tid + 256 * u) * GO_TP + 8 * p), v + 8 * p);
            float sacc = 0.f;
#pragma unroll
            for (int i = 0; i < 32; ++i) sacc += v[i];
            db[u] += sacc;
        }
        if (tid < 32 * (K / 8)) {                          // d_a: (row, 8 columns) per thread, the four waves' partials in a fixed order
            const int row = tid / (K / 8), c8 = (tid % (K / 8)) * 8;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float* p = red + row * 64 + c8 + i;
                v[i] = ((p[0] + p[32 * 64]) + p[2 * 32 * 64]) + p[3 * 32 * 64];
            }
            const int64_t mr = tile * 32 + row;
            if (mr < M) *reinterpret_cast<uint4*>(d_a + mr * a.ld_da + c8) = rp_pack8<T>(v);
        }
        __syncthreads();
    }
    float* dwp = a.dw_partial + (int64_t)blockIdx.x * 2 * GO_C * K;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int k = kb * 32 + r;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (k < K) dwp[(int64_t)((4 * wave + j) * 32 + acc_row(q, hi)) * K + k] = dw[j][kb][q];
        }
    a.db_partial[(int64_t)blockIdx.x * 2 * GO_C + tid] = db[0];
    a.db_partial[(int64_t)blockIdx.x * 2 * GO_C + 256 + tid] = db[1];
}

// (TL: empty, or the live tile list -- the kernels' trailing parameter pack)
template <typename T, int K, typename... TL>
int go_launch(const tgt_edge_gated_args& a, bool bwd, int grid, hipStream_t st, TL... tl) {
    if (!bwd) {
        hipLaunchKernelGGL((edge_gated_fwd_kernel<T, K, TL...>), dim3(grid), dim3(256), 0, st, a, tl...);
        return check_launch("edge_gated_fwd_kernel");
    }
    const int lds = (2 * GO_C + 64) * GO_TP * (int)sizeof(T) + 4 * 32 * 64 * (int)sizeof(float);
    return launch_lds<edge_gated_bwd_kernel<T, K, TL...>>("edge_gated_bwd_kernel", dim3(grid), dim3(256), lds, st, a, tl...);
}

template <typename T, typename... TL>
int go_dispatch(const tgt_edge_gated_args& a, bool bwd, int grid, hipStream_t st, TL... tl) {
    switch (a.K) {
        case 16: return go_launch<T, 16>(a, bwd, grid, st, tl...);
        case 32: return go_launch<T, 32>(a, bwd, grid, st, tl...);
        default: return go_launch<T, 64>(a, bwd, grid, st, tl...);
    }
}

bool go_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int edge_gated_out_supported(const tgt_edge_gated_args* a) {
    return a && (a->dtype == TGT_BF16 || a->dtype == TGT_F16) && a->C == GO_C && (a->K == 16 || a->K == 32 || a->K == 64);
}

int edge_gated_out_parts(int64_t M) { return M > 0 ? edge_linear_parts(M, GO_C) : 0; }

// tiles: NULL, or the live tile list (1 + ceil(M / 32) entries) of tgt_edge_live_tiles
int edge_gated_out_run(const tgt_edge_gated_args* a, bool bwd, const int32_t* tiles, hipStream_t st) {
    const char* what = bwd ? "edge gated output bwd" : "edge gated output fwd";
    if (!a) return set_error(TGT_ERR_INVALID, "%s: null args", what);
    if (a->M < 0 || a->K <= 0 || a->C <= 0) return set_error(TGT_ERR_INVALID, "%s: bad size", what);
    if (!edge_gated_out_supported(a))
        return set_error(TGT_ERR_UNSUPPORTED, "%s: C = %d, K = %d, dtype %d (16-bit, C = 256, K in {16, 32, 64})", what, a->C, a->K, a->dtype);
    if (a->M == 0) return TGT_OK;
    if (!a->a || !a->w || !a->bias) return set_error(TGT_ERR_INVALID, "%s: null operand", what);
    if (a->lda < a->K || a->lda % 8 || a->ldw < a->K || a->ldw % 8)
        return set_error(TGT_ERR_INVALID, "%s: lda %lld / ldw %lld (at least K, a multiple of 8)", what, (long long)a->lda, (long long)a->ldw);
    if (go_misaligned(a->a) || go_misaligned(a->w) || go_misaligned(a->bias)) return set_error(TGT_ERR_INVALID, "%s: operand not 16-byte aligned", what);
    const int64_t row_tiles = (a->M + 31) / 32;
    int grid;
    if (!bwd) {
        if (!a->res || !a->s || !a->y || !a->gamma || !a->beta || !a->mean || !a->rstd) return set_error(TGT_ERR_INVALID, "%s: null tensor", what);
        if (a->row_scale && a->rows_per_sample <= 0) return set_error(TGT_ERR_INVALID, "%s: row_scale without rows_per_sample", what);
        if (go_misaligned(a->res) || go_misaligned(a->s) || go_misaligned(a->y) || go_misaligned(a->gamma) || go_misaligned(a->beta))
            return set_error(TGT_ERR_INVALID, "%s: tensor not 16-byte aligned", what);
        grid = edge_gated_out_parts(a->M);
    } else {
        if (!a->dt || !a->d_a || !a->dw_partial || !a->db_partial) return set_error(TGT_ERR_INVALID, "%s: null tensor", what);
        if (a->ld_da < a->K || a->ld_da % 8) return set_error(TGT_ERR_INVALID, "%s: ld_da %lld (at least K, a multiple of 8)", what, (long long)a->ld_da);
        if (go_misaligned(a->dt) || go_misaligned(a->d_a)) return set_error(TGT_ERR_INVALID, "%s: tensor not 16-byte aligned", what);
        if (a->parts < 1 || a->parts > row_tiles) return set_error(TGT_ERR_INVALID, "%s: %d partial planes for %lld row tiles", what, a->parts, (long long)row_tiles);
        grid = a->parts;
    }
    if (tiles) {
        if (reinterpret_cast<uintptr_t>(tiles) & 3) return set_error(TGT_ERR_INVALID, "%s: live tile list not 4-byte aligned", what);
        if (row_tiles > 0x7ffffffeLL) return set_error(TGT_ERR_INVALID, "%s: too many rows for a live tile list", what);
        return a->dtype == TGT_BF16 ? go_dispatch<bf16_t>(*a, bwd, grid, st, tiles) : go_dispatch<f16_t>(*a, bwd, grid, st, tiles);
    }
    return a->dtype == TGT_BF16 ? go_dispatch<bf16_t>(*a, bwd, grid, st) : go_dispatch<f16_t>(*a, bwd, grid, st);
}

}  // namespace tgt
