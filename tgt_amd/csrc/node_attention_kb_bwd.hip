// Node attention with edge bias and gate (EGT_Attention core), KEY-BLOCKED BACKWARD on 16-wide matrix-core tiles: 16-bit dtypes,
// 65 <= N <= 128, H a multiple of 8, D in {8, 12, 16} -- graphs padded to more than 64 nodes.
//
// Replaces the autograd backward of reference lib/tgt/layers/layers.py:62-77.  Math: SURVEY.md App. A.1 / A.4, the arithmetic of
// node_attention16.hip (tile_bwd) with the softmax statistics READ instead of recomputed.
//
// Why a separate file.  node_attention16.hip keeps the whole key range of a query block in LDS as three pair planes (E, G, dH_hat):
// at N = 128 that is 3 x 16 x (8 heads x 256 B + 16) = 197 KB, more than the CU's 160 KB.  Here the keys of a query block are
// walked in CHUNKS of KC = 4 key blocks (64 keys), so the planes never grow past their N = 64 size.  What the single-pass kernel gets
// from having every key at hand, the forward has saved:
//   P[l,m]   = exp(x[l,m] - lse[l])                       (lse: maximum + log of the sum)
//   dsc_l    = log(1 + gsum[l])                           (gsum: sum of the gates; 1 without the degree scaler)
//   delta_l  = sum_m P dA g = V_att[l,:] . dV_att[l,:]    (V_att = dsc sum_m P g V, dA = dsc V dV_att^T)
// so a chunk needs nothing from the chunks before it: no online softmax, no second pass, no workspace.
//   workgroup = (graph b, 8 heads), 8 waves, wave = head, as node_att16_bwd_kernel; K / V rows of ALL keys staged once;
//   the workgroup walks the query blocks (16 queries), inside each the key chunks; per chunk the pair planes land KEY-MAJOR PER HEAD
//   (node_tiles16.hpp), the head's tile math runs on v_mfma_f32_16x16x16, dE / dG leave through the E / G slots and are stored once;
//   dQ^T of the query block is summed over its chunks in registers and stored after the last one; dK^T / dV^T of every key block
//   (up to 8: 64 fp32 registers at D = 16) are summed over all query blocks in registers and stored at the end.
// Every sum runs inside one wave in a fixed order: no atomics, no partial tiles, two runs are bit-equal.
// LDS: planes 3 x 16 x (KC x 256 + 16) + mask + 3 x 16 node rows + 2 x 16 NQ node rows (Lay): 82 KB (N = 80, D = 8) to 134 KB
// (N = 128, D = 16), ONE workgroup per CU = two waves per SIMD at 145-189 registers, no scratch (DESIGN.md 4.z has the table per
// instantiation).  KC = 2 would fit two workgroups per CU for D = 8 and for D = 12 up to 96 nodes, but the 128 registers that
// leaves a wave spill (13-95 registers per instantiation): not built.
#include <cstdlib>
#include "node_tiles16.hpp"

namespace tgt {
namespace nkbb {

using namespace na16;

constexpr int kLdsMax = 160 * 1024;

// LDS map.  Pitches are 16 bytes past a multiple of 32 with pitch / 16 odd, so the 16 queries (rows) of a half-wave's 8-byte
// accesses fall on 16 different 4-bank groups -- conflict-free per half-wave (node_attention16.hip).
template <int NQ, int D, int KC>
struct Lay {
    static constexpr int NK = 16 * NQ;
    static constexpr int kPitchP = HG * KC * 32 + 16;     // pair plane, per query: 8 heads x (16 KC keys x 2 bytes)
    static constexpr int kPitchM = KC * 64 + 16;          // mask tile (fp32), per query
    static constexpr int kHeadN = D * 2;
    static constexpr int kPitchN = HG * kHeadN + 16;      // node rows
    static constexpr int kOffE = 0;
    static constexpr int kOffG = kOffE + 16 * kPitchP;
    static constexpr int kOffH = kOffG + 16 * kPitchP;                       // dH_hat
    static constexpr int kOffM = kOffH + 16 * kPitchP;
    static constexpr int kOffQ = kOffM + 16 * kPitchM;                       // the block's Q rows; dQ leaves through it
    static constexpr int kOffO = kOffQ + 16 * kPitchN;                       // dV_att rows
    static constexpr int kOffA = kOffO + 16 * kPitchN;                       // V_att rows (for delta)
    static constexpr int kOffK = kOffA + 16 * kPitchN;
    static constexpr int kOffV = kOffK + NK * kPitchN;
    static constexpr int kBytes = kOffV + NK * kPitchN;
    static_assert((kPitchP / 16) % 2 == 1 && (kPitchN / 16) % 2 == 1 && (kPitchM / 16) % 2 == 1, "odd pitches");
};
constexpr int kChunkBlocks = 4;                           // key blocks per chunk

// what the forward saved about query x of this head, and what follows from it
struct RowStat { float lse, dsc, delta, dgsum; };

// ---------------------------------------------------------------------------
// backward tile of head hh: query block (staged) x key chunk C (key blocks KB0 .. KB0 + NB - 1).  dE, dG into the E / G slots,
// dQ^T accumulated into `dq`, dK^T / dV^T of the chunk's key blocks into dk / dv.
//   dA^T[m][l] = dsc_l * V[m,:].dV_att[l,:]      d_dsc = delta / dsc        dgsum = d_dsc / (1 + sum g)
//   dS = P (dA g - delta)         dG = (dA P + dgsum) g (1 - g)            dE = dH_hat + dS
//   dQ^T = s K^T dE^T             dK^T = s Q^T dE                          dV^T = dV_att^T (P g dsc)
// A key masked with -inf has P = exp(-inf) = 0 and g = sigmoid(-inf) = 0 exactly, whatever the chunk it is in.
// ---------------------------------------------------------------------------
template <typename T, int NQ, int D, int KC, int C>
__device__ __forceinline__ void tile_bwd(char* lds, const tgt_node_attention_args& a, const RowStat& rs, float hs, int x, int g, int hh,
                                         f32x4& dq, f32x4 (&dk)[NQ], f32x4 (&dv)[NQ]) {
    using L = Lay<NQ, D, KC>;
    using F = frag4_t<T>;
    constexpr int KB0 = KC * C, NB = NQ - KB0 < KC ? NQ - KB0 : KC, kHeadP = NB * 32;
    const char* rK = lds + L::kOffK;
    const char* rV = lds + L::kOffV;
    const F fq = node_frag<T, D, L::kPitchN>(lds + L::kOffQ, x, g, hh), fo = node_frag<T, D, L::kPitchN>(lds + L::kOffO, x, g, hh);
    const F id = ident4<T>(x, g);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    char* pe = lds + L::kOffE + x * L::kPitchP + hh * kHeadP + g * 8;
    char* pg = lds + L::kOffG + x * L::kPitchP + hh * kHeadP + g * 8;
    const char* ph = lds + L::kOffH + x * L::kPitchP + hh * kHeadP + g * 8;
    const char* pm = lds + L::kOffM + x * L::kPitchM + g * 16;
    float zs[NB][4], ws[NB][4], amax = 0.f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        const F fk = node_frag<T, D, L::kPitchN>(rK, 16 * (KB0 + kb) + x, g, hh);
        const F fv = node_frag<T, D, L::kPitchN>(rV, 16 * (KB0 + kb) + x, g, hh);
        const f32x4 st = mma16(fk, fq, z);                 // S^T[key][query]
        const f32x4 dt = mma16(fv, fo, z);                 // (V dV_att^T)[key][query]
        float e[4], gg[4], dh[4], dE[4], dG[4];
        unpack4<T>(*reinterpret_cast<const uint2*>(pe + kb * 32), e);
        unpack4<T>(*reinterpret_cast<const uint2*>(pg + kb * 32), gg);
        unpack4<T>(*reinterpret_cast<const uint2*>(ph + kb * 32), dh);  // (zeros when there is no d_hhat)
        const float4 mk4 = *reinterpret_cast<const float4*>(pm + kb * 64);
        const float mk[4] = {mk4.x, mk4.y, mk4.z, mk4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float xx = st[q] * a.scale + e[q] + mk[q];        // (mk = -inf past N)
            const float gt = fast_sigmoid(gg[q] + mk[q]);
            const float p = fast_exp(xx - rs.lse);                  // P (lse finite: RowStat)
            const float da = dt[q] * rs.dsc;                        // dA (gradient wrt the unscaled V_att folded in)
            const float dS = p * (da * gt - rs.delta);
            dG[q] = (da * p + rs.dgsum) * gt * (1.f - gt);
            dE[q] = dh[q] * hs + dS;
            ws[kb][q] = p * gt * rs.dsc;                            // the weights (operand of dV)
            zs[kb][q] = dE[q] * a.scale;                            // the logit gradient (operand of dQ, dK)
            amax = fmaxf(amax, fabsf(zs[kb][q]));
        }
        *reinterpret_cast<uint2*>(pe + kb * 32) = pack4u<T>(dE);    // dE, dG leave through the E / G slots of this lane
        *reinterpret_cast<uint2*>(pg + kb * 32) = pack4u<T>(dG);
    }
    float c = 1.f, unscale = 1.f;
    if constexpr (!kIsBf16<T>) {
        // fp16 operands: bring the head's largest |dE| of this tile to 2^13 (an exact power of two, undone on dQ / dK) so that
        // small gradients do not sink into fp16 subnormals on their way through the matrix core (node_attention16.hip)
        amax = group_max<64>(amax);
        const int ex = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xffu);
        if (ex >= 14 && ex <= 253) {
            c = __builtin_bit_cast(float, (uint32_t)(267 - ex) << 23);                     // 2^(13 - (ex - 127))
            unscale = __builtin_bit_cast(float, (uint32_t)(ex - 13) << 23);                // 1 / c
        }
    }
    const f32x4 qt = mma16(fq, id, z), ot = mma16(fo, id, z);          // Q / dV_att rows in accumulator layout = A operands of Q^T / dV_att^T
    const F fqt = pack4<T>(qt), fot = pack4<T>(ot);
    f32x4 dqc = z;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        f32x4 zv, wv;
#pragma unroll
        for (int q = 0; q < 4; ++q) { zv[q] = zs[kb][q] * c; wv[q] = ws[kb][q]; }
        const F zf = pack4<T>(zv), wf = pack4<T>(wv);                   // dE^T / W^T [key 4g + q][query x]: B operands as they are
        const F fk = node_frag<T, D, L::kPitchN>(rK, 16 * (KB0 + kb) + x, g, hh);
        const f32x4 kt = mma16(fk, id, z);                              // K[key][d] in accumulator layout = the A operand of K^T
        dqc = mma16(pack4<T>(kt), zf, dqc);                             // dQ^T[d][query] += K^T[d][key] dE^T[key][query]
        const f32x4 zT = mma16(zf, id, z), wT = mma16(wf, id, z);       // the transposed tiles (node_attention16.hip)
        f32x4 t = mma16(fqt, pack4<T>(zT), z);                          // dK^T[d][key] of this query block
#pragma unroll
        for (int q = 0; q < 4; ++q) dk[KB0 + kb][q] += t[q] * unscale;
        dv[KB0 + kb] = mma16(fot, pack4<T>(wT), dv[KB0 + kb]);          // dV^T[d][key] += dV_att^T[d][query] W[query][key]
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) dq[q] += dqc[q] * unscale;
}

// one key chunk of the staged query block: planes in, tile, dE / dG out.  Chunk 0 also waits for the block's node rows and
// derives the row statistics; the last chunk hands dQ to the Q region and stores it.
template <typename T, int NQ, int D, int KC, int C>
__device__ __forceinline__ void chunk_pass(char* lds, const tgt_node_attention_args& a, const Unit& u, int qb, int tid, int x, int g, int hh,
                                           float lse, float gsum, float hs, RowStat& rs, f32x4& dq, f32x4 (&dk)[NQ], f32x4 (&dv)[NQ]) {
    using L = Lay<NQ, D, KC>;
    constexpr int KB0 = KC * C, NB = NQ - KB0 < KC ? NQ - KB0 : KC, kChunks = (NQ + KC - 1) / KC;
    const int chan_eg[2] = {a.e_off + u.hg * HG, a.g_off + u.hg * HG}, chan_h[1] = {u.hg * HG};
    {
        PairIO<T, NB, 2> pio;
        pio.issue(a.eg, a.ld_eg, chan_eg, a.N, u.b, qb, tid, 16 * KB0);
        PairIO<T, NB, 1> hio;
        hio.issue(a.d_hhat, a.H, chan_h, a.N, u.b, qb, tid, 16 * KB0);
        mask_load<NB, L::kPitchM>(lds + L::kOffM, a, u.b, qb, tid, 16 * KB0);
        char* const planes[2] = {lds + L::kOffE, lds + L::kOffG};
        pio.template land<L::kPitchP>(planes, tid);
        char* const hplane[1] = {lds + L::kOffH};
        hio.template land<L::kPitchP>(hplane, tid);
    }
    __syncthreads();
    if constexpr (C == 0) {
        const frag4_t<T> fo = node_frag<T, D, L::kPitchN>(lds + L::kOffO, x, g, hh), fa = node_frag<T, D, L::kPitchN>(lds + L::kOffA, x, g, hh);
        float o4[4], a4[4];
        uint2 uo, ua;
        __builtin_memcpy(&uo, &fo, 8);
        __builtin_memcpy(&ua, &fa, 8);
        unpack4<T>(uo, o4);
        unpack4<T>(ua, a4);
        rs.delta = qsum(o4[0] * a4[0] + o4[1] * a4[1] + o4[2] * a4[2] + o4[3] * a4[3]);    // V_att . dV_att over d (lanes g hold d = 4g ..)
        rs.lse = lse > -INFINITY ? lse : 0.f;                           // padding / fully masked query: every weight exp(-inf - 0) = 0
        rs.dsc = a.scale_degree ? __logf(1.f + gsum) : 1.f;
        const float d_dsc = rs.dsc != 0.f ? rs.delta * fast_rcp(rs.dsc) : 0.f;     // zero scaler <=> every gate 0 <=> V_att 0
        rs.dgsum = a.scale_degree ? d_dsc * fast_rcp(1.f + gsum) : 0.f;
        dq = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    tile_bwd<T, NQ, D, KC, C>(lds, a, rs, hs, x, g, hh, dq, dk, dv);
    if constexpr (C == kChunks - 1) node_put<T, D, L::kPitchN>(lds + L::kOffQ, dq, x, g, hh);    // dQ leaves through this head's Q columns
    __syncthreads();
    {
        const char* const planes[2] = {lds + L::kOffE, lds + L::kOffG};
        PairIO<T, NB, 2>::template store<L::kPitchP>(planes, a.d_eg, a.ld_eg, chan_eg, a.N, u.b, qb, tid, 16 * KB0);
        if constexpr (C == kChunks - 1) {
            const char* const rq[1] = {lds + L::kOffQ};
            const int off1[1] = {a.q_off}, rows1[1] = {16}, row01[1] = {16 * qb};
            NodeIO<T, D, 1, 16>::template store<L::kPitchN>(rq, a.d_qkv, a.ld_qkv, off1, rows1, row01, a.N, a.H, u, tid);
        }
    }
    __syncthreads();                                       // (the planes are restaged for the next chunk)
    if constexpr (C + 1 < kChunks) chunk_pass<T, NQ, D, KC, C + 1>(lds, a, u, qb, tid, x, g, hh, lse, gsum, hs, rs, dq, dk, dv);
}

template <typename T, int NQ, int D, int KC>
__global__ void __launch_bounds__(kThreads, 2) node_att_kb_bwd_kernel(const tgt_node_attention_args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using L = Lay<NQ, D, KC>;
    const int tid = threadIdx.x, lane = tid & 63, hh = tid >> 6, x = lane & 15, g = lane >> 4;
    const int N = a.N, nqb = (N + 15) / 16, groups = a.H / HG;
    int b, sub;
    if (!unit_of_block(a.B, groups, b, sub)) return;
    const Unit u{b, sub};
    {
        NodeIO<T, D, 2, 2 * L::NK> nio;
        const int off[2] = {a.k_off, a.v_off}, rows[2] = {L::NK, L::NK}, row0[2] = {0, 0};
        nio.issue(a.qkv, a.ld_qkv, off, rows, row0, N, a.H, u, tid);
        char* const regions[2] = {lds + L::kOffK, lds + L::kOffV};
        nio.template land<L::kPitchN>(regions, rows, tid);
    }
    const float hs = a.hhat_scale ? a.hhat_scale[b] : 1.f;              // d_hhat is the gradient of hhat_scale * H_hat
    f32x4 dk[NQ], dv[NQ];
#pragma unroll
    for (int kb = 0; kb < NQ; ++kb) dk[kb] = dv[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < nqb; ++qb) {
        const int row = 16 * qb + x;
        const int64_t si = ((int64_t)b * N + (row < N ? row : 0)) * a.H + u.hg * HG + hh;
        const float lse = row < N ? a.lse[si] : 0.f, gsum = row < N ? a.gsum[si] : 0.f;
        {
            const int off1[1] = {a.q_off}, rows1[1] = {16}, row01[1] = {16 * qb}, off0[1] = {0};
            NodeIO<T, D, 1, 16> qio, oio, aio;
            qio.issue(a.qkv, a.ld_qkv, off1, rows1, row01, N, a.H, u, tid);
            oio.issue(a.d_vatt, (int64_t)D * a.H, off0, rows1, row01, N, a.H, u, tid);
            aio.issue(a.vatt, (int64_t)D * a.H, off0, rows1, row01, N, a.H, u, tid);
            char* const rq[1] = {lds + L::kOffQ};
            char* const ro[1] = {lds + L::kOffO};
            char* const ra[1] = {lds + L::kOffA};
            qio.template land<L::kPitchN>(rq, rows1, tid);
            oio.template land<L::kPitchN>(ro, rows1, tid);
            aio.template land<L::kPitchN>(ra, rows1, tid);
        }
        RowStat rs;
        f32x4 dq;
        chunk_pass<T, NQ, D, KC, 0>(lds, a, u, qb, tid, x, g, hh, lse, gsum, hs, rs, dq, dk, dv);
    }
    // dK^T / dV^T [d 4g + q][key 16 kb + x] of this head: complete sums over every query of the graph
#pragma unroll
    for (int kb = 0; kb < NQ; ++kb) {
        node_put<T, D, L::kPitchN>(lds + L::kOffK, dk[kb], 16 * kb + x, g, hh);
        node_put<T, D, L::kPitchN>(lds + L::kOffV, dv[kb], 16 * kb + x, g, hh);
    }
    __syncthreads();
    {
        const char* const regions[2] = {lds + L::kOffK, lds + L::kOffV};
        const int off[2] = {a.k_off, a.v_off}, rows[2] = {L::NK, L::NK}, row0[2] = {0, 0};
        NodeIO<T, D, 2, 2 * L::NK>::template store<L::kPitchN>(regions, a.d_qkv, a.ld_qkv, off, rows, row0, N, a.H, u, tid);
    }
}

template <typename T, int NQ, int D>
static int launch(const tgt_node_attention_args& a, hipStream_t st) {
    constexpr int KC = kChunkBlocks;
    constexpr int kLds = Lay<NQ, D, KC>::kBytes;
    static_assert(kLds <= kLdsMax, "backward LDS");
    const int grid = ((a.B + 7) / 8) * 8 * (a.H / HG);
    return launch_lds<node_att_kb_bwd_kernel<T, NQ, D, KC>>("node_att_kb_bwd_kernel", dim3(grid), dim3(kThreads), kLds, st, a);
}
template <typename T, int NQ>
static int dispatch_d(const tgt_node_attention_args& a, hipStream_t st) {
    switch (a.D) {
        case 8: return launch<T, NQ, 8>(a, st);
        case 12: return launch<T, NQ, 12>(a, st);
        case 16: return launch<T, NQ, 16>(a, st);
        default: return -1;
    }
}
template <typename T>
static int dispatch(const tgt_node_attention_args& a, hipStream_t st) {
    switch ((a.N + 15) / 16) {
        case 5: return dispatch_d<T, 5>(a, st);
        case 6: return dispatch_d<T, 6>(a, st);
        case 7: return dispatch_d<T, 7>(a, st);
        case 8: return dispatch_d<T, 8>(a, st);
        default: return -1;
    }
}

}  // namespace nkbb

// Shapes the key-blocked backward takes: 16-bit, 65 <= N <= 128, H a multiple of 8, D in {8, 12, 16}, 16-byte aligned rows.
// TGT_NODE_KB_BWD (A/B): 0 off (the lane-per-head pair of node_attention.hip), 1 (default) on.  Host logic only.
bool node_attention_kb_bwd_eligible(const tgt_node_attention_args& a, bool bwd) {
    static const int mode = getenv("TGT_NODE_KB_BWD") ? atoi(getenv("TGT_NODE_KB_BWD")) : 1;
    if (!mode || !bwd || a.logits_only || a.dtype == TGT_F32) return false;
    if (a.N <= 64 || a.N > 128 || a.H % na16::HG || !(a.D == 8 || a.D == 12 || a.D == 16)) return false;
    if (!a.mask || !a.vatt || !a.lse || !a.gsum) return false;
    // per-graph buffer resources: every in-range byte offset must stay below the out-of-range sentinel kOob (node_tiles16.hpp)
    const int64_t per_graph = (int64_t)a.N * a.N * (a.ld_eg > a.H ? a.ld_eg : a.H) * 2, per_graph_q = (int64_t)a.N * a.ld_qkv * 2;
    if (per_graph >= (int64_t)0x7ffffff0 || per_graph_q >= (int64_t)0x7ffffff0) return false;
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    if (a.ld_qkv % 8 || a.q_off % 8 || a.k_off % 8 || a.v_off % 8 || a.ld_eg % 8 || a.e_off % 8 || a.g_off % 8) return false;
    if (!al16(a.qkv) || !al16(a.eg) || !al16(a.vatt) || (a.hhat && !al16(a.hhat))) return false;
    if (!al16(a.d_qkv) || !al16(a.d_eg) || !al16(a.d_vatt) || (a.d_hhat && !al16(a.d_hhat))) return false;
    return true;
}

// returns TGT_OK / an error; call only when node_attention_kb_bwd_eligible()
int node_attention_kb_bwd_run(const tgt_node_attention_args& a, hipStream_t st) {
    int e = a.dtype == TGT_BF16 ? nkbb::dispatch<bf16_t>(a, st) : nkbb::dispatch<f16_t>(a, st);
    if (e < 0) return set_error(TGT_ERR_UNSUPPORTED, "node attention (key-blocked backward): unsupported N=%d D=%d", a.N, a.D);
    return e;
}

}  // namespace tgt
