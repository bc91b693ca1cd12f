"""Node attention: the cases that hold every kernel family to the float64 oracle, with the family each case must take
(tests/test_node_family_cases.py checks the table on the CPU, tests/test_hip_node_families.py runs the kernels).

tgt_node_attention_fwd / _bwd route a call to one of five families (include/tgt_hip.h TGT_NODE_FAMILY_*, node_attention_family() in
csrc/node_attention.hip).  tgt_node_attention_family() names the family, not the variant inside LANE; the variant below is read
off launch_node() / node_vec() of csrc/node_attention.hip and stated per case:

  forward   16-bit, D <= 16, H % 4 == 0, W % 8 == 0   node_att_fwd_lds_kernel, 4 heads per lane, (H + 3) / 4 lanes per node,
                                                      min(512 / lanes, N, 32) queries per workgroup, key tiles of 32
            anything else                             node_att_fwd_kernel at HV = 4 (D <= 16 and H % 4 == 0), else 2 (H % 2 == 0), else 1
  backward  row pass + column pass                    HV = 2 (H % 2 == 0), else 1; a second head block above 64 * HV heads

  hard inputs   the construction of tests/test_hip_ops.py::test_node_attention_arbitrary_mask_and_large_logits: E * 6, +12 on the
                later half of the keys, a per-(query, key) mask of 0 / -inf that is not symmetric -- a random fifth of the pairs, the
                first 16 keys for every third query (the first N // 2 where N <= 16), the first 32 for every fifth where N > 32, the
                last key live for every query (the reference NaNs on an empty row)
  plain inputs  unit-normal columns and golden_util.additive_mask, ragged where B = 2

Plain helper: no pytest hooks or settings."""
import collections
import ctypes as C

import numpy as np
import torch

import golden_util as gu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
BITS16 = (BF16, F16)
BOTH = ('hard', 'plain')

Case = collections.namedtuple('Case', 'shape dtypes fwd bwd kinds')       # shape: (B, N, W, H)

CASES = [
    # MFMA32 both ways: N <= 32, H % 8 == 0, 16-bit
    Case((2, 32, 128, 16), BITS16, 'MFMA32', 'MFMA32', BOTH),             # D = 8, every row and key of the 32-wide tile live
    Case((2, 20, 192, 16), BITS16, 'MFMA32', 'MFMA32', BOTH),             # D = 12
    Case((1, 9, 128, 8), BITS16, 'MFMA32', 'MFMA32', BOTH),               # D = 16, N // 2 = 4 leading keys masked
    # LANE in fp32: plain forward at HV = 4, backward at HV = 2
    Case((2, 40, 96, 8), (F32,), 'LANE', 'LANE', BOTH),                   # D = 12; two lanes per node forward, four backward
    Case((2, 32, 768, 64), (F32,), 'LANE', 'LANE', BOTH),                 # the fp32 shape of the full-model goldens
    # LANE in 16-bit: LDS forward, backward at HV = 2
    Case((2, 40, 48, 4), BITS16, 'LANE', 'LANE', BOTH),                   # D = 12; one lane per node, query groups 32 + 8, key tiles 32 + 8
    Case((1, 70, 240, 20), BITS16, 'LANE', 'LANE', BOTH),                 # D = 12, H % 8 != 0; five lanes per node, query groups 32 + 32 + 6, key tiles 32 + 32 + 6
    # the plain forward kernel in every dtype
    Case((2, 37, 144, 6), (F32,) + BITS16, 'LANE', 'LANE', BOTH),         # D = 24: forward HV = 2 (D > 16), backward HV = 2
    Case((1, 33, 96, 6), (F32,) + BITS16, 'LANE', 'LANE', BOTH),          # D = 16, H % 4 == 2: forward HV = 2, backward HV = 2
    Case((2, 5, 96, 3), (F32,) + BITS16, 'LANE', 'LANE', BOTH),           # D = 32, odd H: HV = 1 both ways
    Case((1, 7, 20, 5), (F32,) + BITS16, 'LANE', 'LANE', BOTH),           # D = 4, odd H: HV = 1 both ways
    # a second head block: the backward at HV = 2 walks heads 0..127 and 128..131 (hb_count = 2); the fp32 forward at HV = 4 has 33 of
    # 64 lanes live, the 16-bit LDS forward 33 lanes per node
    Case((1, 5, 528, 132), (F32, BF16), 'LANE', 'LANE', BOTH),            # D = 4
    # key-blocked forward, lane-per-head backward above its limit of 128 nodes (HV = 2)
    Case((1, 130, 256, 32), (BF16,), 'KB_FWD', 'LANE', BOTH),             # D = 8
    # the plain half of the families whose hard inputs are EXISTING_HARD
    Case((2, 33, 128, 16), BITS16, 'TILES16', 'TILES16', ('plain',)),     # D = 8, one node past two 16-wide blocks
    Case((1, 65, 64, 8), BITS16, 'LANE', 'KB_BWD', ('plain',)),           # D = 8, one key past four blocks; LDS forward
]

# test_hip_ops.py::test_node_attention_arbitrary_mask_and_large_logits (the first four) and
# test_hip_node_kb_bwd.py::test_arbitrary_mask_and_large_logits (the last two)
EXISTING_HARD = [
    Case((2, 32, 768, 64), BITS16, 'KB_FWD', 'MFMA32', ('hard',)),
    Case((2, 48, 768, 64), BITS16, 'KB_FWD', 'TILES16', ('hard',)),
    Case((1, 64, 256, 32), BITS16, 'KB_FWD', 'TILES16', ('hard',)),
    Case((2, 40, 128, 16), BITS16, 'TILES16', 'TILES16', ('hard',)),
    Case((2, 80, 256, 32), BITS16, 'KB_FWD', 'KB_BWD', ('hard',)),
    Case((1, 128, 128, 8), BITS16, 'LANE', 'KB_BWD', ('hard',)),          # LDS forward
]

# ops.edge_logits (logits_only): LANE both ways, whatever the shape
LOGITS_CASES = [  # B, N, W, H
    (1, 40, 96, 8),       # D = 12; 16-bit: LDS forward, key tiles 32 + 8, query groups 32 + 8; fp32: HV = 4 / 2
    (2, 33, 12, 3),       # D = 4, odd H: the plain forward at HV = 1
    (1, 5, 64, 2),        # D = 32: HV = 2 both ways
    (3, 1, 48, 4),        # N = 1
    (1, 70, 240, 20),     # the LDS forward with query groups 32 + 32 + 6
]

# every (family, direction) the library routes to
ROUTES = [('LANE', 0), ('LANE', 1), ('MFMA32', 0), ('MFMA32', 1), ('TILES16', 0), ('TILES16', 1), ('KB_FWD', 0), ('KB_BWD', 1)]


def families(cases):
    """(B, N, W, H, dtype) -> (forward family, backward family), by name"""
    return {c.shape + (dt,): (c.fwd, c.bwd) for c in cases for dt in c.dtypes}


FAMILIES = families(CASES)


def family_id(name):
    from tgt_amd import _lib
    return getattr(_lib, 'NODE_FAMILY_' + name)


def family(qkv, eg, mask3, H, bwd=1, logits_only=False):
    """tgt_node_attention_family for the call ops.node_attention (ops.edge_logits with logits_only) makes with these tensors
    (the addresses are only looked at)"""
    from tgt_amd import _lib, ops
    a, _ = ops._node_args(qkv, eg, mask3, H, not logits_only, logits_only)
    for f in ('vatt', 'hhat', 'lse', 'gsum', 'd_vatt', 'd_hhat', 'd_qkv', 'd_eg'):
        setattr(a, f, qkv.data_ptr())
    return _lib.lib().tgt_node_attention_family(C.byref(a), bwd)


def shape_family(shape, dtype, bwd, logits_only=False):
    """the same query for a shape alone: meta tensors would have no address, so the call is described with a 16-byte aligned fake one
    (what every torch allocation is)"""
    from tgt_amd import _lib, ops
    B, N, W, H = shape
    a = _lib.NodeAttentionArgs()
    a.B, a.N, a.H, a.D = B, N, H, W // H
    a.dtype, a.scale_degree, a.logits_only = ops._DT[dtype], int(not logits_only), int(bool(logits_only))
    a.scale = float(W // H) ** -0.5
    a.ld_qkv = (2 if logits_only else 3) * W
    a.q_off, a.k_off, a.v_off = 0, W, (0 if logits_only else 2 * W)
    a.ld_eg = H if logits_only else 2 * H
    a.e_off, a.g_off = 0, (0 if logits_only else H)
    fields = ('qkv', 'eg', 'vatt', 'hhat', 'lse', 'gsum', 'd_vatt', 'd_hhat', 'd_qkv', 'd_eg') + (() if logits_only else ('mask',))
    for i, f in enumerate(fields):
        setattr(a, f, 0x10000000 + i * 0x1000000)
    return _lib.lib().tgt_node_attention_family(C.byref(a), bwd)


def num_nodes(shape):
    """plain inputs: ragged where B = 2"""
    B, N = shape[0], shape[1]
    return [N, max(1, N - N // 3)][:B] if B == 2 else [N] * B


def hard_mask(B, N, rng):
    """(B,N,N) float32 in {0, -inf}.  rng: a numpy Generator."""
    m = torch.zeros(B, N, N)
    m[torch.from_numpy(rng.random((B, N, N)) < 0.2)] = -float('inf')
    m[:, 1::3, :(16 if N > 16 else N // 2)] = -float('inf')
    if N > 32:
        m[:, 2::5, :32] = -float('inf')
    m[:, :, N - 1] = 0.0
    return m


def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def inputs(shape, dtype, kind):
    """qkv (B,N,3W), eg (B,N,N,2H), d_vatt (B,N,W), d_hhat (B,N,N,H) in dtype and the (B,N,N) float32 mask"""
    B, N, W, H = shape
    rng = np.random.default_rng(1000 * N + W + H + (0 if kind == 'hard' else 500000))
    qkv, eg = _rnd(rng, B, N, 3 * W), _rnd(rng, B, N, N, 2 * H)
    d_v, d_h = _rnd(rng, B, N, W), _rnd(rng, B, N, N, H)
    if kind == 'hard':
        eg[..., :H] *= 6.0                                  # logits spread over ~ +-20
        eg[:, :, N // 2:, :H] += 12.0                       # the later keys carry the maximum
        mask = hard_mask(B, N, rng)
    else:
        mask = gu.additive_mask(num_nodes(shape), N, torch.float32).reshape(B, N, N)
    return qkv.to(dtype), eg.to(dtype), d_v.to(dtype), d_h.to(dtype), mask
