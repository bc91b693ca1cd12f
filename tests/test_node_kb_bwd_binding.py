"""CPU-side checks of tgt_node_attention_family(): which kernel family the node attention entry points launch for a call.  The
query is host logic on sizes, dtype, offsets, pointer nullness and alignment, so the addresses below are fake (never dereferenced).
The key-blocked backward (csrc/node_attention_kb_bwd.hip) takes 16-bit calls with 65 <= N <= 128, H % 8 == 0, D in {8, 12, 16};
everything else keeps the routing it had."""
import ctypes as C

import pytest

F32, BF16, F16 = 0, 1, 2
ADDR = 0x10000000                  # a 16-byte aligned fake address


def _args(N=80, H=8, D=12, dtype=BF16, B=2, logits_only=0):
    from tgt_amd import _lib
    a = _lib.NodeAttentionArgs()
    W = D * H
    a.B, a.N, a.H, a.D = B, N, H, D
    a.dtype, a.scale_degree, a.logits_only = dtype, 1, logits_only
    a.scale = float(D) ** -0.5
    a.qkv, a.ld_qkv = ADDR, 3 * W
    a.q_off, a.k_off, a.v_off = 0, W, 2 * W
    a.eg, a.ld_eg = ADDR + 0x1000000, 2 * H
    a.e_off, a.g_off = 0, H
    for i, f in enumerate(('mask', 'vatt', 'hhat', 'lse', 'gsum', 'd_vatt', 'd_hhat', 'd_qkv', 'd_eg')):
        setattr(a, f, ADDR + (i + 2) * 0x1000000)
    return a


def _family(a, bwd):
    from tgt_amd import _lib
    return _lib.lib().tgt_node_attention_family(C.byref(a), bwd)


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('N', [65, 80, 128])
@pytest.mark.parametrize('H', [8, 16, 64])
@pytest.mark.parametrize('D', [8, 12, 16])
def test_backward_of_65_to_128_nodes_is_key_blocked(dtype, N, H, D):
    from tgt_amd import _lib
    assert _family(_args(N=N, H=H, D=D, dtype=dtype), 1) == _lib.NODE_FAMILY_KB_BWD


def test_backward_outside_the_shape_set_stays_lane_per_head():
    from tgt_amd import _lib
    lane = _lib.NODE_FAMILY_LANE
    assert _family(_args(N=129), 1) == lane
    assert _family(_args(dtype=F32), 1) == lane
    assert _family(_args(D=4), 1) == lane
    assert _family(_args(H=12), 1) == lane
    assert _family(_args(logits_only=1), 1) == lane
    a = _args()
    a.d_eg = a.d_eg + 8                                  # not 16-byte aligned
    assert _family(a, 1) == lane


def test_backward_up_to_64_nodes_is_unchanged():
    from tgt_amd import _lib
    assert _family(_args(N=64), 1) == _lib.NODE_FAMILY_TILES16
    assert _family(_args(N=33), 1) == _lib.NODE_FAMILY_TILES16
    assert _family(_args(N=32), 1) == _lib.NODE_FAMILY_MFMA32


def test_forward_is_unchanged():
    from tgt_amd import _lib
    assert _family(_args(N=80, H=32), 0) == _lib.NODE_FAMILY_KB_FWD
    assert _family(_args(N=80, H=8), 0) == _lib.NODE_FAMILY_LANE


def test_invalid_arguments_are_negative():
    from tgt_amd import _lib
    L = _lib.lib()
    assert L.tgt_node_attention_family(None, 0) < 0 and L.tgt_node_attention_family(None, 1) < 0
    a = _args()
    a.d_qkv = None
    assert _family(a, 1) < 0 and _family(a, 0) == _lib.NODE_FAMILY_LANE     # (the forward does not look at d_qkv)
    assert _family(_args(H=0), 1) < 0
    assert _family(_args(B=0), 1) == _lib.NODE_FAMILY_NONE


def test_constants_mirror_the_header():
    import os
    import re
    from tgt_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')) as fh:
        hdr = fh.read()
    for name in ('NONE', 'LANE', 'MFMA32', 'TILES16', 'KB_FWD', 'KB_BWD'):
        m = re.search(r'TGT_NODE_FAMILY_%s = (\d+)' % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, 'NODE_FAMILY_' + name), name


def test_abi_and_struct_layout_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    assert C.sizeof(_lib.NodeAttentionArgs) == 184       # the value before tgt_node_attention_family() was added
    assert _lib.NodeAttentionArgs._reserved0.offset + 16 == C.sizeof(_lib.NodeAttentionArgs)
