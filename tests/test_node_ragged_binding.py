"""CPU-side checks of node attention's per-graph node counts (tgt_node_attention_fwd_counts / _bwd_counts): NEW symbols only --
header, ctypes mirror and library agree on them, the ABI version and the argument struct stay what they were, the entry points
without counts still resolve, what the plain entry points refuse is refused in the same words before anything is launched, and
the switch ships off."""
import ctypes as C
import inspect
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
NEW = ['tgt_node_attention_fwd_counts', 'tgt_node_attention_bwd_counts']
OLD = ['tgt_node_attention_fwd', 'tgt_node_attention_bwd', 'tgt_node_attention_family']


def _header():
    with open(HEADER) as fh:
        return fh.read()


def test_new_symbols_are_declared_bound_and_exported():
    from tgt_amd import _lib
    declared = set(re.findall(r'^\w[\w \*]*?\b(tgt_\w+)\s*\(', _header(), re.M))
    L = _lib.lib()
    for name in NEW + OLD:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None


def test_signatures_are_the_plain_ones_plus_one_pointer_behind_the_argument_block():
    from tgt_amd import _lib
    S = _lib.SYMBOLS
    h = re.sub(r'\s+', ' ', _header())
    for d in ('fwd', 'bwd'):
        assert f'int tgt_node_attention_{d}(const tgt_node_attention_args* a, void* stream);' in h
        assert f'int tgt_node_attention_{d}_counts(const tgt_node_attention_args* a, const int32_t* node_counts, void* stream);' in h
        res, args = S[f'tgt_node_attention_{d}']
        assert S[f'tgt_node_attention_{d}_counts'] == (res, [args[0], C.c_void_p] + args[1:])
    assert 'tgt_node_attention_fwd_counts / _bwd_counts, under the contract stated there.' in h


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    NA = _lib.NodeAttentionArgs
    assert C.sizeof(NA) == 184
    want = dict(B=0, N=4, H=8, D=12, dtype=16, scale_degree=20, logits_only=24, _pad0=28, scale=32, _pad1=36, qkv=40, ld_qkv=48,
                q_off=56, k_off=60, v_off=64, _pad2=68, eg=72, ld_eg=80, e_off=88, g_off=92, mask=96, vatt=104, hhat=112, lse=120,
                gsum=128, d_vatt=136, d_hhat=144, d_qkv=152, d_eg=160, _reserved0=168, hhat_scale=176)
    assert {name: getattr(NA, name).offset for name, _ in NA._fields_} == want
    assert not any('count' in name for name, _ in NA._fields_)          # the counts travel beside the struct, not in it


def _args(**kw):
    from tgt_amd import _lib
    a = _lib.NodeAttentionArgs()
    a.B, a.N, a.H, a.D, a.dtype = 2, 8, 32, 8, _lib.TGT_BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refusals_are_those_of_the_plain_entry_points_before_any_launch():
    """NULL args, bad sizes, null tensors: TGT_ERR_INVALID (1) with the plain entry point's message, with and without a count
    pointer (a fake address a launch would fault on -- the refusal comes first); then the count pointer's own alignment"""
    from tgt_amd import _lib
    L = _lib.lib()
    null = C.POINTER(_lib.NodeAttentionArgs)()
    fake = C.c_void_p(64)
    for d in ('fwd', 'bwd'):
        plain, counts = getattr(L, f'tgt_node_attention_{d}'), getattr(L, f'tgt_node_attention_{d}_counts')
        for a in (None, _args(B=-1), _args(), _args(qkv=64, eg=64), _args(qkv=64, eg=64, logits_only=1)):
            ref = null if a is None else C.byref(a)
            want = plain(ref, None)
            msg = L.tgt_last_error()
            if d == 'bwd' or not (a is not None and a.logits_only):
                assert want == 1, (d, want, msg)
            for nc in (None, fake):
                assert counts(ref, nc, None) == want
                assert L.tgt_last_error() == msg
        # nothing to do (B == 0): TGT_OK whatever the pointer, as the plain call
        assert plain(C.byref(_args(B=0)), None) == 0 and counts(C.byref(_args(B=0)), fake, None) == 0
    # every tensor present (fake addresses), a misaligned count pointer: refused by the new check, nothing launched
    full = dict(qkv=64, eg=64, mask=64, vatt=64, hhat=64, lse=64, gsum=64, d_vatt=64, d_hhat=64, d_qkv=64, d_eg=64,
                ld_qkv=3 * 256, ld_eg=64, k_off=256, v_off=512, g_off=32)
    for d in ('fwd', 'bwd'):
        assert getattr(L, f'tgt_node_attention_{d}_counts')(C.byref(_args(**full)), C.c_void_p(66), None) == 1
        assert b'node_counts' in L.tgt_last_error() and b'aligned' in L.tgt_last_error()


def test_routing_does_not_look_at_the_counts():
    """tgt_node_attention_family is the router with and without counts: its signature has no count argument"""
    from tgt_amd import _lib
    assert _lib.SYMBOLS['tgt_node_attention_family'] == (C.c_int, [C.POINTER(_lib.NodeAttentionArgs), C.c_int32])


def test_knob_defaults_off():
    from tgt_amd import knobs
    assert knobs._SPEC['node_ragged'][:3] == ('TGT_NODE_RAGGED', False, 'flag')
    assert knobs._read('TGT_NODE_RAGGED_never_set', False, 'flag') is False
    assert 'node_ragged' in {f.name for f in __import__('dataclasses').fields(knobs.Knobs)}


def test_python_surface():
    from tgt_amd import ops
    from tgt_amd.tgt import stack
    from tgt_amd.tgt.layers import blocks
    assert inspect.signature(ops.node_attention).parameters['node_counts'].default is None
    assert inspect.signature(blocks.EGT_Attention.attend).parameters['node_counts'].default is None
    assert 'node_counts' not in inspect.signature(blocks.EdgeUpdate.forward).parameters
    assert stack._NODE_RAGGED is False or os.environ.get('TGT_NODE_RAGGED') == '1'
    assert hasattr(stack.TGT_Encoder, '_node_ragged_ok')
