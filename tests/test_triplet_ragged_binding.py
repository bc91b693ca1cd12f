"""CPU-side checks of the per-graph node counts of the triplet attention kernels (tgt_triplet_attention_fwd_counts / _bwd_counts /
_proj_fwd_counts, tgt_mask_node_counts): NEW symbols only -- header, ctypes mirror and library agree on them, the ABI version
and the argument struct stay what they were, the old entry points still resolve, and the new ones refuse a NULL argument block
before anything is launched."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
NEW = ['tgt_mask_node_counts', 'tgt_triplet_attention_fwd_counts', 'tgt_triplet_attention_bwd_counts', 'tgt_triplet_attention_proj_fwd_counts']
OLD = ['tgt_triplet_attention_fwd', 'tgt_triplet_attention_bwd', 'tgt_triplet_attention_proj_fwd', 'tgt_triplet_attention_proj_supported',
       'tgt_triplet_attention_workspace_bytes']


def _declared():
    with open(HEADER) as fh:
        return set(re.findall(r'^\w[\w \*]*?\b(tgt_\w+)\s*\(', fh.read(), re.M))


def test_new_symbols_are_declared_bound_and_exported():
    from tgt_amd import _lib
    declared = _declared()
    L = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None


def test_counts_signatures_are_the_plain_ones_plus_one_pointer():
    from tgt_amd import _lib
    S = _lib.SYMBOLS
    for name in ('tgt_triplet_attention_fwd', 'tgt_triplet_attention_bwd', 'tgt_triplet_attention_proj_fwd'):
        res, args = S[name]
        res_c, args_c = S[name + '_counts']
        assert res_c is res
        assert args_c == [args[0], C.c_void_p] + args[1:], name          # node_counts right behind the argument block
    assert S['tgt_mask_node_counts'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p])


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    TA = _lib.TripletAttentionArgs
    assert C.sizeof(TA) == 312
    assert TA.workspace.offset + 16 == C.sizeof(TA)
    assert not hasattr(TA, 'node_counts')                                # the counts travel beside the struct, not in it


def test_old_entry_points_still_resolve():
    from tgt_amd import _lib
    L = _lib.lib()
    declared = _declared()
    for name in OLD:
        assert name in declared and name in _lib.SYMBOLS and getattr(L, name) is not None, name


def test_null_argument_block_is_refused_before_any_launch():
    """NULL args: TGT_ERR_INVALID (1) from every new entry point; the counts pointer given is a host address that a launch would
    fault on -- it is never looked at"""
    from tgt_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.POINTER(_lib.TripletAttentionArgs)()
    assert L.tgt_triplet_attention_fwd_counts(null, p, None) == 1
    assert b'null args' in L.tgt_last_error()
    assert L.tgt_triplet_attention_bwd_counts(null, p, None) == 1
    assert L.tgt_triplet_attention_proj_fwd_counts(null, p, p, 256, p, p, None) == 1
    assert b'null argument' in L.tgt_last_error()
    # the old entry points forward with NULL counts and answer the same
    assert L.tgt_triplet_attention_fwd(null, None) == 1 and L.tgt_triplet_attention_bwd(null, None) == 1
    assert L.tgt_triplet_attention_proj_fwd(null, p, 256, p, p, None) == 1
    # the count kernel: null tensors / bad sizes are refused, an empty batch is a no-op
    assert L.tgt_mask_node_counts(None, 2, 4, None, None) == 1
    assert L.tgt_mask_node_counts(p, -1, 4, p, None) == 1
    assert L.tgt_mask_node_counts(None, 0, 4, None, None) == 0


def test_knob_defaults_off():
    from tgt_amd import knobs
    assert knobs._SPEC['tri_ragged'][:3] == ('TGT_TRI_RAGGED', False, 'flag')


def test_python_signatures_take_node_counts_last():
    import inspect
    from tgt_amd import ops
    from tgt_amd.tgt.layers.triplet import TripletAttention, TripletAttentionUngated, AxialAttention, TripletAggregate
    for fn in (ops.triplet_attention, ops.projected_triplet_attention):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == 'node_counts' and params[-1].default is None, fn
    for cls in (TripletAttention, TripletAttentionUngated, AxialAttention):
        assert cls.takes_node_counts is True
        assert 'node_counts' in inspect.signature(cls.attend).parameters
        assert 'node_counts' in inspect.signature(cls.forward_normed).parameters
    assert not getattr(TripletAggregate, 'takes_node_counts', False)     # the aggregate family takes no counts
