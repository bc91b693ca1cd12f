"""CPU-side checks of TGT_TRI_NO_QKV_STORE (tgt_triplet_attention_proj_fwd without the Q/K/V rows): the flag is a VALUE only --
header, ctypes mirror, ABI version and argument struct stay as they were -- and the entry point takes the flagged call before it
looks at tensors."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')


def _header_tri_flags():
    with open(HEADER) as fh:
        text = fh.read()
    return {name: int(val, 0) for name, val in re.findall(r'^\s*(TGT_TRI_\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)\s*,', text, re.M)}


def test_flag_constant_mirrors_the_header():
    from tgt_amd import _lib
    flags = _header_tri_flags()
    assert 'TGT_TRI_NO_QKV_STORE' in flags, sorted(flags)
    assert _lib.TRI_NO_QKV_STORE == flags['TGT_TRI_NO_QKV_STORE']
    assert (_lib.TRI_BIASED, _lib.TRI_GATED, _lib.TRI_MASK_OUT) == (flags['TGT_TRI_BIASED'], flags['TGT_TRI_GATED'], flags['TGT_TRI_MASK_OUT'])


def test_flag_is_one_bit_that_no_other_triplet_flag_uses():
    flags = _header_tri_flags()
    v = flags['TGT_TRI_NO_QKV_STORE']
    assert v > 0 and v & (v - 1) == 0
    for name, other in flags.items():
        if name != 'TGT_TRI_NO_QKV_STORE':
            assert not (v & other), (name, other)
    assert len(set(flags.values())) == len(flags)


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    TA = _lib.TripletAttentionArgs
    assert C.sizeof(TA) == 312                                   # the struct of ABI 32 (tests/test_triplet_kb_binding.py pins its tail)
    assert TA.workspace.offset + 16 == C.sizeof(TA)
    assert TA.flags.offset == 20 and TA.flags.size == 4


def test_knob_defaults_on():
    from tgt_amd import knobs
    assert knobs._SPEC['tri_proj_infer'][:2] == ('TGT_TRI_PROJ_INFER', True)
    assert knobs._read('TGT_TRI_PROJ_INFER_unset_', True, 'flag') is True


def test_flagged_call_with_null_tensors_is_invalid_not_unsupported():
    """flag set, qkv NULL and x / w / bias / out / mask NULL: the shape is ACCEPTED (not TGT_ERR_UNSUPPORTED) and the call is
    refused for its null tensors, before any launch.  (A regression guard: the unflagged call answers the same.)"""
    from tgt_amd import _lib
    L = _lib.lib()
    a = _lib.TripletAttentionArgs()
    a.B, a.N, a.H, a.D, a.dtype = 2, 20, 16, 16, _lib.TGT_BF16
    a.flags = _lib.TRI_BIASED | _lib.TRI_GATED | _lib.TRI_NO_QKV_STORE
    a.scale = 0.25
    assert L.tgt_triplet_attention_proj_supported(C.byref(a), 256) == 1          # (the flag widens nothing ...)
    a.N = 33
    assert L.tgt_triplet_attention_proj_supported(C.byref(a), 256) == 0          # (... and nothing above N = 32)
    a.N = 20
    assert L.tgt_triplet_attention_proj_fwd(C.byref(a), None, 256, None, None, None) == 1      # TGT_ERR_INVALID
    # with x / w / bias given (host addresses: never dereferenced, nothing is launched) the refusal is still INVALID, for out / mask
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.tgt_triplet_attention_proj_fwd(C.byref(a), p, 256, p, p, None) == 1
    assert b'null tensor' in L.tgt_last_error()
