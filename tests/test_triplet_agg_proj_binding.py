"""CPU-side checks of the projection-fused triplet aggregate forward (tgt_triplet_aggregate_proj_supported / _proj_fwd,
csrc/triplet_aggregate_proj.hip): two NEW symbols next to an unchanged ABI -- version, argument struct -- whose entry point
checks sizes, then the supported predicate, then the tensors, before anything is launched.  Host pointers are never dereferenced."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
# sizeof(tgt_triplet_aggregate_args) of ABI 32, from the struct as it stood before these symbols: 6 int32 (24) | v[2], ld_v[2] (32)
# | v_off[2] (8) | eg[2], ld_eg[2] (32) | e_off[2], g_off[2] (16) | mask, out, ld_out (24) | o_off[2] (8) | d_out (8) | d_v[2],
# d_eg[2] (32) | dropout_p, _pad1 (8) | dropout_seed (8)
AGG_ARGS_BYTES = 24 + 32 + 8 + 32 + 16 + 24 + 8 + 8 + 32 + 8 + 8


def _args(N=20, H=16, D=16, dtype=None, gated=True):
    from tgt_amd import _lib
    a = _lib.TripletAggregateArgs()
    a.B, a.N, a.H, a.D = 2, N, H, D
    a.dtype = _lib.TGT_BF16 if dtype is None else dtype
    a.flags = (_lib.TRI_BIASED | _lib.TRI_GATED) if gated else (_lib.TRI_BIASED | _lib.TRI_MASK_OUT)
    return a


def test_symbols_exist_with_the_declared_signatures():
    from tgt_amd import _lib
    TA, vp, i32 = C.POINTER(_lib.TripletAggregateArgs), C.c_void_p, C.c_int32
    assert _lib.SYMBOLS['tgt_triplet_aggregate_proj_supported'] == (C.c_int, [TA, i32])
    assert _lib.SYMBOLS['tgt_triplet_aggregate_proj_fwd'] == (C.c_int, [TA, vp, i32, vp, vp, vp])
    L = _lib.lib()
    for name in ('tgt_triplet_aggregate_proj_supported', 'tgt_triplet_aggregate_proj_fwd'):
        fn = getattr(L, name)                                   # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    with open(HEADER) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert 'int tgt_triplet_aggregate_proj_supported(const tgt_triplet_aggregate_args* a, int32_t C);' in text
    assert ('int tgt_triplet_aggregate_proj_fwd(const tgt_triplet_aggregate_args* a, const void* x, int32_t C, const void* w, '
            'const void* b, void* stream);') in text


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    assert AGG_ARGS_BYTES == 200
    assert C.sizeof(_lib.TripletAggregateArgs) == AGG_ARGS_BYTES
    assert _lib.TripletAggregateArgs.dropout_seed.offset + 8 == AGG_ARGS_BYTES
    assert 'tgt_triplet_aggregate_proj.hip' not in _lib.SOURCES and 'triplet_aggregate_proj.hip' in _lib.SOURCES


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('N', [20, 32])
def test_supported_shapes(N, dtype, gated):
    from tgt_amd import _lib
    a = _args(N=N, dtype=dict(bf16=_lib.TGT_BF16, f16=_lib.TGT_F16)[dtype], gated=gated)
    assert _lib.lib().tgt_triplet_aggregate_proj_supported(C.byref(a), 256) == 1


@pytest.mark.parametrize('change', ['N=33', 'D=8', 'H=8', 'fp32', 'C=128'])
def test_unsupported_shapes_are_refused_before_the_tensors_are_looked_at(change):
    from tgt_amd import _lib
    L = _lib.lib()
    a, width = _args(), 256
    if change == 'N=33':
        a.N = 33
    elif change == 'D=8':
        a.D = 8
    elif change == 'H=8':
        a.H = 8
    elif change == 'fp32':
        a.dtype = _lib.TGT_F32
    else:
        width = 128
    assert L.tgt_triplet_aggregate_proj_supported(C.byref(a), width) == 0
    # every tensor NULL: the answer is UNSUPPORTED, not "null tensor" -- the predicate comes first, and nothing is launched
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), None, width, None, None, None) == ERR_UNSUPPORTED
    assert b'projected triplet aggregate needs' in L.tgt_last_error()


def test_bad_sizes_come_before_the_predicate():
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args()
    a.N, a.D = -1, 8
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), None, 256, None, None, None) == ERR_INVALID
    assert b'bad sizes' in L.tgt_last_error()
    assert L.tgt_triplet_aggregate_proj_fwd(None, None, 256, None, None, None) == ERR_INVALID


@pytest.mark.parametrize('gated', [True, False])
def test_supported_call_with_null_tensors_is_invalid(gated):
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args(gated=gated)
    assert L.tgt_triplet_aggregate_proj_supported(C.byref(a), 256) == 1
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), None, 256, None, None, None) == ERR_INVALID
    assert b'null tensor' in L.tgt_last_error()
    # with x / w / b given (host addresses: never dereferenced, nothing is launched) the refusal is still INVALID, for eg / mask / out
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
    assert b'null tensor' in L.tgt_last_error()
    # ... and a->v is never examined: giving it changes nothing
    a.v = (C.c_void_p * 2)(p, p)
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
    assert b'null tensor' in L.tgt_last_error()


def test_eg_columns_outside_their_row_are_refused():
    """every tensor given (host addresses: never dereferenced), a pitch that cannot hold the E / G columns: INVALID, nothing launched"""
    from tgt_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    for ld, e_off, g_off in ((8, 0, 0), (64, 56, 16), (64, 0, 49), (64, -1, 16)):
        a = _args()
        a.eg = (C.c_void_p * 2)(p, p)
        a.mask, a.out, a.ld_out = p, p, 512
        a.o_off = (C.c_int32 * 2)(0, 256)
        a.ld_eg = (C.c_int64 * 2)(ld, ld)
        a.e_off, a.g_off = (C.c_int32 * 2)(e_off, e_off), (C.c_int32 * 2)(g_off, g_off)
        assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
        assert b'outside the E/G row' in L.tgt_last_error()


def test_knob_is_a_flag_read_through_the_spec():
    """TGT_AGG_PROJ_INFER ships ON: in the A/B run of DESIGN.md 4.za the slowest knob-on run of the config-5 inference benchmark
    beat the fastest knob-off run"""
    from tgt_amd import knobs, ops
    assert knobs._SPEC['agg_proj_infer'][:3] == ('TGT_AGG_PROJ_INFER', True, 'flag')
    assert knobs._read('TGT_AGG_PROJ_INFER_unset_', True, 'flag') is True
    assert isinstance(knobs.K.agg_proj_infer, bool)
    assert ops._AGG_PROJ_INFER == knobs.K.agg_proj_infer
