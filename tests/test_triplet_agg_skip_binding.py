"""CPU-side checks of the triplet aggregate entry points that take the per-graph DropPath factor (tgt_triplet_aggregate_fwd_skip /
_bwd_skip / _proj_fwd_skip): three NEW symbols next to an unchanged ABI -- version, argument struct -- the factor travels as an
extra argument.  Every check of the entry points without _skip keeps its place and words; one new check (a factor that is not
4-byte aligned) comes after them.  Nothing is launched and no host pointer is dereferenced."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
NAMES = ('tgt_triplet_aggregate_fwd_skip', 'tgt_triplet_aggregate_bwd_skip', 'tgt_triplet_aggregate_proj_fwd_skip')


def _args(N=20, H=16, D=16, dtype=None, gated=True):
    from tgt_amd import _lib
    a = _lib.TripletAggregateArgs()
    a.B, a.N, a.H, a.D = 2, N, H, D
    a.dtype = _lib.TGT_BF16 if dtype is None else dtype
    a.flags = (_lib.TRI_BIASED | _lib.TRI_GATED) if gated else (_lib.TRI_BIASED | _lib.TRI_MASK_OUT)
    return a


def _host():
    """(buffer, its 64-byte aligned address): host memory standing in for tensors and factors -- never dereferenced"""
    buf = (C.c_char * 256)()
    return buf, (C.addressof(buf) + 63) & ~63


def _factors():
    """the factor arguments of every refusal below: none, and a host address"""
    buf, p = _host()
    return buf, (None, C.c_void_p(p))


def _valid_looking(a, p, bwd=False):
    """every tensor given (host address p, 64-byte aligned), rows and offsets aligned"""
    vp = C.c_void_p
    a.v, a.eg = (vp * 2)(p, p), (vp * 2)(p, p)
    a.ld_v, a.ld_eg = (C.c_int64 * 2)(576, 576), (C.c_int64 * 2)(576, 576)
    a.v_off, a.e_off, a.g_off = (C.c_int32 * 2)(0, 256), (C.c_int32 * 2)(512, 544), (C.c_int32 * 2)(528, 560)
    a.mask, a.out, a.ld_out = p, p, 512
    a.o_off = (C.c_int32 * 2)(0, 256)
    if bwd:
        a.d_out, a.d_v, a.d_eg = p, (vp * 2)(p, p), (vp * 2)(p, p)
    return a


def test_symbols_exist_with_the_declared_signatures():
    from tgt_amd import _lib
    TA, vp, i32 = C.POINTER(_lib.TripletAggregateArgs), C.c_void_p, C.c_int32
    assert _lib.SYMBOLS['tgt_triplet_aggregate_fwd_skip'] == (C.c_int, [TA, vp, vp])
    assert _lib.SYMBOLS['tgt_triplet_aggregate_bwd_skip'] == (C.c_int, [TA, vp, vp])
    assert _lib.SYMBOLS['tgt_triplet_aggregate_proj_fwd_skip'] == (C.c_int, [TA, vp, vp, i32, vp, vp, vp])
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)                                   # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    with open(HEADER) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert 'int tgt_triplet_aggregate_fwd_skip(const tgt_triplet_aggregate_args* a, const float* graph_scale, void* stream);' in text
    assert 'int tgt_triplet_aggregate_bwd_skip(const tgt_triplet_aggregate_args* a, const float* graph_scale, void* stream);' in text
    assert ('int tgt_triplet_aggregate_proj_fwd_skip(const tgt_triplet_aggregate_args* a, const float* graph_scale, const void* x, '
            'int32_t C, const void* w, const void* b, void* stream);') in text
    assert 'The aggregate and node attention families take no counts' in text


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    assert C.sizeof(_lib.TripletAggregateArgs) == 200
    assert _lib.TripletAggregateArgs.dropout_seed.offset + 8 == 200
    assert not hasattr(_lib.TripletAggregateArgs, 'graph_scale')


@pytest.mark.parametrize('name', NAMES[:2])
def test_plain_entry_points_keep_their_checks_and_their_order(name):
    from tgt_amd import _lib
    fn = getattr(_lib.lib(), name)
    L = _lib.lib()
    keep, factors = _factors()
    for gs in factors:
        assert fn(None, gs, None) == ERR_INVALID and b'null args' in L.tgt_last_error()
        a = _args()
        a.N = -1
        assert fn(C.byref(a), gs, None) == ERR_INVALID and b'bad sizes' in L.tgt_last_error()
        a = _args()
        a.H = 0
        assert fn(C.byref(a), gs, None) == ERR_INVALID and b'bad sizes' in L.tgt_last_error()
        # N > 128 before D != 16 at N > 64, both before the tensors (all NULL here)
        a = _args(N=129, D=8)
        assert fn(C.byref(a), gs, None) == ERR_UNSUPPORTED and b'> 128 not supported' in L.tgt_last_error()
        a = _args(N=72, D=8)
        assert fn(C.byref(a), gs, None) == ERR_UNSUPPORTED and b'D = 16 only' in L.tgt_last_error()
        for N in (20, 72):
            a = _args(N=N)
            assert fn(C.byref(a), gs, None) == ERR_INVALID and b'null tensor' in L.tgt_last_error()
        # an empty batch is done before anything is looked at
        a = _args()
        a.B = 0
        assert fn(C.byref(a), gs, None) == 0
    # tensors given (host addresses: never dereferenced), a row that is not 16-byte aligned: refused before the factor is looked at
    buf, p = _host()
    a = _valid_looking(_args(), p, bwd=True)
    a.ld_out = 513
    assert fn(C.byref(a), C.c_void_p(p + 1), None) == ERR_INVALID and b'16-byte aligned' in L.tgt_last_error()


def test_backward_gradient_tensors_are_checked_before_the_factor():
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    a = _valid_looking(_args(), p, bwd=False)                   # no d_out / d_v / d_eg
    assert L.tgt_triplet_aggregate_bwd_skip(C.byref(a), C.c_void_p(p + 1), None) == ERR_INVALID
    assert b'null/misaligned gradient tensor' in L.tgt_last_error()


def test_proj_entry_point_keeps_its_checks_and_their_order():
    from tgt_amd import _lib
    L = _lib.lib()
    fn = L.tgt_triplet_aggregate_proj_fwd_skip
    keep, factors = _factors()
    for gs in factors:
        assert fn(None, gs, None, 256, None, None, None) == ERR_INVALID
        a = _args()
        a.N, a.D = -1, 8
        assert fn(C.byref(a), gs, None, 256, None, None, None) == ERR_INVALID and b'bad sizes' in L.tgt_last_error()
        # the supported predicate comes before the tensors (all NULL)
        for change in ('N=33', 'D=8', 'H=8', 'fp32', 'C=128'):
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
            assert fn(C.byref(a), gs, None, width, None, None, None) == ERR_UNSUPPORTED
            assert b'projected triplet aggregate needs' in L.tgt_last_error()
        a = _args()
        assert fn(C.byref(a), gs, None, 256, None, None, None) == ERR_INVALID and b'null tensor' in L.tgt_last_error()
    # E/G columns outside their row: refused before the factor is looked at
    buf, p = _host()
    a = _valid_looking(_args(), p)
    a.ld_eg = (C.c_int64 * 2)(8, 8)
    assert fn(C.byref(a), C.c_void_p(p + 1), p, 256, p, p, None) == ERR_INVALID and b'outside the E/G row' in L.tgt_last_error()


@pytest.mark.parametrize('name,N', [(NAMES[0], 20), (NAMES[0], 72), (NAMES[1], 20), (NAMES[1], 72), (NAMES[2], 20)])
def test_factor_at_an_odd_address_is_invalid(name, N):
    """every other argument looks valid (host addresses, aligned): the one new check refuses, nothing is launched"""
    from tgt_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    buf, p = _host()
    proj = name.endswith('proj_fwd_skip')
    a = _valid_looking(_args(N=N), p, bwd='bwd' in name)
    for odd in (1, 2, 3):
        gs = C.c_void_p(p + 64 + odd)
        rc = fn(C.byref(a), gs, p, 256, p, p, None) if proj else fn(C.byref(a), gs, None)
        assert rc == ERR_INVALID
        assert b'graph_scale must be 4-byte aligned' in L.tgt_last_error()
