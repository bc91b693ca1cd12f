"""CPU-side checks of the projection-fused triplet aggregate forward for 33..64 nodes (tgt_triplet_aggregate_proj64_supported /
_proj64_fwd / _proj64_fwd_skip, csrc/triplet_aggregate_proj64.hip): three NEW symbols next to an unchanged ABI -- version,
argument struct -- and next to the unchanged entry points of the N <= 32 kernel.  The entry point checks sizes, then the supported
predicate, then the tensors, the E/G row bounds and the factor's alignment, before anything is launched.  Host pointers are never
dereferenced."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
NAMES = ('tgt_triplet_aggregate_proj64_supported', 'tgt_triplet_aggregate_proj64_fwd', 'tgt_triplet_aggregate_proj64_fwd_skip')


def _args(N=48, H=16, D=16, dtype=None, gated=True):
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


def _valid_looking(a, p):
    """every tensor given (host address p, 64-byte aligned), rows and offsets aligned, E/G in a row of their own"""
    vp = C.c_void_p
    a.eg = (vp * 2)(p, p)
    a.ld_eg = (C.c_int64 * 2)(64, 64)
    a.e_off, a.g_off = (C.c_int32 * 2)(0, 32), (C.c_int32 * 2)(16, 48)
    a.mask, a.out, a.ld_out = p, p, 512
    a.o_off = (C.c_int32 * 2)(0, 256)
    return a


def _calls(L):
    """the two launching entry points as fn(a, x, C, w, b) -- the second with a NULL factor pointer"""
    return (lambda a, x, c, w, b: L.tgt_triplet_aggregate_proj64_fwd(a, x, c, w, b, None),
            lambda a, x, c, w, b: L.tgt_triplet_aggregate_proj64_fwd_skip(a, None, x, c, w, b, None))


def test_symbols_exist_with_the_declared_signatures():
    from tgt_amd import _lib
    TA, vp, i32 = C.POINTER(_lib.TripletAggregateArgs), C.c_void_p, C.c_int32
    assert _lib.SYMBOLS[NAMES[0]] == (C.c_int, [TA, i32])
    assert _lib.SYMBOLS[NAMES[1]] == (C.c_int, [TA, vp, i32, vp, vp, vp])
    assert _lib.SYMBOLS[NAMES[2]] == (C.c_int, [TA, vp, vp, i32, vp, vp, vp])
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)                                   # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    with open(HEADER) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert 'int tgt_triplet_aggregate_proj64_supported(const tgt_triplet_aggregate_args* a, int32_t C);' in text
    assert ('int tgt_triplet_aggregate_proj64_fwd(const tgt_triplet_aggregate_args* a, const void* x, int32_t C, const void* w, '
            'const void* b, void* stream);') in text
    assert ('int tgt_triplet_aggregate_proj64_fwd_skip(const tgt_triplet_aggregate_args* a, const float* graph_scale, const void* x, '
            'int32_t C, const void* w, const void* b, void* stream);') in text


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    assert C.sizeof(_lib.TripletAggregateArgs) == 200
    assert _lib.TripletAggregateArgs.dropout_seed.offset + 8 == 200
    assert 'triplet_aggregate_proj64.hip' in _lib.SOURCES and 'triplet_aggregate_proj.hip' in _lib.SOURCES


@pytest.mark.parametrize('gated', [True, False])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('N', [33, 48, 64])
def test_supported_shapes(N, dtype, gated):
    from tgt_amd import _lib
    a = _args(N=N, dtype=dict(bf16=_lib.TGT_BF16, f16=_lib.TGT_F16)[dtype], gated=gated)
    assert _lib.lib().tgt_triplet_aggregate_proj64_supported(C.byref(a), 256) == 1
    # the two kernels' domains are disjoint
    assert _lib.lib().tgt_triplet_aggregate_proj_supported(C.byref(a), 256) == 0


@pytest.mark.parametrize('change', ['N=32', 'N=65', 'D=8', 'H=8', 'fp32', 'C=128'])
def test_unsupported_shapes_are_refused_before_the_tensors_are_looked_at(change):
    from tgt_amd import _lib
    L = _lib.lib()
    a, width = _args(), 256
    if change.startswith('N='):
        a.N = int(change[2:])
    elif change == 'D=8':
        a.D = 8
    elif change == 'H=8':
        a.H = 8
    elif change == 'fp32':
        a.dtype = _lib.TGT_F32
    else:
        width = 128
    assert L.tgt_triplet_aggregate_proj64_supported(C.byref(a), width) == 0
    # every tensor NULL: the answer is UNSUPPORTED, not "null tensor" -- the predicate comes first, and nothing is launched
    for call in _calls(L):
        assert call(C.byref(a), None, width, None, None) == ERR_UNSUPPORTED
        assert b'needs 33 <= N <= 64' in L.tgt_last_error()


def test_bad_sizes_come_before_the_predicate():
    from tgt_amd import _lib
    L = _lib.lib()
    for call in _calls(L):
        a = _args()
        a.N, a.D = -1, 8
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID
        assert b'bad sizes' in L.tgt_last_error()
        assert call(None, None, 256, None, None) == ERR_INVALID
        assert b'null args' in L.tgt_last_error()


@pytest.mark.parametrize('gated', [True, False])
def test_supported_call_with_null_tensors_is_invalid(gated):
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args(gated=gated)
    assert L.tgt_triplet_aggregate_proj64_supported(C.byref(a), 256) == 1
    buf, p = _host()
    for call in _calls(L):
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID
        assert b'null tensor' in L.tgt_last_error()
        # with x / w / b given (host addresses: nothing is launched) the refusal is still INVALID, for eg / mask / out
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID
        assert b'null tensor' in L.tgt_last_error()
    # ... and a->v is never examined: giving it changes nothing
    a.v = (C.c_void_p * 2)(p, p)
    assert L.tgt_triplet_aggregate_proj64_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
    assert b'null tensor' in L.tgt_last_error()


def test_an_empty_batch_is_done_after_the_predicate_and_before_the_tensors():
    from tgt_amd import _lib
    L = _lib.lib()
    for call in _calls(L):
        a = _args()
        a.B = 0
        assert call(C.byref(a), None, 256, None, None) == 0
        a.N = 20                                                # (not this kernel's shape: the predicate comes first)
        assert call(C.byref(a), None, 256, None, None) == ERR_UNSUPPORTED


def test_eg_columns_outside_their_row_are_refused():
    """every tensor given (host addresses: never dereferenced), a pitch that cannot hold the E / G columns: INVALID, nothing launched
    -- and before the factor is looked at (an odd address)"""
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    for ld, e_off, g_off in ((8, 0, 0), (64, 56, 16), (64, 0, 49), (64, -1, 16)):
        a = _valid_looking(_args(), p)
        a.ld_eg = (C.c_int64 * 2)(ld, ld)
        a.e_off, a.g_off = (C.c_int32 * 2)(e_off, e_off), (C.c_int32 * 2)(g_off, g_off)
        assert L.tgt_triplet_aggregate_proj64_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
        assert b'outside the E/G row' in L.tgt_last_error()
        assert L.tgt_triplet_aggregate_proj64_fwd_skip(C.byref(a), C.c_void_p(p + 1), p, 256, p, p, None) == ERR_INVALID
        assert b'outside the E/G row' in L.tgt_last_error()
    # ungated: the G offsets are not looked at
    a = _valid_looking(_args(gated=False), p)
    a.g_off = (C.c_int32 * 2)(-5, 600)
    a.ld_out = 513                                              # (so that the call still ends in a refusal: nothing is launched)
    assert L.tgt_triplet_aggregate_proj64_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
    assert b'16-byte aligned' in L.tgt_last_error()


@pytest.mark.parametrize('N', [33, 64])
def test_factor_at_an_odd_address_is_invalid(N):
    """every other argument looks valid (host addresses, aligned): the last check refuses, nothing is launched"""
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    a = _valid_looking(_args(N=N), p)
    for odd in (1, 2, 3):
        rc = L.tgt_triplet_aggregate_proj64_fwd_skip(C.byref(a), C.c_void_p(p + 64 + odd), p, 256, p, p, None)
        assert rc == ERR_INVALID
        assert b'graph_scale must be 4-byte aligned' in L.tgt_last_error()


def test_the_n32_entry_points_answer_as_they_did():
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args(N=33)
    assert L.tgt_triplet_aggregate_proj_supported(C.byref(a), 256) == 0
    assert L.tgt_triplet_aggregate_proj_fwd(C.byref(a), None, 256, None, None, None) == ERR_UNSUPPORTED
    assert b'projected triplet aggregate needs N <= 32' in L.tgt_last_error()
    a = _args(N=32)
    assert L.tgt_triplet_aggregate_proj_supported(C.byref(a), 256) == 1


def test_predicate_of_ops_is_the_kernels():
    """ops._agg_proj64_ok on CPU tensors is False whatever the shape (the ops run on the GPU only); its shape terms are checked
    against the library's predicate with the device term taken out"""
    import torch
    from tgt_amd import ops, _lib

    class OnDevice:                                             # (stands in for a CUDA tensor: is_cuda and numel are all that is read)
        is_cuda = True

        def __init__(self, B, N):
            self.n = B * N * N * 256

        def numel(self):
            return self.n
    L = ops.AggregateLayout(256, 16, gated=True)
    assert not ops._agg_proj64_ok(torch.empty(64, 48, 48, 256, dtype=torch.bfloat16, device='meta'), 48, L, torch.bfloat16)
    for N in (32, 33, 48, 64, 65):
        B = -(-ops._SPLIT_MIN_ROWS // (N * N))
        a = _args(N=N)
        want = bool(_lib.lib().tgt_triplet_aggregate_proj64_supported(C.byref(a), 256))
        assert ops._agg_proj64_ok(OnDevice(B, N), N, L, torch.bfloat16) is want
        assert ops._agg_proj64_ok(OnDevice(B, N), N, L, torch.float32) is False
    assert ops._agg_proj64_ok(OnDevice(1, 48), 48, L, torch.bfloat16) is False      # too few edge rows
    # _agg_proj_ok is what it was
    assert ops._agg_proj_ok(OnDevice(64, 32), 32, L, torch.bfloat16) is True
    assert ops._agg_proj_ok(OnDevice(64, 33), 33, L, torch.bfloat16) is False


def test_knob_is_a_flag_read_through_the_spec():
    """TGT_AGG_PROJ64_INFER ships ON by the rule of DESIGN.md 4.za: the slowest knob-on run of the inference benchmark beat the fastest
    knob-off run of the same build (profiles/agg_proj64_infer_ab.txt; tools/infer_bench.py --only cfg5 --nodes 48 --batch 256, fresh
    processes, alternating):
        TGT_AGG_PROJ64_INFER=0   584.7 / 583.8 / 580.9 graphs/s
        TGT_AGG_PROJ64_INFER=1   697.3 / 703.7 / 693.3 graphs/s
    and tools/kernel_bench.py --only aggproj, narrow Linear + kernel against library GEMM + plain kernel, median ms:
        N = 48, B = 256   fp16 0.5666 / 1.0074   bf16 0.5561 / 0.9879
        N = 64, B = 128   fp16 0.4256 / 0.8098   bf16 0.4152 / 0.7937"""
    from tgt_amd import knobs, ops
    assert knobs._SPEC['agg_proj64_infer'][:3] == ('TGT_AGG_PROJ64_INFER', True, 'flag')
    assert knobs._read('TGT_AGG_PROJ64_INFER_unset_', True, 'flag') is True
    assert isinstance(knobs.K.agg_proj64_infer, bool)
    assert ops._AGG_PROJ64_INFER == knobs.K.agg_proj64_infer
    # the N <= 32 knob is untouched
    assert knobs._SPEC['agg_proj_infer'][:3] == ('TGT_AGG_PROJ_INFER', True, 'flag')
