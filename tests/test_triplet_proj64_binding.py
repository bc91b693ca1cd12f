"""CPU-side checks of the projection-fused triplet attention forward for 33..64 nodes (tgt_triplet_attention_proj64_supported /
_proj64_fwd / _proj64_fwd_counts, csrc/triplet_attention_proj64.hip): three NEW symbols next to an unchanged ABI -- version,
argument struct -- and next to the unchanged entry points of the N <= 32 kernel.  The entry point checks the argument block, the
sizes, then the supported predicate, then the tensors and the factor's alignment, before anything is launched.  Host pointers are
never dereferenced."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
NAMES = ('tgt_triplet_attention_proj64_supported', 'tgt_triplet_attention_proj64_fwd', 'tgt_triplet_attention_proj64_fwd_counts')
VARIANTS = ['gated', 'ungated', 'axial']


def _args(N=48, H=16, D=16, dtype=None, variant='gated', flag=True):
    from tgt_amd import _lib
    a = _lib.TripletAttentionArgs()
    a.B, a.N, a.H, a.D = 2, N, H, D
    a.dtype = _lib.TGT_BF16 if dtype is None else dtype
    a.flags = {'gated': _lib.TRI_BIASED | _lib.TRI_GATED, 'ungated': _lib.TRI_BIASED, 'axial': 0}[variant]
    if flag:
        a.flags |= _lib.TRI_NO_QKV_STORE
    a.scale = 0.25
    return a


def _host():
    """(buffer, its 64-byte aligned address): host memory standing in for tensors and factors -- never dereferenced"""
    buf = (C.c_char * 256)()
    return buf, (C.addressof(buf) + 63) & ~63


def _valid_looking(a, p):
    """every tensor but Q/K/V given (host address p, 64-byte aligned), rows and offsets aligned"""
    vp = C.c_void_p
    a.eg = (vp * 2)(p, p)
    a.ld_eg = (C.c_int64 * 2)(64, 64)
    a.e_off, a.g_off = (C.c_int32 * 2)(0, 32), (C.c_int32 * 2)(16, 48)
    a.q_off, a.k_off, a.v_off = (C.c_int32 * 2)(0, 768), (C.c_int32 * 2)(256, 1024), (C.c_int32 * 2)(512, 1280)
    a.mask, a.out, a.ld_out = p, p, 512
    a.o_off = (C.c_int32 * 2)(0, 256)
    return a


def _calls(L):
    """the two launching entry points as fn(a, x, C, w, bias) -- the second with NULL node counts"""
    return (lambda a, x, c, w, b: L.tgt_triplet_attention_proj64_fwd(a, x, c, w, b, None),
            lambda a, x, c, w, b: L.tgt_triplet_attention_proj64_fwd_counts(a, None, x, c, w, b, None))


def test_symbols_exist_with_the_declared_signatures():
    from tgt_amd import _lib
    TA, vp, i32 = C.POINTER(_lib.TripletAttentionArgs), C.c_void_p, C.c_int32
    assert _lib.SYMBOLS[NAMES[0]] == (C.c_int, [TA, i32])
    assert _lib.SYMBOLS[NAMES[1]] == (C.c_int, [TA, vp, i32, vp, vp, vp])
    assert _lib.SYMBOLS[NAMES[2]] == (C.c_int, [TA, vp, vp, i32, vp, vp, vp])
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)                                   # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1]
    with open(HEADER) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert 'int tgt_triplet_attention_proj64_supported(const tgt_triplet_attention_args* a, int32_t C);' in text
    assert ('int tgt_triplet_attention_proj64_fwd(const tgt_triplet_attention_args* a, const void* x, int32_t C, const void* w, '
            'const void* bias, void* stream);') in text
    assert ('int tgt_triplet_attention_proj64_fwd_counts(const tgt_triplet_attention_args* a, const int32_t* node_counts, const void* x, '
            'int32_t C, const void* w, const void* bias, void* stream);') in text


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    TA = _lib.TripletAttentionArgs
    assert C.sizeof(TA) == 312
    assert TA.workspace.offset + 16 == C.sizeof(TA)
    assert TA.flags.offset == 20 and TA.flags.size == 4
    assert 'triplet_attention_proj64.hip' in _lib.SOURCES and 'triplet_attention_proj.hip' in _lib.SOURCES


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('N', [33, 48, 64])
def test_supported_shapes(N, dtype, variant):
    from tgt_amd import _lib
    a = _args(N=N, dtype=dict(bf16=_lib.TGT_BF16, f16=_lib.TGT_F16)[dtype], variant=variant)
    assert _lib.lib().tgt_triplet_attention_proj64_supported(C.byref(a), 256) == 1
    # the two kernels' domains are disjoint
    assert _lib.lib().tgt_triplet_attention_proj_supported(C.byref(a), 256) == 0


@pytest.mark.parametrize('change', ['N=32', 'N=65', 'D=8', 'H=8', 'fp32', 'C=128', 'flag clear', 'dropout_p=0.1'])
def test_unsupported_calls_are_refused_before_the_tensors_are_looked_at(change):
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
    elif change == 'C=128':
        width = 128
    elif change == 'flag clear':
        a.flags &= ~_lib.TRI_NO_QKV_STORE
    else:
        a.dropout_p = 0.1
    assert L.tgt_triplet_attention_proj64_supported(C.byref(a), width) == 0
    # every tensor NULL: the answer is UNSUPPORTED, not "null tensor" -- the predicate comes first, and nothing is launched
    for call in _calls(L):
        assert call(C.byref(a), None, width, None, None) == ERR_UNSUPPORTED
        msg = L.tgt_last_error()
        assert b'needs 33 <= N <= 64' in msg and b'TGT_TRI_NO_QKV_STORE' in msg


def test_null_args_and_bad_sizes_come_before_the_predicate():
    from tgt_amd import _lib
    L = _lib.lib()
    assert L.tgt_triplet_attention_proj64_supported(None, 256) == 0
    for call in _calls(L):
        a = _args()
        a.N, a.D = -1, 8
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID
        assert b'bad sizes' in L.tgt_last_error()
        assert call(None, None, 256, None, None) == ERR_INVALID
        assert b'null args' in L.tgt_last_error()


def test_an_empty_batch_is_done_after_the_predicate_and_before_the_tensors():
    from tgt_amd import _lib
    L = _lib.lib()
    for call in _calls(L):
        a = _args()
        a.B = 0
        assert call(C.byref(a), None, 256, None, None) == 0
        a.N = 20                                                # (not this kernel's shape: the predicate comes first)
        assert call(C.byref(a), None, 256, None, None) == ERR_UNSUPPORTED


@pytest.mark.parametrize('variant', VARIANTS)
def test_supported_call_with_null_tensors_is_invalid(variant):
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args(variant=variant)
    assert L.tgt_triplet_attention_proj64_supported(C.byref(a), 256) == 1
    buf, p = _host()
    for call in _calls(L):
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID
        assert b'null tensor' in L.tgt_last_error()
        # with x / w / bias given (host addresses: nothing is launched) the refusal is still INVALID, for mask / out
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID
        assert b'null tensor' in L.tgt_last_error()
    # mask and out given: a third-arm flag without eg is refused, the axial variant goes on to the alignment checks
    a.mask, a.out, a.ld_out = p, p, 513
    assert L.tgt_triplet_attention_proj64_fwd(C.byref(a), p, 256, p, p, None) == ERR_INVALID
    assert (b'16-byte aligned' if variant == 'axial' else b'eg missing') in L.tgt_last_error()
    # misaligned x
    a = _valid_looking(_args(variant=variant), p)
    assert L.tgt_triplet_attention_proj64_fwd(C.byref(a), C.c_void_p(p + 2), 256, p, p, None) == ERR_INVALID
    assert b'16-byte aligned' in L.tgt_last_error()


@pytest.mark.parametrize('N', [33, 64])
def test_factor_at_an_odd_address_is_invalid(N):
    """every other argument looks valid (host addresses, aligned): the last check refuses, nothing is launched"""
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    for call in _calls(L):
        for odd in (1, 2, 3):
            a = _valid_looking(_args(N=N), p)
            a.graph_scale = p + 64 + odd
            assert call(C.byref(a), p, 256, p, p) == ERR_INVALID
            assert b'graph_scale must be 4-byte aligned' in L.tgt_last_error()


def test_the_n32_entry_points_answer_as_they_did():
    from tgt_amd import _lib
    L = _lib.lib()
    for flag in (True, False):
        a = _args(N=33, flag=flag)
        assert L.tgt_triplet_attention_proj_supported(C.byref(a), 256) == 0
        buf, p = _host()                                       # (that entry point looks at x / w / bias first: host addresses)
        assert L.tgt_triplet_attention_proj_fwd(C.byref(a), p, 256, p, p, None) == ERR_UNSUPPORTED
        assert b'projected triplet attention needs N <= 32' in L.tgt_last_error()
        assert L.tgt_triplet_attention_proj_fwd_counts(C.byref(a), None, p, 256, p, p, None) == ERR_UNSUPPORTED
        a = _args(N=32, flag=flag)
        assert L.tgt_triplet_attention_proj_supported(C.byref(a), 256) == 1
        assert L.tgt_triplet_attention_proj64_supported(C.byref(a), 256) == 0
        a = _args(N=20, H=8, flag=flag)                         # (one head group: the N <= 32 kernel's alone)
        assert L.tgt_triplet_attention_proj_supported(C.byref(a), 256) == 1


def test_predicate_of_ops_is_the_kernels():
    """ops._proj64_fused_ok's shape terms against the library's predicate (flag set, no dropout: what the caller adds)"""
    import torch
    from tgt_amd import ops, _lib

    class OnDevice:                                             # (stands in for a CUDA tensor: is_cuda and numel are all that is read)
        is_cuda = True

        def __init__(self, B, N):
            self.n = B * N * N * 256

        def numel(self):
            return self.n
    for variant in VARIANTS:
        L = ops.TripletLayout(256, 16, gated=variant == 'gated', biased=variant != 'axial')
        for N in (32, 33, 48, 64, 65):
            B = -(-ops._SPLIT_MIN_ROWS // (N * N))
            a = _args(N=N, variant=variant)
            want = bool(_lib.lib().tgt_triplet_attention_proj64_supported(C.byref(a), 256))
            assert ops._proj64_fused_ok(OnDevice(B, N), N, L, torch.bfloat16) is want
            assert ops._proj64_fused_ok(OnDevice(B, N), N, L, torch.float16) is want
            assert ops._proj64_fused_ok(OnDevice(B, N), N, L, torch.float32) is False
        assert ops._proj64_fused_ok(OnDevice(1, 48), 48, L, torch.bfloat16) is False      # too few edge rows
    L8 = ops.TripletLayout(256, 8)                              # D = 32
    assert ops._proj64_fused_ok(OnDevice(64, 48), 48, L8, torch.bfloat16) is False
    # _proj_fused_ok is what it was
    L = ops.TripletLayout(256, 16)
    assert bool(ops._proj_fused_ok(OnDevice(64, 32), 32, L, torch.bfloat16)) is bool(ops._TRI_PROJ)
    assert not ops._proj_fused_ok(OnDevice(64, 33), 33, L, torch.bfloat16)


def test_knob_is_a_flag_read_through_the_spec():
    """TGT_TRI_PROJ64_INFER ships ON by the rule of DESIGN.md 4.za: the slowest knob-on run of the inference benchmark beat the fastest
    knob-off run of the same build (profiles/tri_proj64_infer_ab.txt; tools/infer_bench.py --only tgt_at --nodes 48 --batch 128, fresh
    processes, alternating):
        TGT_TRI_PROJ64_INFER=0   3596.9 / 3594.9 / 3605.7 graphs/s
        TGT_TRI_PROJ64_INFER=1   3883.4 / 3893.1 / 3888.7 graphs/s
    and tools/kernel_bench.py --only triproj64 --B 128, narrow Linear + kernel against split GEMMs + tgt_triplet_attention_fwd, median ms:
        N = 48   fp16 0.5740 / 0.7248   bf16 0.5744 / 0.7150
        N = 64   fp16 1.0149 / 1.3293   bf16 1.0446 / 1.3189"""
    from tgt_amd import knobs, ops
    assert knobs._SPEC['tri_proj64_infer'][:3] == ('TGT_TRI_PROJ64_INFER', True, 'flag')
    assert knobs._read('TGT_TRI_PROJ64_INFER_unset_', True, 'flag') is True
    assert isinstance(knobs.K.tri_proj64_infer, bool)
    assert ops._TRI_PROJ64_INFER == knobs.K.tri_proj64_infer
    # the N <= 32 knobs are untouched
    assert knobs._SPEC['tri_proj_infer'][:3] == ('TGT_TRI_PROJ_INFER', True, 'flag')
    assert knobs._SPEC['tri_proj'][:3] == ('TGT_TRI_PROJ', True, 'flag')
