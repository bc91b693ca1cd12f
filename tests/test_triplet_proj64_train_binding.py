"""CPU-side checks of the TRAINING form of the projection-fused triplet attention forward for 33..64 nodes
(tgt_triplet_attention_proj64_train_supported / _train_fwd / _train_fwd_counts, csrc/triplet_attention_proj64.hip built with
-DTGT_TRI_PROJ64_INST=2): three NEW symbols next to an unchanged ABI and next to the unchanged inference entry points, which go on
refusing a cleared TGT_TRI_NO_QKV_STORE.  Modelled on tests/test_triplet_proj64_binding.py.  The entry point checks the argument
block, the sizes, the supported predicate, the empty batch, the tensors the inference entry checks and, last, the Q/K/V tensor,
before anything is launched.  Host pointers are never dereferenced."""
import ctypes as C
import os
import re

import pytest

from test_triplet_proj64_binding import _args, _host, _valid_looking

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
NAMES = ('tgt_triplet_attention_proj64_train_supported', 'tgt_triplet_attention_proj64_train_fwd',
         'tgt_triplet_attention_proj64_train_fwd_counts')
VARIANTS = ['gated', 'ungated', 'axial']


def _train_args(**kw):
    return _args(flag=False, **kw)


def _with_qkv(a, p, ld=1536):
    a.qkv = (C.c_void_p * 2)(p, p)
    a.ld_qkv = (C.c_int64 * 2)(ld, ld)
    return a


def _calls(L):
    """the two launching entry points as fn(a, x, C, w, bias) -- the second with NULL node counts"""
    return (lambda a, x, c, w, b: L.tgt_triplet_attention_proj64_train_fwd(a, x, c, w, b, None),
            lambda a, x, c, w, b: L.tgt_triplet_attention_proj64_train_fwd_counts(a, None, x, c, w, b, None))


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
    assert 'int tgt_triplet_attention_proj64_train_supported(const tgt_triplet_attention_args* a, int32_t C);' in text
    assert ('int tgt_triplet_attention_proj64_train_fwd(const tgt_triplet_attention_args* a, const void* x, int32_t C, const void* w, '
            'const void* bias, void* stream);') in text
    assert ('int tgt_triplet_attention_proj64_train_fwd_counts(const tgt_triplet_attention_args* a, const int32_t* node_counts, '
            'const void* x, int32_t C, const void* w, const void* bias, void* stream);') in text


def test_abi_version_struct_and_the_inference_unit_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32
    assert C.sizeof(_lib.TripletAttentionArgs) == 312
    # the storing instantiations are a translation unit of their own, next to the inference unit's plain entry
    assert 'triplet_attention_proj64.hip' in _lib.SOURCES
    assert ('triplet_attention_proj64.hip', ['-DTGT_TRI_PROJ64_INST=2'], '.train') in _lib.SOURCES


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('N', [33, 48, 64])
def test_supported_shapes(N, dtype, variant):
    from tgt_amd import _lib
    a = _train_args(N=N, dtype=dict(bf16=_lib.TGT_BF16, f16=_lib.TGT_F16)[dtype], variant=variant)
    assert _lib.lib().tgt_triplet_attention_proj64_train_supported(C.byref(a), 256) == 1
    # the old predicates still answer 0 with the flag clear above 32 nodes
    assert _lib.lib().tgt_triplet_attention_proj64_supported(C.byref(a), 256) == 0
    assert _lib.lib().tgt_triplet_attention_proj_supported(C.byref(a), 256) == 0


@pytest.mark.parametrize('change', ['N=32', 'N=65', 'D=8', 'H=8', 'fp32', 'C=128', 'flag set', 'dropout_p=0.1'])
def test_unsupported_calls_are_refused_before_the_tensors_are_looked_at(change):
    from tgt_amd import _lib
    L = _lib.lib()
    a, width = _train_args(), 256
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
    elif change == 'flag set':
        a.flags |= _lib.TRI_NO_QKV_STORE
    else:
        a.dropout_p = 0.1
    assert L.tgt_triplet_attention_proj64_train_supported(C.byref(a), width) == 0
    for call in _calls(L):
        assert call(C.byref(a), None, width, None, None) == ERR_UNSUPPORTED
        msg = L.tgt_last_error()
        assert b'needs 33 <= N <= 64' in msg and b'D = 16' in msg and b'H = 16' in msg and b'C = 256' in msg
        assert b'TGT_TRI_NO_QKV_STORE clear' in msg


def test_the_inference_entry_points_still_refuse_a_cleared_flag():
    from tgt_amd import _lib
    L = _lib.lib()
    a = _train_args()
    assert L.tgt_triplet_attention_proj64_supported(C.byref(a), 256) == 0
    for code in (L.tgt_triplet_attention_proj64_fwd(C.byref(a), None, 256, None, None, None),
                 L.tgt_triplet_attention_proj64_fwd_counts(C.byref(a), None, None, 256, None, None, None)):
        assert code == ERR_UNSUPPORTED
        msg = L.tgt_last_error()
        assert b'needs 33 <= N <= 64' in msg and b'TGT_TRI_NO_QKV_STORE' in msg


def test_check_order():
    """null args, sizes (INVALID) -> the predicate (UNSUPPORTED) -> B == 0 (OK) -> the inference entry's checks -> qkv, last"""
    from tgt_amd import _lib
    L = _lib.lib()
    assert L.tgt_triplet_attention_proj64_train_supported(None, 256) == 0
    buf, p = _host()
    for call in _calls(L):
        assert call(None, None, 256, None, None) == ERR_INVALID and b'null args' in L.tgt_last_error()
        a = _train_args()
        a.N, a.D = -1, 8                                        # (bad size AND unsupported: the size comes first)
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID and b'bad sizes' in L.tgt_last_error()
        a = _train_args()
        a.B = 0
        assert call(C.byref(a), None, 256, None, None) == 0     # (every tensor NULL: an empty batch is done before them)
        a.N = 20
        assert call(C.byref(a), None, 256, None, None) == ERR_UNSUPPORTED      # (the predicate comes before the empty batch)
        # the inference entry's checks, each with a NULL qkv behind it that is not reached
        a = _train_args()
        assert call(C.byref(a), None, 256, None, None) == ERR_INVALID and b'null tensor' in L.tgt_last_error()
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID and b'null tensor' in L.tgt_last_error()       # (mask / out)
        a.mask, a.out, a.ld_out = p, p, 512
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID and b'eg missing' in L.tgt_last_error()
        a = _valid_looking(_train_args(), p)
        assert call(C.byref(a), p + 2, 256, p, p) == ERR_INVALID and b'16-byte aligned' in L.tgt_last_error()
        a.graph_scale = p + 65
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID and b'graph_scale must be 4-byte aligned' in L.tgt_last_error()
        # everything else valid-looking: the Q/K/V tensor is what is left
        a = _valid_looking(_train_args(), p)
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID and b'null qkv' in L.tgt_last_error()
        a.qkv = (C.c_void_p * 2)(p, None)
        a.ld_qkv = (C.c_int64 * 2)(1536, 1536)
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID and b'null qkv' in L.tgt_last_error()


@pytest.mark.parametrize('what', ['ld', 'pointer', 'q_off', 'v_off', 'row too short', 'graph too large'])
def test_misaligned_qkv_is_invalid(what):
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    for call in _calls(L):
        a = _with_qkv(_valid_looking(_train_args(), p), p)
        if what == 'ld':
            a.ld_qkv = (C.c_int64 * 2)(1536, 1540)
        elif what == 'pointer':
            a.qkv = (C.c_void_p * 2)(p, p + 8)
        elif what == 'q_off':
            a.q_off = (C.c_int32 * 2)(4, 768)
        elif what == 'v_off':
            a.v_off = (C.c_int32 * 2)(512, 1284)
        elif what == 'row too short':
            a.ld_qkv = (C.c_int64 * 2)(1536, 1528)              # (V_out's 256 columns at 1280 end at 1536)
        else:
            a.ld_qkv = (C.c_int64 * 2)(1536, 1 << 20)           # (48 * 48 * 2^20 * 2 bytes: past the kernel's 32-bit offsets)
        assert call(C.byref(a), p, 256, p, p) == ERR_INVALID
        assert b'qkv rows and offsets must be 16-byte aligned' in L.tgt_last_error()


def test_knob_is_off_by_default_and_read_through_the_spec():
    from tgt_amd import knobs, ops
    assert knobs._SPEC['tri_proj64_train'][:3] == ('TGT_TRI_PROJ64_TRAIN', False, 'flag')
    assert knobs._read('TGT_TRI_PROJ64_TRAIN_unset_', False, 'flag') is False
    assert isinstance(knobs.K.tri_proj64_train, bool)
    assert ops._TRI_PROJ64_TRAIN == knobs.K.tri_proj64_train
    assert knobs._SPEC['tri_proj64_infer'][:3] == ('TGT_TRI_PROJ64_INFER', True, 'flag')
