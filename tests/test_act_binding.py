"""CPU-side checks of the plain-activation feature (relu / silu / elu): the C ABI declares and exports tgt_act_dropout_fwd / _bwd
and the TGT_EPI_ACT / TGT_EPI_ACT_BWD epilogues of tgt_edge_linear, and refuses bad arguments before anything touches a device; the
module layer routes the three names and has its A/B knob."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ['relu', 'silu', 'elu']


def test_binding_and_header_declare_the_act_entries():
    from tgt_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tgt_hip.h')).read()
    for name in ('tgt_act_dropout_fwd', 'tgt_act_dropout_bwd'):
        assert name in _lib.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(_lib.lib(), name)
    # the arguments of tgt_gelu_dropout_scaled_fwd / _bwd plus the kind (behind n)
    for d in ('fwd', 'bwd'):
        gelu, act = _lib.SYMBOLS[f'tgt_gelu_dropout_scaled_{d}'], _lib.SYMBOLS[f'tgt_act_dropout_{d}']
        k = 3 if d == 'fwd' else 4
        assert act[0] is gelu[0] and act[1][:k] == gelu[1][:k] and act[1][k] is C.c_int32 and act[1][k + 1:] == gelu[1][k:]
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32              # new symbols and enum values only
    enums = dict(re.findall(r'\b(TGT_(?:ACT|EPI|EDGE)_[A-Z_]+)\s*=\s*(\d+)', header))
    assert [int(enums['TGT_ACT_' + k.upper()]) for k in KINDS] == [_lib.ACT_KINDS[k] for k in KINDS] == [0, 1, 2]
    assert set(_lib.ACT_KINDS) == set(KINDS)
    assert int(enums['TGT_EPI_ACT']) == _lib.EPI_ACT == 6 and int(enums['TGT_EPI_ACT_BWD']) == _lib.EPI_ACT_BWD == 7
    assert int(enums['TGT_EDGE_ACT_KIND_SHIFT']) == _lib.EDGE_ACT_KIND_SHIFT == _lib.EDGE_GLU_KIND_SHIFT
    assert int(enums['TGT_EDGE_ACT_KIND_MASK']) == 3 << _lib.EDGE_ACT_KIND_SHIFT and not int(enums['TGT_EDGE_ACT_KIND_MASK']) & _lib.EDGE_BIAS_SCALED
    # no struct changes: the argument block has the size the GLU change left
    assert C.sizeof(_lib.EdgeLinearArgs) == 240


def test_act_entries_refuse_bad_arguments():
    from tgt_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64            # host memory: every check below fails before a launch
    x, y, dy = base, base + 1024, base + 2048
    ok = dict(n=16, kind=_lib.ACT_SILU, dtype=_lib.TGT_BF16, p=0.1)

    def fwd(x=x, y=y, scale=None, eps_=0, **kw):
        a = dict(ok, **kw)
        return L.tgt_act_dropout_fwd(x, y, a['n'], a['kind'], a['dtype'], a['p'], 1, scale, eps_, None)

    def bwd(x=x, dy=dy, dx=y, **kw):
        a = dict(ok, **kw)
        return L.tgt_act_dropout_bwd(x, dy, dx, a['n'], a['kind'], a['dtype'], a['p'], 1, None, 0, None)

    for code, msg, call in ((1, b'null', lambda: fwd(x=None)), (1, b'null', lambda: fwd(y=None)), (1, b'null', lambda: bwd(dy=None)),
                            (1, b'null', lambda: fwd(n=-1)),
                            (1, b'outside [0,1)', lambda: fwd(p=1.0)), (1, b'outside [0,1)', lambda: bwd(p=-0.5)),
                            (1, b'bad kind', lambda: fwd(kind=3)), (1, b'bad kind', lambda: bwd(kind=-1)),
                            (1, b'bad dtype', lambda: fwd(dtype=7)),
                            (1, b'16-byte aligned', lambda: fwd(x=x + 2)), (1, b'16-byte aligned', lambda: bwd(dx=y + 8)),
                            (1, b'multiple of 8', lambda: fwd(scale=base + 3072, eps_=12)),
                            (1, b'multiple of 8', lambda: fwd(scale=base + 3072, eps_=0))):
        assert call() == code, (msg, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (msg, L.tgt_last_error())
    assert fwd(n=0) == 0                                  # nothing to do is not an error


def _args(_lib, epilogue, K=256, N=256, dtype=None, kind=0, **kw):
    q = _lib.EdgeLinearArgs()
    q.M, q.K, q.N, q.dtype, q.epilogue = 128, K, N, _lib.TGT_BF16 if dtype is None else dtype, epilogue
    q.flags = kind << _lib.EDGE_ACT_KIND_SHIFT
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_act_epilogues_supported_shapes_and_refusals():
    """all NULL tensors, nothing launched: tgt_edge_linear_supported / _live_supported answer from the argument block alone"""
    from tgt_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)
    for epi in (_lib.EPI_ACT, _lib.EPI_ACT_BWD):
        scale = {'row_scale' if epi == _lib.EPI_ACT else 'out_scale': one, 'rows_per_sample': 1}
        for K in (64, 128, 256):
            for dtype in (_lib.TGT_BF16, _lib.TGT_F16):
                for kind in range(3):
                    assert L.tgt_edge_linear_supported(_args(_lib, epi, K=K, dtype=dtype, kind=kind)) == 1
                    assert L.tgt_edge_linear_live_supported(_args(_lib, epi, K=K, dtype=dtype, kind=kind, **scale)) == 1
        for bad in (dict(dtype=_lib.TGT_F32), dict(N=128), dict(N=512), dict(K=512), dict(K=32), dict(kind=3), dict(dw_partial=one),
                    dict(gamma=one), dict(flags=_lib.EDGE_BIAS_SCALED)):
            q = _args(_lib, epi, **bad)
            assert L.tgt_edge_linear_supported(q) == 0, (epi, bad)
            assert L.tgt_edge_linear_live_supported(q) == 0, (epi, bad)
            q.a = q.w = q.out = q.out2 = q.res = one          # (host checks only: the refusal comes before any pointer is used)
            assert L.tgt_edge_linear(q, None) == 2 and b'unsupported' in L.tgt_last_error(), (epi, bad, L.tgt_last_error())
    # colsum_partial rows as for the GELU pair: one per persistent workgroup of an N = 256 launch
    assert L.tgt_edge_linear_parts(64, 256) == 2 and L.tgt_edge_linear_parts(1, 256) == 1
    # a NULL argument block / NULL tensors are refused, not dereferenced
    assert L.tgt_edge_linear(_args(_lib, _lib.EPI_ACT), None) == 1 and b'null' in L.tgt_last_error()


def test_ffn_routes_the_three_names_and_the_knob_exists():
    from tgt_amd import knobs, ops
    from tgt_amd.tgt.layers.blocks import FFN, get_activation
    assert sorted(ops.ACT_KINDS) == sorted(KINDS)
    for name in KINDS:
        fn, mul = get_activation(name)
        assert mul == 1 and fn is getattr(torch.nn.functional, name)
        ffn = FFN(32, 1., activation=name)
        assert not ffn.can_fold_scale()                 # TGT_Layer hands these names no per-sample factor
        assert tuple(ffn.lin_W1.weight.shape) == (32, 32)
    for fn_name in ('act_dropout', 'linear_act_dropout', 'linear_act_dropout_ok'):
        assert callable(getattr(ops, fn_name))
    assert knobs._SPEC['ffn_act_epi'][:3] == ('TGT_FFN_ACT_EPI', True, 'flag')
    assert isinstance(knobs.K.ffn_act_epi, bool) and ops._FFN_ACT_EPI == knobs.K.ffn_act_epi
    assert knobs._read('TGT_FFN_ACT_EPI', True, 'flag') is (os.environ.get('TGT_FFN_ACT_EPI') != '0')
    with pytest.raises(RuntimeError, match='unknown activation'):
        ops.act_dropout(torch.zeros(4, 16), 'tanh', 0.0, False)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_act_ops_fail_loudly_without_gpu():
    from tgt_amd import ops
    from tgt_amd.tgt.layers.blocks import FFN
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.act_dropout(torch.zeros(4, 16), 'relu', 0.0, False)
    assert not ops.linear_act_dropout_ok(torch.zeros(4, 256), torch.zeros(256, 256))
    with pytest.raises(RuntimeError):
        FFN(32, 1., activation='silu')(torch.zeros(2, 32))
