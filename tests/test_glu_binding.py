"""CPU-side checks of the GLU-family feature (ABI 31): the C ABI declares and exports tgt_glu_dropout_fwd / _bwd and refuses bad
arguments with an error code and a message before anything touches a device; the module layer knows the three gated activations."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ['geglu', 'glu', 'swiglu']


def test_binding_and_header_declare_the_glu_entries():
    from tgt_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tgt_hip.h')).read()
    for name in ('tgt_glu_dropout_fwd', 'tgt_glu_dropout_bwd'):
        assert name in _lib.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(_lib.lib(), name)
    assert len(_lib.SYMBOLS['tgt_glu_dropout_fwd'][1]) == 11 and len(_lib.SYMBOLS['tgt_glu_dropout_bwd'][1]) == 12
    assert _lib.ABI_VERSION >= 31 and _lib.lib().tgt_abi_version() == _lib.ABI_VERSION
    # enum values of the header = constants of the binding
    enums = dict(re.findall(r'\b(TGT_(?:GLU|EPI|EDGE)_[A-Z_]+)\s*=\s*(\d+)', header))
    assert [int(enums['TGT_GLU_' + k.upper()]) for k in KINDS] == [_lib.GLU_KINDS[k] for k in KINDS] == [0, 1, 2]
    assert int(enums['TGT_EPI_GLU']) == _lib.EPI_GLU == 5
    assert int(enums['TGT_EDGE_GLU_KIND_SHIFT']) == _lib.EDGE_GLU_KIND_SHIFT
    assert int(enums['TGT_EDGE_GLU_KIND_MASK']) == 3 << _lib.EDGE_GLU_KIND_SHIFT and not int(enums['TGT_EDGE_GLU_KIND_MASK']) & _lib.EDGE_BIAS_SCALED


def test_glu_entries_refuse_bad_arguments():
    from tgt_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64            # host memory: every check below fails before a launch
    x, y, dy = base, base + 1024, base + 2048
    ok = dict(rows=2, cols=8, kind=_lib.GLU_SWIGLU, dtype=_lib.TGT_BF16, p=0.1)

    def fwd(x=x, y=y, scale=None, eps_=0, **kw):
        a = dict(ok, **kw)
        return L.tgt_glu_dropout_fwd(x, y, a['rows'], a['cols'], a['kind'], a['dtype'], a['p'], 1, scale, eps_, None)

    def bwd(x=x, dy=dy, dx=y, **kw):
        a = dict(ok, **kw)
        return L.tgt_glu_dropout_bwd(x, dy, dx, a['rows'], a['cols'], a['kind'], a['dtype'], a['p'], 1, None, 0, None)

    for code, msg, call in ((1, b'null', lambda: fwd(x=None)), (1, b'null', lambda: fwd(y=None)), (1, b'null', lambda: bwd(dy=None)),
                            (1, b'outside [0,1)', lambda: fwd(p=1.0)), (1, b'outside [0,1)', lambda: bwd(p=-0.5)),
                            (1, b'bad kind', lambda: fwd(kind=3)), (1, b'bad dtype', lambda: fwd(dtype=7)),
                            (2, b'multiple of 8', lambda: fwd(cols=12)), (2, b'multiple of 4', lambda: bwd(cols=6, dtype=_lib.TGT_F32)),
                            (1, b'bad sizes', lambda: fwd(cols=0)), (1, b'16-byte aligned', lambda: fwd(x=x + 2)),
                            (1, b'16-byte aligned', lambda: bwd(dx=y + 8)),
                            (1, b'whole number of rows', lambda: fwd(scale=base + 3072, eps_=12))):
        assert call() == code, (msg, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (msg, L.tgt_last_error())
    assert fwd(rows=0) == 0                               # nothing to do is not an error


def test_get_activation_multipliers_and_fold():
    from tgt_amd.tgt.layers.blocks import FFN, get_activation
    from tgt_amd import ops
    assert sorted(ops.GLU_KINDS) == sorted(KINDS)
    for name in KINDS:
        fn, mul = get_activation(name)
        assert mul == 2 and callable(fn)
        ffn = FFN(32, 1., activation=name)
        assert ffn.can_fold_scale()
        assert tuple(ffn.lin_W1.weight.shape) == (64, 32) and tuple(ffn.lin_W2.weight.shape) == (32, 32)
    assert get_activation('gelu')[1] == 1 and FFN(32, 1., activation='gelu').can_fold_scale()
    assert not FFN(32, 1., activation='relu').can_fold_scale()
    for fn_name in ('glu_dropout', 'linear_glu_dropout', 'linear_glu_dropout_ok'):
        assert callable(getattr(ops, fn_name))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_glu_ops_fail_loudly_without_gpu():
    from tgt_amd import ops
    from tgt_amd.tgt.layers.blocks import FFN
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.glu_dropout(torch.zeros(4, 16), 'geglu', 0.0, False)
    assert not ops.linear_glu_dropout_ok(torch.zeros(4, 256), torch.zeros(512, 256))
    with pytest.raises(RuntimeError):
        FFN(32, 1., activation='swiglu')(torch.zeros(2, 32))
