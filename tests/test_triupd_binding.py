"""CPU-side checks of TriangularUpdate inside a TGT layer: the C ABI declares and exports the tiled core
(tgt_triangular_update_tiled_*) and the gated output stage (tgt_edge_gated_out_*), both answer `supported` from their arguments
alone and refuse bad arguments before anything touches a device; the module has its own attend / out_proj_residual_ln, keeps the
oracle's state_dict keys, and the two A/B knobs exist."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('tgt_triangular_update_tiled_supported', 'tgt_triangular_update_tiled_fwd', 'tgt_triangular_update_tiled_bwd',
           'tgt_edge_gated_out_supported', 'tgt_edge_gated_out_parts', 'tgt_edge_gated_out_fwd', 'tgt_edge_gated_out_bwd')


def test_binding_and_header_declare_the_seven_entries():
    from tgt_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tgt_hip.h')).read()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32              # new symbols and a new struct only
    assert C.sizeof(_lib.EdgeLinearArgs) == 240
    # the existing entries keep their signatures
    assert _lib.SYMBOLS['tgt_triangular_update_fwd'][1] == [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p]


def test_edge_gated_args_match_the_header():
    from tgt_amd import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "tgt_hip.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(tgt_edge_gated_args), offsetof(tgt_edge_gated_args, a), offsetof(tgt_edge_gated_args, res),
        offsetof(tgt_edge_gated_args, eps), offsetof(tgt_edge_gated_args, row_scale), offsetof(tgt_edge_gated_args, db_partial));
 return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(td, 't')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    G = _lib.EdgeGatedArgs
    assert v == [C.sizeof(G), G.a.offset, G.res.offset, G.eps.offset, G.row_scale.offset, G.db_partial.offset]


def test_supported_answers_from_the_arguments_alone():
    from tgt_amd import _lib
    L = _lib.lib()
    for dtype in (_lib.TGT_BF16, _lib.TGT_F16):
        for N in (1, 5, 32, 33, 64):
            for H in (8, 16, 32):
                assert L.tgt_triangular_update_tiled_supported(N, H, dtype) == 1, (N, H, dtype)
        for N, H in ((65, 16), (128, 16), (0, 16), (20, 3), (20, 0), (20, 6)):
            assert L.tgt_triangular_update_tiled_supported(N, H, dtype) == 0, (N, H, dtype)
    assert L.tgt_triangular_update_tiled_supported(20, 16, _lib.TGT_F32) == 0

    def gated(K=32, C_=256, dtype=_lib.TGT_BF16):
        a = _lib.EdgeGatedArgs()
        a.M, a.K, a.C, a.dtype = 64, K, C_, dtype
        return a
    for dtype in (_lib.TGT_BF16, _lib.TGT_F16):
        for K in (16, 32, 64):
            assert L.tgt_edge_gated_out_supported(C.byref(gated(K=K, dtype=dtype))) == 1
    for bad in (dict(K=8), dict(K=128), dict(K=48), dict(C_=128), dict(C_=512), dict(dtype=_lib.TGT_F32)):
        assert L.tgt_edge_gated_out_supported(C.byref(gated(**bad))) == 0, bad
    assert L.tgt_edge_gated_out_supported(None) == 0
    # one partial plane per persistent workgroup, never more than there are 32-row tiles
    assert L.tgt_edge_gated_out_parts(1) == 1 and L.tgt_edge_gated_out_parts(64) == 2 and L.tgt_edge_gated_out_parts(0) == 0


def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 63) // 64 * 64          # host memory: every refusal below comes before a launch


def test_tiled_core_refuses_bad_arguments_before_a_launch():
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    ok = dict(e4=p, ld_e=64, v4=p + 1024, ld_v=64, mask=p + 2048, out=p + 3072, d_out=p + 3072, d_e4=p + 4096, ld_de=64,
              d_v4=p + 5120, ld_dv=64, B=1, N=20, H=16, dtype=_lib.TGT_BF16)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.tgt_triangular_update_tiled_fwd(a['e4'], a['ld_e'], a['v4'], a['ld_v'], a['mask'], a['out'], a['B'], a['N'], a['H'],
                                                 a['dtype'], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return L.tgt_triangular_update_tiled_bwd(a['e4'], a['ld_e'], a['v4'], a['ld_v'], a['mask'], a['d_out'], a['d_e4'], a['ld_de'],
                                                 a['d_v4'], a['ld_dv'], a['B'], a['N'], a['H'], a['dtype'], None)

    for code, msg, call in ((1, b'null', lambda: fwd(e4=None)), (1, b'null', lambda: fwd(mask=None)), (1, b'null', lambda: fwd(out=None)),
                            (1, b'null', lambda: bwd(d_out=None)), (1, b'null', lambda: bwd(d_v4=None)),
                            (2, b'dtype 0', lambda: fwd(dtype=_lib.TGT_F32)), (2, b'dtype 0', lambda: bwd(dtype=_lib.TGT_F32)),
                            (2, b'N = 65', lambda: fwd(N=65)), (2, b'N = 65', lambda: bwd(N=65)),
                            (2, b'H = 3', lambda: fwd(H=3)), (2, b'H = 3', lambda: bwd(H=3)),
                            (1, b'row stride', lambda: fwd(ld_e=56)), (1, b'row stride', lambda: fwd(ld_v=68)),
                            (1, b'row stride', lambda: bwd(ld_de=63)), (1, b'row stride', lambda: bwd(ld_dv=32)),
                            (1, b'16-byte aligned', lambda: fwd(v4=p + 1024 + 8)), (1, b'16-byte aligned', lambda: fwd(out=p + 3072 + 2)),
                            (1, b'16-byte aligned', lambda: bwd(d_e4=p + 4096 + 4)),
                            (1, b'bad size', lambda: fwd(B=-1)), (1, b'bad dtype', lambda: fwd(dtype=5))):
        assert call() == code, (msg, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (msg, L.tgt_last_error())
    assert fwd(B=0) == 0 and bwd(B=0) == 0                  # nothing to do is not an error
    # the packed form: the two halves of one (rows, 8H) buffer
    assert fwd(B=0, v4=p + 128, ld_e=128, ld_v=128) == 0


def test_gated_stage_refuses_bad_arguments_before_a_launch():
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()

    def args(**kw):
        a = _lib.EdgeGatedArgs()
        a.M, a.K, a.C, a.dtype, a.parts = 64, 32, 256, _lib.TGT_BF16, 2
        a.a, a.lda, a.w, a.ldw, a.bias = p, 32, p + 256, 32, p + 512
        a.res, a.s, a.y, a.gamma, a.beta, a.mean, a.rstd = p + 768, p + 1024, p + 1280, p + 1536, p + 1792, p + 2048, p + 2304
        a.eps = 1e-5
        a.dt, a.d_a, a.ld_da, a.dw_partial, a.db_partial = p + 2560, p + 2816, 32, p + 3072, p + 3328
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    fwd = lambda **kw: L.tgt_edge_gated_out_fwd(C.byref(args(**kw)), None)
    bwd = lambda **kw: L.tgt_edge_gated_out_bwd(C.byref(args(**kw)), None)
    assert L.tgt_edge_gated_out_fwd(None, None) == 1 and b'null' in L.tgt_last_error()
    assert L.tgt_edge_gated_out_bwd(None, None) == 1 and b'null' in L.tgt_last_error()
    for code, msg, call in ((1, b'null', lambda: fwd(a=None)), (1, b'null', lambda: fwd(bias=None)), (1, b'null', lambda: fwd(res=None)),
                            (1, b'null', lambda: fwd(rstd=None)), (1, b'null', lambda: bwd(dt=None)), (1, b'null', lambda: bwd(db_partial=None)),
                            (2, b'dtype 0', lambda: fwd(dtype=_lib.TGT_F32)), (2, b'dtype 0', lambda: bwd(dtype=_lib.TGT_F32)),
                            (2, b'C = 128', lambda: fwd(C=128)), (2, b'C = 128', lambda: bwd(C=128)),
                            (2, b'K = 48', lambda: fwd(K=48)),
                            (1, b'ldw 24', lambda: fwd(ldw=24)), (1, b'ldw 36', lambda: bwd(ldw=36)), (1, b'lda 20', lambda: fwd(lda=20)),
                            (1, b'ld_da 12', lambda: bwd(ld_da=12)),
                            (1, b'16-byte aligned', lambda: fwd(a=p + 8)), (1, b'16-byte aligned', lambda: fwd(s=p + 1024 + 2)),
                            (1, b'16-byte aligned', lambda: bwd(d_a=p + 2816 + 4)),
                            (1, b'rows_per_sample', lambda: fwd(row_scale=p + 4096, rows_per_sample=0)),
                            (1, b'partial planes', lambda: bwd(parts=0)), (1, b'partial planes', lambda: bwd(parts=3)),
                            (1, b'bad size', lambda: fwd(M=-1))):
        assert call() == code, (msg, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (msg, L.tgt_last_error())
    assert fwd(M=0) == 0 and bwd(M=0) == 0


def test_layer_module_has_its_own_attend_and_output_stage():
    from oracle import modules as om
    from tgt_amd.tgt.layers import blocks, triplet
    kw = dict(node_width=48, edge_width=32, num_heads=4, triplet_heads=4, triplet_type='tiangular_update')
    layer = blocks.TGT_Layer(**kw)
    tria = layer.tria
    assert type(tria) is triplet.TriangularUpdate
    assert callable(getattr(tria, 'attend', None))
    assert type(tria).out_proj_residual_ln is not triplet._TripletBase.out_proj_residual_ln
    assert 'out_proj_residual_ln' in vars(triplet.TriangularUpdate) and 'attend' in vars(triplet.TriangularUpdate)
    # the index table of the fused projection is no registered buffer: the keys stay the reference's
    assert list(layer.state_dict()) == list(om.TGT_Layer(**kw).state_dict())
    assert tria._table.n_rows == 32 and tria._table.n_src == 2
    assert tria._table.row_src.tolist() == [0] * 16 + [1] * 16 and tria._table.row_idx.tolist() == list(range(16)) * 2


def test_the_two_knobs_exist_and_are_read_as_the_others():
    from tgt_amd import knobs, ops
    for field, var, name in (('triupd_tiled', 'TGT_TRIUPD_TILED', '_TRIUPD_TILED'), ('triupd_gated', 'TGT_TRIUPD_GATED', '_TRIUPD_GATED')):
        spec = knobs._SPEC[field]
        assert spec[0] == var and spec[2] == 'flag' and isinstance(spec[1], bool)
        assert isinstance(getattr(knobs.K, field), bool) and getattr(ops, name) == getattr(knobs.K, field)
        assert knobs._read(var + '_never_set', spec[1], 'flag') is spec[1]
        flipped = knobs.Knobs(**{**{f: getattr(knobs.K, f) for f in knobs._SPEC}, field: not spec[1]})
        assert flipped.non_default().get(var) is (not spec[1])
    assert callable(ops.triangular_update_packed) and callable(ops.gated_linear_residual_layer_norm)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_new_ops_fail_loudly_without_gpu():
    from tgt_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.triangular_update_packed(torch.zeros(1, 4, 4, 64), torch.zeros(1, 4, 4), 8)
    with pytest.raises(ValueError):
        ops.triangular_update_packed(torch.zeros(1, 4, 4, 60), torch.zeros(1, 4, 4), 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.gated_linear_residual_layer_norm(torch.zeros(4, 32), torch.zeros(512, 32), torch.zeros(512), torch.zeros(4, 256), None,
                                             torch.ones(256), torch.zeros(256))
