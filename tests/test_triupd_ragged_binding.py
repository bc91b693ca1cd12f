"""CPU-side checks of TriangularUpdate on ragged batches: the tiled core with per-graph node counts
(tgt_triangular_update_tiled_fwd_counts / _bwd_counts) and the gated output stage on a live tile list
(tgt_edge_gated_out_fwd_live / _bwd_live).  NEW symbols only -- header, ctypes mirror and library agree on them, the ABI version
and the argument structs stay what they were, a NULL count / list is the plain call, every refusal comes before a launch in the
order the plain entry points document, and the module declares what TGT_Encoder's ragged switches ask for."""
import ctypes as C
import inspect
import os
import re
import warnings

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
NEW = ['tgt_triangular_update_tiled_fwd_counts', 'tgt_triangular_update_tiled_bwd_counts',
       'tgt_edge_gated_out_fwd_live', 'tgt_edge_gated_out_bwd_live']
OLD = ['tgt_triangular_update_tiled_fwd', 'tgt_triangular_update_tiled_bwd', 'tgt_edge_gated_out_fwd', 'tgt_edge_gated_out_bwd']


def _header():
    with open(HEADER) as fh:
        return fh.read()


def test_new_symbols_are_declared_bound_and_exported():
    from tgt_amd import _lib
    declared = set(re.findall(r'^\w[\w \*]*?\b(tgt_\w+)\s*\(', _header(), re.M))
    L = _lib.lib()
    for name in NEW + OLD:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None


def test_signatures_match_the_header_and_extend_the_plain_ones():
    from tgt_amd import _lib
    S = _lib.SYMBOLS
    h = re.sub(r'\s+', ' ', _header())
    assert ('int tgt_triangular_update_tiled_fwd_counts(const void* e4, int64_t ld_e, const void* v4, int64_t ld_v, const float* mask, '
            'void* out, int32_t B, int32_t N, int32_t H, int32_t dtype, const int32_t* node_counts, void* stream);') in h
    assert ('int tgt_triangular_update_tiled_bwd_counts(const void* e4, int64_t ld_e, const void* v4, int64_t ld_v, const float* mask, '
            'const void* d_out, void* d_e4, int64_t ld_de, void* d_v4, int64_t ld_dv, int32_t B, int32_t N, int32_t H, int32_t dtype, '
            'const int32_t* node_counts, void* stream);') in h
    assert 'int tgt_edge_gated_out_fwd_live(const tgt_edge_gated_args* a, const int32_t* tiles, void* stream);' in h
    assert 'int tgt_edge_gated_out_bwd_live(const tgt_edge_gated_args* a, const int32_t* tiles, void* stream);' in h
    for plain, new in zip(OLD, NEW):
        res, args = S[plain]
        # the counts / the list right in front of the stream; everything else as the plain entry point has it
        assert S[new] == (res, args[:-1] + [C.c_void_p] + args[-1:]), new
    assert S[NEW[0]][1][-2:] == [C.c_void_p, C.c_void_p] and len(S[NEW[0]][1]) == len(S[OLD[0]][1]) + 1
    assert S[NEW[2]] == (C.c_int, [C.POINTER(_lib.EdgeGatedArgs), C.c_void_p, C.c_void_p])


def test_abi_version_and_structs_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32
    assert C.sizeof(_lib.EdgeLinearArgs) == 240
    G = _lib.EdgeGatedArgs
    assert C.sizeof(G) == 184
    assert [name for name, _ in G._fields_] == ['M', 'K', 'C', 'dtype', 'parts', 'a', 'lda', 'w', 'ldw', 'bias', 'res', 's', 'y', 'gamma',
                                                'beta', 'eps', '_pad0', 'mean', 'rstd', 'row_scale', 'rows_per_sample', 'dt', 'd_a',
                                                'ld_da', 'dw_partial', 'db_partial']
    assert not hasattr(G, 'tiles')                                       # the list travels beside the struct, not in it


def _host():
    buf = (C.c_char * 8192)()
    return buf, (C.addressof(buf) + 63) // 64 * 64          # host memory: every refusal below comes before a launch


def test_tiled_core_with_counts_refuses_before_a_launch_in_the_plain_order():
    from tgt_amd import _lib
    L = _lib.lib()
    buf, p = _host()
    ok = dict(e4=p, ld_e=64, v4=p + 1024, ld_v=64, mask=p + 2048, out=p + 3072, d_out=p + 3072, d_e4=p + 4096, ld_de=64,
              d_v4=p + 5120, ld_dv=64, B=1, N=20, H=16, dtype=_lib.TGT_BF16, counts=p + 6144)

    def fwd(entry=L.tgt_triangular_update_tiled_fwd_counts, **kw):
        a = dict(ok, **kw)
        tail = () if entry is L.tgt_triangular_update_tiled_fwd else (a['counts'],)
        return entry(a['e4'], a['ld_e'], a['v4'], a['ld_v'], a['mask'], a['out'], a['B'], a['N'], a['H'], a['dtype'], *tail, None)

    def bwd(entry=L.tgt_triangular_update_tiled_bwd_counts, **kw):
        a = dict(ok, **kw)
        tail = () if entry is L.tgt_triangular_update_tiled_bwd else (a['counts'],)
        return entry(a['e4'], a['ld_e'], a['v4'], a['ld_v'], a['mask'], a['d_out'], a['d_e4'], a['ld_de'], a['d_v4'], a['ld_dv'],
                     a['B'], a['N'], a['H'], a['dtype'], *tail, None)

    cases = ((1, b'null', fwd, dict(e4=None)), (1, b'null', fwd, dict(mask=None)), (1, b'null', fwd, dict(out=None)),
             (1, b'null', bwd, dict(d_out=None)), (1, b'null', bwd, dict(d_v4=None)),
             (2, b'dtype 0', fwd, dict(dtype=_lib.TGT_F32)), (2, b'dtype 0', bwd, dict(dtype=_lib.TGT_F32)),
             (2, b'N = 65', fwd, dict(N=65)), (2, b'N = 65', bwd, dict(N=65)), (2, b'H = 3', fwd, dict(H=3)), (2, b'H = 3', bwd, dict(H=3)),
             (1, b'row stride', fwd, dict(ld_e=56)), (1, b'row stride', fwd, dict(ld_v=68)),
             (1, b'row stride', bwd, dict(ld_de=63)), (1, b'row stride', bwd, dict(ld_dv=32)),
             (1, b'16-byte aligned', fwd, dict(v4=p + 1024 + 8)), (1, b'16-byte aligned', fwd, dict(out=p + 3072 + 2)),
             (1, b'16-byte aligned', bwd, dict(d_e4=p + 4096 + 4)),
             (1, b'bad size', fwd, dict(B=-1)), (1, b'bad dtype', fwd, dict(dtype=5)),
             # the order: the predicate before null tensors, null tensors before strides, strides before alignment
             (2, b'N = 65', fwd, dict(N=65, e4=None)), (1, b'null', fwd, dict(e4=None, ld_e=56)),
             (1, b'row stride', fwd, dict(ld_e=56, out=p + 3072 + 2)), (1, b'16-byte aligned', fwd, dict(out=p + 3072 + 2, counts=p + 6146)),
             # the counts pointer comes last
             (1, b'node_counts not 4-byte aligned', fwd, dict(counts=p + 6146)), (1, b'node_counts not 4-byte aligned', bwd, dict(counts=p + 6145)))
    for code, msg, call, kw in cases:
        assert call(**kw) == code, (kw, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (kw, L.tgt_last_error())
    assert fwd(B=0) == 0 and bwd(B=0) == 0                  # nothing to do is not an error, with counts or without
    assert fwd(B=0, counts=None) == 0 and bwd(B=0, counts=None) == 0
    # a NULL count is the plain entry point: the same code and the same message on everything the plain one refuses
    for call, plain in ((fwd, L.tgt_triangular_update_tiled_fwd), (bwd, L.tgt_triangular_update_tiled_bwd)):
        for kw in (dict(e4=None), dict(N=65), dict(ld_v=68), dict(dtype=5), dict(B=0)):
            want = call(entry=plain, **kw)
            want_msg = L.tgt_last_error() if want else None
            assert call(counts=None, **kw) == want, kw
            assert want == 0 or L.tgt_last_error() == want_msg, kw


def test_gated_stage_with_a_list_refuses_before_a_launch_in_the_plain_order():
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

    tiles = p + 4096
    fwd = lambda tiles=tiles, **kw: L.tgt_edge_gated_out_fwd_live(C.byref(args(**kw)), tiles, None)
    bwd = lambda tiles=tiles, **kw: L.tgt_edge_gated_out_bwd_live(C.byref(args(**kw)), tiles, None)
    null = C.POINTER(_lib.EdgeGatedArgs)()
    assert L.tgt_edge_gated_out_fwd_live(null, tiles, None) == 1 and b'null' in L.tgt_last_error()
    assert L.tgt_edge_gated_out_bwd_live(null, tiles, None) == 1 and b'null' in L.tgt_last_error()
    cases = ((1, b'null', fwd, dict(a=None)), (1, b'null', fwd, dict(bias=None)), (1, b'null', fwd, dict(res=None)),
             (1, b'null', fwd, dict(rstd=None)), (1, b'null', bwd, dict(dt=None)), (1, b'null', bwd, dict(db_partial=None)),
             (2, b'dtype 0', fwd, dict(dtype=_lib.TGT_F32)), (2, b'dtype 0', bwd, dict(dtype=_lib.TGT_F32)),
             (2, b'C = 128', fwd, dict(C=128)), (2, b'C = 128', bwd, dict(C=128)), (2, b'K = 48', fwd, dict(K=48)),
             (1, b'ldw 24', fwd, dict(ldw=24)), (1, b'ldw 36', bwd, dict(ldw=36)), (1, b'lda 20', fwd, dict(lda=20)),
             (1, b'ld_da 12', bwd, dict(ld_da=12)),
             (1, b'16-byte aligned', fwd, dict(a=p + 8)), (1, b'16-byte aligned', fwd, dict(s=p + 1024 + 2)),
             (1, b'16-byte aligned', bwd, dict(d_a=p + 2816 + 4)),
             (1, b'rows_per_sample', fwd, dict(row_scale=p + 4096, rows_per_sample=0)),
             (1, b'partial planes', bwd, dict(parts=0)), (1, b'partial planes', bwd, dict(parts=3)),
             (1, b'bad size', fwd, dict(M=-1)),
             # the order: sizes, the predicate, null tensors, strides, alignment, parts -- and the list last
             (2, b'K = 48', fwd, dict(K=48, a=None)), (1, b'null', fwd, dict(a=None, lda=20)), (1, b'lda 20', fwd, dict(lda=20, w=p + 256 + 8)),
             (1, b'partial planes', bwd, dict(parts=3, tiles=p + 4098)),
             (1, b'live tile list not 4-byte aligned', fwd, dict(tiles=p + 4098)), (1, b'live tile list not 4-byte aligned', bwd, dict(tiles=p + 4097)))
    for code, msg, call, kw in cases:
        assert call(**kw) == code, (kw, L.tgt_last_error())
        assert msg in L.tgt_last_error(), (kw, L.tgt_last_error())
    assert fwd(M=0) == 0 and bwd(M=0) == 0 and fwd(M=0, tiles=None) == 0 and bwd(M=0, tiles=None) == 0
    # a NULL list is the plain entry point
    for live, plain in ((fwd, L.tgt_edge_gated_out_fwd), (bwd, L.tgt_edge_gated_out_bwd)):
        for kw in (dict(a=None), dict(C=128), dict(ldw=24), dict(M=-1), dict(M=0)):
            want = plain(C.byref(args(**kw)), None)
            want_msg = L.tgt_last_error() if want else None
            assert live(tiles=None, **kw) == want, kw
            assert want == 0 or L.tgt_last_error() == want_msg, kw


def test_module_and_ops_surface():
    from tgt_amd import ops
    from tgt_amd.tgt.layers.triplet import TriangularUpdate, TripletAggregate, TripletAggregateUngated, TripletAttention
    assert TriangularUpdate.takes_node_counts is True
    assert TriangularUpdate.node_counts_bound_rows is True                       # its counts bound the rows of the mask too
    assert not getattr(TriangularUpdate, 'takes_graph_scale', False)             # DropPath skipping stays out
    for cls in (TripletAggregate, TripletAggregateUngated):
        assert not getattr(cls, 'takes_node_counts', False)                      # the aggregate family still takes no counts
        assert not getattr(cls, 'node_counts_bound_rows', False)
    assert not getattr(TripletAttention, 'node_counts_bound_rows', False)
    for fn in (TriangularUpdate.attend, TriangularUpdate.forward_normed):
        params = list(inspect.signature(fn).parameters.values())
        assert [q.name for q in params] == ['self', 'x', 'mask', 'node_counts'] and params[-1].default is None
    assert list(inspect.signature(TriangularUpdate.forward).parameters) == ['self', 'e', 'mask']
    params = list(inspect.signature(ops.triangular_update_packed).parameters.values())
    assert [q.name for q in params] == ['ev', 'mask3', 'num_heads', 'node_counts'] and params[-1].default is None
    assert list(inspect.signature(ops.triangular_update).parameters) == ['e4', 'v4', 'mask3', 'num_heads']


def test_padding_is_unread_for_a_triangular_update_stack_only():
    from tgt_amd import ops
    from tgt_amd.tgt.stack import TGT_Encoder
    kw = dict(model_height=2, node_width=48, edge_width=32, num_heads=4, triplet_heads=4)
    tri = TGT_Encoder(triplet_type='tiangular_update', **kw)
    agg = TGT_Encoder(triplet_type='aggregate', **kw)
    att = TGT_Encoder(triplet_type='attention', **kw)
    said = set(ops._slow_path_said)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')                                       # no notice for these two
            ops._slow_path_said.clear()
            assert tri._padding_is_unread('k', 'n') is True and tri._edge_ragged_ok() and tri._node_ragged_ok()
            assert att._padding_is_unread('k', 'n') is True
            assert tri._counts_bound_rows() is True and att._counts_bound_rows() is False and agg._counts_bound_rows() is False
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            assert agg._padding_is_unread('triupd_ragged_test', 'has no effect on this model') is False
            assert not agg._edge_ragged_ok() and not agg._node_ragged_ok()
        assert sum('has no effect on this model' in str(x.message) for x in w) == 3
    finally:
        ops._slow_path_said.clear()
        ops._slow_path_said.update(said)
