"""CPU-side checks of the live tile lists of the edge row kernels (tgt_edge_live_tiles, tgt_edge_linear_live,
tgt_edge_linear_live_supported): NEW symbols only -- header, ctypes mirror and library agree on them, the ABI version and the
argument struct stay what they were, a NULL list is the plain call, and what a list cannot go with is refused before anything
is launched."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')
NEW = ['tgt_edge_live_tiles', 'tgt_edge_linear_live', 'tgt_edge_linear_live_supported']
OLD = ['tgt_edge_linear', 'tgt_edge_linear_supported', 'tgt_edge_linear_parts', 'tgt_edge_linear_set_grid_cap']


def _header():
    with open(HEADER) as fh:
        return fh.read()


def _declared():
    return set(re.findall(r'^\w[\w \*]*?\b(tgt_\w+)\s*\(', _header(), re.M))


def _args(K, N, epilogue, fake=True):
    """an argument block whose tensors are a fake non-null address (never dereferenced on the host; nothing here reaches a launch)"""
    from tgt_amd import _lib
    g = _lib.EdgeLinearArgs()
    g.M, g.K, g.N, g.dtype, g.epilogue = 3 * 20 * 20, K, N, _lib.TGT_BF16, epilogue
    if fake:
        one = C.c_void_p(16)
        g.a = g.w = g.out = g.out2 = g.res = one
        g.lda, g.ldw, g.ldo, g.ldo2, g.ldr = K, K, N, N, N
        if epilogue == _lib.EPI_LN_BWD:
            g.gamma = g.beta = g.mean = g.rstd = one
    return g


def test_new_symbols_are_declared_bound_and_exported():
    from tgt_amd import _lib
    declared = _declared()
    L = _lib.lib()
    for name in NEW + OLD:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name) is not None


def test_signatures_match_the_header():
    from tgt_amd import _lib
    S = _lib.SYMBOLS
    h = re.sub(r'\s+', ' ', _header())
    assert 'int tgt_edge_live_tiles(const int32_t* node_counts, int32_t B, int32_t N, int32_t* tiles, void* stream);' in h
    assert 'int tgt_edge_linear_live_supported(const tgt_edge_linear_args* a);' in h
    assert 'int tgt_edge_linear_live(const tgt_edge_linear_args* a, const int32_t* tiles, void* stream);' in h
    assert S['tgt_edge_live_tiles'] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p])
    assert S['tgt_edge_linear_live_supported'] == S['tgt_edge_linear_supported']
    res, args = S['tgt_edge_linear']
    assert S['tgt_edge_linear_live'] == (res, [args[0], C.c_void_p] + args[1:])      # the list right behind the argument block


def test_abi_version_and_argument_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    EA = _lib.EdgeLinearArgs
    assert C.sizeof(EA) == 240
    want = dict(M=0, K=8, N=12, dtype=16, epilogue=20, a=24, lda=32, w=40, ldw=48, bias=56, gamma=64, beta=72, eps=80, colsum_rows=84,
                mean=88, rstd=96, y=104, ldy=112, out=120, ldo=128, out2=136, ldo2=144, res=152, ldr=160, ds_in=168, ld_ds=176,
                row_scale=184, out_scale=192, rows_per_sample=200, dropout_p=208, flags=212, dropout_seed=216, colsum_partial=224,
                dw_partial=232)
    assert {name: getattr(EA, name).offset for name, _ in EA._fields_} == want
    assert not hasattr(EA, 'tiles')                                      # the list travels beside the struct, not in it


def test_null_list_is_the_plain_call():
    """tiles == NULL forwards to tgt_edge_linear: the same answer, and the same message, on a NULL block and on null tensors"""
    from tgt_amd import _lib
    L = _lib.lib()
    null = C.POINTER(_lib.EdgeLinearArgs)()
    for g in (None, _args(256, 256, _lib.EPI_GELU, fake=False), _args(256, 100, _lib.EPI_BIAS, fake=False)):
        ref = null if g is None else C.byref(g)
        want = L.tgt_edge_linear(ref, None)
        want_msg = L.tgt_last_error()
        assert want == 1                                                 # TGT_ERR_INVALID: null argument
        assert L.tgt_edge_linear_live(ref, None, None) == want
        assert L.tgt_last_error() == want_msg
    g = _args(96, 256, _lib.EPI_GELU)                                    # an unsupported K: UNSUPPORTED either way
    assert L.tgt_edge_linear(C.byref(g), None) == 2
    assert L.tgt_edge_linear_live(C.byref(g), None, None) == 2


def test_what_a_list_cannot_go_with_is_refused_before_any_launch():
    """the slice kernel's shapes (64 / 128-row tiles) and the fused weight gradient: TGT_ERR_UNSUPPORTED (2).  The tensors and the list
    are fake addresses a launch would fault on -- the refusal comes first"""
    from tgt_amd import _lib
    L = _lib.lib()
    tiles = C.c_void_p(16)
    for K, N, epi in ((256, 128, _lib.EPI_BIAS), (256, 64, _lib.EPI_BIAS), (64, 128, _lib.EPI_RESID), (256, 128, _lib.EPI_LN_BWD)):
        g = _args(K, N, epi)
        assert L.tgt_edge_linear_supported(C.byref(g)) == 1, (K, N, epi)            # the plain call takes it (on the slice kernel)
        assert L.tgt_edge_linear_live_supported(C.byref(g)) == 0, (K, N, epi)
        assert L.tgt_edge_linear_live(C.byref(g), tiles, None) == 2, (K, N, epi)
        assert b'live tile list' in L.tgt_last_error()
    g = _args(256, 256, _lib.EPI_GELU_BWD)
    assert L.tgt_edge_linear_live_supported(C.byref(g)) == 1
    g.dw_partial = C.c_void_p(16)
    assert L.tgt_edge_linear_live_supported(C.byref(g)) == 0
    assert L.tgt_edge_linear_live(C.byref(g), tiles, None) == 2


def test_the_row_kernels_take_a_list():
    from tgt_amd import _lib
    L = _lib.lib()
    E = _lib
    for K, N, epi in ((64, 256, E.EPI_GELU), (128, 256, E.EPI_RESID), (256, 256, E.EPI_GELU_BWD), (256, 256, E.EPI_LN_BWD),
                      (512, 256, E.EPI_RESID), (256, 512, E.EPI_BIAS), (256, 512, E.EPI_GLU)):
        assert L.tgt_edge_linear_live_supported(C.byref(_args(K, N, epi))) == 1, (K, N, epi)
    assert L.tgt_edge_linear_live_supported(None) == 0


def test_list_builder_refuses_null_tensors_and_bad_sizes():
    from tgt_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(16)
    assert L.tgt_edge_live_tiles(None, 2, 4, p, None) == 1
    assert L.tgt_edge_live_tiles(p, 2, 4, None, None) == 1
    assert L.tgt_edge_live_tiles(p, -1, 4, p, None) == 1
    assert L.tgt_edge_live_tiles(p, 2, -4, p, None) == 1


def test_knob_defaults_off():
    from tgt_amd import knobs
    assert knobs._SPEC['edge_ragged'][:3] == ('TGT_EDGE_RAGGED', False, 'flag')
    assert knobs._read('TGT_EDGE_RAGGED_never_set', False, 'flag') is False
    assert 'edge_ragged' in {f.name for f in __import__('dataclasses').fields(knobs.Knobs)}


def test_python_surface():
    import inspect
    from tgt_amd import ops
    from tgt_amd.tgt import stack
    p = inspect.signature(ops.edge_linear_raw).parameters
    assert p['live'].default is None and p['live'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(ops.edge_live_tiles).parameters) == ['node_counts', 'N']
    assert ops._edge_live is None
    token = object()
    with ops.edge_live(token) as got:
        assert got is token and ops._edge_live is token
        with ops.edge_live(None):
            assert ops._edge_live is None
        assert ops._edge_live is token
    assert ops._edge_live is None
    assert stack._EDGE_RAGGED is False or os.environ.get('TGT_EDGE_RAGGED') == '1'
