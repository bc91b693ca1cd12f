"""CPU-side checks of attention dropout on the round-4 triplet backward (tri_att_bwd2, N <= 32) and of the routing function that
came with it: tgt_triplet_attention_family is host logic (no tensor is needed, nothing is dereferenced), a call with
dropout_p > 0 that qualifies for tri_att_bwd2 is routed there, TGT_TRI_DROP_FAST=0 gives the routing of before, and ABI number
and argument struct are untouched.  The projection-fused FORWARD keeps refusing dropout_p > 0 (its p > 0 kernels would carry the 12-16
bytes of scratch the p = 0 kernels have: profiles/tri_drop_fast_isa.txt), which is asserted here too."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tgt_hip.h')
FAMILIES = ('NONE', 'GENERAL', 'BWD2', 'TILES16', 'KB')


def _args(N=32, H=16, D=16, dtype=None, p=0.3, flags=None, colsum=False, **kw):
    """the argument block of the headline call (16-bit, C = 256, H = 16, D = 16): sizes, layout numbers and -- where a check looks
    at alignment -- fake 16-byte aligned addresses that nothing dereferences"""
    from tgt_amd import _lib
    a = _lib.TripletAttentionArgs()
    a.B, a.N, a.H, a.D = 2, N, H, D
    a.dtype = _lib.TGT_BF16 if dtype is None else dtype
    a.flags = (_lib.TRI_BIASED | _lib.TRI_GATED) if flags is None else flags
    a.scale, a.dropout_p, a.dropout_seed = 0.25, p, 0x1234567890ABCDEF
    C_ = H * D
    for d in (0, 1):
        a.ld_qkv[d], a.ld_eg[d] = 6 * C_, 4 * H
        a.q_off[d], a.k_off[d], a.v_off[d] = 3 * C_ * d, C_ + 3 * C_ * d, 2 * C_ + 3 * C_ * d
        a.e_off[d], a.g_off[d] = 2 * H * d, 2 * H * d + H
        a.ld_dqkv[d] = a.ld_deg[d] = 6 * C_ + 4 * H
        if colsum:
            a.d_qkv_colsum[d] = a.d_eg_colsum[d] = 0x10000
    a.ld_out = 2 * C_
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _family(a, bwd):
    from tgt_amd import _lib
    return _lib.lib().tgt_triplet_attention_family(C.byref(a), bwd)


def test_symbol_enum_and_abi():
    from tgt_amd import _lib
    L = _lib.lib()
    assert 'tgt_triplet_attention_family' in _lib.SYMBOLS and L.tgt_triplet_attention_family is not None
    with open(HEADER) as fh:
        hdr = fh.read()
    assert 'int tgt_triplet_attention_family(const tgt_triplet_attention_args* a, int32_t bwd);' in hdr
    for value, name in enumerate(FAMILIES):
        assert int(re.search(r'TGT_TRI_FAMILY_%s = (\d+)' % name, hdr).group(1)) == value == getattr(_lib, 'TRI_FAMILY_' + name)
    # new symbols only
    assert _lib.ABI_VERSION == 32 and L.tgt_abi_version() == 32
    assert C.sizeof(_lib.TripletAttentionArgs) == 312


def test_knob_is_declared_and_the_host_binds_it():
    from tgt_amd import knobs, ops
    assert knobs._SPEC['tri_drop_fast'][0] == 'TGT_TRI_DROP_FAST' and knobs._SPEC['tri_drop_fast'][2] == 'flag'
    assert 'profiles/tri_drop_fast_ab.txt' in knobs._SPEC['tri_drop_fast'][3]
    assert ops._TRI_DROP_FAST == knobs.K.tri_drop_fast


def test_dropout_backward_is_routed_to_the_round4_kernel():
    """fails on the parent commit (no such symbol; its library sends every p > 0 backward to tri_att_bwd_kernel)"""
    from tgt_amd import _lib
    assert os.environ.get('TGT_TRI_DROP_FAST', '1') != '0'
    for colsum in (False, True):
        assert _family(_args(colsum=colsum), 1) == _lib.TRI_FAMILY_BWD2
        assert _family(_args(colsum=colsum, p=0.0), 1) == _lib.TRI_FAMILY_BWD2
        assert _family(_args(colsum=colsum, N=11, p=0.05), 1) == _lib.TRI_FAMILY_BWD2
    assert _family(_args(), 0) == _lib.TRI_FAMILY_GENERAL                      # the forward of that call: 32-wide tiles
    assert _family(_args(dtype=_lib.TGT_F16), 1) == _lib.TRI_FAMILY_BWD2
    assert _family(_args(H=8), 1) == _lib.TRI_FAMILY_BWD2                      # one head group


def test_family_of_the_other_shapes():
    from tgt_amd import _lib
    assert _family(_args(H=4), 1) == _lib.TRI_FAMILY_GENERAL
    assert _family(_args(dtype=_lib.TGT_F32), 1) == _lib.TRI_FAMILY_GENERAL
    assert _family(_args(D=8, H=32), 1) == _lib.TRI_FAMILY_GENERAL
    for bwd in (0, 1):
        assert _family(_args(N=40, p=0.0), bwd) == _lib.TRI_FAMILY_TILES16
        assert _family(_args(N=40, p=0.3), bwd) == _lib.TRI_FAMILY_GENERAL    # the 16-wide tiles keep p == 0
        assert _family(_args(N=72), bwd) == _lib.TRI_FAMILY_KB
        assert _family(_args(N=0), bwd) == _lib.TRI_FAMILY_NONE
        assert _family(_args(B=0), bwd) == _lib.TRI_FAMILY_NONE
    # third-arm rows that are not whole 16-byte pieces: the round-4 kernel steps aside, with and without dropout
    assert _family(_args(e_off=(C.c_int32 * 2)(4, 36)), 1) == _lib.TRI_FAMILY_GENERAL


@pytest.mark.parametrize('change', ['null', 'N=129', 'N=-1', 'H=0', 'p=1.0', 'p=-0.1', 'dtype=7', 'D=12', 'N=72,D=32', 'H=3,D=4'])
def test_family_is_negative_where_the_entry_point_refuses(change):
    from tgt_amd import _lib
    L = _lib.lib()
    if change == 'null':
        assert L.tgt_triplet_attention_family(None, 1) < 0
        return
    kw = {}
    for item in change.split(','):
        k, v = item.split('=')
        kw[{'p': 'p'}.get(k, k)] = float(v) if k == 'p' else int(v)
    a = _args(**kw)
    for bwd in (0, 1):
        assert _family(a, bwd) < 0
        entry = L.tgt_triplet_attention_bwd if bwd else L.tgt_triplet_attention_fwd
        assert entry(C.byref(a), None) != 0                   # refused before any launch (no tensor here is real)


def test_projection_fused_forward_still_refuses_dropout():
    """that kernel did not get dropout (module docstring): its predicate answers as on the parent commit, at every N"""
    from tgt_amd import _lib
    L = _lib.lib()
    assert L.tgt_triplet_attention_proj_supported(C.byref(_args(p=0.0)), 256) == 1
    assert L.tgt_triplet_attention_proj_supported(C.byref(_args(p=0.3)), 256) == 0
    for kw, width in ((dict(N=33), 256), (dict(dtype=_lib.TGT_F32), 256), (dict(D=8, H=32), 256), (dict(), 128)):
        assert L.tgt_triplet_attention_proj_supported(C.byref(_args(p=0.0, **kw)), width) == 0


_CHILD = """
import ctypes as C, sys
sys.path[:0] = [%r, %r]
import test_triplet_drop_fast_binding as t
from tgt_amd import _lib, knobs
assert knobs.K.tri_drop_fast is False
for colsum in (False, True):
    assert t._family(t._args(colsum=colsum), 1) == _lib.TRI_FAMILY_GENERAL
    assert t._family(t._args(colsum=colsum, p=0.0), 1) == _lib.TRI_FAMILY_BWD2
assert t._family(t._args(N=40, p=0.0), 1) == _lib.TRI_FAMILY_TILES16
assert t._family(t._args(N=72), 1) == _lib.TRI_FAMILY_KB
assert _lib.lib().tgt_triplet_attention_proj_supported(C.byref(t._args(p=0.3)), 256) == 0
print('child ok')
"""


def test_switch_off_gives_the_routing_of_before():
    """TGT_TRI_DROP_FAST=0 in a fresh process: p > 0 leaves the round-4 kernel, everything else stays"""
    env = dict(os.environ, TGT_TRI_DROP_FAST='0')
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, os.path.join(ROOT, 'tests'))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b'child ok' in r.stdout, r.stdout.decode(errors='replace')


def test_library_reads_the_switch_per_call(monkeypatch):
    """only calls with p > 0 ask for the variable, so one process can run both arms (the GPU A/B does)"""
    from tgt_amd import _lib
    a = _args()
    monkeypatch.setenv('TGT_TRI_DROP_FAST', '0')
    assert _family(a, 1) == _lib.TRI_FAMILY_GENERAL
    monkeypatch.setenv('TGT_TRI_DROP_FAST', '1')
    assert _family(a, 1) == _lib.TRI_FAMILY_BWD2
    monkeypatch.delenv('TGT_TRI_DROP_FAST')
    assert _family(a, 1) == _lib.TRI_FAMILY_BWD2
