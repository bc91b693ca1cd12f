"""CPU-side checks of attention dropout on the 16-wide-tile triplet kernels (tri_att16_fwd_kernel / tri_att16_bwd_kernel, 33..64 nodes)
and of its switch: tgt_triplet_attention_family is host logic (no tensor is needed, nothing is dereferenced); with TGT_TRI_DROP16=1 in
the environment a call with dropout_p > 0 that qualifies for the 16-wide tiles with p == 0 stays on them, forward and backward each by
its own conditions; with the variable unset or 0 the routing is the one of before (GENERAL); the library reads the variable per call.
ABI number and argument struct are untouched."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from test_triplet_drop_fast_binding import ROOT, _args, _family


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv('TGT_TRI_DROP16', '1')


def test_knob_is_declared_off_and_the_host_binds_it():
    from tgt_amd import knobs, ops
    spec = knobs._SPEC['tri_drop16']
    assert spec[0] == 'TGT_TRI_DROP16' and spec[1] is False and spec[2] == 'flag'
    assert 'profiles/tri_drop16_ab.txt' in spec[3]
    assert knobs._read('TGT_TRI_DROP16_not_set', spec[1], spec[2]) is False
    assert ops._TRI_DROP16 == knobs.K.tri_drop16
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32 and C.sizeof(_lib.TripletAttentionArgs) == 312


def test_dropout_at_33_to_64_nodes_is_routed_to_the_16_wide_tiles(on):
    """fails on the parent commit: its library ignores the variable and sends every p > 0 call of these sizes to GENERAL"""
    from tgt_amd import _lib
    for bwd in (0, 1):
        for dtype in (_lib.TGT_BF16, _lib.TGT_F16):
            assert _family(_args(N=40, p=0.3, H=16, D=16, dtype=dtype), bwd) == _lib.TRI_FAMILY_TILES16
        for N in (33, 48, 49, 64):
            for colsum in (False, True):
                assert _family(_args(N=N, colsum=colsum), bwd) == _lib.TRI_FAMILY_TILES16, (N, bwd)
                assert _family(_args(N=N, p=0.0, colsum=colsum), bwd) == _lib.TRI_FAMILY_TILES16, (N, bwd)
        assert _family(_args(N=40, p=0.05, flags=0), bwd) == _lib.TRI_FAMILY_TILES16           # axial: no third arm to look at


def test_forward_and_backward_route_independently(on):
    """N = 56, H = 2: the forward needs H % 4 (GENERAL, one head per workgroup), the backward of 49..64 nodes H % 2"""
    from tgt_amd import _lib
    assert _family(_args(N=56, H=2), 0) == _lib.TRI_FAMILY_GENERAL
    assert _family(_args(N=56, H=2), 1) == _lib.TRI_FAMILY_TILES16
    assert _family(_args(N=56, H=2, p=0.0), 0) == _lib.TRI_FAMILY_GENERAL
    assert _family(_args(N=56, H=2, p=0.0), 1) == _lib.TRI_FAMILY_TILES16
    assert _family(_args(N=40, H=2), 1) == _lib.TRI_FAMILY_GENERAL                             # (33..48 nodes: H % 4 both ways)


def test_still_general_with_the_switch_on(on):
    from tgt_amd import _lib
    for bwd in (0, 1):
        assert _family(_args(N=40, dtype=_lib.TGT_F32), bwd) == _lib.TRI_FAMILY_GENERAL
        assert _family(_args(N=40, D=8, H=32), bwd) == _lib.TRI_FAMILY_GENERAL
        # E / G column blocks that do not start at a multiple of H: the dropout kernels step aside (p == 0 does not look at them)
        assert _family(_args(N=40, e_off=(C.c_int32 * 2)(4, 36)), bwd) == _lib.TRI_FAMILY_GENERAL
        assert _family(_args(N=40, p=0.0, e_off=(C.c_int32 * 2)(4, 36)), bwd) == _lib.TRI_FAMILY_TILES16


@pytest.mark.parametrize('value', [None, '0', '1'])
def test_other_sizes_do_not_see_the_switch(value, monkeypatch):
    from tgt_amd import _lib
    if value is None:
        monkeypatch.delenv('TGT_TRI_DROP16', raising=False)
    else:
        monkeypatch.setenv('TGT_TRI_DROP16', value)
    monkeypatch.delenv('TGT_TRI_DROP_FAST', raising=False)
    for p in (0.0, 0.3):
        assert _family(_args(N=32, p=p), 0) == _lib.TRI_FAMILY_GENERAL
        assert _family(_args(N=32, p=p), 1) == _lib.TRI_FAMILY_BWD2
        assert _family(_args(N=11, p=p), 1) == _lib.TRI_FAMILY_BWD2
        for bwd in (0, 1):
            assert _family(_args(N=65, p=p), bwd) == _lib.TRI_FAMILY_KB
            assert _family(_args(N=72, p=p), bwd) == _lib.TRI_FAMILY_KB
            assert _family(_args(N=0, p=p), bwd) == _lib.TRI_FAMILY_NONE
            assert _family(_args(N=129, p=p), bwd) < 0
    for bwd in (0, 1):
        assert _family(_args(N=40, p=1.0), bwd) < 0


def test_library_reads_the_switch_per_call_and_defaults_off(monkeypatch):
    """only calls with p > 0 ask for the variable, so one process can run both arms (the GPU A/B does)"""
    from tgt_amd import _lib
    for bwd in (0, 1):
        a, a0 = _args(N=40, p=0.3), _args(N=40, p=0.0)
        monkeypatch.delenv('TGT_TRI_DROP16', raising=False)
        assert _family(a, bwd) == _lib.TRI_FAMILY_GENERAL and _family(a0, bwd) == _lib.TRI_FAMILY_TILES16
        monkeypatch.setenv('TGT_TRI_DROP16', '0')
        assert _family(a, bwd) == _lib.TRI_FAMILY_GENERAL and _family(a0, bwd) == _lib.TRI_FAMILY_TILES16
        monkeypatch.setenv('TGT_TRI_DROP16', '1')
        assert _family(a, bwd) == _lib.TRI_FAMILY_TILES16 and _family(a0, bwd) == _lib.TRI_FAMILY_TILES16
        monkeypatch.delenv('TGT_TRI_DROP16')
        assert _family(a, bwd) == _lib.TRI_FAMILY_GENERAL


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import test_triplet_drop_fast_binding as t
from tgt_amd import _lib, knobs, ops
assert knobs.K.tri_drop16 is True and ops._TRI_DROP16 is True and knobs.K.non_default().get('TGT_TRI_DROP16') is True
for bwd in (0, 1):
    assert t._family(t._args(N=40, p=0.3), bwd) == _lib.TRI_FAMILY_TILES16
    assert t._family(t._args(N=72), bwd) == _lib.TRI_FAMILY_KB
print('child ok')
"""


def test_switch_on_in_a_fresh_process():
    """TGT_TRI_DROP16=1 from the start: the knob record, what bench.py would report, and the library agree"""
    env = dict(os.environ, TGT_TRI_DROP16='1')
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, os.path.join(ROOT, 'tests'))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b'child ok' in r.stdout, r.stdout.decode(errors='replace')
